"""Raw frames with the erase and alpha operators for k2_tiles<7>, checked against tests/alpha_modes_model.py: frames written directly
as swfr_upload_edges arrays (composite_scenes.RawFrame, which here takes the operator names "erase" and "alpha" and grows an ALPHA
group's rectangle as the rectangle rule asks), each aimed at one branch of the walk over a strip's list -- and strip_alpha_reach,
what a frame's strips see of the two operators, from the arrays alone.  Frames are 128 x 32 (two tile columns, two tile rows, eight
strips) unless a test says otherwise."""
import numpy as np

import alpha_modes_model as am
import composite_scenes as cs
from composite_scenes import BEGIN, END, MODES, STRIP_H, STRIP_W, add_member, premultiplied

MASK = 4
W, H = 128, 32
ALL_MODES = list(MODES) + ["erase"]                                  # what a path can be composited with
END_MODES = ALL_MODES + ["alpha"]


class AlphaRawFrame(cs.RawFrame):
    def _path(self, kind, rows, rect, argb, lerp, op, even_odd=False, style=None):
        if op != "erase":
            return super()._path(kind, rows, rect, argb, lerp, op, even_odd, style)
        assert not lerp
        super()._path(kind, rows, rect, argb, 0, "normal", even_odd, style)
        self.paths[-1][5] = am.OP_ERASE << 8
        return self

    def end(self, op="normal", opacity=255, grow=True):
        """grow=False: an ALPHA group keeps the union of its members' rectangles (what upload refuses when earlier paths lie outside)"""
        if op not in am.OPERATORS:
            return super().end(op, opacity)
        b, m = self.open[-1], self.masks[-1]
        super().end("normal", opacity)
        e = self.paths[-1]
        e[5] = am.OPERATORS[op] << 8 | (255 - int(opacity)) << 24
        if op == "alpha" and grow:
            # everything drawn since the surface the group is composited onto began: the enclosing BEGIN or, behind it, its MASK
            start = 0 if not self.open else (self.masks[-1] if self.masks[-1] is not None else self.open[-1]) + 1
            rects = [p[6:10] for p in self.paths[start:b] if p[6] < p[8] and p[7] < p[9]] + ([e[6:10]] if e[6] < e[8] and e[7] < e[9] else [])
            if rects:
                was_empty = not (e[6] < e[8] and e[7] < e[9])
                rect = [min(r[0] for r in rects), min(r[1] for r in rects), max(r[2] for r in rects), max(r[3] for r in rects)]
                for i in [b, len(self.paths) - 1] + ([m] if m is not None else []):
                    self.paths[i][6:10] = rect
                if was_empty:                                        # (a group empty as a whole was parked at a corner of its own: keep it inside)
                    for i in range(b + 1, len(self.paths) - 1):
                        if i != m:
                            self.paths[i][6:10] = [rect[0], rect[1], rect[0], rect[1]]
        return self


def op_of(path):
    return (int(path["lerp"]) >> 8) & 0xff


def _ground(fr, rng, x0=-1, y0=-1, x1=None, y1=None):
    """a translucent rectangle and a triangle over it: every strip they cover holds pixels an ALPHA END must clear"""
    x1, y1 = fr.W + 1 if x1 is None else x1, fr.H + 1 if y1 is None else y1
    fr.rect_tor(x0, y0, x1, y1, premultiplied(rng, 150), 1)
    fr.tor([(x0 + 3, y0 + 2), (x1 - 2, y0 + 4), ((x0 + x1) / 2, y1 - 1.5)], premultiplied(rng, 90))


def cleared_strips_frame(mode="alpha", cut=False, opacity=255, seed=0, far=False):
    """One `mode` group over a ground: its members reach strip (0, 0) alone; every other strip of the ground the group reaches by its
    rectangle alone: under ALPHA they are cleared -- both tile columns, both strips of a tile -- under ERASE left alone.
    cut: the ground, and so the group's rectangle, ends inside strips in x and in y.
    far: a second member in the opposite corner (an ERASE group's rectangle is the union of its members': it then spans strips none reaches)."""
    rng = np.random.default_rng(seed)
    fr = AlphaRawFrame(W, H)
    if cut:
        _ground(fr, rng, 9.5, 3.25, 101, 21.5)
        x, y = 12, 4
    else:
        _ground(fr, rng)
        x, y = 5, 1
    fr.begin()
    fr.tor([(x, y), (x + 40, y + 1), (x + 15, y + 3.5)], premultiplied(rng, 200), 1)
    fr.box(x + 5.5, y + 0.25, x + 30, y + 3, premultiplied(rng, 120), 0, "multiply")
    if far:
        fr.tor([(x + 70, y + 13.5), (x + 85, y + 14), (x + 75, y + 16.5)], premultiplied(rng, 160))
    fr.end(mode, opacity)
    fr.tor([(5, 30), (100, 2), (126, 25)], premultiplied(rng, 120), 0, "overlay")
    return fr


def masked_reach_frame(mode="alpha", seed=0):
    """A masked `mode` group over a ground: content and mask both reach strip (0, 0); the content alone strip (1, 0); the mask alone
    strip (0, 1); neither the other five"""
    rng = np.random.default_rng(seed)
    fr = AlphaRawFrame(W, H)
    _ground(fr, rng)
    fr.begin()
    fr.tor([(5, 1), (50, 2), (20, 7)], premultiplied(rng, 220), 1)
    fr.box(10.5, 9.25, 40, 14.5, premultiplied(rng, 180))
    fr.mask()
    fr.rect_tor(8, 0.5, 45, 6.5, premultiplied(rng, 200), 1)
    fr.tor([(70, 1), (120, 3), (90, 7.5)], premultiplied(rng, 140))
    fr.end(mode)
    fr.tor([(5, 30), (100, 2), (126, 25)], premultiplied(rng, 120))
    return fr


def sizes_frame(what, n_before, n_members=3, n_after=2, seed=0):
    """`n_before` plain entries, then `what` -- "erase_path", or a group of `n_members` members closed by "erase" or "alpha" --, then
    `n_after` plain entries, every one reaching strip (0, 0): the path sits at list position n_before, a group's END at
    n_before + n_members + 1"""
    rng = np.random.default_rng(7000 + 100 * n_before + seed)
    fr = AlphaRawFrame(W, H)
    for i in range(n_before):
        add_member(fr, rng, ("full_translucent", "box", "partial")[i % 3], ALL_MODES[(seed + i) % 10] if i else "normal", 0, 0, first=i == 0)
    if what == "erase_path":
        add_member(fr, rng, ("partial", "box", "full_translucent")[n_before % 3], "erase", 0, 0)
    else:
        fr.begin()
        for i in range(n_members):
            add_member(fr, rng, cs.MEMBER_CLASSES[(seed + i) % 6], ALL_MODES[(seed + 3 * i) % 10], 0, 0, first=i == 0)
        fr.end(what, (255, 200)[n_before % 2])
    for i in range(n_after):
        add_member(fr, rng, ("partial", "full_translucent", "box")[i % 3], ALL_MODES[(seed + 2 * i) % 10], 0, 0)
    return fr


def cover_frame(seed=0):
    """an ERASE path below and above an opaque full cover of strip row 0 (the walk starts behind the cover), and an ALPHA group above it"""
    rng = np.random.default_rng(seed)
    fr = AlphaRawFrame(W, H)
    _ground(fr, rng)
    fr.tor([(5, 1), (100, 2), (60, 7)], premultiplied(rng, 200), 0, "erase")
    fr.rect_tor(-1, 0, W + 1, 8, premultiplied(rng, 255), 1)          # the cover
    fr.tor([(8, 1), (120, 3), (40, 7.5)], premultiplied(rng, 160), 0, "erase")
    fr.box(70.5, 2.25, 110, 6, premultiplied(rng, 255), 0, "erase")
    fr.begin()
    fr.tor([(3, 2), (60, 1), (30, 7)], premultiplied(rng, 230), 1)
    fr.end("alpha")
    return fr


def partial_rows_frame(seed=0):
    """an ERASE box path and an ERASE tor path that cover some rows of their strip only, over a ground, in both tile columns"""
    rng = np.random.default_rng(seed)
    fr = AlphaRawFrame(W, H)
    _ground(fr, rng)
    fr.box(4.5, 2.25, 50, 5.5, premultiplied(rng, 190), 0, "erase")
    fr.tor([(70, 10.5), (120, 11), (90, 14.25)], premultiplied(rng, 210), 0, "erase")
    fr.tor([(10, 17.5), (100, 18), (60, 30.25)], premultiplied(rng, 99), 0, "erase")
    return fr


def nesting_frame(depth, where, seed=0):
    """groups nested `depth` deep over a ground, the ALPHA group outermost or innermost (`where`), ERASE and the nine in turn at the
    other levels; every level's first path arrives in another strip, so strips see the levels set aside together and one by one"""
    rng = np.random.default_rng(seed + 10 * depth)
    fr = AlphaRawFrame(W, H)
    _ground(fr, rng)
    modes = [("erase", "multiply", "normal", "screen")[k % 4] for k in range(depth)]
    modes[0 if where == "outer" else depth - 1] = "alpha"
    for k in range(depth):
        fr.begin()
        add_member(fr, rng, ("partial", "box", "full_translucent", "partial")[k], "normal", 64 * (k % 2), 8 * (k % 4), first=True)
    add_member(fr, rng, "partial", "normal", 0, 0)
    add_member(fr, rng, "box", "erase", 64, 24)
    for k in reversed(range(depth)):
        fr.end(modes[k], 255 if k % 2 else 180)
        add_member(fr, rng, "partial", ALL_MODES[(k + seed) % 10], 64 * ((k + 1) % 2), 8 * ((k + 2) % 4))
    return fr


def rand_frame(rng, w=W, h=H, items=40):
    """random nesting of plain, faded and masked groups closed by the eleven operators, members under the ten, scattered over the strips"""
    fr = AlphaRawFrame(w, h)
    painted = [False]
    will_mask = []
    n = 0

    def member():
        x, y = float(rng.uniform(-5, w)), float(rng.uniform(-5, h))
        op = ALL_MODES[int(rng.integers(0, 10))] if rng.integers(0, 2) else "normal"
        add_member(fr, rng, cs.MEMBER_CLASSES[int(rng.integers(0, 6))], op, (int(x) // 64) * 64 if x >= 0 else 0, (int(max(y, 0)) // 8) * 8, first=not painted[-1])
        painted[-1] = True

    while n < items or fr.depth:
        r = 0.95 if n >= items else float(rng.random())
        if r < 0.5 or (r >= 0.78 and not fr.depth):
            member()
            n += 1
        elif r < 0.78:
            masked = rng.integers(0, 3) == 0
            if fr.levels + sum(will_mask) + (2 if masked else 1) <= 4:
                fr.begin()
                will_mask.append(bool(masked))
                painted.append(False)
                n += 1
        elif will_mask[-1]:
            fr.mask()
            will_mask[-1] = False
            painted[-1] = False
            n += 1
        else:
            plain = fr.masks[-1] is not None or rng.integers(0, 3) == 0
            fr.end(END_MODES[int(rng.integers(0, 11))] if rng.integers(0, 3) else ("alpha", "erase")[int(rng.integers(0, 2))],
                   255 if plain else int(rng.choice([0, 1, 127, 254, int(rng.integers(2, 254))])))
            will_mask.pop()
            painted.pop()
            painted[-1] = True
    return fr


def strip_alpha_reach(width, height, paths, styles=None):
    """What the walk of each strip meets of the two operators, from the arrays alone (by path rectangle).  Returns a dict:
    ends          {(operator, "plain" | "faded" | "masked", what reached the strip)}: for every ERASE / ALPHA END in every strip it reaches;
                  what reached: for a plain or faded group whether a path of it did (True / False), for a masked group the pair
                  (content reached, mask reached)
    cleared       the strips (row, column) in which an ALPHA END found its group never set aside, while the surface below held a path
    cut           whether some ALPHA END's rectangle ends inside a strip it reaches, in x and in y
    fades         the fades (255 - opacity) of the ALPHA ENDs
    end_pos       {(operator, position in the strip's list)} of those ENDs;  path_pos: the positions of ERASE paths
    band_pos      the same positions in the tile row's list (where the class bytes of a strip are indexed)
    erase_kinds   {(path kind, whether some row of the strip lies outside the path's rectangle)} of the ERASE paths
    depths        {(depth of the group, deepest nesting inside it)} of the ALPHA ENDs
    behind_cover  {"below", "above"}: an ERASE path before, and one behind, an opaque lerp path that covers its whole strip (`styles` given)"""
    bands = cs.band_positions(height, paths)
    out = dict(ends=set(), cleared=set(), cut=False, fades=set(), end_pos=set(), path_pos=set(), band_pos=set(), erase_kinds=set(), depths=set(),
               behind_cover=set())
    for (sy, sx), lst in cs.strip_lists(width, height, paths).items():
        band = bands[sy * STRIP_H // cs.TILE_H]
        groups = []                                                  # [content reached, mask reached or None, deepest nesting inside]
        surface = [False]                                            # per open surface: has a path reached the strip
        cover_seen = False
        for pos, i in enumerate(lst):
            p = paths[i]
            kind, op = int(p["kind"]), op_of(p)
            if kind == BEGIN:
                groups.append([False, None, 0])
                surface.append(False)
                for d, g in enumerate(groups[:-1]):
                    g[2] = max(g[2], len(groups) - 1 - d)
            elif kind == MASK:
                groups[-1][1] = False
                surface[-1] = False
            elif kind == END:
                g = groups.pop()
                surface.pop()
                if op in (am.OP_ERASE, am.OP_ALPHA):
                    fade = (int(p["lerp"]) & 0xffffffff) >> 24
                    form = "masked" if g[1] is not None else ("faded" if fade else "plain")
                    reached = (g[0], g[1]) if g[1] is not None else g[0]
                    out["ends"].add((op, form, reached))
                    out["end_pos"].add((op, pos))
                    out["band_pos"].add((op, band[i]))
                    if op == am.OP_ALPHA:
                        out["fades"].add(fade)
                        out["depths"].add((len(groups) + 1, g[2]))
                        if not g[0] and not g[1] and surface[-1]:
                            out["cleared"].add((sy, sx))
                        if int(p["x_max"]) % STRIP_W and int(p["x_max"]) < width and int(p["y_max"]) % STRIP_H and int(p["y_max"]) < height \
                                and int(p["x_min"]) % STRIP_W and int(p["y_min"]) % STRIP_H:
                            out["cut"] = True
                surface[-1] = surface[-1] or g[0] or bool(g[1])
            else:
                for g in groups:
                    if g[1] is None:
                        g[0] = True
                    else:
                        g[1] = True
                surface[-1] = True
                y0, y1 = sy * STRIP_H, min((sy + 1) * STRIP_H, height)
                if op == am.OP_ERASE:
                    out["path_pos"].add(pos)
                    out["band_pos"].add((op, band[i]))
                    out["erase_kinds"].add((kind, int(p["y_min"]) > y0 or int(p["y_max"]) < y1))
                    if not groups:
                        out["behind_cover"].add("above" if cover_seen else "below")
                elif not groups and styles is not None and (int(p["lerp"]) & 1) and (int(styles[int(p["style"])].pixel) & 0xffffffff) >> 24 == 255 and int(p["x_min"]) <= sx * STRIP_W and int(p["x_max"]) >= min((sx + 1) * STRIP_W, width) \
                        and int(p["y_min"]) <= y0 and int(p["y_max"]) >= y1:
                    cover_seen = True
    return out
