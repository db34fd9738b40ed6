"""Raw frames with faded groups for the instance of the tile kernel that fades, checked against tests/frame_model.py: frames
written directly as swfr_upload_edges arrays (composite_scenes.RawFrame with faded ENDs), aimed at the walk of k2_tiles<6>
over one strip's list -- a faded END in a strip its group reached and in one it reached by its rectangle alone, the faded END on
either side of the staging rounds (16 entries), the class-byte chunks (64) and the prefetched class bytes (128), four nested faded
groups set aside by one path, a faded group around a masked one whose content misses the strip, the opacities at both ends of the
range, a thousand small faded groups -- and strip_fade_reach, what a frame's strips see, from the arrays alone."""
import numpy as np

import composite_scenes as cs
import mask_raw as mr
from composite_scenes import BEGIN, END, MODES, STRIP_H, add_member, premultiplied

MASK = mr.MASK


def fade_of(path):
    return (int(path["lerp"]) & 0xffffffff) >> 24


def reach_cases_frame(op="normal", opacity=128, W=256, H=16, seed=0):
    """One faded group over a translucent ground and a plain path, over 4 x 2 strips: its members reach tile columns 0 and 2 of the upper
    strip row and column 3 of the lower one; every other strip the group reaches by its rectangle alone -- there the faded END finds
    the parent's pixels in place and must leave them alone.  Plain paths before and after in every strip."""
    rng = np.random.default_rng(seed)
    fr = cs.RawFrame(W, H)
    fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, 150), 1)
    fr.tor([(2, 1), (250, 3), (120, 15)], premultiplied(rng, 90))
    t = lambda: premultiplied(rng, int(rng.integers(60, 250)))      # (members kept inside their own tile column and strip row)
    fr.begin()
    fr.tor([(5, 1), (50, 2), (20, 7)], t(), 1)
    fr.box(10.5, 2.25, 40, 6.5, t(), 0, "multiply")
    fr.rect_tor(130, 1, 190, 7, t())
    fr.tor([(135, 2), (180, 3), (150, 7)], t(), 0, "add")
    fr.box(200, 9, 240, 15, t())
    fr.end(op, opacity)
    fr.tor([(5, 14), (200, 2), (254, 12)], premultiplied(rng, 120), 0, "overlay")
    return fr


def fade_sizes_frame(rng, n_members, n_before, n_after=3, W=70, H=13, end_op=None, opacity=None):
    """composite_scenes.raw_group_sizes_frame with a faded END: `n_before` plain entries, ONE faded group of `n_members` members,
    `n_after` plain entries, every one reaching the strip in the frame's top left corner: BEGIN sits at list position n_before, the
    faded END at n_before + n_members + 1"""
    fr = cs.RawFrame(W, H)
    c0, o0 = int(rng.integers(0, 6)), int(rng.integers(0, 9))
    for i in range(n_before):
        add_member(fr, rng, ("full_translucent", "box", "partial")[i % 3], MODES[(o0 + i) % 9] if i else "normal", 0, 0, first=i == 0)
    fr.begin()
    for i in range(n_members):
        add_member(fr, rng, cs.MEMBER_CLASSES[(c0 + i) % 6], MODES[(o0 + i) % 9], 0, 0, first=i == 0)
    fr.end(end_op or MODES[(o0 + n_members) % 9], int(rng.integers(1, 255)) if opacity is None else opacity)
    for i in range(n_after):
        add_member(fr, rng, ("partial", "full_translucent", "box")[i % 3], MODES[(o0 + 2 * i) % 9], 0, 0)
    return fr


def nested_fades_frame(which, W=200, H=45, seed=0):
    """which = "four_by_one_path": four faded groups nested, the only path to reach strip column 0 since the outermost BEGIN is the
    innermost group's: four levels set aside by one path there and four fades applied on the way out, while column 2 sees every level
    arrive on its own.
    which = "around_masked_missing": a faded group in whose strip (0, 0) a path has arrived, around a masked group whose content never
    reaches that strip while its mask does: the mask step drops the product, the faded END fades what the outer group holds.
    which = "around_masked_alone": a faded group whose only member is a masked group whose content misses strip (0, 0): the faded END
    there meets pixels the mask step has just cleared, set aside by the mask's path alone."""
    rng = np.random.default_rng(seed + len(which))
    fr = cs.RawFrame(W, H)
    add_member(fr, rng, "partial", "normal", 0, 0, first=True)
    fr.rect_tor(0, 2, W, 5, premultiplied(rng, 120))
    if which == "four_by_one_path":
        for k in range(3):
            fr.begin()
            add_member(fr, rng, ("partial", "box", "full_translucent")[k], "normal", 128, 16, first=True)
        fr.begin()
        add_member(fr, rng, "partial", "normal", 0, 0, first=True)       # the first path of strip (0, 0) since the outermost BEGIN
        add_member(fr, rng, "full_translucent", "normal", 128, 16)
        fr.end("screen", 200)
        add_member(fr, rng, "partial", "multiply", 0, 0)
        fr.end("hardlight", 90)
        fr.end("add", 254)
        fr.end("normal", 1)
    elif which == "around_masked_missing":
        fr.begin()
        add_member(fr, rng, "full_translucent", "normal", 0, 0, first=True)
        add_member(fr, rng, "partial", "normal", 0, 0)
        fr.begin()
        add_member(fr, rng, "partial", "normal", 128, 16, first=True)   # the content: elsewhere
        fr.mask()
        add_member(fr, rng, "partial", "normal", 0, 0, first=True)
        add_member(fr, rng, "box", "normal", 128, 16)
        fr.end("add")
        add_member(fr, rng, "box", "difference", 0, 0)
        fr.end("multiply", 140)
    else:
        fr.begin()
        fr.begin()
        fr.rect_tor(70, 9.5, 190.25, 30, premultiplied(rng, 180), 1)    # the content: right of tile column 0, below strip row 0
        fr.mask()
        add_member(fr, rng, "partial", "normal", 0, 0, first=True)
        fr.rect_tor(60, 10, 180, 28.5, premultiplied(rng, 200))
        fr.end("normal")
        fr.end("screen", 77)
    add_member(fr, rng, "partial", "overlay", 0, 0)
    return fr


def rand_raw_faded_frame(rng, W=200, H=45, items=60):
    """mask_raw.rand_raw_masked_frame's walk with fades: random nesting of plain, faded and masked groups up to the four levels, small
    members scattered over several tile rows and columns"""
    fr = cs.RawFrame(W, H)
    painted = [False]

    def member():
        x, y = float(rng.uniform(-5, W)), float(rng.uniform(-5, H))
        op = MODES[int(rng.integers(0, 9))] if rng.integers(0, 2) else "normal"
        first = not painted[-1]
        if rng.random() < 0.5:
            add_member(fr, rng, cs.MEMBER_CLASSES[int(rng.integers(0, 4))], op, (int(x) // 64) * 64 if x >= 0 else 0, (int(max(y, 0)) // 8) * 8, first=first)
        else:
            lerp = 1 if first and op in ("normal", "add") else 0
            s = float(rng.uniform(3, 40))
            pts = [(x + float(rng.uniform(0, s)), y + float(rng.uniform(0, s * 0.6))) for _ in range(int(rng.integers(3, 6)))]
            fr.tor(pts, premultiplied(rng), lerp, "normal" if lerp else op, even_odd=bool(rng.integers(0, 2)))
        painted[-1] = True

    n = 0
    will_mask = []
    while n < items or fr.depth:
        r = float(rng.random())
        if n >= items:
            r = 0.95
        if r < 0.5:
            member()
            n += 1
        elif r < 0.78:
            masked = rng.integers(0, 3) == 0
            if fr.levels + sum(will_mask) + (2 if masked else 1) <= mr.mk.MAX_DEPTH:
                fr.begin()
                will_mask.append(bool(masked))
                painted.append(False)
                n += 1
        elif fr.depth:
            if will_mask[-1]:
                fr.mask()
                will_mask[-1] = False
                painted[-1] = False
                n += 1
            else:
                plain = fr.masks[-1] is not None or rng.integers(0, 4) == 0        # (a masked group takes no fade)
                fr.end(MODES[int(rng.integers(0, 9))], 255 if plain else int(rng.choice([0, 1, 254, int(rng.integers(2, 254)), int(rng.integers(2, 254))])))
                will_mask.pop()
                painted.pop()
                painted[-1] = True
        else:
            member()
            n += 1
    return fr


def many_faded_groups_frame(rng, W=512, H=256, groups=1000):
    """a thousand small faded groups of one to three members, now and then one inside another, plain paths between them"""
    fr = cs.RawFrame(W, H)
    fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, 200), 1)

    def members(x, y):
        for i in range(int(rng.integers(1, 4))):
            op = MODES[int(rng.integers(0, 9))]
            lerp = 1 if i == 0 and op in ("normal", "add") else 0
            if rng.integers(0, 3):
                fr.tor([(x + float(rng.uniform(0, 12)), y + float(rng.uniform(0, 12))) for _ in range(3)], premultiplied(rng), lerp, "normal" if lerp else op)
            else:
                fr.box(x, y, x + float(rng.uniform(1, 14)), y + float(rng.uniform(1, 14)), premultiplied(rng), lerp, "normal" if lerp else op)

    for g in range(groups):
        x, y = float(rng.uniform(-4, W - 4)), float(rng.uniform(-4, H - 4))
        fr.begin()
        members(x, y)
        if g % 7 == 0:
            fr.begin()
            fr.box(x + 1, y + 2, x + 9.5, y + 7.25, premultiplied(rng), 1)
            fr.end(MODES[int(rng.integers(0, 9))], int(rng.integers(0, 256)))
        fr.end(MODES[g % 9], 1 + (g * 37) % 254)
        if g % 5 == 0:
            fr.tor([(x + float(rng.uniform(0, 30)), y + float(rng.uniform(0, 30))) for _ in range(3)], premultiplied(rng), 0, MODES[int(rng.integers(0, 9))])
    return fr


def strip_fade_reach(width, height, paths):
    """What the walk of each strip meets of faded groups, from the arrays alone (by path rectangle).  Returns a dict:
    cases         the set of "a path of the group (or of a group inside it) reached the strip" over all faded ENDs and strips they reach
    markers       [(position in the strip's list, position in its tile row's list)] of every faded END
    together      the most faded groups whose first path in a strip was one and the same path
    after_dropped whether some strip saw a faded END right behind the END of a masked group whose content had not reached the strip
                  while its mask had"""
    bands = cs.band_positions(height, paths)
    cases, markers, together, after_dropped = set(), [], 0, False
    closes = {}                                                      # END index -> its BEGIN's
    opened = []
    for i, p in enumerate(paths):
        if int(p["kind"]) == BEGIN:
            opened.append(i)
        elif int(p["kind"]) == END:
            closes[i] = opened.pop()
    for (sy, sx), lst in cs.strip_lists(width, height, paths).items():
        band = bands[sy * STRIP_H // cs.TILE_H]
        groups = []                                                  # open groups: [BEGIN index, content reached, mask reached or None, first path]
        dropped_at = None
        for pos, i in enumerate(lst):
            kind = int(paths[i]["kind"])
            if kind == BEGIN:
                groups.append([i, False, None, None])
            elif kind == MASK:
                groups[-1][2] = False
            elif kind == END:
                g = groups.pop()
                if fade_of(paths[i]):
                    markers.append((pos, band[i]))
                    cases.add(g[1])
                    if dropped_at == pos - 1:
                        after_dropped = True
                if g[2] is not None and not g[1] and g[2]:
                    dropped_at = pos
            elif groups:
                fresh = [g for g in groups if g[3] is None]
                together = max(together, sum(1 for g in fresh if fade_of(paths[[e for e, b in closes.items() if b == g[0]][0]])))
                for g in groups:
                    if g[3] is None:
                        g[3] = i
                    if g[2] is None:
                        g[1] = True
                    else:
                        g[2] = True
    return dict(cases=cases, markers=markers, together=together, after_dropped=after_dropped)
