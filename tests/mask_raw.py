"""Raw frames with masked groups for the mask instance of the tile kernel, checked against tests/frame_model.py: frames
written directly as swfr_upload_edges arrays (composite_scenes.RawFrame with MASK markers), aimed at the walk of k2_tiles<5> over one
strip's list -- the four reach cases of a strip (content reaches it or not, mask reaches it or not), MASK and the masked END on either
side of the staging rounds (16 entries), the class-byte chunks (64) and the prefetched class bytes (128), halves of 15 .. 65 members,
nesting, all nine operators, groups across tile rows -- and strip_mask_reach, what a frame's strips see, from the arrays alone."""
import numpy as np

import composite_scenes as cs
import mask_model as mk
from composite_scenes import BEGIN, END, MODES, STRIP_H, STRIP_W, add_member, premultiplied

MASK = mk.PATH_GROUP_MASK


def masked_sizes_frame(rng, n_content, n_mask, n_before, n_after=3, W=70, H=13, end_op=None):
    """`n_before` plain entries, ONE masked group of `n_content` content and `n_mask` mask members, `n_after` plain entries, every one
    reaching the strip in the frame's top left corner: BEGIN sits at list position n_before, MASK at n_before + n_content + 1, END at
    n_before + n_content + n_mask + 2"""
    fr = cs.RawFrame(W, H)
    c0, o0 = int(rng.integers(0, 6)), int(rng.integers(0, 9))
    for i in range(n_before):
        add_member(fr, rng, ("full_translucent", "box", "partial")[i % 3], MODES[(o0 + i) % 9] if i else "normal", 0, 0, first=i == 0)
    fr.begin()
    for i in range(n_content):
        add_member(fr, rng, cs.MEMBER_CLASSES[(c0 + i) % 6], MODES[(o0 + i) % 9], 0, 0, first=i == 0)
    fr.mask()
    for i in range(n_mask):
        add_member(fr, rng, ("partial", "full_translucent", "box", "full_lerp", "partial", "full_opaque")[(c0 + i) % 6], MODES[(o0 + 2 * i) % 9], 0, 0, first=i == 0)
    fr.end(end_op or MODES[(o0 + n_content + n_mask) % 9])
    for i in range(n_after):
        add_member(fr, rng, ("partial", "full_translucent", "box")[i % 3], MODES[(o0 + 2 * i) % 9], 0, 0)
    return fr


def reach_cases_frame(op="normal", W=256, H=16, seed=0):
    """One masked group over a translucent ground and a plain path, over 4 x 2 strips: content and mask both reach tile column 0, the
    content alone column 1, the mask alone column 2, neither column 3 (which the group reaches by its rectangle alone: a member of each
    half lies in column 3 of the OTHER strip row).  Plain paths before and after in every strip."""
    rng = np.random.default_rng(seed)
    fr = cs.RawFrame(W, H)
    fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, 150), 1)
    fr.tor([(2, 1), (250, 3), (120, 15)], premultiplied(rng, 90))
    t = lambda: premultiplied(rng, int(rng.integers(60, 250)))      # (members kept inside their own tile column and strip row)
    fr.begin()
    fr.tor([(5, 1), (50, 2), (20, 7)], t(), 1)
    fr.box(10.5, 2.25, 40, 6.5, t(), 0, "multiply")
    fr.tor([(70, 1), (120, 3), (90, 7.5)], t(), 0, "screen")
    fr.box(80, 2, 100, 6, t())
    fr.box(200, 9, 240, 15, t())
    fr.mask()
    fr.tor([(2, 0.5), (60, 4), (10, 7.8)], t(), 1)
    fr.box(20, 1, 55, 5.5, t())
    fr.rect_tor(130, 1, 190, 7, t())
    fr.tor([(135, 2), (180, 3), (150, 7)], t(), 0, "add")
    fr.tor([(195, 9), (250, 10), (220, 15.5)], t())
    fr.end(op)
    fr.tor([(5, 14), (200, 2), (254, 12)], premultiplied(rng, 120), 0, "overlay")
    return fr


def nested_masks_frame(which, W=200, H=45, seed=0):
    """which = "four_by_one_path": masked inside masked (in the mask half), the only path to reach strip column 0 before the inner
    mask's first path IS that path: four levels set aside by one path there, while column 2 sees every level arrive on its own.
    which = "outer_survives": a plain group whose pixels are set aside in column 0, inside it a masked group whose content never reaches
    column 0 while its mask does: the outer group's pixels must survive the mask step untouched.
    which = "in_content": masked inside the content half of a masked group, both reaching every column."""
    rng = np.random.default_rng(seed + len(which))
    fr = cs.RawFrame(W, H)
    add_member(fr, rng, "partial", "normal", 0, 0, first=True)
    fr.rect_tor(0, 2, W, 5, premultiplied(rng, 120))
    if which == "four_by_one_path":
        fr.begin()
        add_member(fr, rng, "partial", "normal", 128, 16, first=True)
        fr.mask()
        add_member(fr, rng, "box", "normal", 128, 16, first=True)
        fr.begin()
        add_member(fr, rng, "partial", "normal", 128, 16, first=True)
        fr.mask()
        add_member(fr, rng, "partial", "normal", 0, 0, first=True)       # the first path of strip (0, 0) since the outermost BEGIN
        add_member(fr, rng, "full_translucent", "normal", 128, 16)
        fr.end("screen")
        add_member(fr, rng, "partial", "multiply", 0, 0)
        fr.end("hardlight")
    elif which == "outer_survives":
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
        fr.end("multiply")
    else:
        fr.begin()
        add_member(fr, rng, "partial", "normal", 0, 0, first=True)
        fr.begin()
        for x, y in ((0, 0), (64, 8), (128, 16)):
            add_member(fr, rng, "partial", "normal", x, y, first=x == 0)
        fr.mask()
        for x, y in ((0, 0), (64, 8), (128, 16)):
            add_member(fr, rng, "full_translucent", "normal", x, y, first=x == 0)
        fr.end("overlay")
        add_member(fr, rng, "box", "screen", 0, 0)
        fr.mask()
        fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, 170), 1)
        fr.end("darken")
    add_member(fr, rng, "partial", "overlay", 0, 0)
    return fr


def rand_raw_masked_frame(rng, W=200, H=45, items=60):
    """composite_scenes.rand_raw_nested_frame with masks: random nesting of plain and masked groups up to the four levels, small
    members scattered over several tile rows and columns, so that every strip takes its own branch of the reach cases"""
    fr = cs.RawFrame(W, H)
    painted = [False]

    def member():
        x, y = float(rng.uniform(-5, W)), float(rng.uniform(-5, H))
        op = MODES[int(rng.integers(0, 9))] if rng.integers(0, 2) else "normal"
        first = not painted[-1]
        r = float(rng.random())
        if r < 0.4:
            add_member(fr, rng, cs.MEMBER_CLASSES[int(rng.integers(0, 4))], op, (int(x) // 64) * 64 if x >= 0 else 0, (int(max(y, 0)) // 8) * 8, first=first)
        else:
            lerp = 1 if first and op in ("normal", "add") else 0
            s = float(rng.uniform(3, 40))
            if r < 0.65:
                fr.box(x, y, x + s, y + float(rng.uniform(1, 20)), premultiplied(rng), lerp, "normal" if lerp else op)
            else:
                pts = [(x + float(rng.uniform(0, s)), y + float(rng.uniform(0, s * 0.6))) for _ in range(int(rng.integers(3, 6)))]
                fr.tor(pts, premultiplied(rng), lerp, "normal" if lerp else op, even_odd=bool(rng.integers(0, 2)))
        painted[-1] = True

    n = 0
    will_mask = []                                                   # per open group: it is a masked one whose MASK is still to come
    while n < items or fr.depth:
        r = float(rng.random())
        if n >= items:
            r = 0.95
        if r < 0.5:
            member()
            n += 1
        elif r < 0.78:
            masked = bool(rng.integers(0, 2))
            # (a masked group's two levels count from its BEGIN on, also before its MASK)
            if fr.levels + sum(will_mask) + (2 if masked else 1) <= mk.MAX_DEPTH:
                fr.begin()
                will_mask.append(masked)
                painted.append(False)
                n += 1
        elif fr.depth:
            if will_mask[-1]:
                fr.mask()
                will_mask[-1] = False
                painted[-1] = False
                n += 1
            else:
                fr.end(MODES[int(rng.integers(0, 9))])
                will_mask.pop()
                painted.pop()
                painted[-1] = True
        else:
            member()
            n += 1
    return fr


def many_masked_groups_frame(rng, W=512, H=256, groups=1000):
    """a thousand small masked groups of one to three members a half, now and then one inside another, plain paths between them"""
    fr = cs.RawFrame(W, H)
    fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, 200), 1)

    def half(x, y):
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
        half(x, y)
        if g % 7 == 0:
            fr.begin()
            fr.box(x + 1, y + 2, x + 9.5, y + 7.25, premultiplied(rng), 1)
            fr.mask()
            fr.box(x + 2, y + 1, x + 8.5, y + 9.25, premultiplied(rng), 1)
            fr.end(MODES[int(rng.integers(0, 9))])
        fr.mask()
        half(x + float(rng.uniform(-3, 3)), y + float(rng.uniform(-3, 3)))
        fr.end(MODES[g % 9])
        if g % 5 == 0:
            fr.tor([(x + float(rng.uniform(0, 30)), y + float(rng.uniform(0, 30))) for _ in range(3)], premultiplied(rng), 0, MODES[int(rng.integers(0, 9))])
    return fr


def strip_mask_reach(width, height, paths):
    """What the walk of each strip meets of masked groups, from the arrays alone (by path rectangle).  Returns a dict:
    cases         the set of (content reached the strip, mask reached the strip) over all masked groups and strips their markers reach
    markers       [(kind, position in the strip's list, position in its tile row's list)] of every MASK and every masked END
    together      the most levels (a MASK opens one) whose first path in a strip was one and the same path
    outer_kept    whether some strip saw a masked group whose content did not reach it while its mask did, inside a group that had"""
    bands = cs.band_positions(height, paths)
    cases, markers, together, outer_kept = set(), [], 0, False
    for (sy, sx), lst in cs.strip_lists(width, height, paths).items():
        band = bands[sy * STRIP_H // cs.TILE_H]
        groups = []                                                  # open groups: [content reached, mask reached or None before MASK]
        levels = []                                                  # per open level (BEGIN or MASK): a path has arrived since
        for pos, i in enumerate(lst):
            kind = int(paths[i]["kind"])
            if kind == BEGIN:
                groups.append([False, None])
                levels.append(False)
            elif kind == MASK:
                markers.append((MASK, pos, band[i]))
                groups[-1][1] = False
                levels.append(False)
            elif kind == END:
                g = groups.pop()
                levels.pop()
                if g[1] is not None:
                    levels.pop()
                    markers.append((END, pos, band[i]))
                    cases.add((g[0], g[1]))
                    if not g[0] and g[1] and groups and (groups[-1][0] if groups[-1][1] is None else groups[-1][1]):
                        outer_kept = True
            elif groups:
                together = max(together, levels.count(False))
                levels[:] = [True] * len(levels)
                for g in groups:                                     # (a path inside a nested group arrives in the half of every group around it)
                    if g[1] is None:
                        g[0] = True
                    else:
                        g[1] = True
    return dict(cases=cases, markers=markers, together=together, outer_kept=outer_kept)
