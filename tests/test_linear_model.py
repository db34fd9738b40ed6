"""tests/linear_model.py -- pixman's linear gradient and libcairo's pieces in Python integers and floats -- against live libcairo
(skipped where libcairo is absent) and against the committed libcairo goldens of the single-shape scenes.  No GPU, no kernel.

Inside the documented range (linear_model.accepted) the model is libcairo byte for byte, bar the frames where the 8-bit coverage does
not show where a row's first span begins (linear_model.py: a first pixel whose area rounds to coverage 0): those are counted, the count
is asserted, and each must differ in the rows of such a pixel only."""
import numpy as np
import pytest

import linear_fuzz as lf
import linear_model as lm
import linear_scenes as ls
import spread_model as sm
import spread_scenes as ss

FRAMES = 110                                     # per spread and frame size: 660 random gradients, a third per extend
# frames (of 220 a spread) that differ from libcairo because a row's first span is invisible in the 8-bit coverage
HIDDEN_FIRST_SPAN = {"pad": {((96, 48), 13): [30]}, "reflect": {((96, 48), 17): [5], ((96, 48), 33): [44], ((96, 48), 73): [22]}, "repeat": {}}
STATE_COLUMNS = {"box_exact_r25_coincident": [75, 105], "box_exact_r32_coincident": [15, 115]}     # (other strips than the rectangle's first)
HIDDEN_IN_GOLDENS = {"pad": ["notched"], "reflect": ["notched"], "repeat": ["notched"]}       # the single-shape golden scenes with such a row


@pytest.mark.parametrize("spread", ls.SPREADS)
def test_model_is_libcairo_on_random_frames(spread):
    from oracle import cairo_backend as cb
    if not cb.available():
        pytest.skip("libcairo not available")
    done = caveat = one_piece_differs = 0
    differing = {}
    seen = {}
    for size in lf.SIZES:
        for case in lf.cases(spread, size, FRAMES):
            want = ss.cairo_render(case["scene"])
            alpha = ss.cairo_render(case["white"])[..., 3]
            e = lf.expected(case, alpha)
            msg = (spread, size, case["index"], case["shape"], case["kind"])
            assert (lf.coverage(case) == alpha).all(), msg
            d = (e["truth"] != want).any(-1)
            if d.any():
                rows = sorted(set(np.nonzero(d)[0].tolist()))
                differing[tuple(size), case["index"]] = rows
                print("linear model differs from libcairo:", msg, int(d.sum()), "pixels in rows", rows)
                md = case["model"]
                again = lm.frame(sm.pattern_matrix(md["matrices"]), lf.LINE, md["stops"], lf.EXTEND[spread], md["rect"], alpha, hidden_rows=rows)
                assert not case["whole_box"] and (again["truth"] == want).all(), msg     # ... for that reason alone
            one_piece_differs += bool((e["one_piece"] != want).any())
            caveat += int(e["caveat"].sum())
            seen[case["shape"], case["kind"]] = seen.get((case["shape"], case["kind"]), 0) + 1
            done += 1
    print("linear model,", spread, ":", done, "frames,", len(differing), "differ from libcairo,", one_piece_differs,
          "would differ with the rectangle as one piece,", caveat, "caveat pixels (a walker that sees every sample of a piece)")
    assert done == 2 * FRAMES and len(seen) == len(lf.SHAPES) * len(lf.KINDS)
    assert differing == HIDDEN_FIRST_SPAN[spread]
    assert one_piece_differs > 0, "the random frames no longer tell libcairo's pieces from the whole rectangle"


@pytest.mark.parametrize("spread", ls.SPREADS)
def test_model_paints_the_single_shape_goldens(spread):
    """the committed goldens of the one-shape scenes on a clear frame (no libcairo needed): polygons through the span renderer's pieces
    -- the 600-pixel ones with rows cut at runs of 256 full pixels --, boxes on whole pixels as one piece"""
    gold = np.load(ls.golden_path("cairo_linear_%s_plain" % spread))
    from helpers import oracle_render
    n, hidden = 0, []
    for name, sc in sorted(ls.plain_scenes(spread).items()):
        kids = sc["stage"]["children"]
        if len(kids) != 1 or name in ("config_fill",):
            continue
        f = kids[0]["definition"]["shape"]["initial_styles"]["fill"][0]
        white = dict(sc, stage={"children": [dict(kids[0], definition=dict(kids[0]["definition"], shape=dict(
            kids[0]["definition"]["shape"], initial_styles={"fill": [{"type": "solid", "color": {"r": 255, "g": 255, "b": 255, "a": 255}}], "line": []})))]})
        alpha = oracle_render(white)[..., 3]
        ys, xs = np.nonzero(alpha)
        b = kids[0]["definition"]["bounds"]
        rect = (max(b["x_min"] // 20, 0), max(b["y_min"] // 20, 0), min(-(-b["x_max"] // 20), sc["width"]), min(-(-b["y_max"] // 20), sc["height"]))
        stops = [(c["ratio"] / 255, c["color"]["r"] / 255, c["color"]["g"] / 255, c["color"]["b"] / 255, c["color"]["a"] / 255) for c in f["gradient"]["colors"]]
        m = sm.pattern_matrix([f["matrix"]])
        assert lm.accepted(m, lf.LINE, rect), name
        whole = name.startswith("box_") and name != "box_off_grid"
        e = lm.frame(m, lf.LINE, stops, lf.EXTEND[spread], rect, alpha, boxes=[rect] if whole else None)
        if name.startswith("box_exact_"):                            # the aimed boxes: the walker's state decides pixels under reflect, only there
            state = lm.state_pixels(m, lf.LINE, stops, lf.EXTEND[spread], rect)
            cols = sorted(set((np.nonzero(state)[1] + rect[0]).tolist()))
            print("linear model,", spread, name, "columns where the walker's state decides:", cols, int(state.sum()), "pixels")
            assert cols == (STATE_COLUMNS[name] if spread == "reflect" else []) and state.sum() == len(cols) * state.shape[0]
        d = (e["truth"] != gold[name]).any(-1)
        if d.any():                                                  # (a row whose first span the 8-bit coverage hides: linear_model.py)
            rows = sorted(set(np.nonzero(d)[0].tolist()))
            print("linear model differs from the golden:", spread, name, int(d.sum()), "pixels in rows", rows)
            e = lm.frame(m, lf.LINE, stops, lf.EXTEND[spread], rect, alpha, hidden_rows=rows)
            assert not whole and (e["truth"] == gold[name]).all(), (spread, name)
            hidden.append(name)
        n += 1
    assert n >= 16 and hidden == HIDDEN_IN_GOLDENS[spread]
