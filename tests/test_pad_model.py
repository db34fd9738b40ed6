"""tests/pad_model.py -- the source pixel of a padded bitmap fill, bilinear and separable convolution -- against live libcairo
(no GPU): random pixel-aligned boxes on a still-clear surface, so that the frame holds the source samples themselves.  Zero differing
bytes.  The same boxes go to the device in tests/test_pad_gpu.py, held against the model there."""
import numpy as np
import pytest

import pad_model as pm
import pad_scenes as ps
from oracle import cairo_backend as cb

pytestmark = pytest.mark.skipif(not cb.available(), reason="needs the system libcairo")

CASES = 2400            # per filter: half of them


def expected(case, extend=pm.PAD):
    """the frame of a random_box_case by the model"""
    md = case["model"]
    out = np.zeros((ps.FH, ps.FW, 4), np.uint8)
    src = pm.source(md["matrices"], pm.premultiply(md["bitmap"]), md["rect"], extend)
    if src is not None:
        x0, y0, x1, y1 = md["rect"]
        out[y0:y1, x0:x1] = pm.rgba_bytes(src["pixels"])
    return out, src


def _kind(places):
    return "inside" if places["rim"] == places["outside"] == 0 else ("outside" if places["rim"] == places["inside"] == 0 else "rim")


def test_the_model_is_libcairo_on_random_boxes():
    rng = np.random.default_rng(20261019)
    seen = {(f, k): 0 for f in ("bilinear", "convolution") for k in ps.PLACES}
    bad = 0
    for it in range(CASES):
        case = ps.random_box_case(rng, minified=bool(it & 1))
        want, src = expected(case)
        assert src is not None
        seen["bilinear" if src["bilinear"] else "convolution", _kind(src["placements"])] += 1
        got = ps.cairo_render(case["scene"])
        n = int((got != want).sum())
        if n:
            bad += 1
            print("case", it, case["aim"], case["model"]["matrices"], case["model"]["rect"], case["model"]["bitmap"].shape, "differing bytes", n)
    print("placements", seen)
    assert bad == 0, "%d of %d boxes differ from libcairo" % (bad, CASES)
    assert all(n >= 200 for n in seen.values()), seen


@pytest.mark.parametrize("extend", [pm.NONE, pm.REPEAT])
def test_the_model_knows_the_other_two_rules(extend):
    """the same model with the taps of EXTEND_NONE and EXTEND_REPEAT is libcairo too: what it says of PAD is the clamp alone.
    (Under EXTEND_NONE the operation is cut to the bitmap's rectangle; only pixels inside the cut are compared.)"""
    rng = np.random.default_rng(77 + extend)
    name = {pm.NONE: "none", pm.REPEAT: "repeat"}[extend]
    for it in range(300):
        case = ps.random_box_case(rng, minified=bool(it & 1))
        want, _ = expected(case, extend)
        got = ps.cairo_render(dict(case["scene"], stage=ps.with_extend(case["scene"]["stage"], name)))
        where = got.any(-1) if extend == pm.NONE else np.ones(got.shape[:2], bool)
        assert (got[where] == want[where]).all(), (it, case["aim"], case["model"]["matrices"], case["model"]["rect"])
