"""Random one-shape frames of pixman-exact linear gradients on the device against tests/linear_model.py (tests/linear_fuzz.py: the cases
tests/test_linear_model.py holds against live libcairo): 204 frames of 48 x 12 and 96 x 48, a third per extend, boxes, quadrilaterals,
convex and notched polygons under horizontal, vertical, steep, rotated and sheared matrices.

Zero differing bytes off the model's caveat pixels; on those the device equals the every-sample rule (a walker that sees every sample of
a piece, covered or not -- DESIGN.md, "Pixman-exact linear gradients").  The model sees the 8-bit coverage only and misses a row's first
span where its area rounds to coverage 0 (linear_model.py); the device has the cells and does not.  A frame that differs must
therefore be exact once the model is told those rows, and how many do is asserted: the frames tests/test_linear_model.py counts against
libcairo.  Runs on an MI355X (-m gpu) and under tools/emu/run.py (every fourth frame)."""
import numpy as np
import pytest

import device_routes as dr
import linear_fuzz as lf
import linear_model as lm
import linear_scenes as ls
import spread_model as sm
from device_routes import EMU
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)

pytestmark = pytest.mark.gpu
FRAMES = 34                                      # per spread and frame size
# the frames whose model needs a hidden row, and the rows: (frame size, case index) -> rows.  The cases are a prefix of those
# tests/test_linear_model.py holds against live libcairo, where the same frames need the same rows to equal libcairo.
HIDDEN_FIRST_SPAN = {"pad": {((96, 48), 13): [30]}, "reflect": {((96, 48), 17): [5], ((96, 48), 33): [44]}, "repeat": {}}


@pytest.mark.parametrize("spread", ls.SPREADS)
def test_random_frames_are_the_model(spread):
    done = caveat = 0
    hidden = {}
    for size in lf.SIZES:
        for case in lf.cases(spread, size, FRAMES)[:: 4 if EMU else 1]:
            e = lf.expected(case)
            got = dr.through_render(case["scene"], linear="pixman")
            msg = (spread, size, case["index"], case["shape"], case["kind"])
            d = (got != e["truth"]).any(-1) & ~e["caveat"]
            if d.any():
                rows = sorted(set(np.nonzero(d)[0].tolist()))
                md = case["model"]
                e = lm.frame(sm.pattern_matrix(md["matrices"]), lf.LINE, md["stops"], lf.EXTEND[spread], md["rect"], e["alpha"], hidden_rows=rows)
                assert not case["whole_box"], msg
                hidden[tuple(size), case["index"]] = rows
                print("linear fuzz: rows with a hidden first span", msg, rows)
            off = ~e["caveat"]
            assert (got[off] == e["truth"][off]).all(), msg
            assert (got[e["caveat"]] == e["every_sample"][e["caveat"]]).all(), msg
            caveat += int(e["caveat"].sum())
            done += 1
    print("linear fuzz,", spread, ":", done, "frames,", hidden, "with a hidden first span,", caveat, "caveat pixels")
    assert all(HIDDEN_FIRST_SPAN[spread].get(k) == v for k, v in hidden.items()), hidden
    if not EMU:
        assert done == 2 * FRAMES and hidden == HIDDEN_FIRST_SPAN[spread]
