"""Gradient spread modes on the device (raster_common.hip, spread_walker_pixel: every k2_tiles instance from 2 up runs it).

Every libcairo golden of tests/spread_scenes.py's files() (the run-start scenes, where the device keeps a rule of its own, and random
frames are in tests/test_spread_fuzz_gpu.py) -- reflected and repeated radial and focal gradients, antialiased and aliased -- through
render (also with the instance forced to 2), swfr_render_edges (+ resident frames), SWFR_GRAPHS=1, two-band handles (contiguous and
interleaved) and render_batch with unlike frames (padded and spread gradients, and plain frames, in one launch); the structure file
once through each of the instances 3 to 6.  Zero differing bytes; the padded linear scene alone stays at LINEAR_BOUND.

The oracle knows nothing of spread (it paints these scenes padded), so nothing here is held against it bar the plain frames of the
batch route.  On a library without the feature every golden comparison of a non-pad scene fails: the generator's gate makes sure
each differs from its padded rendering.

Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import numpy as np
import pytest

import device_routes as dr
import spread_scenes as ss
from device_routes import EMU, renderer_for
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)

pytestmark = pytest.mark.gpu
FAMILY = dr.Family("spread", ss, "2", True, (True, False))
FILES = sorted(ss.files())


@pytest.mark.parametrize("forced", [False, True], ids=["picked", "forced"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render(fname, forced, monkeypatch):
    dr.goldens_through_render(FAMILY, fname, monkeypatch, forced)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_edges(fname):
    dr.goldens_through_render_edges(FAMILY, fname)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_with_graphs(fname, monkeypatch):
    dr.goldens_with_graphs(FAMILY, fname, monkeypatch)


@pytest.mark.parametrize("contiguous", FAMILY.layouts, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_two_band_handles(fname, contiguous):
    dr.goldens_through_two_band_handles(FAMILY, fname, contiguous)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_batch_with_unlike_frames(fname):
    dr.goldens_through_render_batch_with_unlike_frames(FAMILY, fname)


@pytest.mark.parametrize("instance", ["3", "4", "5", "6"])
@pytest.mark.parametrize("spread", ss.SPREADS)
def test_structure_through_instance(spread, instance, monkeypatch):
    """the heavier instances shade through the same call: the structure file (every fourth scene on the emulator) forced through each"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)
    fname = "cairo_spread_%s_structure" % spread
    gold = np.load(ss.golden_path(fname))
    for name, sc in sorted(ss.GROUPS["structure"](spread).items())[int(instance) % 4 if EMU else 0:: 4 if EMU else 1]:
        r = renderer_for(sc, False)
        try:
            r.render(sc["stage"])
            dr.check(FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "instance", instance))
            dr.not_refused(r, name)
        finally:
            r.close()


def test_a_spread_is_visible():
    """every non-pad golden differs from what the same scene gives padded (a single stop is one colour under any rule)"""
    for spread in ss.SPREADS:
        gold = np.load(ss.golden_path("cairo_spread_%s_radial" % spread))
        for name, sc in sorted(ss.GROUPS["radial"](spread).items()):
            if name.endswith("_single"):
                continue
            r = renderer_for(sc, False)
            try:
                r.render(ss.with_spread(sc["stage"], "pad"))
                assert (r.read_image(premultiplied=True) != gold[name]).any(), name
            finally:
                r.close()
