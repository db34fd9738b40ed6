"""Blend modes on the device: every libcairo golden of tests/blend_scenes.py -- every file, every scene -- through render,
swfr_render_edges (+ resident frames), SWFR_GRAPHS=1, two contiguous-band handles and render_batch with unlike frames, zero
differing bytes (linear-gradient scenes: LINEAR_BOUND, see blend_scenes.py).  Under the emulator the routes other than render take
every fourth scene of a file.  And the existing corpus through the blend instance of the tile kernel
(SWFR_TILES_SHADERS=3), byte-identical to what instances 0-2 give.  Runs on an MI355X (-m gpu) and under tools/emu/run.py."""
import numpy as np
import pytest

import blend_scenes as bs
import device_routes as dr
import scenarios
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats, product_render

pytestmark = pytest.mark.gpu
SC = scenarios.scenarios()
FAMILY = dr.FAMILIES["blend"]
FILES = sorted(FAMILY.scenes.files())


# ---- 1. every golden through every route of tests/device_routes.py
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render(fname, monkeypatch):
    dr.goldens_through_render(FAMILY, fname, monkeypatch)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_edges(fname):
    dr.goldens_through_render_edges(FAMILY, fname)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_with_graphs(fname, monkeypatch):
    dr.goldens_with_graphs(FAMILY, fname, monkeypatch)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_two_contiguous_band_handles(fname):
    dr.goldens_through_two_band_handles(FAMILY, fname, True)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_batch_with_unlike_frames(fname):
    dr.goldens_through_render_batch_with_unlike_frames(FAMILY, fname)


@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_s1_4k_every_third_star_blended(aliased):
    dr.s1_4k_crops(FAMILY, "cairo_blend_aliased_s1_crops" if aliased else "cairo_blend_s1_crops", aliased)


# ---- 2. the culling rules
@pytest.mark.parametrize("mode", ["multiply", "add", "overlay"])
def test_blended_cover_does_not_cull_and_an_opaque_cover_above_does(mode):
    gold = np.load(bs.golden_path("cairo_blend_structure"))
    scenes = bs.structure_scenes()
    for name in ("cover_below_" + mode, "cover_above_" + mode):
        sc = scenes[name]
        got = product_render(sc)
        assert diff_stats(got, gold[name]) == (0, 0), name
    # what is below a blended full cover shows through it: the frame differs from the one without the inner rectangle
    below = scenes["cover_below_" + mode]
    without = dict(below, stage={"children": below["stage"]["children"][:1] + below["stage"]["children"][2:]})
    assert (product_render(without) != gold["cover_below_" + mode]).any()
    # what is below an opaque cover does not: in the cover's columns the frame is the one without the blended path
    above = scenes["cover_above_" + mode]
    bare = dict(above, stage={"children": above["stage"]["children"][:1] + above["stage"]["children"][2:]})
    assert (product_render(bare)[:, :100] == gold["cover_above_" + mode][:, :100]).all()


# ---- 3. the existing corpus through the blend instance: byte-identical to what instances 0-2 give
@pytest.mark.parametrize("rows", ["narrow", "wide"])
@pytest.mark.parametrize("name", sorted(SC))
def test_scenario_through_instance_3(name, rows, monkeypatch):
    dr.scenario_through_instance(FAMILY, SC[name], name, rows, monkeypatch)


def test_aliased_scenarios_through_instance_3(monkeypatch):
    dr.aliased_scenarios_through_instance(FAMILY, SC, monkeypatch)


@pytest.mark.parametrize("rows", ["narrow", "wide"])
def test_structural_scenes_through_instance_3(rows, monkeypatch):
    dr.structural_scenes_through_instance(FAMILY, rows, monkeypatch)


def test_s1_4k_known_answer_through_instance_3(monkeypatch):
    dr.s1_4k_known_answer_through_instance(FAMILY, monkeypatch)
