"""Isolated layers on the device: every libcairo golden of tests/layer_scenes.py -- every file, every scene -- through render,
swfr_render_edges (+ resident frames), SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and render_batch with layered and
plain frames in one group, zero differing bytes (linear-gradient scenes: LINEAR_BOUND, see layer_scenes.py); the plain frames of a
batch are held against the oracle, the aliased ones against tests/frame_model.py's render(..., aliased=True).  Under the emulator the
routes other than render take every fourth scene of a file.  One 4K frame, S1 with its stars in layers.  And the existing corpus through
the layer instance of the tile kernel (SWFR_TILES_SHADERS=4), byte-identical to what instances 0-2 give.  Runs on an MI355X (-m gpu) and
under tools/emu/run.py.

Observed on an MI355X: every exact scene 0 differing bytes; the linear-gradient scenes at most 2 LSB (bound 3).
"""
import numpy as np
import pytest

import device_routes as dr
import layer_scenes as bs
import scenarios
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats, product_render

pytestmark = pytest.mark.gpu
SC = scenarios.scenarios()
FAMILY = dr.FAMILIES["layer"]
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


@pytest.mark.parametrize("contiguous", FAMILY.layouts, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_two_band_handles(fname, contiguous):
    dr.goldens_through_two_band_handles(FAMILY, fname, contiguous)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_batch_with_unlike_frames(fname):
    dr.goldens_through_render_batch_with_unlike_frames(FAMILY, fname)


def test_s1_4k_stars_in_layers():
    dr.s1_4k_crops(FAMILY, "cairo_layer_s1_crops")


# ---- 2. the culling rules
@pytest.mark.parametrize("mode", ["normal", "multiply", "add", "overlay"])
def test_cover_inside_a_group_does_not_cull_and_an_opaque_cover_above_does(mode):
    gold = np.load(bs.golden_path("cairo_layer_structure_" + mode))
    scenes = bs.structure_scenes([mode])
    for name in ("cover_inside_" + mode, "cover_above_" + mode):
        assert diff_stats(product_render(scenes[name]), gold[name]) == (0, 0), name
    # what is below a group that holds an opaque full cover shows through it wherever the composite lets it: the frame differs from
    # the one without the inner rectangle below the groups
    inside = scenes["cover_inside_" + mode]
    kids = inside["stage"]["children"]
    if mode != "normal":                                         # (an opaque group pixel composited with OVER does hide what is below)
        assert (product_render(dict(inside, stage={"children": kids[:1] + kids[2:]})) != gold["cover_inside_" + mode]).any()
    # what is below an opaque cover does not: in the cover's columns the frame is the one without the group
    above = scenes["cover_above_" + mode]
    kids = above["stage"]["children"]
    assert (product_render(dict(above, stage={"children": kids[:1] + kids[2:]}))[:, :100] == gold["cover_above_" + mode][:, :100]).all()


def test_a_layer_is_not_the_per_path_rule():
    """the feature is visible: overlapping translucent children as one layer and each on its own differ under every operator"""
    scenes = bs.overlap_scenes()
    gold = np.load(bs.golden_path("cairo_layer_overlap"))
    for mode in bs.MODES:
        sc = scenes[mode + "_opaque"]
        kids = sc["stage"]["children"]
        per_path = dict(sc, stage={"children": kids[:-1] + [dict({k: v for k, v in kids[-1].items() if k != "layer"}, blend_mode=mode)]})
        assert (product_render(per_path) != gold[mode + "_opaque"]).any(), mode


# ---- 3. the existing corpus through the layer instance: byte-identical to what instances 0-2 give
@pytest.mark.parametrize("rows", ["narrow", "wide"])
@pytest.mark.parametrize("name", sorted(SC))
def test_scenario_through_instance_4(name, rows, monkeypatch):
    dr.scenario_through_instance(FAMILY, SC[name], name, rows, monkeypatch)


def test_aliased_scenarios_through_instance_4(monkeypatch):
    dr.aliased_scenarios_through_instance(FAMILY, SC, monkeypatch)


@pytest.mark.parametrize("rows", ["narrow", "wide"])
def test_structural_scenes_through_instance_4(rows, monkeypatch):
    dr.structural_scenes_through_instance(FAMILY, rows, monkeypatch)


def test_s1_4k_known_answer_through_instance_4(monkeypatch):
    dr.s1_4k_known_answer_through_instance(FAMILY, monkeypatch)
