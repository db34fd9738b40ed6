"""Filter lists on the device ("Filter lists").

1. the chain inside render: a frame's content is rendered plain over a clear frame (the group G) and again inside a "filters" container
   -- against tests/filter_model.py (itself held against libcairo + pixman by tests/test_filters_model.py) applied to G, zero differing
   bytes, at the sizes at which the passes' segments and tails can go wrong;
2. a list of one entry is the existing layer: every cairo_blur_* and cairo_shadow_* golden scene with its "blur" or "shadow" rewritten as a
   one-entry "filters", byte for byte;
3. every cairo_filters_* golden (libcairo + pixman) through render, and again through render_resident, zero differing bytes;
4. ALPHA and ERASE on a flagged handle, against the frame model of the composite;
5. the routes that do not draw filtered layers refuse by name, and the handle renders correctly afterwards;
6. a frame without "filters" behind a filtered one is the frame a fresh handle renders, and the other way round;
7. a slot set anew changes the next walk only.
Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import itertools

import numpy as np
import pytest

import blur_scenes as bl
import device_routes as dr
import filter_model as fm
import filter_scenes as fsc
import shadow_scenes as ss
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats

pytestmark = pytest.mark.gpu

FAMILY = dr.FAMILIES["filters"]
# the shared sizes below the one that only makes shadow.hip's loops run twice (the kernels are unchanged)
SIZES = dr.SIZES
ODD = "blur_odd"                                  # three box steps: the result changes buffers
_content = dr.content


def _lists():
    """the ordered pairs of the six entries that begin or end with the blur of an odd number of box steps, and the chain of four"""
    E = fsc.ENTRIES
    out = {"%s,%s" % (a, b): [E[a], E[b]] for a, b in itertools.product(sorted(E), repeat=2) if ODD in (a, b)}
    assert len(out) == 11
    out["chain_of_four"] = fsc.CHAIN_OF_FOUR
    return out


# ---- 1. the chain inside render
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_chain_inside_render_against_the_model(size):
    w, h = size
    r = dr.handle(w, h)
    try:
        kids = _content(w, h)
        r.render({"children": kids})
        G = r.read_image(premultiplied=True)
        assert len(np.unique(G[..., 3])) > 8 and (G[..., 3] == 0).any(), "the group holds many alphas, and clear pixels"
        for name, chain in sorted(_lists().items()):
            r.render({"children": [{"type": "container", "children": kids, "filters": chain}]})
            dr.not_refused(r, name)
            assert r.built_filters() == [fm.as_dicts(chain)]
            n, mx = diff_stats(r.read_image(premultiplied=True), fm.apply(G, chain))
            print("filters %dx%d %s: differing pixels %d max %d" % (w, h, name, n, mx))
            assert (n, mx) == (0, 0), (size, name)
    finally:
        r.close()


# ---- 2. a list of one entry is the existing layer
@pytest.mark.parametrize("fname", sorted(bl.files()) + sorted(ss.files()))
def test_a_list_of_one_entry_is_the_existing_layer(fname):
    family = bl if fname in bl.files() else ss
    make, aliased = family.files()[fname]
    gold = np.load(family.golden_path(fname))
    scenes = make()
    assert sorted(scenes) == sorted(gold.files)
    for name, sc in sorted(scenes.items()):
        stage = {"children": fsc.as_filter_lists(sc["stage"]["children"])}
        r = dr.renderer_for(sc, aliased)
        try:
            r.render(stage)
            assert r.built_filters() and all(len(f) == 1 for f in r.built_filters()) and all(len(l) == 4 for l in r.built_layers()), name
            n, mx = diff_stats(r.read_image(premultiplied=True), gold[name])
            print(fname, name, "as a list of one: differing pixels", n, "max", mx)
            assert (n, mx) == (0, 0), (fname, name)
        finally:
            r.close()


# ---- 3. the goldens of libcairo + pixman
@pytest.mark.parametrize("fname", sorted(fsc.files()))
def test_goldens_through_render(fname):
    dr.goldens_through_render_and_resident(FAMILY, fname)


# ---- 4. ALPHA and ERASE
def test_alpha_and_erase_filtered_layers():
    dr.alpha_and_erase(FAMILY, "cairo_filters_operators", "glow_drop_normal_clear", "glow_drop_normal_opaque")


# ---- 5. the routes not taken refuse by name
def test_refused_routes_and_the_handle_afterwards():
    sc = fsc.operator_scenes()["blur_drop_multiply_opaque"]
    plain = dict(sc, stage={"children": fsc.without_filters(sc["stage"]["children"])})
    dr.refused_routes(FAMILY, sc, plain, np.load(fsc.golden_path("cairo_filters_operators"))["blur_drop_multiply_opaque"], dr.through_render(plain))


# ---- 6. nothing of a filtered frame stays behind
def test_a_plain_frame_after_a_filtered_one_is_a_fresh_handles_frame():
    dr.plain_frame_after(FAMILY, ("filtered_blurred_shadowed", "chain_of_four", "filters_mask_opacity"), "cairo_filters_structure")


# ---- 7. the slot is read at the walk
def test_the_slots_list_at_the_walk_is_the_list():
    """a slot set anew through set_filters changes the next walk only"""
    scenes = fsc.structure_scenes()
    gold = np.load(fsc.golden_path("cairo_filters_structure"))
    a, b = scenes["order_glow_drop"], scenes["order_drop_glow"]
    r = dr.renderer_for(a, False)
    try:
        r.render(a["stage"])                                          # (render assigns slot 0 to the stage's one list)
        assert diff_stats(r.read_image(premultiplied=True), gold["order_glow_drop"]) == (0, 0)
        r.set_filters(0, [fsc.ENTRIES["drop"], fsc.ENTRIES["glow"]])
        r.render_resident(1)
        assert diff_stats(r.read_image(premultiplied=True), gold["order_glow_drop"]) == (0, 0)
        assert r.built_filters() == [fm.as_dicts([fsc.ENTRIES["glow"], fsc.ENTRIES["drop"]])]
        r.render(b["stage"])
        assert diff_stats(r.read_image(premultiplied=True), gold["order_drop_glow"]) == (0, 0)
        assert r.built_filters() == [fm.as_dicts([fsc.ENTRIES["drop"], fsc.ENTRIES["glow"]])]
    finally:
        r.close()
