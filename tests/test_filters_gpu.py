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
import layer_scenes as ls
import shadow_model as sm
import shadow_scenes as ss
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats
from swf_renderer_amd import api

pytestmark = pytest.mark.gpu

# the sizes of tests/test_shadow_gpu.py and tests/test_blur_gpu.py below the one that only makes shadow.hip's loops run twice (the kernels
# are unchanged): 257 x 3 and 3 x 257 leave tails behind the groups of four words and cut the box passes' runs; 2100 x 150 spans three
# segments of both box passes
SIZES = ((13, 11), (257, 3), (3, 257), (2100, 150))
ODD = "blur_odd"                                  # three box steps: the result changes buffers


def _content(w, h):
    """translucent and opaque shapes all over a w x h frame, some across its edges, clear pixels between them (as tests/test_shadow_gpu.py)"""
    rng = np.random.default_rng(w * 1000 + h)
    kids = []
    for i in range(16):
        cx, cy = rng.uniform(-0.1, 1.1) * w, rng.uniform(-0.1, 1.1) * h
        pts = [(cx + rng.uniform(-0.25, 0.25) * w, cy + rng.uniform(-0.5, 0.5) * h) for _ in range(3)]
        a = 255 if i % 5 == 0 else int(rng.integers(30, 250))
        kids.append(bl._shape(pts, (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), a)))
    kids.append(bl._rect(0, 0, 1, h / 2, (255, 255, 255, 255)))                  # opaque white against the left edge
    return kids


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
    make, aliased = fsc.files()[fname]
    gold = np.load(fsc.golden_path(fname))
    scenes = make()
    assert sorted(scenes) == sorted(gold.files)
    for name, sc in sorted(scenes.items()):
        r = dr.renderer_for(sc, aliased)
        try:
            r.render(sc["stage"])
            dr.not_refused(r, name)
            n, mx = diff_stats(r.read_image(premultiplied=True), gold[name])
            print(fname, name, "differing pixels", n, "max", mx)
            assert (n, mx) == (0, 0), (fname, name)
            # the textures stay: the resident parent frame renders again to the same pixels
            r.render_resident(1)
            assert diff_stats(r.read_image(premultiplied=True), gold[name]) == (0, 0), (fname, name, "resident")
        finally:
            r.close()


# ---- 4. ALPHA and ERASE
def test_alpha_and_erase_filtered_layers():
    """on a flagged handle the last result is the source of DEST_OUT / DEST_IN: against the frame model of the composite -- the last
    result from the goldens' normal scene over clear, where the frame IS that surface"""
    gold = np.load(fsc.golden_path("cairo_filters_operators"))
    final = gold["glow_drop_normal_clear"].astype(np.int64)
    sc = fsc.operator_scenes()["glow_drop_normal_opaque"]
    ground = dr.through_render(dict(sc, stage={"children": sc["stage"]["children"][:-1]})).astype(np.int64)
    for mode, factor in (("erase", 255 - final[..., 3:]), ("alpha", final[..., 3:])):
        want = sm.mul_un8(ground, factor).astype(np.uint8)
        assert (want != ground).any()
        kids = sc["stage"]["children"][:-1] + [dict(sc["stage"]["children"][-1], layer=mode)]
        got = dr.through_render(dict(sc, stage={"children": kids}), alpha_modes=True)
        assert diff_stats(got, want) == (0, 0), mode


# ---- 5. the routes not taken refuse by name
def test_refused_routes_and_the_handle_afterwards():
    sc = fsc.operator_scenes()["blur_drop_multiply_opaque"]
    plain = dict(sc, stage={"children": fsc.without_filters(sc["stage"]["children"])})
    want_plain = dr.through_render(plain)
    want = np.load(fsc.golden_path("cairo_filters_operators"))["blur_drop_multiply_opaque"]
    r = dr.renderer_for(sc, False)
    try:
        def refused(call, code, name):
            with pytest.raises(api.SwfrError) as e:
                call()
            assert e.value.code == code and name in str(e.value), (code, name, str(e.value))
            r.render(plain["stage"])                                  # the handle renders a frame without filters correctly afterwards
            assert diff_stats(r.read_image(premultiplied=True), want_plain) == (0, 0), name
        refused(lambda: r.render_batch([plain["stage"], sc["stage"], plain["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        refused(lambda: r.render_sequence([plain["stage"], sc["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        refused(lambda: r.render_sequence_readback([sc["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        r.render(sc["stage"])
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
    finally:
        r.close()
    for contiguous in (False, True):
        b = dr.renderer_for(sc, False, band_index=0, band_count=2, contiguous_bands=contiguous)
        try:
            with pytest.raises(api.SwfrError) as e:
                b.render(sc["stage"])
            assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedBlurBands" in str(e.value)
            b.render(plain["stage"])
        finally:
            b.close()


# ---- 6. nothing of a filtered frame stays behind
def test_a_plain_frame_after_a_filtered_one_is_a_fresh_handles_frame():
    scenes = fsc.structure_scenes()
    plain_sc = ls.overlap_scenes()["multiply_translucent"]
    assert (plain_sc["width"], plain_sc["height"]) == (fsc.W, fsc.H)
    fresh = dr.through_render(plain_sc)
    gold = np.load(fsc.golden_path("cairo_filters_structure"))
    r = dr.renderer_for(plain_sc, False)
    try:
        for name in ("filtered_blurred_shadowed", "chain_of_four", "filters_mask_opacity"):
            r.render(scenes[name]["stage"])
            r.render(plain_sc["stage"])
            assert diff_stats(r.read_image(premultiplied=True), fresh) == (0, 0), name
            r.render_resident(3)
            assert diff_stats(r.read_image(premultiplied=True), fresh) == (0, 0), name
            # and the other way round: the filtered frame behind the plain one, then resident
            r.render(scenes[name]["stage"])
            r.render_resident(2)
            assert diff_stats(r.read_image(premultiplied=True), gold[name]) == (0, 0), name
    finally:
        r.close()


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
