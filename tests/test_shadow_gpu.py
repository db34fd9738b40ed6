"""Shadowed layers on the device ("Shadowed layers").

1. the kernels alone: a frame is rendered, captured as a bitmap, given its shadow (swfr_shadow_bitmap), drawn 1:1 with a nearest fill and
   read back -- against tests/shadow_model.py (itself held against libcairo + pixman by tests/test_shadow_model.py) on the first frame's
   pixels, zero differing bytes;
2. a shadow that adds nothing (1 x 1 box, no offset, strength 1, a colour of alpha 0) is the plain layer: the scenes of the existing
   layer goldens with "layer" turned into such a "shadow", byte for byte;
3. every cairo_shadow_* golden (libcairo + pixman) through render, and again through render_resident, zero differing bytes;
4. the routes that do not draw shadowed layers refuse by name, and the handle renders correctly afterwards;
5. a frame without "shadow" behind a shadowed one is the frame a fresh handle renders.
Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import itertools

import numpy as np
import pytest

import blur_scenes as bl
import device_routes as dr
import layer_scenes as ls
import scenarios
import shadow_model as sm
import shadow_scenes as ss
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats
from swf_renderer_amd import api
from shadow_model import COLORS, FLAGS, STRENGTHS, offsets

pytestmark = pytest.mark.gpu

# shadow.hip: a lane takes four words, 2048 workgroups of 256 lanes stride over the image -- 2 097 152 words a stride.  2051 x 1029 is
# 2 110 479 words: both kernels' loops over groups of four words run a second, partial time (3 331 groups), and three words are left for
# the word loop (which takes more than three only in a buffer that is not 16-byte aligned: none of the handle's own is).  The blur passes
# between them have their own sizes (tests/test_blur_gpu.py): 2100 x 150 spans three segments of both.  On the emulator 2051 x 1029 is a
# matter of minutes and left out
LOOPS_TWICE = (2051, 1029)
SIZES = ((13, 11), (257, 3), (3, 257), (2100, 150)) + (() if dr.EMU else (LOOPS_TWICE,))
SRC, DST = 7, 9


def _content(w, h):
    """translucent and opaque shapes all over a w x h frame, some across its edges, clear pixels between them"""
    rng = np.random.default_rng(w * 1000 + h)
    kids = []
    for i in range(16):
        cx, cy = rng.uniform(-0.1, 1.1) * w, rng.uniform(-0.1, 1.1) * h
        pts = [(cx + rng.uniform(-0.25, 0.25) * w, cy + rng.uniform(-0.5, 0.5) * h) for _ in range(3)]
        a = 255 if i % 5 == 0 else int(rng.integers(30, 250))
        kids.append(bl._shape(pts, (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), a)))
    kids.append(bl._rect(0, 0, 1, h / 2, (255, 255, 255, 255)))                  # opaque white against the left edge
    return kids


def _whole_frame_bitmap(w, h, bitmap_id):
    fill = {"type": "bitmap", "bitmap_id": bitmap_id, "repeating": False, "smoothed": False, "filter": "nearest",
            "matrix": scenarios._m(20, 20, 0, 0)}
    return {"type": "shape", "definition": scenarios._poly_shape([(0, 0), (w * 20, 0), (w * 20, h * 20), (0, h * 20)], fill)}


def _cases(w, h):
    """every offset, strength, colour and flag state of tests/test_shadow_model.py: their whole product on the smallest image, on the
    others each value at least once (the passes are pointwise in strength, colour and flag: the image's size changes nothing there)"""
    offs, boxes = offsets(w, h), ((3, 4, 1), (1, 1, 1), (2, 0, 3), (64, 255, 1))
    if w * h <= 13 * 11:
        for n, ((dx, dy), strength, color, flags) in enumerate(itertools.product(offs, STRENGTHS, sorted(COLORS), sorted(FLAGS))):
            yield (dx, dy), boxes[n % 3], strength, color, flags
        yield (1, -1), boxes[3], 2, "translucent", "over"
        return
    few = 3 if w * h > 1000000 else 6
    for n in range(few):
        yield offs[n % len(offs)], boxes[n % len(boxes)], STRENGTHS[n % len(STRENGTHS)], sorted(COLORS)[n % 3], sorted(FLAGS)[n % 3]
    if few > 3:
        yield offs[4], boxes[1], 255, "translucent", "knockout"


def _shadow(off, box, strength, color, flags):
    return dict(FLAGS[flags], color=COLORS[color], dx=off[0], dy=off[1], x=box[0], y=box[1], passes=box[2], strength=strength)


# ---- 1. the kernels alone
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_shadow_bitmap_against_the_model(size):
    w, h = size
    r = dr.handle(w, h)
    try:
        r.render({"children": _content(w, h)})
        frame = r.read_image(premultiplied=True)
        assert len(np.unique(frame[..., 3])) > 8 and (frame[..., 3] == 0).any(), "the frame holds many alphas, and clear pixels"
        r.capture_bitmap(SRC)
        draw = {"children": [_whole_frame_bitmap(w, h, DST)]}
        seen = set()
        for case in _cases(w, h):
            sh = _shadow(*case)
            r.shadow_bitmap(DST, SRC, sh)
            r.render(draw)
            n, mx = diff_stats(r.read_image(premultiplied=True), sm.shadow(frame, sh))
            if (n, mx) != (0, 0) or w * h > 13 * 11:
                print("shadow %dx%d %r: differing pixels %d max %d" % (w, h, sh, n, mx))
            assert (n, mx) == (0, 0), (size, sh)
            seen.add(case[0]), seen.add(case[2]), seen.add(case[3]), seen.add(case[4])
        assert seen >= (set(offsets(w, h)) | set(STRENGTHS) if w * h <= 1000000 else set()) | set(COLORS) | set(FLAGS)
        # the source is untouched; then the shadow in place (dst == src), and the shadow of that
        r.render({"children": [_whole_frame_bitmap(w, h, SRC)]})
        assert diff_stats(r.read_image(premultiplied=True), frame) == (0, 0), "the source bitmap is still the frame"
        first, second = _shadow((2, 1), (3, 2, 1), 2, "translucent", "over"), _shadow((-1, 0), (2, 2, 1), 1, "opaque", "knockout")
        r.shadow_bitmap(SRC, SRC, first)
        r.render({"children": [_whole_frame_bitmap(w, h, SRC)]})
        want = sm.shadow(frame, first)
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), "in place"
        r.shadow_bitmap(SRC, SRC, second)
        r.render({"children": [_whole_frame_bitmap(w, h, SRC)]})
        assert diff_stats(r.read_image(premultiplied=True), sm.shadow(want, second)) == (0, 0), "in place, twice"
        with pytest.raises(api.SwfrError) as e:
            r.shadow_bitmap(DST, SRC + 100, first)
        assert e.value.code == api.ERR_NOT_FOUND
        # a bitmap with a shadow has no straight texels to transform
        with pytest.raises(api.SwfrError) as e:
            r.render({"children": [dict(draw["children"][0], color_transform={"red_mult": 0.5})]})
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedCapturedBitmapTransform" in str(e.value)
    finally:
        r.close()


# ---- 2. a shadow that adds nothing is the plain layer
NOTHING = {"color": (255, 255, 255, 0), "x": 1, "y": 1}


def _layers_to_shadows(obj, count):
    if isinstance(obj, list):
        return [_layers_to_shadows(o, count) for o in obj]
    out = dict(obj)
    if out.get("layer") is not None and out.get("layer") is not False and out.get("mask") is None and out.get("opacity") is None:
        out["shadow"] = dict(NOTHING)
        count[0] += 1
    if "children" in out:
        out["children"] = _layers_to_shadows(out["children"], count)
    return out


@pytest.mark.parametrize("aliased", (False, True), ids=("antialiased", "aliased"))
def test_a_shadow_that_adds_nothing_is_the_plain_layer_overlap(aliased):
    gold = np.load(ls.golden_path("cairo_layer_aliased_overlap" if aliased else "cairo_layer_overlap"))
    scenes = ls.overlap_scenes()
    assert len(scenes) == 27
    for name, sc in sorted(scenes.items()):
        count = [0]
        stage = {"children": _layers_to_shadows(sc["stage"]["children"], count)}
        assert count[0] == 1, name
        got = dr.through_render(dict(sc, stage=stage), aliased)
        n, mx = diff_stats(got, gold[name])
        print("nothing", name, "aliased" if aliased else "", "differing pixels", n, "max", mx)
        assert (n, mx) == (0, 0), name


@pytest.mark.parametrize("mode", ls.MODES)
def test_a_shadow_that_adds_nothing_is_the_plain_layer_sources(mode):
    gold = np.load(ls.golden_path("cairo_layer_sources_" + mode))
    done = 0
    for name, sc in sorted(ls.source_scenes(mode).items()):
        count = [0]
        stage = {"children": _layers_to_shadows(sc["stage"]["children"], count)}
        if not sc["exact"] or not 1 <= count[0] <= api.MAX_BLUR_LAYERS:
            continue
        r = dr.renderer_for(sc, False)
        try:
            r.render(stage)
            n, mx = diff_stats(r.read_image(premultiplied=True), gold[name])
        finally:
            r.close()
        print("nothing", name, "differing pixels", n, "max", mx)
        assert (n, mx) == (0, 0), name
        done += 1
    assert done >= 6


# ---- 3. the goldens of libcairo + pixman
@pytest.mark.parametrize("fname", sorted(ss.files()))
def test_goldens_through_render(fname):
    make, aliased = ss.files()[fname]
    gold = np.load(ss.golden_path(fname))
    scenes = make()
    assert sorted(scenes) == sorted(gold.files)
    for name, sc in sorted(scenes.items()):
        r = dr.renderer_for(sc, aliased)
        try:
            r.render(sc["stage"])
            dr.not_refused(r, name)
            got = r.read_image(premultiplied=True)
            n, mx = diff_stats(got, gold[name])
            print(fname, name, "differing pixels", n, "max", mx)
            assert (n, mx) == (0, 0), (fname, name)
            # the textures stay: the resident parent frame renders again to the same pixels
            r.render_resident(1)
            assert diff_stats(r.read_image(premultiplied=True), gold[name]) == (0, 0), (fname, name, "resident")
        finally:
            r.close()


def test_alpha_and_erase_shadowed_layers():
    """on a flagged handle the final surface is the source of DEST_OUT / DEST_IN: against the frame model of the composite -- the final
    surface from the goldens' normal scene over clear, where the frame IS that surface"""
    gold = np.load(ss.golden_path("cairo_shadow_operators"))
    final = gold["drop_normal_clear"].astype(np.int64)
    sc = ss.operator_scenes()["drop_normal_opaque"]
    ground = dr.through_render(dict(sc, stage={"children": sc["stage"]["children"][:-1]})).astype(np.int64)
    for mode, factor in (("erase", 255 - final[..., 3:]), ("alpha", final[..., 3:])):
        want = sm.mul_un8(ground, factor).astype(np.uint8)
        kids = sc["stage"]["children"][:-1] + [dict(sc["stage"]["children"][-1], layer=mode)]
        got = dr.through_render(dict(sc, stage={"children": kids}), alpha_modes=True)
        assert diff_stats(got, want) == (0, 0), mode


# ---- 4. the routes not taken refuse by name
def test_refused_routes_and_the_handle_afterwards():
    sc = ss.operator_scenes()["glow_multiply_opaque"]
    plain = dict(sc, stage={"children": ss.without_shadow(sc["stage"]["children"])})
    want_plain = dr.through_render(plain)
    want_shadow = np.load(ss.golden_path("cairo_shadow_operators"))["glow_multiply_opaque"]
    r = dr.renderer_for(sc, False)
    try:
        def refused(call, code, name):
            with pytest.raises(api.SwfrError) as e:
                call()
            assert e.value.code == code and name in str(e.value), (code, name, str(e.value))
            r.render(plain["stage"])                                  # the handle renders a frame without shadows correctly afterwards
            assert diff_stats(r.read_image(premultiplied=True), want_plain) == (0, 0), name
        refused(lambda: r.render_batch([plain["stage"], sc["stage"], plain["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        refused(lambda: r.render_sequence([plain["stage"], sc["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        refused(lambda: r.render_sequence_readback([sc["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        if not dr.EMU:
            import torch
            dst = torch.zeros((3, sc["height"], sc["width"], 4), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            refused(lambda: r.render_batch([plain["stage"], sc["stage"], plain["stage"]], dst.data_ptr(), dst.stride(0)),
                    api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        # the shadow's texture named in a caller's scene: not found -- also right behind a render that made one
        r.render(sc["stage"])
        assert diff_stats(r.read_image(premultiplied=True), want_shadow) == (0, 0)
        edges, paths, styles = r.build_frame(sc["stage"])
        assert any(s.kind == api.STYLE_BITMAP and s.bitmap == api.BLUR_BASE for s in styles)
        refused(lambda: r.upload_edges(edges, paths, styles), api.ERR_NOT_FOUND, "BitmapNotFound")
        r.render(sc["stage"])
        assert diff_stats(r.read_image(premultiplied=True), want_shadow) == (0, 0)
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


# ---- 5. nothing of a shadowed frame stays behind
def test_a_plain_frame_after_a_shadowed_one_is_a_fresh_handles_frame():
    scenes = ss.structure_scenes()
    plain_sc = ls.overlap_scenes()["multiply_translucent"]
    assert (plain_sc["width"], plain_sc["height"]) == (ss.W, ss.H)
    fresh = dr.through_render(plain_sc)
    gold = np.load(ss.golden_path("cairo_shadow_structure"))
    r = dr.renderer_for(plain_sc, False)
    try:
        for name in ("two_shadows_and_a_blur", "shadow_wider_than_frame", "shadow_mask_opacity"):
            r.render(scenes[name]["stage"])
            r.render(plain_sc["stage"])
            assert diff_stats(r.read_image(premultiplied=True), fresh) == (0, 0), name
            r.render_resident(3)
            assert diff_stats(r.read_image(premultiplied=True), fresh) == (0, 0), name
            # and the other way round: the shadowed frame behind the plain one, then resident
            r.render(scenes[name]["stage"])
            r.render_resident(2)
            assert diff_stats(r.read_image(premultiplied=True), gold[name]) == (0, 0), name
    finally:
        r.close()


def test_the_slots_value_at_the_walk_is_the_shadow():
    """a caller's own type-19 object: the slot is read when the frame is built, so a slot set anew changes the next frame only"""
    sc = ss.operator_scenes()["drop_normal_translucent"]
    gold = np.load(ss.golden_path("cairo_shadow_operators"))
    glow = ss.operator_scenes()["glow_normal_translucent"]
    r = dr.renderer_for(sc, False)
    try:
        r.render(sc["stage"])                                         # (render assigns slot 0 to the stage's one shadow)
        assert diff_stats(r.read_image(premultiplied=True), gold["drop_normal_translucent"]) == (0, 0)
        r.set_shadow(0, ss.GLOW)
        r.render_resident(1)
        assert diff_stats(r.read_image(premultiplied=True), gold["drop_normal_translucent"]) == (0, 0)
        r.render(glow["stage"])
        assert diff_stats(r.read_image(premultiplied=True), gold["glow_normal_translucent"]) == (0, 0)
        assert r.built_layers()[0][4] == sm.as_dict(ss.GLOW)
    finally:
        r.close()
