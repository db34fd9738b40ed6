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

import device_routes as dr
import layer_scenes as ls
import shadow_model as sm
import shadow_scenes as ss
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats
from swf_renderer_amd import api
from shadow_model import COLORS, FLAGS, STRENGTHS, offsets

pytestmark = pytest.mark.gpu

FAMILY = dr.FAMILIES["shadow"]
SIZES = dr.SIZES_AND_LOOPS_TWICE                  # (the blur passes between shadow.hip's two kernels have their own sizes: tests/test_blur_gpu.py)
SRC, DST = 7, 9
_content, _whole_frame_bitmap = dr.content, dr.whole_frame_bitmap


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
    dr.goldens_through_render_and_resident(FAMILY, fname)


def test_alpha_and_erase_shadowed_layers():
    dr.alpha_and_erase(FAMILY, "cairo_shadow_operators", "drop_normal_clear", "drop_normal_opaque")


# ---- 4. the routes not taken refuse by name
def test_refused_routes_and_the_handle_afterwards():
    sc = ss.operator_scenes()["glow_multiply_opaque"]
    plain = dict(sc, stage={"children": ss.without_shadow(sc["stage"]["children"])})
    dr.refused_routes(FAMILY, sc, plain, np.load(ss.golden_path("cairo_shadow_operators"))["glow_multiply_opaque"], dr.through_render(plain))


# ---- 5. nothing of a shadowed frame stays behind
def test_a_plain_frame_after_a_shadowed_one_is_a_fresh_handles_frame():
    dr.plain_frame_after(FAMILY, ("two_shadows_and_a_blur", "shadow_wider_than_frame", "shadow_mask_opacity"), "cairo_shadow_structure")


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
