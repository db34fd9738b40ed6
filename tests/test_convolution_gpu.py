"""Convolution filters on the device ("Convolution filters").

1. convolve_bitmap against tests/convolution_model.py (itself held against live pixman by tests/test_convolution_model.py), zero differing
   bytes: every kernel size on a 13 x 11 image, and six kernels at the image sizes at which the tile pass of convolve.hip can go wrong
   -- one pixel, smaller than the kernel, one short of and one past its 64 x 16 tile on either axis, two tiles and a pixel, rows and
   columns of 257;
2. the chain inside render against the list model: a convolution as the first entry (the framebuffer instance) and behind, before and
   between the other kinds, built_filters() each time;
3. every cairo_convolution_* golden (libcairo + pixman) through render, and again through render_resident, zero differing bytes;
4. a convolution as the first entry on a handle whose caller-owned target is 4 and 12 bytes modulo 16: the word paths, guards intact;
5. the routes that do not draw filtered layers refuse by name, and the handle renders correctly afterwards.
Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import itertools

import numpy as np
import pytest

import convolution_model as cm
import convolution_scenes as csc
import device_routes as dr
import filter_model as fm
import filter_scenes as fsc
from device_routes import GuardedFrames, need_gpu  # noqa: F401 (need_gpu: the module's autouse fixture)
from helpers import diff_stats
from shadow_scenes import DROP, GLOW
from swf_renderer_amd import api

pytestmark = pytest.mark.gpu

T_W, T_H = 64, 16                                  # convolve.hip's output tile (CONV_TILE_W x CONV_TILE_H)
ALL_SIZES_AT = (13, 11)
IMAGE_SIZES = ((1, 1), (3, 2), ALL_SIZES_AT, (T_W - 1, T_H + 1), (2 * T_W + 1, T_H - 1), (257, 3), (3, 257))
CHAIN_SIZES = ((13, 11), (257, 3), (2 * T_W + 1, T_H + 1))
BITMAP = 7
FAMILY = dr.FAMILIES["convolution"]
Cv = cm.convolution


_content, _whole_frame_bitmap = dr.content, dr.whole_frame_bitmap


def _six_kernels(w, h):
    rng = np.random.default_rng(7 * w + h)
    return {"sharpen": cm.SHARPEN, "random_7x7": cm.random_kernel(rng, 7, 7), "even_2x2": cm.EVEN_2X2, "even_4x6": cm.EVEN_4X6, "motion_7x1": cm.MOTION_7X1,
            "motion_1x7": cm.MOTION_1X7}


def _all_sizes():
    rng = np.random.default_rng(4949)
    kinds = ("signed", "sparse", "bound")
    out = {"%dx%d" % (kw, kh): cm.random_kernel(rng, kw, kh, kinds[n % 3]) for n, (kw, kh) in enumerate(itertools.product(range(1, 8), repeat=2))}
    assert len(out) == 49
    return out


# ---- 1. the primitive
@pytest.mark.parametrize("size", IMAGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_convolve_bitmap_against_the_model(size):
    w, h = size
    r = dr.handle(w, h)
    try:
        first = {"children": _content(w, h)}
        r.render(first)
        frame = r.read_image(premultiplied=True)
        if w * h > 6:
            assert len(np.unique(frame[..., 3])) > 4, "the frame holds many alphas"
        assert frame.any()
        draw = {"children": [_whole_frame_bitmap(w, h, BITMAP)]}
        kernels = _all_sizes() if size == ALL_SIZES_AT else _six_kernels(w, h)
        changed = 0
        for name, value in sorted(kernels.items()):
            r.render(first)
            r.capture_bitmap(BITMAP)
            r.convolve_bitmap(BITMAP, value)
            r.render(draw)
            want = cm.convolve(frame, value)
            n, mx = diff_stats(r.read_image(premultiplied=True), want)
            print("convolve %dx%d kernel %s: differing pixels %d max %d" % (w, h, name, n, mx))
            assert (n, mx) == (0, 0), (size, name)
            changed += int((want != frame).any())
        assert changed > len(kernels) // 2, "the kernels change the image"
        # convolving twice is convolving the convolved bitmap; the identity and the clear kernel
        r.convolve_bitmap(BITMAP, cm.EMBOSS)
        r.render(draw)
        twice = cm.convolve(want, cm.EMBOSS)
        assert diff_stats(r.read_image(premultiplied=True), twice) == (0, 0), "twice"
        r.convolve_bitmap(BITMAP, cm.IDENTITY)
        r.render(draw)
        assert diff_stats(r.read_image(premultiplied=True), twice) == (0, 0), "the identity"
        r.convolve_bitmap(BITMAP, {"taps": [[0, 0], [0, 0]]})
        r.render(draw)
        assert not r.read_image(premultiplied=True).any(), "all taps zero: a clear surface"
        with pytest.raises(api.SwfrError) as e:
            r.convolve_bitmap(BITMAP + 1, cm.SHARPEN)
        assert e.value.code == api.ERR_NOT_FOUND
        with pytest.raises(api.SwfrError) as e:
            r.convolve_bitmap(BITMAP, {"taps": [[cm.MAX_ABS_SUM, 1]]})
        assert e.value.code == api.ERR_INVALID and "InvalidKernel" in str(e.value)
        # a convolved bitmap has no straight texels to transform
        with pytest.raises(api.SwfrError) as e:
            r.render({"children": [dict(draw["children"][0], color_transform={"red_mult": 0.5})]})
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedCapturedBitmapTransform" in str(e.value)
    finally:
        r.close()


def test_convolve_bitmap_of_a_registered_bitmap_counts_as_captured():
    """a bitmap registered from straight texels: convolved, it is a new generation without straight texels"""
    w, h = 40, 24
    r = dr.handle(w, h)
    try:
        rgba = np.random.default_rng(5).integers(0, 256, (h, w, 4), dtype=np.uint8)
        r.register_bitmap(BITMAP, w, h, rgba.tobytes())
        draw = {"children": [_whole_frame_bitmap(w, h, BITMAP)]}
        r.render(draw)
        texels = r.read_image(premultiplied=True)
        stage = {"children": [dict(draw["children"][0], color_transform={"red_mult": 0.5})]}
        r.render(stage)                                               # fine while the bitmap is as registered
        r.convolve_bitmap(BITMAP, cm.GAUSS5)
        with pytest.raises(api.SwfrError) as e:
            r.render(stage)
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedCapturedBitmapTransform" in str(e.value)
        r.render(draw)
        assert diff_stats(r.read_image(premultiplied=True), cm.convolve(texels, cm.GAUSS5)) == (0, 0)
    finally:
        r.close()


# ---- 2. the chain inside render
INNER = dict(GLOW, inner=True)
LISTS = {
    "alone_sharpen": [Cv(cm.SHARPEN)],
    "alone_even_4x6": [Cv(cm.EVEN_4X6)],
    "alone_7x7": [Cv(cm.random_kernel(np.random.default_rng(77), 7, 7))],
    "after_blur_odd": [fsc.BLUR_ODD, Cv(cm.EMBOSS)],
    "after_blur_even": [fsc.BLUR_EVEN, Cv(cm.EMBOSS)],
    "before_drop": [Cv(cm.EDGE), fm.shadow(DROP)],
    "after_drop": [fm.shadow(DROP), Cv(cm.EDGE)],
    "before_inner": [Cv(cm.SHARPEN), {"shadow": INNER}],
    "after_inner": [{"shadow": INNER}, Cv(cm.SHARPEN)],
    "two_in_a_row": [Cv(cm.EVEN_2X2), Cv(cm.MOTION_7X1)],
    "two_after_blur_odd": [fsc.BLUR_ODD, Cv(cm.MOTION_1X7), Cv(cm.BOX3)],
    "four": [Cv(cm.EMBOSS), fm.shadow(GLOW, knockout=True), Cv(cm.GAUSS5), fsc.BLUR_ODD],
    "four_convolution_last": [fsc.BLUR_EVEN, fm.shadow(DROP), fsc.BLUR_ODD, Cv(cm.SHARPEN)],
}


@pytest.mark.parametrize("size", CHAIN_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_chain_inside_render_against_the_model(size):
    w, h = size
    r = dr.handle(w, h)
    try:
        kids = _content(w, h)
        r.render({"children": kids})
        G = r.read_image(premultiplied=True)
        assert len(np.unique(G[..., 3])) > 8 and (G[..., 3] == 0).any(), "the group holds many alphas, and clear pixels"
        for name, chain in sorted(LISTS.items()):
            r.render({"children": [{"type": "container", "children": kids, "filters": chain}]})
            dr.not_refused(r, name)
            assert r.built_filters() == [cm.as_dicts(chain)]
            want = cm.apply(G, chain)
            n, mx = diff_stats(r.read_image(premultiplied=True), want)
            print("convolution %dx%d %s: differing pixels %d max %d" % (w, h, name, n, mx))
            assert (n, mx) == (0, 0), (size, name)
            assert (want != G).any(), name
    finally:
        r.close()


# ---- 3. the goldens of libcairo + pixman
@pytest.mark.parametrize("fname", sorted(csc.files()))
def test_goldens_through_render(fname):
    assert all(sc["width"] <= 96 and sc["height"] <= 64 for sc in csc.files()[fname][0]().values())
    dr.goldens_through_render_and_resident(FAMILY, fname)


# ---- 4. a caller-owned target that is word aligned only
@pytest.mark.parametrize("offset", (4, 12))
def test_first_entry_on_a_handle_with_an_unaligned_target(offset):
    for w, h in ((2 * T_W + 4, T_H + 1), (13, 11)):                  # (a width that is a multiple of four: only the base keeps the quads out)
        kids = _content(w, h)
        G = dr.through_render(dict(width=w, height=h, stage={"children": kids}))
        g = GuardedFrames(1, h, w, offset=offset)
        r = dr.handle(w, h)
        try:
            r.set_targets(g.addresses())
            for name in ("alone_sharpen", "alone_even_4x6", "before_drop", "two_in_a_row"):
                chain = LISTS[name]
                g.refill()
                r.render({"children": [{"type": "container", "children": kids, "filters": chain}]})
                dr.not_refused(r, name)
                want = cm.apply(G, chain)
                frames = g.guards_intact()
                dr.zero(frames[0], want, (name, offset, "the caller's buffer"))
                dr.zero(r.read_image(premultiplied=True), want, (name, offset, "read_image"))
            # the target as the source of a capture, convolved and drawn 1 : 1 into the target again
            r.render({"children": kids})
            r.capture_bitmap(BITMAP)
            r.convolve_bitmap(BITMAP, cm.EMBOSS)
            g.refill()
            r.render({"children": [_whole_frame_bitmap(w, h, BITMAP)]})
            dr.zero(g.guards_intact()[0], cm.convolve(G, cm.EMBOSS), ("convolve_bitmap", offset))
        finally:
            r.close()


# ---- 5. the routes not taken refuse by name
def test_refused_routes_and_the_handle_afterwards():
    sc = csc.structure_scenes()["multiply_opaque_ground"]
    plain = dict(sc, stage={"children": csc.without_filters(sc["stage"]["children"])})
    dr.refused_routes(FAMILY, sc, plain, np.load(csc.golden_path("cairo_convolution_structure"))["multiply_opaque_ground"], dr.through_render(plain))


# ---- 6. the slot is read at the walk
def test_the_slots_kernel_at_the_walk_is_the_kernel():
    """a kernel slot set anew through set_kernel changes the next walk only"""
    sc = csc.kernel_scenes()["sharpen"]
    gold = np.load(csc.golden_path("cairo_convolution_kernels"))
    r = dr.renderer_for(sc, False)
    try:
        r.render(sc["stage"])                                         # (render assigns kernel slot 0 to the stage's one kernel)
        assert diff_stats(r.read_image(premultiplied=True), gold["sharpen"]) == (0, 0)
        r.set_kernel(0, cm.EDGE)
        r.render_resident(1)
        assert diff_stats(r.read_image(premultiplied=True), gold["sharpen"]) == (0, 0)
        assert r.built_filters() == [cm.as_dicts([Cv(cm.SHARPEN)])]
        r.render(csc.kernel_scenes()["edge"]["stage"])
        assert diff_stats(r.read_image(premultiplied=True), gold["edge"]) == (0, 0)
        assert r.built_filters() == [cm.as_dicts([Cv(cm.EDGE)])]
    finally:
        r.close()
