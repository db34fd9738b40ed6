"""Bitmap and gradient sources under compositing (the transposed bilinear fetch of blend8, blend8_op's per-pixel shading, group
set-aside, the mask multiply of k2_tiles<5> and the fade of k2_tiles<6> with shaded members) against tests/frame_model.py on random
frames: every comparison is zero differing bytes.  Runs on an MI355X (-m gpu) and, with smaller counts, under tools/emu/run.py.

a. Display trees of tests/composite_scenes.py's rand_composited_scene(shaded=True) -- two leaves in five a bitmap fill (three edge
   rules, magnified and minified, translucent and alpha-0 texels registered as straight RGBA) or a radial / focal gradient (three
   spreads) -- through render, swfr_render_edges + resident frames, SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and
   render_batch with a shaded tree, a solid tree and an empty stage in one launch; both antialias modes.
b. Raw frames of 130 x 21 and 70 x 13 (composite_scenes.shaded_frames): one member of each class of SHADED_CLASSES -- each aimed at
   one branch of the bitmap fetch -- unblended, with the lerp bit as a first paint and under each of the eight operators; alone, in
   a group, as the content and as the mask of a masked group, in a group faded at opacity 1, 128 and 254, and two groups deep; behind
   0, 15, 16 and 17 plain entries.  The same frames without their markers through the blend instance, every frame forced through
   the heavier instances that can draw it, and through two band handles.  A lerp-bit bitmap path whose rectangle is clear in a
   painted strip (lerp_beside_painted_frame) and strips one texel column short of the all-inside shortcut (last_column_frame).
c. tests/test_shaded_frame_model.py (no GPU) asserts from the model's sample positions that these frames reach every branch
   (composite_scenes.shaded_reach); after every frame the handle's swfr_stats show no capacity refusal.

Observed on an MI355X: 31 passed, every comparison 0 differing bytes, 13 s (tests/test_composite_fuzz_gpu.py and tests/test_pad_gpu.py
beside it: 143 passed, 33 s).  DESIGN.md, section 5 ("The frame model", "Shaded sources"), has the table of kernel mutations this file
catches.
"""
import numpy as np
import pytest

import composite_scenes as cs
import frame_model as fm
from device_routes import EMU, handle, not_refused, through_edges, through_render, two_bands, zero
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from host_frames import bitmaps_of, build_on_host

pytestmark = pytest.mark.gpu


def _want(sc, aliased):
    arrays = build_on_host(sc, aliased)
    return arrays, fm.render(*arrays, sc["width"], sc["height"], aliased=aliased, bitmaps=bitmaps_of(sc))


# ---------------------------------------------------------------------------------------------------------------- a. display trees
@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_shaded_stage_fuzz_through_render(aliased):
    for seed in range(3 if EMU else 24):
        sc = cs.rand_composited_scene(np.random.default_rng(8000 + seed + 100 * aliased), shaded=True)
        zero(through_render(sc, aliased), _want(sc, aliased)[1], ("render", aliased, seed))


@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_shaded_stage_fuzz_through_render_edges_and_resident_frames(aliased):
    for seed in range(2 if EMU else 12):
        sc = cs.rand_composited_scene(np.random.default_rng(8300 + seed), shaded=True)
        arrays, want = _want(sc, aliased)
        zero(through_edges(sc["width"], sc["height"], arrays, aliased, resident=3, bitmaps=sc["raw_bitmaps"]), want, ("render_edges", aliased, seed))


def test_shaded_stage_fuzz_with_graphs(monkeypatch):
    monkeypatch.setenv("SWFR_GRAPHS", "1")
    for seed in range(2 if EMU else 8):
        aliased = bool(seed % 2)
        sc = cs.rand_composited_scene(np.random.default_rng(8400 + seed), shaded=True)
        arrays, want = _want(sc, aliased)
        zero(through_edges(sc["width"], sc["height"], arrays, aliased, resident=3, bitmaps=sc["raw_bitmaps"]), want, ("graphs", aliased, seed))


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "interleaved"])
def test_shaded_stage_fuzz_through_two_band_handles(contiguous):
    for seed in range(2 if EMU else 8):
        aliased = bool(seed % 2)
        sc = cs.rand_composited_scene(np.random.default_rng(8500 + seed), height=int(16 * (2 + seed % 4) + 1 + seed), shaded=True)
        got = two_bands(sc["width"], sc["height"], contiguous, lambda r: r.render(sc["stage"]), aliased, bitmaps=sc["raw_bitmaps"])
        zero(got, _want(sc, aliased)[1], ("bands", contiguous, aliased, seed))


@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_shaded_stage_fuzz_through_render_batch_with_unlike_frames(aliased):
    """shaded trees, a solid tree and an empty stage of one size as ONE batch: into a device tensor where there is a device for it (every frame checked), and by the per-frame route"""
    W, H = 150, 90
    rng = np.random.default_rng(8600)
    first = cs.rand_composited_scene(rng, width=W, height=H, leaves=14, shaded=True)
    frames = [first]
    for k in range(2 if EMU else 6):
        if k % 3 == 0:
            frames.append(cs.rand_composited_scene(rng, width=W, height=H, leaves=14))
        if k % 3 == 1:
            frames.append(dict(width=W, height=H, stage={"children": []}))
        sc = cs.rand_composited_scene(rng, width=W, height=H, leaves=14, shaded=True)
        frames.append(sc)
    frames = [dict(sc, raw_bitmaps=first["raw_bitmaps"]) for sc in frames]       # (one handle: the ids of every tree name the first one's texels)
    wants = [_want(sc, aliased)[1] for sc in frames]
    stages = [sc["stage"] for sc in frames]
    r = handle(W, H, aliased, first["raw_bitmaps"])
    try:
        if not EMU:                                               # (device tensors need the GPU)
            import torch
            out = torch.zeros((len(stages), H, W, 4), dtype=torch.uint8, device="cuda")
            r.render_batch(stages, out.data_ptr(), H * W * 4)
            got = out.cpu().numpy()
            for k, want in enumerate(wants):
                zero(got[k], want, ("batch", aliased, k))
        for cut in sorted({1, 2, len(frames) // 2, len(frames)}):
            r.render_batch(stages[:cut])
            zero(r.read_image(premultiplied=True), wants[cut - 1], ("per-frame route", aliased, cut))
        not_refused(r, "batch")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- b. raw frames
def _lowest_instance(label):
    """the lightest k2_tiles instance that draws the frame (SWFR_TILES_SHADERS is a floor: a lighter one changes nothing).  The solid
    path on top of every frame carries an operator, so it is the blend instance at the least"""
    setting = label[2]
    return 6 if setting.startswith("fade") else (5 if setting in ("mask", "mask_content") else (4 if setting in ("group", "nested") else 3))


@pytest.mark.parametrize("cls", cs.SHADED_CLASSES)
def test_shaded_members_in_every_setting(cls, monkeypatch):
    """every frame as the instance picked for it draws it and forced through each heavier one; without its markers through the blend
    instance"""
    for n, (label, fr) in enumerate(cs.shaded_frames(cls)):
        if EMU and n % 9:
            continue
        arrays, texels = fr.arrays(), fr.model_bitmaps()
        want = fm.render(*arrays, fr.W, fr.H, bitmaps=texels)
        monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
        zero(through_edges(fr.W, fr.H, arrays, bitmaps=fr.bitmaps), want, (label, "picked"))
        for forced in range(_lowest_instance(label) + 1, 7):
            if EMU and forced % 3 != n % 3:
                continue
            monkeypatch.setenv("SWFR_TILES_SHADERS", str(forced))
            zero(through_edges(fr.W, fr.H, arrays, bitmaps=fr.bitmaps), want, (label, "instance", forced))
        monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
        if label[1] != "lerp":                                       # (without the group around it a lerp-bit member is no first paint)
            plain = cs.without_markers(*arrays)
            zero(through_edges(fr.W, fr.H, plain, bitmaps=fr.bitmaps), fm.render(*plain, fr.W, fr.H, bitmaps=texels), (label, "markerless"))


@pytest.mark.parametrize("instance", ["1", "2", "3", "4", "5", "6"])
def test_plain_bitmap_frames_through_every_instance(instance, monkeypatch):
    """a bitmap member alone on a clear frame, unblended and as a lerp-bit first paint: every instance from 1 up can draw it"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)
    for ci, cls in enumerate(cs.SHADED_CLASSES[:-1]):
        for mode in ("plain", "lerp"):
            size, strips = cs.SHADED_SIZES[ci % 2]
            fr = cs.shaded_frame(cls, mode, "alone", 0, size, strips[ci % len(strips)], 7900 + ci)
            arrays = fr.arrays()
            paths = arrays[1].copy()
            paths["lerp"][1:] &= 1                                    # (the solid path on top without its operator: no operator table)
            arrays = (arrays[0], paths, arrays[2])
            zero(through_edges(fr.W, fr.H, arrays, bitmaps=fr.bitmaps), fm.render(*arrays, fr.W, fr.H, bitmaps=fr.model_bitmaps()), (cls, mode, "instance", instance))


@pytest.mark.parametrize("instance", ["1", "3", "4", "6"])
def test_lerp_bit_first_paint_beside_painted_pixels(instance, monkeypatch):
    """the lerp bit on a bitmap path whose rectangle is clear while its strip is not (composite_scenes.lerp_beside_painted_frame)"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)
    for seed in range(4 if EMU else 12):
        fr = cs.lerp_beside_painted_frame(seed)
        arrays = fr.arrays()
        zero(through_edges(fr.W, fr.H, arrays, bitmaps=fr.bitmaps), fm.render(*arrays, fr.W, fr.H, bitmaps=fr.model_bitmaps()), ("lerp beside", seed, instance))


@pytest.mark.parametrize("instance", ["1", "4"])
def test_one_column_short_of_the_inside_shortcut(instance, monkeypatch):
    """the left taps of a strip's samples reach the bitmap's last column (composite_scenes.last_column_frame): the general fetch, whose
    right taps wrap, clamp or read transparent black -- an `inside` test that let the last column in would read the next row"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)
    for seed in range(6 if EMU else 12):
        fr = cs.last_column_frame(seed)[0]
        arrays = fr.arrays()
        zero(through_edges(fr.W, fr.H, arrays, bitmaps=fr.bitmaps), fm.render(*arrays, fr.W, fr.H, bitmaps=fr.model_bitmaps()), ("last column", seed, instance))


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "interleaved"])
def test_shaded_members_through_two_band_handles(contiguous):
    for ci, cls in enumerate(cs.SHADED_CLASSES):
        for n, (label, fr) in enumerate(cs.shaded_frames(cls)):
            if n % (40 if EMU else 7) != ci % 7 or fr.H < 17:        # (two tile rows: one per handle)
                continue
            arrays = fr.arrays()
            got = two_bands(fr.W, fr.H, contiguous, lambda r: r.render_edges(*arrays), bitmaps=fr.bitmaps)
            zero(got, fm.render(*arrays, fr.W, fr.H, bitmaps=fr.model_bitmaps()), (label, "bands", contiguous))
