"""The blend and layer instances of the tile kernel (k2_tiles<3>, k2_tiles<4>) against tests/frame_model.py on random frames: every
comparison is zero differing bytes.  Runs on an MI355X (-m gpu) and, with smaller counts, under tools/emu/run.py.

a. Display trees of tests/composite_scenes.py's rand_composited_scene through render, swfr_render_edges + resident frames,
   SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and render_batch with unlike frames in one launch; both antialias
   modes, the narrow and the wide row kernel, one 4K frame.
b. Frames written directly as swfr_upload_edges arrays, aimed at the walk of one strip's list: one group of N members behind k plain
   entries, so that BEGIN, the first member and END fall on either side of a 16-entry staging round, a 64-entry class-byte chunk and
   the 128 prefetched class bytes; members of every class and operator; nesting one to four deep with the strip's first path at every
   level, ENDs of levels never set aside, sibling groups, groups present by their rectangle alone; opaque covers around and inside
   groups; frame edges and band boundaries; the same frames without their markers (the blend instance, operators at list positions
   past 16, 64 and 128), and those forced through the layer instance; several thousand groups in one frame; one frame at 4K.
c. test_the_raw_corpus_reaches_what_it_claims computes from the arrays what the strips of these frames see (composite_scenes.
   strip_reach) and asserts it; after every frame the handle's swfr_stats show no capacity refusal.

Observed on an MI355X: 66 passed, every comparison 0 differing bytes, 32 s (tests/test_layer_gpu.py beside it: 41 s).  DESIGN.md,
section 5 ("The frame model"), has the table of kernel mutations this file catches.
"""
import numpy as np
import pytest

import composite_scenes as cs
import frame_model as fm
import helpers
from device_routes import EMU, handle, not_refused, through_edges, through_render, two_bands, zero
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from host_frames import build_on_host

pytestmark = pytest.mark.gpu
GROUP_SIZES, NESTINGS = cs.GROUP_SIZES, cs.NESTINGS


# ---------------------------------------------------------------------------------------------------------------- a. display trees
@pytest.mark.parametrize("rows", ["narrow", "wide"])
@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_stage_fuzz_through_render(aliased, rows, monkeypatch):
    if rows == "wide":
        monkeypatch.setenv("SWFR_ROWS_WIDE", "1")
    else:
        monkeypatch.delenv("SWFR_ROWS_WIDE", raising=False)
    for seed in range(3 if EMU else 24):
        sc = cs.rand_composited_scene(np.random.default_rng(5000 + seed + 100 * aliased))
        want = fm.render(*build_on_host(sc, aliased), sc["width"], sc["height"], aliased=aliased)
        zero(through_render(sc, aliased), want, ("render", aliased, rows, seed))


@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_stage_fuzz_through_render_edges_and_resident_frames(aliased):
    for seed in range(2 if EMU else 12):
        sc = cs.rand_composited_scene(np.random.default_rng(5300 + seed))
        arrays = build_on_host(sc, aliased)
        want = fm.render(*arrays, sc["width"], sc["height"], aliased=aliased)
        zero(through_edges(sc["width"], sc["height"], arrays, aliased, resident=3), want, ("render_edges", aliased, seed))


def test_stage_fuzz_with_graphs(monkeypatch):
    monkeypatch.setenv("SWFR_GRAPHS", "1")
    for seed in range(2 if EMU else 8):
        aliased = bool(seed % 2)
        sc = cs.rand_composited_scene(np.random.default_rng(5400 + seed))
        arrays = build_on_host(sc, aliased)
        want = fm.render(*arrays, sc["width"], sc["height"], aliased=aliased)
        zero(through_edges(sc["width"], sc["height"], arrays, aliased, resident=3), want, ("graphs", aliased, seed))


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "interleaved"])
def test_stage_fuzz_through_two_band_handles(contiguous):
    for seed in range(2 if EMU else 8):
        aliased = bool(seed % 2)
        sc = cs.rand_composited_scene(np.random.default_rng(5500 + seed), height=int(16 * (2 + seed % 4) + 1 + seed))
        want = fm.render(*build_on_host(sc, aliased), sc["width"], sc["height"], aliased=aliased)
        got = two_bands(sc["width"], sc["height"], contiguous, lambda r: r.render(sc["stage"]), aliased)
        zero(got, want, ("bands", contiguous, aliased, seed))


@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_stage_fuzz_through_render_batch_with_unlike_frames(aliased):
    """composited trees, a plain polygon frame (no operator table), an empty stage and a blend-only frame of one size as ONE batch: one
    launch of the layer instance.  Into a device tensor where there is a device for it (every frame checked), and by the per-frame route."""
    W, H = 150, 90
    rng = np.random.default_rng(5600)
    frames = []
    for k in range(3 if EMU else 9):
        frames.append(cs.rand_composited_scene(rng, width=W, height=H, leaves=14))
        if k % 3 == 0:
            frames.append(helpers.rand_layered_translucent_scene(rng))
        if k % 3 == 1:
            frames.append(dict(width=W, height=H, stage={"children": []}))
        if k % 3 == 2:
            sc = helpers.rand_layered_translucent_scene(rng)
            frames.append(dict(sc, stage={"children": [dict(kid, blend_mode=cs.MODES[1 + i % 8]) if i else kid for i, kid in enumerate(sc["stage"]["children"])]}))
    wants = [fm.render(*build_on_host(sc, aliased), W, H, aliased=aliased) for sc in frames]
    stages = [sc["stage"] for sc in frames]
    r = handle(W, H, aliased)
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


def test_stage_fuzz_one_4k_frame():
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    sc = cs.rand_composited_scene(np.random.default_rng(5700), width=3840, height=2160, leaves=24)
    want = fm.render(*build_on_host(sc), 3840, 2160)
    zero(through_render(sc), want, "4K stage")


# ---------------------------------------------------------------------------------------------------------------- b. raw frames
def _check_raw(fr, msg, monkeypatch, also_markerless=True, **kw):
    """the frame through the layer instance; without its markers through the blend instance, and that one forced through the layer
    instance (SWFR_TILES_SHADERS is read when the handle is created)"""
    arrays = fr.arrays()
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    zero(through_edges(fr.W, fr.H, arrays, **kw), fm.render(*arrays, fr.W, fr.H), (msg, "groups"))
    if also_markerless:
        plain = cs.without_markers(*arrays)
        want = fm.render(*plain, fr.W, fr.H)
        zero(through_edges(fr.W, fr.H, plain, **kw), want, (msg, "markerless"))
        monkeypatch.setenv("SWFR_TILES_SHADERS", "4")
        zero(through_edges(fr.W, fr.H, plain, **kw), want, (msg, "markerless, instance 4"))
        monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)


@pytest.mark.parametrize("n", GROUP_SIZES)
def test_group_sizes_across_staging_boundaries(n, monkeypatch):
    for k, fr in cs.group_size_frames(n):
        if EMU and k not in (0, 1, 2, 15, 16, 17):
            continue
        _check_raw(fr, ("group of", n, "behind", k), monkeypatch, also_markerless=not EMU or k in (0, 16))


def test_begin_across_chunk_boundaries(monkeypatch):
    for k, fr in cs.late_group_frames():
        _check_raw(fr, ("group of", 5 + k % 3, "behind", k), monkeypatch, also_markerless=False)


@pytest.mark.parametrize("op", cs.MODES)
def test_every_operator_on_members_and_end(op, monkeypatch):
    """one operator on every member and on END, every member class, the group longer than a staging round"""
    rng = np.random.default_rng(6500 + cs.MODES.index(op))
    fr = cs.RawFrame(70, 13)
    cs.add_member(fr, rng, "partial", "normal", 0, 0, first=True)
    cs.add_member(fr, rng, "full_translucent", "normal", 0, 0)
    fr.begin()
    for i in range(20):
        cs.add_member(fr, rng, cs.MEMBER_CLASSES[i % 6], op, 0, 0, first=i == 0)
    fr.end(op)
    cs.add_member(fr, rng, "partial", op, 0, 0)
    _check_raw(fr, ("operator", op), monkeypatch)


@pytest.mark.parametrize("first_level,depth", NESTINGS)
def test_lazy_set_aside_at_every_level(first_level, depth, monkeypatch):
    _check_raw(cs.raw_nesting_frame(first_level, depth), ("nesting", first_level, depth), monkeypatch)


def test_random_nesting_and_frame_edges(monkeypatch):
    for seed, fr in cs.nested_frames(4 if EMU else cs.NESTED_SEEDS):
        _check_raw(fr, ("random nesting", seed, fr.W, fr.H), monkeypatch, also_markerless=seed % 2 == 0)


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "interleaved"])
def test_groups_across_tile_rows_and_band_boundaries(contiguous):
    for seed in range(2 if EMU else 10):
        W, H = ((203, 45), (130, 37), (70, 77))[seed % 3]
        fr = cs.rand_raw_nested_frame(np.random.default_rng(6800 + seed), W=W, H=H, items=50, member_size=(10, 70))
        arrays = fr.arrays()
        got = two_bands(W, H, contiguous, lambda r: r.render_edges(*arrays))
        zero(got, fm.render(*arrays, W, H), ("raw bands", contiguous, seed))


@pytest.mark.parametrize("kind", ["tor", "box"])
@pytest.mark.parametrize("place", cs.COVER_PLACES)
def test_opaque_covers_around_and_inside_groups(place, kind, monkeypatch):
    for seed in range(1 if EMU else 3):
        _check_raw(cs.raw_cover_frame(place, kind, seed=seed), ("cover", place, kind, seed), monkeypatch)


def test_several_thousand_groups(monkeypatch):
    fr = cs.raw_many_groups_frame(np.random.default_rng(6900), *((260, 120, 300) if EMU else (1000, 520, 3000)))
    _check_raw(fr, "many groups", monkeypatch)


def test_random_nesting_at_4k(monkeypatch):
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    fr = cs.rand_raw_nested_frame(np.random.default_rng(6950), W=3840, H=2160, items=2500, member_size=(10, 300), cover_chance=0.002, spread=500)
    _check_raw(fr, "4K nesting", monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- c. reach
def test_the_raw_corpus_reaches_what_it_claims():
    cs.assert_reach(cs.raw_corpus_reach())
