"""Rendering into caller-owned device memory at every word alignment (swfr_set_targets, swfr_render_resident_async[_to],
swfr_render_resident_group_to, swfr_render_batch with a destination): what the multi-GPU pipelines of swf_renderer_amd/distributed.py do.

A handle's own framebuffer is 256-byte aligned and zero-filled; a caller's need be neither.  Every target here is a
tests/device_routes.py GuardedFrames: frames at 0, 4, 8 or 12 bytes modulo 16 inside one allocation of 0xA5 bytes, so that a pixel left
unwritten, a row that is not the handle's own and a store that runs past the frame all show.  The expected bytes never come from the
device: the CPU oracle, a committed libcairo golden (tests/caller_target_scenes.py), or the numpy models of the filters over a group
picture that is itself held against the oracle.  Every scene has clear pixels; every comparison is zero differing bytes.

1. the store epilogue of k2_tiles (raster2.hip, vec_ok): a target that is not 16-byte aligned takes the per-pixel stores in every
   strip, whole interior ones too, also where (width & 3) == 0 -- through every tile instance, both row kernels, an aliased handle,
   and the layer, mask, fade and bitmap instances with group and bitmap content;
2. filtered layers on such a handle: the first entry of a filter list reads the target, and the finish passes go word by word over
   the whole image (shadow_quads() == 0) in k_shadow_finish_fb and k_shadow_inner_fb; capture, shadow and blur of a bitmap from it;
3. swfr_render_batch into an offset destination with a stride that rotates the alignment, grouped and per frame;
4. several targets in rotation, back to the handle's own buffer, band handles that write their own rows only, block targets;
5. an address or stride that is no multiple of four is refused by name before anything is launched.
Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import numpy as np
import pytest

import blend_scenes as bs
import blur_model
import caller_target_scenes as cts
import device_routes as dr
import frame_model
import inner_model as im
import inner_scenes as isc
import filter_model as fm
import filter_scenes as fsc
import pad_scenes
import test_gpu_batches as tb
import test_shadow_gpu as tsh
from device_routes import GuardedFrames, SENTINEL, need_gpu  # noqa: F401 (need_gpu: the module's autouse fixture)
from helpers import oracle_render
from swf_renderer_amd import api, distributed as D

pytestmark = pytest.mark.gpu

OFFSETS = (0, 4, 8, 12)                                # 0: the control, the 16-byte stores
# raster2.hip: TILE_W 64, STRIP_H 8, TILE_H 16.  64 x 8: one strip, wholly inside.  192 x 24: three tile columns, interior strips, a
# half tile row at the bottom (y >= height in the second row group).  132 x 20: (width & 3) == 0 with a partial last tile column -- at
# offset 0 the clipped path's 16-byte store, else its per-pixel one.  130 x 20: no 16-byte store at any offset
SIZES = ((64, 8), (192, 24), (132, 20), (130, 20))
FAMILIES = dict(dr.FAMILIES, pad=dr.Family("pad", pad_scenes, "1", True, (True, False)))


def _solid_scene(w, h):
    """translucent and opaque polygons across all four edges of a w x h frame, clear pixels between and around them"""
    kids = [bs._shape([(-3, -2), (0.45 * w, -4), (0.3 * w, 0.7 * h), (-5, 0.55 * h)], (200, 40, 30, 255)),       # left and top edge
            bs._shape([(0.6 * w, 0.35 * h), (w + 6, 0.2 * h), (w + 3, h + 4), (0.7 * w, h + 2)], (20, 90, 220, 140)),  # right and bottom
            bs._shape([(0.2 * w, 0.5 * h), (0.8 * w, 0.1 * h), (0.55 * w, h + 5)], (30, 200, 60, 90)),            # bottom edge, over both
            bs._rect(w - 1.5, -1, w + 2, 0.3 * h, (255, 255, 255, 255)),                                            # the last column
            bs._shape([(0.35 * w, -3), (0.5 * w, 0.4 * h), (0.62 * w, -1)], (240, 200, 10, 201))]                  # top edge
    return dict(width=w, height=h, exact=True, stage={"children": kids})


_ORACLE = {}


def _want(sc, key, edges=True):
    """the oracle's frame of a scene, computed once per module; it has clear pixels and (`edges`) covered ones in its first and last
    row and column"""
    if key not in _ORACLE:
        img = oracle_render(sc)
        a = img[..., 3]
        assert (a == 0).any() and (not edges or (a[0].any() and a[-1].any() and a[:, 0].any() and a[:, -1].any())), key
        img.setflags(write=False)
        _ORACLE[key] = img
    return _ORACLE[key]


def _device_framebuffer(r):
    return r.L.swfr_device_framebuffer(r.h)


def _frame_in_target(r, g, want, msg, k=0):
    """target k holds `want` and nothing around it was touched; read_image() and swfr_device_framebuffer() are that target"""
    frames = g.guards_intact()
    dr.zero(frames[k], want, (msg, "the caller's buffer"))
    dr.zero(r.read_image(premultiplied=True), want, (msg, "read_image"))
    assert _device_framebuffer(r) == g.address(k), msg


def _render_into(sc, want, offset, msg, aliased=False, resident=3):
    w, h = sc["width"], sc["height"]
    g = GuardedFrames(1, h, w, offset=offset)
    r = dr.renderer_for(sc, aliased)
    try:
        r.set_targets(g.addresses())
        r.render(sc["stage"])
        dr.not_refused(r, msg)
        _frame_in_target(r, g, want, msg)
        g.refill()                                                   # (every resident frame writes every pixel again)
        r.render_resident(resident)
        _frame_in_target(r, g, want, (msg, "resident"))
    finally:
        r.close()


def _no_knobs(monkeypatch, **env):
    for k in ("SWFR_BATCH_FRAMES", "SWFR_FRAMES_IN_FLIGHT", "SWFR_ROWS_WIDE", "SWFR_TILES_SHADERS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


# ---- 1. the tile epilogue
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_solid_frame_into_a_target_at_every_alignment(size, offset, monkeypatch):
    _no_knobs(monkeypatch)
    sc = _solid_scene(*size)
    _render_into(sc, _want(sc, size), offset, (size, offset))


@pytest.mark.parametrize("rows", ("narrow", "wide"))
@pytest.mark.parametrize("instance", range(8))
def test_every_tile_instance_stores_per_pixel_into_an_unaligned_target(instance, rows, monkeypatch):
    _no_knobs(monkeypatch, SWFR_TILES_SHADERS=instance, **({"SWFR_ROWS_WIDE": 1} if rows == "wide" else {}))
    sc = _solid_scene(192, 24)
    _render_into(sc, _want(sc, (192, 24)), 4, ("instance", instance, rows))


def test_aliased_handle_into_an_unaligned_target(monkeypatch):
    """the aliased rule has no oracle: tests/frame_model.py, its exact model over the frame builder's arrays (tests/test_frame_model.py)"""
    _no_knobs(monkeypatch)
    sc = _solid_scene(132, 20)
    want = frame_model.render(*dr.built_for_another_handle(sc, True), 132, 20, aliased=True)
    assert (want[..., 3] == 0).any() and (want[..., 3] == 255).any()
    _render_into(sc, want, 4, "aliased", aliased=True)


@pytest.mark.parametrize("offset", (4, 12))
@pytest.mark.parametrize("family", sorted(cts.PICKS))
def test_golden_scene_of_a_family_into_an_unaligned_target(family, offset, monkeypatch):
    """the layer, mask, fade and bitmap instances of k2_tiles, picked by the scene itself: group and bitmap content at 192 x 24"""
    _no_knobs(monkeypatch)
    _, _, fname, name = cts.PICKS[family]
    items, aliased, _ = dr.golden_scenes(FAMILIES[family], fname, 4, thin=False)
    sc = cts.reframed(dict(items)[name])
    want = np.load(cts.GOLDEN)[family]
    assert not aliased and (sc["width"], sc["height"]) == (192, 24) == want.shape[1::-1] and (want[..., 3] == 0).any()
    _render_into(sc, want, offset, (family, name, offset))


# ---- 2. filtered layers on a handle with an unaligned target
E = isc.E
CHAINS = {"drop": [E["drop"]], "drop_knockout": [fm.shadow(fsc.DROP, knockout=True)], "drop_hide_object": [fsc.ENTRIES["hdrop"]],
          "inner": [E["inner"]], "inner_knockout": [fm.shadow(isc.INNER, knockout=True)], "blur": [E["blur"]],
          "inner_blur_odd_drop": [E["inner"], E["blur_odd"], E["drop"]], "blur_odd_inner": [E["blur_odd"], E["inner"]]}
# shadow_passes.hip: with quads == 0 the finish grid is shadow_blocks(n, 0), at most 2048 workgroups of 256 lanes = 524 288 words a
# stride: 1024 x 513 = 525 312 words is the smallest frame whose whole-image word loop runs a second, partial time.  13 x 11 is one
# workgroup, 257 x 3 a few
WORD_LOOP_TWICE = (1024, 513)
FILTER_SIZES = ((13, 11), (257, 3)) + (() if dr.EMU else (WORD_LOOP_TWICE,))
SRC, DST = 7, 9


def _group(w, h):
    """(the children, their plain frame G): rendered on an ordinary handle, and the oracle's frame"""
    kids = tsh._content(w, h)
    sc = dict(width=w, height=h, exact=True, stage={"children": kids})
    want = _want(sc, ("content", w, h), edges=False)
    dr.zero(dr.through_render(sc), want, ("the group on an ordinary handle", w, h))
    assert len(np.unique(want[..., 3])) > 8
    return kids, want


@pytest.mark.parametrize("offset", (4, 12))
@pytest.mark.parametrize("size", FILTER_SIZES, ids=lambda s: "%dx%d" % s)
def test_filtered_layers_into_an_unaligned_target(size, offset, monkeypatch):
    _no_knobs(monkeypatch)
    w, h = size
    kids, G = _group(w, h)
    chains = CHAINS if size != WORD_LOOP_TWICE else {k: CHAINS[k] for k in ("drop", "inner")}      # (the two _fb kernels)
    g = GuardedFrames(1, h, w, offset=offset)
    r = dr.handle(w, h)
    try:
        r.set_targets(g.addresses())
        changed = False                                              # (a 3-row frame has no room for the drop shadow's offset: not every chain shows)
        for name, chain in sorted(chains.items()):
            g.refill()
            r.render({"children": [{"type": "container", "children": kids, "filters": chain}]})
            dr.not_refused(r, name)
            assert r.built_filters() == [im.as_dicts(chain)]
            want = im.apply(G, chain)
            changed = changed or bool((want != G).any())
            _frame_in_target(r, g, want, ("filters", size, offset, name))
        assert changed, "some chain changes the group"
        if size == WORD_LOOP_TWICE:
            return
        # the target as the source of a capture; the capture's shadow, inner shadow and blur, drawn 1 : 1 into the target again
        r.render({"children": kids})
        _frame_in_target(r, g, G, ("plain", size, offset))
        r.capture_bitmap(SRC)
        draw = {"children": [tsh._whole_frame_bitmap(w, h, DST)]}
        for sh in (fsc.DROP, dict(isc.INNER, knockout=True)):
            r.shadow_bitmap(DST, SRC, sh)
            r.render(draw)
            _frame_in_target(r, g, im.shadow(G, sh), ("shadow_bitmap", size, offset, sorted(sh)))
        r.blur_bitmap(SRC, 3, 2, 2)
        r.render({"children": [tsh._whole_frame_bitmap(w, h, SRC)]})
        _frame_in_target(r, g, blur_model.blur(G, 3, 2, 2), ("blur_bitmap", size, offset))
        # nothing of it stays behind: a plain frame, and resident frames of it
        g.refill()
        r.render({"children": kids})
        _frame_in_target(r, g, G, ("plain after filters", size, offset))
        g.refill()
        r.render_resident(3)
        _frame_in_target(r, g, G, ("plain after filters, resident", size, offset))
    finally:
        r.close()


# ---- 3. render_batch into an offset destination whose stride rotates the alignment
@pytest.mark.parametrize("route", ("grouped", "per_frame"))
def test_render_batch_into_an_offset_destination_with_a_rotating_stride(route, monkeypatch):
    _no_knobs(monkeypatch, **({"SWFR_BATCH_FRAMES": 3} if route == "grouped" else {"SWFR_BATCH_FRAMES": 1, "SWFR_FRAMES_IN_FLIGHT": 4}))
    kinds = tb.KINDS                                                 # one frame of each kind
    d = GuardedFrames(len(kinds), tb.H, tb.W, offset=4, gap=4)
    assert [a % 16 for a in d.addresses()[:5]] == [4, 8, 12, 0, 4] and d.stride % 16 == 4
    r = tb._renderer()
    try:
        r.render_batch([tb.CORPUS[k]["stage"] for k in kinds], d.ptr, d.stride)
        got = d.guards_intact()
        for i, k in enumerate(kinds):
            tb._check(got[i], k, "nonzero", (route, i))
            print(route, i, k, "clear pixels", int((got[i][..., 3] == 0).sum()))
    finally:
        r.close()


# ---- 4. rotation, ownership and return
@pytest.mark.parametrize("in_flight", (None, 2))
def test_three_targets_in_rotation_and_back_to_the_handles_own_buffer(in_flight, monkeypatch):
    _no_knobs(monkeypatch, **({} if in_flight is None else {"SWFR_FRAMES_IN_FLIGHT": in_flight}))
    w, h = 132, 20
    sc = _solid_scene(w, h)
    want = _want(sc, (w, h))
    scene = dr.built_for_another_handle(sc, False)
    targets = [GuardedFrames(1, h, w, offset=o) for o in (0, 4, 8)]
    r = dr.handle(w, h)
    try:
        r.set_targets([t.ptr for t in targets])
        r.upload_edges(*scene)
        sets = [r.render_resident_async() for _ in range(5)]
        r.wait()
        assert len(set(sets)) == (4 if in_flight is None else in_flight) and sets[0] == 0, sets
        written = {k % 3 for k in sets}
        assert written == ({0, 1, 2} if in_flight is None else {0, 1})
        for k, t in enumerate(targets):
            frame = t.guards_intact()[0]
            if k in written:
                dr.zero(frame, want, ("rotation", k))
            else:
                assert (frame == SENTINEL).all(), ("a target no frame set maps to", k)
        dr.zero(r.read_image(premultiplied=True), want, "read_image is the last set's target")
        assert _device_framebuffer(r) == targets[sets[-1] % 3].ptr
        # back to the handle's own buffer
        for t in targets:
            t.refill()
        r.set_targets([])
        r.upload_edges(*scene)
        r.render_resident(1)
        dr.zero(r.read_image(premultiplied=True), want, "the handle's own buffer")
        assert _device_framebuffer(r) not in [t.ptr for t in targets]
        r.render(sc["stage"])
        r.render_resident(3)
        dr.zero(r.read_image(premultiplied=True), want, "the handle's own buffers, resident")
        for k, t in enumerate(targets):
            assert (t.guards_intact()[0] == SENTINEL).all(), ("a target given up", k)
    finally:
        r.close()


def _own_rows(h, rank):
    n = D.block_rows(h, 2) * D.TILE_H
    y = np.arange(h)
    return (y >= rank * n) & (y < (rank + 1) * n)


def test_band_handles_write_their_own_rows_only_and_block_targets(monkeypatch):
    _no_knobs(monkeypatch)
    w, h = 132, 40                                                   # three tile rows: handle 0 owns two, handle 1 the half one
    sc = _solid_scene(w, h)
    want = _want(sc, (w, h))
    scene = dr.built_for_another_handle(sc, False)
    rows_of_block = D.block_rows(h, 2) * D.TILE_H
    for rank in range(2):
        own = _own_rows(h, rank)
        assert own.any() and not own.all()
        g = GuardedFrames(1, h, w, offset=8)
        # a block target holds the handle's block alone; the kernels are given its address less the rows above the block: a pad of a
        # whole frame on both sides keeps every address a frame's store could reach inside the allocation
        blocks = GuardedFrames(2, rows_of_block, w, offset=4, pad=h * w * 4)
        r = dr.handle(w, h, band_index=rank, band_count=2, contiguous_bands=True)
        try:
            r.set_targets(g.addresses())
            r.upload_edges(*scene)
            assert r.render_resident_async() == 0
            r.wait()
            dr.not_refused(r, ("band", rank))
            frame = g.guards_intact()[0]
            dr.zero(frame[own], want[own], ("band handle, its own rows", rank))
            assert (frame[~own] == SENTINEL).all(), ("band handle, the other handle's rows", rank)
            used = r.render_resident_group_to(blocks.addresses())
            assert used != 0
            r.wait()
            got = blocks.guards_intact()
            n_own = int(own.sum())
            for f in range(2):
                dr.zero(got[f][:n_own], want[own], ("block target", rank, f))
                assert (got[f][n_own:] == SENTINEL).all(), ("block target, rows below the frame", rank, f)
            assert (g.guards_intact()[0] == frame).all(), "the full-frame target is as it was"
        finally:
            r.close()


# ---- 5. addresses and strides that cannot be uint32_t*
@pytest.mark.parametrize("odd", (1, 2, 3))
def test_misaligned_addresses_are_refused_before_any_launch(odd, monkeypatch):
    _no_knobs(monkeypatch)
    w, h = 132, 20
    sc = _solid_scene(w, h)
    want = _want(sc, (w, h))
    scene = dr.built_for_another_handle(sc, False)
    bad, good = GuardedFrames(2, h, w, offset=odd), GuardedFrames(2, h, w, offset=4)
    skewed = GuardedFrames(2, h, w, offset=0, gap=odd)               # aligned, but its stride is not

    def refused(call, what):
        with pytest.raises(api.SwfrError) as e:
            call()
        assert e.value.code == api.ERR_INVALID and "MisalignedTarget" in str(e.value), (what, str(e.value))

    r = dr.handle(w, h)
    try:
        r.set_targets([good.address(0)])
        r.upload_edges(*scene)
        r.render_resident(1)
        refused(lambda: r.set_targets([bad.address(0)]), "set_targets")
        refused(lambda: r.set_targets([good.address(1), bad.address(1)]), "set_targets, the second of two")
        # the handle keeps its target and its scene
        good.refill()
        r.render_resident(1)
        _frame_in_target(r, good, want, ("after refused targets", odd))
        stages = [sc["stage"], sc["stage"]]
        refused(lambda: r.render_batch(stages, bad.ptr, bad.stride), "render_batch, destination")
        refused(lambda: r.render_batch(stages, skewed.ptr, skewed.stride), "render_batch, stride")
        r.render_batch(stages, good.ptr, good.stride)
        got = good.guards_intact()
        for f in range(2):
            dr.zero(got[f], want, ("batch after refused batches", odd, f))
    finally:
        r.close()
    b = dr.handle(w, h, band_index=0, band_count=2, contiguous_bands=True)
    try:
        b.upload_edges(*scene)
        refused(lambda: b.render_resident_async_to(bad.address(0)), "render_resident_async_to")
        refused(lambda: b.render_resident_group_to([good.address(0), bad.address(1)]), "render_resident_group_to")
        b.wait()
        good.refill()
        b.render_resident_group_to([good.address(0)])
        b.wait()
        got = good.guards_intact()
        dr.zero(got[0][:16], want[:16], ("block target after refused ones", odd))
        assert (got[0][16:] == SENTINEL).all() and (got[1] == SENTINEL).all()
    finally:
        b.close()
    for g in (bad, skewed):
        assert (g.guards_intact() == SENTINEL).all(), "nothing was written through a refused address"
