"""The two instances of k2_bin -- workgroups of 256 and of 1024 threads (SWFR_BIN_THREADS forces one; the launch plan chooses by the
frames' paths and by whether frames overlap) -- and the order of its workgroups (the eight that order the strips come first).  Every
frame is compared with the oracle, zero differing bytes, under both instances, at the smallest shapes where an instance takes
another path:

* frames of 192x24 and 130x20 (the last tile column and the last tile-row cut by the frame) through render, render_resident with
  1 and 4 frames in flight, and render_batch;
* 4 095, 4 096 and 4 097 tiny opaque and translucent triangles on a 192x72 frame: the small instance tests 4 096 paths per round of
  its tile-row step, and the last triangles lie on top of each other -- painter's order must survive the round boundary;
* one more path than an instance's hit list holds (1 024 and 4 096 entries), all in ONE tile-row: a second window;
* a 1024x16400 frame, 32 800 strips: more than 4 096 per XCD class, two rounds of the small instance's ordering step -- three
  frames on ONE frame set, so that the second and third are launched in the cost order, and again with SWFR_STRIP_ORDER=0;
* the tile pass in its paired shape, which reads the ordered list two grids ahead;
* box paths (a full-frame opaque box, a rectilinear stroke): their class bytes and strip records are written in k2_bin;
* an aliased frame (no edge workgroups), a scene with queued rows (SWFR_FAST_LIMIT=0: the 64-bit edge records), and two handles
  with band_count = 2;
* a batch into a device tensor (one launch per kernel) of one frame above the path threshold and one below: the launch takes the
  large instance, every frame is exact;
* the plan's rule as the handle reports it: the small instance for overlapping frames of few paths, else the large one.

Runs on the GPU (-m gpu) and under tools/emu/run.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import scenarios
from helpers import diff_stats, golden, oracle_render, product_render
from host_frames import build_on_host
from test_resident_waves_gpu import KNOBS, SIZES, _rows_case, _store, _through
from test_tile_walk_gpu import _paired_grid, _shape

pytestmark = pytest.mark.gpu

EMU = bool(os.environ.get("SWFR_EMULATOR"))
THREADS = ["256", "1024"]
SMALL_ROUND = 16 * 256                                                # paths per round of the small instance's tile-row step: the plan's threshold
HIT_LIST = {"256": 1024, "1024": 4096}
ROUTES = ["render", "resident_1", "resident_4", "batch"]


@pytest.fixture(scope="module", autouse=True)
def need_library(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS + ("SWFR_BIN_THREADS",):
        monkeypatch.delenv(k, raising=False)


def _bin_threads_of(r):
    """the instance the handle's last launch chain ran"""
    v = C.c_uint32(0)
    assert r.L.swfr_debug_copy(r.h, 2, C.byref(v), 4) == 4
    return v.value


# ---- scenes
@functools.lru_cache(maxsize=None)
def _tiny(n, W, H, y_span):
    """n triangles of a few pixels with their tops in rows 0 .. y_span, opaque and translucent in turn, one path each; the last six lie
    on top of each other, each smaller than the one below: every one of them shows only if they are painted in list order"""
    kids = []
    for k in range(n - 6):
        x0, y0 = 0.6 + (k * 37) % (W - 8) + 0.1 * (k % 7), 0.4 + ((k * 17) % (10 * y_span)) / 10.0
        col = ((53 * k) % 256, (97 * k + 40) % 256, (29 * k + 150) % 256, 255 if k % 2 == 0 else 90 + k % 120)
        kids.append(_shape([(x0, y0), (x0 + 4.4, y0 + 1.3), (x0 + 1.7, y0 + 3.4)], col))
    for i in range(6):
        a, b = 0.55 * W + 0.3 + 0.7 * i, 0.5 * y_span + 0.2 + 0.35 * i
        col = ((200 * i + 10) % 256, (90 * i + 120) % 256, (140 * i + 60) % 256, 255 if i % 2 else 140)
        kids.append(_shape([(a, b), (a + 11.0 - 1.6 * i, b + 0.4), (a + 5.0 - 0.7 * i, b + 4.6 - 0.7 * i)], col))
    sc = dict(width=W, height=H, stage={"children": kids})
    paths = build_on_host(sc)[1]
    assert len(paths) == n, (len(paths), n)
    return sc, oracle_render(sc)


def _rounds_case(n):
    return _tiny(n, 192, 72, 66)


def _one_row_case(n):
    sc, want = _tiny(n, 192, 24, 11)
    paths = build_on_host(sc)[1]
    assert int(paths["y_max"].max()) <= 16 and int(paths["y_min"].min()) >= 0       # every path in the first tile-row, and only there
    return sc, want


TALL_W, TALL_H = 1024, 16400


@functools.lru_cache(maxsize=None)
def _tall_case():
    kids = [_shape([(3.3, 1.2), (TALL_W - 2.6, 9.0), (0.35 * TALL_W, 30.7)], (230, 120, 10, 255)),
            _shape([(100.5, 4.25), (700.0, 2.0), (400.0, 27.5)], (10, 200, 90, 77)),
            _shape([(5.5, TALL_H - 25.0), (TALL_W - 7.0, TALL_H - 18.5), (300.0, TALL_H - 1.25)], (40, 90, 200, 150)),
            _shape([(600.25, TALL_H - 30.0), (900.0, TALL_H - 3.0), (500.0, TALL_H - 6.5)], (255, 255, 255, 254))]
    sc = dict(width=TALL_W, height=TALL_H, stage={"children": kids})
    tiles_x, tile_rows = (TALL_W + 63) // 64, (TALL_H + 15) // 16
    assert 2 * tiles_x * tile_rows == 32800 and 2 * tiles_x * ((tile_rows + 7) // 8) > SMALL_ROUND      # strips; those of the largest class
    return sc, oracle_render(sc)


@functools.lru_cache(maxsize=None)
def _boxes_case():
    W, H = 192, 24
    kids = [_shape([(0, 0), (W, 0), (W, H), (0, H)], (12, 34, 56, 255)),                          # one box that contains every tile: full cover
            _shape([(3.3, 1.2), (W - 2.6, 0.4 * H), (0.35 * W, H - 0.7)], (230, 120, 10, 140)),
            _shape([(70.0, 3.0), (150.0, 3.0), (150.0, 19.0), (70.0, 19.0)], (10, 200, 90, 77)),   # a box inside tiles
            _shape([(10.35, 2.25), (W + 3.0, 2.25), (W + 3.0, H - 1.4), (10.35, H - 1.4)], (200, 20, 90, 200))]
    sc = dict(width=W, height=H, stage={"children": kids})
    kinds = [int(k) for k in build_on_host(sc)[1]["kind"]]
    assert kinds == [1, 0, 1, 1], kinds                                                             # (1: SWFR_PATH_BOXES)
    return sc, oracle_render(sc)


@functools.lru_cache(maxsize=None)
def _stroke_case():
    sc = scenarios.scenarios()["stroke_rectilinear_loop_scaled"]
    assert 1 in [int(k) for k in build_on_host(sc)[1]["kind"]]
    return sc, oracle_render(sc)


# ---- 1. routes
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("size", SIZES, ids=["192x24", "130x20"])
def test_routes(size, route, threads, monkeypatch):
    sc, want = _store(size)
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    if route.startswith("resident"):
        monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
    assert diff_stats(_through(route, sc), want) == (0, 0), (size, route, threads)


# ---- 2. path rounds of the small instance
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("n", [SMALL_ROUND - 1, SMALL_ROUND, SMALL_ROUND + 1])
def test_path_rounds(n, threads, monkeypatch):
    sc, want = _rounds_case(n)
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    for route in ("render", "resident_4"):
        if route.startswith("resident"):
            monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
        assert diff_stats(_through(route, sc), want) == (0, 0), (n, threads, route)


def test_the_stacked_triangles_show_in_list_order():
    """what test_path_rounds relies on: painting the last paths in another order gives another frame"""
    sc, want = _rounds_case(SMALL_ROUND + 1)
    kids = list(sc["stage"]["children"])
    kids[-1], kids[-2] = kids[-2], kids[-1]
    assert diff_stats(oracle_render(dict(sc, stage={"children": kids})), want)[0] > 0


# ---- 3. hit-list windows
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("n", [1025, 4097])
def test_hit_list_windows(n, threads, monkeypatch):
    assert n - 1 in HIT_LIST.values()
    sc, want = _one_row_case(n)
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    assert diff_stats(_through("render", sc), want) == (0, 0), (n, threads)


# ---- 4. ordering rounds
@pytest.mark.skipif(EMU, reason="a 16 400-row frame is only a matter of time on the emulator")
@pytest.mark.parametrize("strip_order", [None, "0"], ids=["by_cost", "row_major"])
@pytest.mark.parametrize("threads", THREADS)
def test_ordering_rounds(threads, strip_order, monkeypatch):
    import swf_renderer_amd as S
    sc, want = _tall_case()
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", "1")                  # ONE frame set: frames two and three are ordered by the costs of the frame before
    if strip_order is not None:
        monkeypatch.setenv("SWFR_STRIP_ORDER", strip_order)
    r = S.Renderer(TALL_W, TALL_H)
    try:
        r.upload_edges(*build_on_host(sc))
        r.render_resident(3)
        assert _bin_threads_of(r) == int(threads)
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), (threads, strip_order)
    finally:
        r.close()


# ---- 5. the paired tile grid
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("size", SIZES, ids=["192x24", "130x20"])
def test_paired_tile_grid(size, threads, monkeypatch):
    sc, want = _store(size)
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    monkeypatch.setenv("SWFR_TILES_GRID", _paired_grid(*size))
    for route in ("render", "resident_1", "resident_4"):
        if route.startswith("resident"):
            monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
        assert diff_stats(_through(route, sc), want) == (0, 0), (size, threads, route)


# ---- 6. box paths
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("case", [_boxes_case, _stroke_case], ids=["full_frame_box", "rectilinear_stroke"])
def test_box_paths(case, threads, monkeypatch):
    sc, want = case()
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    for route in ("render", "resident_4"):
        if route.startswith("resident"):
            monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
        assert diff_stats(_through(route, sc), want) == (0, 0), (threads, route)


# ---- 7. the other routes that enter k2_bin
@pytest.mark.parametrize("threads", THREADS)
def test_aliased_frame(threads, monkeypatch):
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    sc = scenarios.scenarios()["nonzero_pentagram"]
    assert diff_stats(product_render(sc, antialias="none"), golden("cairo_aliased_nonzero_pentagram", "rgba_premul")) == (0, 0), threads


@pytest.mark.parametrize("threads", THREADS)
def test_queued_rows(threads, monkeypatch):
    sc, want = _rows_case()
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    monkeypatch.setenv("SWFR_FAST_LIMIT", "0")
    for route in ("render", "resident_1"):
        if route.startswith("resident"):
            monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
        assert diff_stats(_through(route, sc), want) == (0, 0), (threads, route)


@pytest.mark.parametrize("threads", THREADS)
def test_two_handles_share_the_tile_rows(threads, monkeypatch):
    from swf_renderer_amd import distributed as D
    sc, want = _rows_case()
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    slabs = [D.extract_slab(_through("render", sc, band_index=rank, band_count=2), rank, 2) for rank in range(2)]
    assert diff_stats(np.asarray(D.assemble(slabs, sc["width"], sc["height"])), want) == (0, 0), threads


# ---- 8. a batch of unlike frames, and the plan's rule
def _few_paths_case():
    sc, _ = _rounds_case(SMALL_ROUND + 1)
    few = dict(sc, stage={"children": sc["stage"]["children"][-9:]})
    return few, _few_want()


@functools.lru_cache(maxsize=None)
def _few_want():
    sc, _ = _rounds_case(SMALL_ROUND + 1)
    return oracle_render(dict(sc, stage={"children": sc["stage"]["children"][-9:]}))


@pytest.mark.skipif(EMU, reason="device tensors need the GPU")
@pytest.mark.parametrize("threads", [None] + THREADS, ids=["plan", "256", "1024"])
def test_batch_of_unlike_frames_takes_the_large_instance(threads, monkeypatch):
    """frames into a device tensor are ONE launch per kernel (without a destination render_batch launches frame by frame)"""
    import torch
    import swf_renderer_amd as S
    many, want_many = _rounds_case(SMALL_ROUND + 1)
    few, want_few = _few_paths_case()
    W, H = many["width"], many["height"]
    if threads is not None:
        monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    for stages, wants in (([few["stage"], many["stage"]], [want_few, want_many]), ([many["stage"], few["stage"], few["stage"]], [want_many, want_few, want_few])):
        r = S.Renderer(W, H)
        try:
            out = torch.zeros((len(stages), H, W, 4), dtype=torch.uint8, device="cuda")
            r.render_batch(stages, out.data_ptr(), H * W * 4)
            got = out.cpu().numpy()
            assert _bin_threads_of(r) == int(threads or 1024)             # the plan: over the frames of the launch
        finally:
            r.close()
        for k, want in enumerate(wants):
            assert diff_stats(got[k], want) == (0, 0), (threads, len(stages), k)


def test_the_plans_rule(monkeypatch):
    """the small instance where frames of up to 4 096 paths overlap; the large one for a frame alone and above the threshold"""
    import swf_renderer_amd as S
    few, want_few = _few_paths_case()
    at, want_at = _rounds_case(SMALL_ROUND)
    above, want_above = _rounds_case(SMALL_ROUND + 1)
    for sc, want, in_flight, frames, expect in ((few, want_few, "4", 5, 256), (at, want_at, "4", 5, 256), (above, want_above, "4", 5, 1024),
                                                (few, want_few, "1", 2, 1024), (few, want_few, "4", 1, 1024)):
        monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", in_flight)
        r = S.Renderer(sc["width"], sc["height"])
        try:
            r.upload_edges(*build_on_host(sc))
            r.render_resident(frames)
            assert _bin_threads_of(r) == expect, (in_flight, frames, expect)
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        finally:
            r.close()
    r = S.Renderer(few["width"], few["height"])
    try:
        r.render(few["stage"])                                        # a blocking render: the frame has the GPU to itself
        assert _bin_threads_of(r) == 1024
        r.render_batch([few["stage"], few["stage"]])
        assert _bin_threads_of(r) == 256
    finally:
        r.close()
