"""k2_bin of a frame set's NEXT frame inside the row launch (k2_rows_ahead_b; DESIGN.md 6.1, "k2_bin of the next frame in the row
launch"): a resident call without per-kernel events launches k2_bin once per group of frame sets and then two kernels a frame pair,
the frames alternating between a set's two descriptors (parity 0 and 1, frame_layout.hpp).  Every frame is compared byte for byte with
the oracle, and with the same scene under SWFR_BIN_AHEAD=0, at the smallest shapes where the fused launch can go wrong:

* parity and call ends: 1 .. 8 frames per call, 1, 2 and 4 frames in flight, one and two frames per launch; calls back to back; a
  swfr_render of another stage between two resident calls;
* stale buffers of the other parity: a smaller and then a larger scene uploaded into the same handle;
* the rounds and windows of the one-wavefront bin instance: 1 100 paths (two rounds of its tile-row step), 300 hits in one tile-row
  (two windows of its 256-entry list), a 2112x2064 frame (8 514 strips: two ordering rounds per class, and the paired tile grid),
  each with the strips ordered by cost and row-major;
* box paths, whose class bytes and strip records k2_bin writes, through both parities;
* the calls that keep the three-launch chain: queued rows, a path of more than 32 edges, an aliased handle, SWFR_BIN_THREADS.

Which chain a call took is read from the handle (swfr_debug_copy, what = 3: the k2_rows_ahead_b launches of the last call), never
from a clock.  Runs on the GPU (-m gpu) and under tools/emu/run.py."""
import ctypes as C
import functools
import math
import os

import pytest

import scenarios
from helpers import diff_stats, golden, oracle_render, product_render
from host_frames import build_on_host
from test_bin_instances_gpu import _boxes_case, _tiny
from test_resident_waves_gpu import KNOBS, _rows_case
from test_tile_walk_gpu import _shape

pytestmark = pytest.mark.gpu

EMU = bool(os.environ.get("SWFR_EMULATOR"))
ALL_KNOBS = KNOBS + ("SWFR_BIN_THREADS", "SWFR_BIN_AHEAD", "SWFR_RESIDENT_BATCH", "SWFR_EVENT_STRIDE")
W, H = 200, 120


@pytest.fixture(scope="module", autouse=True)
def need_library(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SWFR_EVENT_STRIDE", "1000000")                # no per-kernel events, as in the benchmark's timed calls


def _ahead_launches(r):
    """the row launches of the handle's last resident call that binned the next frame"""
    v = C.c_uint32(0)
    assert r.L.swfr_debug_copy(r.h, 3, C.byref(v), 4) == 4
    return v.value


def _expected_ahead(frames, in_flight, per_launch):
    """render_resident's rule: groups of `per_launch` frame sets alternate; all but a group's last launch of the call bin ahead"""
    n_sets = min(in_flight, 4) if frames > 1 else 1
    rb = per_launch if per_launch >= 2 else 1
    while rb > 1 and (rb > n_sets or n_sets % rb):
        rb -= 1
    if rb < 2 or frames < 2:
        return 0
    return max(0, (frames + rb - 1) // rb - n_sets // rb)


# ---- scenes
def _star(cx, cy, r_out, r_in, phase, rgba, points=5):
    pts = []
    for k in range(2 * points):
        a = phase + math.pi * k / points
        rr = r_out if k % 2 == 0 else r_in
        pts.append((cx + rr * math.cos(a), cy + rr * math.sin(a)))
    return _shape(pts, rgba)


def _stars(n, width, height, seed=0):
    kids = []
    for k in range(n):
        cx, cy = 12.3 + ((k + seed) * 53) % (width - 20), 9.7 + ((k + seed) * 31) % (height - 16)
        col = ((53 * k + 20) % 256, (97 * k + 40) % 256, (29 * k + 150) % 256, 255 if k % 2 == 0 else 70 + (k * 23) % 150)
        kids.append(_star(cx, cy, 14.5 + (k % 5) * 4.25, 5.5 + (k % 3) * 2.1, 0.3 * k, col))
    return kids


def _box(x0, y0, x1, y1, rgba):
    return _shape([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], rgba)


def _case(kids, width=W, height=H):
    sc = dict(width=width, height=height, stage={"children": kids})
    return sc, oracle_render(sc)


@functools.lru_cache(maxsize=None)
def _main_case():
    kids = _stars(9, W, H)
    kids.insert(3, _box(30, 20, 150, 90, (10, 200, 90, 77)))
    kids.append(_box(64, 16, 128, 48, (200, 20, 90, 255)))
    sc, want = _case(kids)
    kinds = [int(k) for k in build_on_host(sc)[1]["kind"]]
    assert kinds.count(1) == 2 and kinds.count(0) == 9, kinds         # (1: SWFR_PATH_BOXES)
    return sc, want


@functools.lru_cache(maxsize=None)
def _other_case(n, width, height):
    return _case(_stars(n, width, height, seed=5) + [_box(8, 4, width - 40, height - 30, (90, 30, 200, 120))], width, height)


def _resident(sc, calls, in_flight=None, per_launch=None, **kw):
    """one handle: the scene uploaded, one frame rendered (the scene is then known to have no queued rows, or to have some), then
    render_resident(K) for every K of `calls`: the image and the fused launches after each"""
    import swf_renderer_amd as S
    r = S.Renderer(sc["width"], sc["height"], **kw)
    out = []
    try:
        r.upload_edges(*build_on_host(sc, aliased=kw.get("antialias") == "none"))
        r.render_resident(1)
        for k in calls:
            r.render_resident(k)
            out.append((r.read_image(premultiplied=True), _ahead_launches(r)))
        return out
    finally:
        r.close()


# ---- 1. parity and call ends
@pytest.mark.parametrize("per_launch", [1, 2])
@pytest.mark.parametrize("in_flight", [1, 2, 4])
def test_frames_per_call(in_flight, per_launch, monkeypatch):
    sc, want = _main_case()
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", str(in_flight))
    monkeypatch.setenv("SWFR_RESIDENT_BATCH", str(per_launch))
    calls = [1, 2, 3, 4, 5, 7, 8]
    got = _resident(sc, calls)
    monkeypatch.setenv("SWFR_BIN_AHEAD", "0")
    plain = _resident(sc, calls)
    for k, (img, fused), (img0, fused0) in zip(calls, got, plain):
        assert diff_stats(img, want) == (0, 0), (in_flight, per_launch, k)
        assert diff_stats(img0, want) == (0, 0) and fused0 == 0, (in_flight, per_launch, k, "SWFR_BIN_AHEAD=0")
        assert fused == _expected_ahead(k, in_flight, per_launch), (in_flight, per_launch, k, fused)
    if in_flight >= 2 and per_launch == 2:
        assert max(f for _, f in got) == (3 if in_flight == 2 else 2)  # (8 frames: all but each group's last launch)


def test_calls_back_to_back_and_a_render_between(monkeypatch):
    import swf_renderer_amd as S
    sc, want = _main_case()
    other, want_other = _other_case(5, W, H)
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", "2")
    r = S.Renderer(W, H)
    try:
        r.upload_edges(*build_on_host(sc))
        r.render_resident(1)
        for k in (3, 2, 3):                                           # a call starts at parity 0 again, behind one that ended on parity 1 or 0
            r.render_resident(k)
            assert _ahead_launches(r) == (1 if k == 3 else 0), k
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), k
        r.render_resident(7)
        assert _ahead_launches(r) == 3
        r.render(other["stage"])                                      # another scene through frame set 0, parity 0
        assert diff_stats(r.read_image(premultiplied=True), want_other) == (0, 0)
        r.upload_edges(*build_on_host(sc))
        for k in (1, 5):
            r.render_resident(k)
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), ("after render", k)
        assert _ahead_launches(r) == 2
    finally:
        r.close()


# ---- 2. stale buffers of the other parity
def test_smaller_and_larger_scenes_on_one_handle(monkeypatch):
    import swf_renderer_amd as S
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", "2")                  # ONE group of two sets: a call of K frames bins ahead in all but its last launch
    first, want_first = _main_case()
    small, want_small = _other_case(2, W, H)
    large, want_large = _other_case(23, W, H)
    counts = [tuple(len(a) for a in build_on_host(s)[:2]) for s in (first, small, large)]
    assert counts[1][1] < counts[0][1] < counts[2][1], counts        # paths (and with them band slots and chunks)
    r = S.Renderer(W, H)
    try:
        r.upload_edges(*build_on_host(first))
        r.render_resident(1)
        r.render_resident(4)
        assert _ahead_launches(r) == 1
        assert diff_stats(r.read_image(premultiplied=True), want_first) == (0, 0)
        for sc, want, name in ((small, want_small, "smaller"), (large, want_large, "larger")):
            r.upload_edges(*build_on_host(sc))
            r.render_resident(3)                                      # (the scene's first call: not yet verified, three launches a frame)
            assert _ahead_launches(r) == 0
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), (name, "first call")
            r.render_resident(3)
            assert _ahead_launches(r) == 1
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), name
            r.render_resident(6)
            assert _ahead_launches(r) == 2
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), (name, "both parities")
    finally:
        r.close()


# ---- 3. rounds and windows of the one-wavefront instance
@functools.lru_cache(maxsize=None)
def _big_case():
    bw, bh = 2112, 2064
    kids = [_shape([(3.3, 1.2), (bw - 2.6, 9.0), (0.35 * bw, 930.7)], (230, 120, 10, 255)),
            _shape([(100.5, 4.25), (1700.0, 2.0), (400.0, 1527.5)], (10, 200, 90, 77)),
            _shape([(5.5, bh - 625.0), (bw - 7.0, bh - 18.5), (300.0, bh - 1.25)], (40, 90, 200, 150)),
            _box(640, 1024, 1280, 1600, (255, 255, 255, 254))]
    tiles_x, tile_rows = (bw + 63) // 64, (bh + 15) // 16
    assert 2 * tiles_x * tile_rows == 8514 and 2 * tiles_x * ((tile_rows + 7) // 8) > 16 * 64      # strips; those of the largest class against an ordering round
    return _case(kids, bw, bh)


ROUND_CASES = {"two_path_rounds": lambda: _tiny(1100, 192, 72, 66), "hit_windows": lambda: _tiny(300, 192, 24, 11), "two_ordering_rounds": _big_case}


@pytest.mark.parametrize("strip_order", [None, "0"], ids=["by_cost", "row_major"])
@pytest.mark.parametrize("case", sorted(ROUND_CASES))
def test_rounds_and_windows(case, strip_order, monkeypatch):
    if EMU and case == "two_ordering_rounds":
        pytest.skip("a 2112x2064 frame is only a matter of time on the emulator")
    sc, want = ROUND_CASES[case]()
    if case == "hit_windows":
        paths = build_on_host(sc)[1]
        assert len(paths) == 300 and int(paths["y_max"].max()) <= 16      # every path in the first tile-row: more hits than the 256-entry list
    if strip_order is not None:
        monkeypatch.setenv("SWFR_STRIP_ORDER", strip_order)
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", "2")                  # ONE group: every launch but the last bins ahead, with the costs of two frames before
    (img, fused), = _resident(sc, [5])
    assert fused == 2, (case, fused)
    assert diff_stats(img, want) == (0, 0), (case, strip_order)
    monkeypatch.setenv("SWFR_BIN_AHEAD", "0")
    (img0, fused0), = _resident(sc, [5])
    assert fused0 == 0 and diff_stats(img0, img) == (0, 0), (case, strip_order, "SWFR_BIN_AHEAD=0")


# ---- 4. box paths through the other parity
@functools.lru_cache(maxsize=None)
def _box_cases():
    full = _box(0, 0, W, H, (12, 34, 56, 255))
    out = {"alone": _case([full]), "under": _case([full] + _stars(6, W, H)), "over": _case(_stars(6, W, H) + [full])}
    for name, (sc, _) in out.items():
        assert 1 in [int(k) for k in build_on_host(sc)[1]["kind"]], name
    return out


@pytest.mark.parametrize("in_flight", [2, 4])
@pytest.mark.parametrize("name", ["alone", "under", "over"])
def test_box_paths(name, in_flight, monkeypatch):
    sc, want = _box_cases()[name]
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", str(in_flight))
    calls = [4, 4] if in_flight == 2 else [8, 8]                      # four frames per set and call: both parities' class bytes and records, used and cleared twice
    for img, fused in _resident(sc, calls):
        assert fused == _expected_ahead(calls[0], in_flight, 2) and fused >= 1, (name, fused)
        assert diff_stats(img, want) == (0, 0), (name, in_flight)
    sc2, want2 = _boxes_case()                                         # (a frame whose last tile column and tile-row are cut)
    for img, fused in _resident(sc2, [4]):
        assert diff_stats(img, want2) == (0, 0), (in_flight, "192x24")


# ---- 5. the calls that keep the three-launch chain
def test_queued_rows_keep_the_chain(monkeypatch):
    sc, want = _rows_case()                                            # (a row with a ninth active edge)
    for img, fused in _resident(sc, [3, 6]):
        assert fused == 0
        assert diff_stats(img, want) == (0, 0)


def test_a_wide_path_keeps_the_chain():
    kids = _stars(4, W, H) + [_star(100.2, 60.1, 55.0, 21.0, 0.1, (240, 200, 30, 200), points=17)]      # 34 edges: the wide row kernel
    sc, want = _case(kids)
    assert max(int(n) for n in build_on_host(sc)[1]["n_edges"]) > 32
    for img, fused in _resident(sc, [3, 6]):
        assert fused == 0
        assert diff_stats(img, want) == (0, 0)


def test_an_aliased_handle_keeps_the_chain():
    sc = scenarios.scenarios()["nonzero_pentagram"]
    want = golden("cairo_aliased_nonzero_pentagram", "rgba_premul")
    assert diff_stats(product_render(sc, antialias="none"), want) == (0, 0)
    for img, fused in _resident(sc, [3, 6], even_odd=bool(sc.get("even_odd")), antialias="none"):
        assert fused == 0
        assert diff_stats(img, want) == (0, 0)


@pytest.mark.parametrize("threads", ["256", "1024"])
def test_a_forced_bin_instance_keeps_the_chain(threads, monkeypatch):
    sc, want = _main_case()
    monkeypatch.setenv("SWFR_BIN_THREADS", threads)
    for img, fused in _resident(sc, [3, 6]):
        assert fused == 0
        assert diff_stats(img, want) == (0, 0)


def test_the_fused_chain_from_the_second_call():
    """a scene's first call still launches the queued-row kernels (what it needs of them is not known yet); from the second on a scene
    without queued rows bins ahead, and the handle's k2_bin instance is what the plan chose for the prologue"""
    import swf_renderer_amd as S
    sc, want = _main_case()
    r = S.Renderer(W, H)
    try:
        r.upload_edges(*build_on_host(sc))
        r.render_resident(6)
        assert _ahead_launches(r) == 0
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        r.render_resident(6)
        assert _ahead_launches(r) == 1                                 # three launches over two groups: the first group's first
        v = C.c_uint32(0)
        assert r.L.swfr_debug_copy(r.h, 2, C.byref(v), 4) == 4 and v.value == 256
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        st = r.stats()
        assert st["queued_rows"] == 0 and st["crowded_rows"] == 0, st
    finally:
        r.close()


def test_counters_of_a_parity_1_frame(monkeypatch):
    """four frame sets, two frames per launch, eight frames: every set's last frame of the call ran with its parity-1 descriptor, whose
    counters lie four sets further on.  What the call reports of them -- the records of set 0's last frame, and what every set's
    frame adds to swfr_stats -- is what the same call reports under the three-launch chain."""
    import swf_renderer_amd as S
    sc, want = _main_case()
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", "4")
    monkeypatch.setenv("SWFR_RESIDENT_BATCH", "2")

    def call():
        r = S.Renderer(W, H)
        try:
            r.upload_edges(*build_on_host(sc))
            r.render_resident(1)
            before = r.stats()
            r.render_resident(8)
            after = r.stats()
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
            return _ahead_launches(r), r.timing()["n_records"], {k: after[k] - before[k] for k in after}
        finally:
            r.close()

    fused, records, delta = call()
    monkeypatch.setenv("SWFR_BIN_AHEAD", "0")
    fused0, records0, delta0 = call()
    print("ahead launches %d / %d, n_records %d / %d, stats %r / %r" % (fused, fused0, records, records0, delta, delta0))
    assert fused > 0 and fused0 == 0, (fused, fused0)
    assert records == records0, (records, records0)
    assert delta == delta0, (delta, delta0)
