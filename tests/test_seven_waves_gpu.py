"""What the register diet for seven resident wavefronts touches in k2_tiles' solid instance: the class bytes a strip reads beyond the
ONE chunk of 64 that is fetched up front (entries 64 and later are fetched when the walk gets there, the second chunk included, which
used to be prefetched), and the descriptor fields no longer held in registers (`cls`, `cell_slice`: read where they are used).  Every
frame is compared with the oracle, zero differing bytes.

* Frames of 192x24 and 130x20: three tile columns, two tile-rows, the last column and the last tile-row cut by the frame.
* The first tile-row carries 70, 130 or 200 paths -- small tor triangles, dealt over its six strips so that every strip paints up to
  the list's end, with opaque covers of the whole frame and an opaque and a translucent cover of a part of it among them.  The
  topmost opaque cover of the whole frame sits at list position 0, 63, 64, 65, 127, 128, 129 or last: walks start in the first, the
  second and the third chunk of class bytes (and behind it) and end in a later one.
* Each frame goes through render, render_resident with 1 and 4 frames in flight, render_batch, and the three launch shapes of
  k2_tiles (one wavefront per strip, two strips per wavefront, seven persistent wavefronts).
* One StripTop record is read, cleared and filled again on one frame set, the cover at position 64.

Runs on the GPU (-m gpu) and under tools/emu/run.py."""
import functools
import os

import numpy as np
import pytest

from helpers import diff_stats, oracle_render
from host_frames import build_on_host
from test_tile_walk_gpu import _cover, _paired_grid, _shape

pytestmark = pytest.mark.gpu

KNOBS = ("SWFR_TILES_GRID", "SWFR_TILES_SHADERS", "SWFR_FRAMES_IN_FLIGHT", "SWFR_CHUNK_ROWS", "SWFR_FAST_LIMIT", "SWFR_ROWS_WIDE", "SWFR_BATCH_FRAMES", "SWFR_STRIP_ORDER")
SIZES = [(192, 24), (130, 20)]
COUNTS = [70, 130, 200]
POSITIONS = [0, 63, 64, 65, 127, 128, 129, -1]                         # of the topmost opaque cover (-1: the list's last entry)
GRIDS = ["one_per_strip", "paired", "seven"]
ROUTES = ["render", "resident_1", "resident_4", "batch"]
COVER = (12, 34, 56, 255)


@pytest.fixture(scope="module", autouse=True)
def need_library(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _small(k, W):
    """Path k of the first tile-row: a triangle inside strip k % 6 (tile column k % 3, rows 0..7 or 8..15), wholly inside the frame's
    rows and reaching into its columns, so that it is entry k of the tile-row's list; in the cut column it hangs over the frame's edge."""
    col, ty0 = k % 3, 8 * ((k // 3) % 2)
    lo, hi = 64 * col + 4, min(64 * col + 52, W - 8)
    if hi <= lo:
        lo, hi = W - 12, W - 6
    p = lo + (11 * k) % (hi - lo)
    alpha = (255, 140, 255, 31, 254, 1)[k % 6]
    return _shape([(p + 0.4, ty0 + 0.3 + (k % 3)), (p + 9.0 + (k % 7), ty0 + 7.6), (p - 3.3, ty0 + 5.1)], ((37 * k) % 256, (91 * k + 50) % 256, (17 * k + 200) % 256, alpha))


def positions(n):
    return sorted({n - 1 if p < 0 else p for p in POSITIONS if p < n})


def scene(W, H, n, pos, with_cover=True):
    """n paths in the first tile-row's list, the topmost opaque cover of the whole frame at position `pos`.  Below it (where there is
    room) another opaque cover of the whole frame; above it a translucent cover of the frame's right part and an opaque cover of its left
    part, their slanted sides in the middle tile column with a gap between them: full in some strips, partial in others, missing in the rest."""
    special = {pos: _cover(W, H, COVER)} if with_cover else {}
    if pos // 3 not in special and pos // 3 < pos:
        special[pos // 3] = _cover(W, H, (200, 10, 20, 255))
    above = (pos + n) // 2
    if pos < above < n - 2:
        special[above] = _shape([(0.45 * W, -30.0), (W + 40.0, -30.0), (W + 40.0, 3.0 * H), (0.7 * W, 3.0 * H)], (90, 160, 30, 120))
        special[above + 1] = _shape([(-40.0, -30.0), (0.55 * W, -30.0), (0.3 * W, 3.0 * H), (-40.0, 3.0 * H)], (5, 6, 7, 255))
    kids = [special.get(k) or _small(k, W) for k in range(n)]
    kids += [_shape([(5.5 + 40 * j, 16.4), (30.0 + 40 * j, H - 0.8), (9.0 + 40 * j, H - 1.9)], (60 * j, 255 - 50 * j, 99, 255 - 40 * j)) for j in range(4)]     # the cut tile-row
    return dict(width=W, height=H, stage={"children": kids})


@functools.lru_cache(maxsize=None)
def _case(size, n, pos):
    sc = scene(size[0], size[1], n, pos)
    return sc, oracle_render(sc)


def _through(route, sc):
    """the frame of `sc` by one route (resident_N: N frames in flight, one frame more than that rendered: a frame set is used again)"""
    import swf_renderer_amd as S
    r = S.Renderer(sc["width"], sc["height"])
    try:
        if route == "render":
            r.render(sc["stage"])
        elif route == "batch":
            plain = {"children": [_shape([(2, 2), (40, 5), (20, 18)], (90, 90, 200, 255))]}
            r.render_batch([plain, sc["stage"], plain, sc["stage"]])
        else:
            r.upload_edges(*build_on_host(sc))
            r.render_resident(int(route[-1]) + 1)
        st = r.stats()
        assert st["frames"] >= 1 and all(st[k] == 0 for k in ("pairtest_limit", "start_group_limit", "history_limit")), st
        return r.read_image(premultiplied=True)
    finally:
        r.close()


def _grid(monkeypatch, grid, W, H):
    monkeypatch.setenv("SWFR_TILES_GRID", {"one_per_strip": "100000", "paired": _paired_grid(W, H), "seven": "7"}[grid])


def test_the_cases_reach_the_later_chunks():
    """the scenes are what the docstring says: the counts straddle the chunks of 64, every position asked for occurs, and the cover
    at `pos` shows in the frame (it is not hidden: the walk above it matters) next to pixels of the paths above it"""
    assert [positions(n) for n in COUNTS] == [[0, 63, 64, 65, 69], [0, 63, 64, 65, 127, 128, 129], [0, 63, 64, 65, 127, 128, 129, 199]]
    for n in COUNTS:
        for pos in positions(n):
            sc, want = _case(SIZES[0], n, pos)
            assert len(sc["stage"]["children"]) == n + 4
            shows = (want == np.array(COVER, np.uint8)).all(-1)
            assert shows.any() and (pos == n - 1 or not shows[:16].all()), (n, pos)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("size", SIZES, ids=["192x24", "130x20"])
def test_routes(size, n, monkeypatch):
    for pos in positions(n):
        sc, want = _case(size, n, pos)
        for route in ROUTES:
            if route.startswith("resident"):
                monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
            assert diff_stats(_through(route, sc), want) == (0, 0), (size, n, pos, route)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("size", SIZES, ids=["192x24", "130x20"])
def test_launch_shapes(size, n, grid, monkeypatch):
    _grid(monkeypatch, grid, *size)
    for pos in positions(n):
        sc, want = _case(size, n, pos)
        assert diff_stats(_through("render", sc), want) == (0, 0), (size, n, pos, grid)


@pytest.mark.parametrize("size", SIZES, ids=["192x24", "130x20"])
def test_strip_record_is_cleared_and_refilled(size, monkeypatch):
    import swf_renderer_amd as S
    W, H = size
    with_cover, want_cover = _case(size, 130, 64)
    without = scene(W, H, 130, 64, with_cover=False)
    want_plain = oracle_render(without)
    cover = np.array(COVER, np.uint8)
    assert (want_cover == cover).all(-1).any() and not (want_plain == cover).all(-1).any()       # the cover shows, and only where it is
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", "1")                  # ONE frame set: every frame reads the records the last one cleared
    r = S.Renderer(W, H)
    try:
        r.upload_edges(*build_on_host(with_cover))
        r.render_resident(3)
        assert diff_stats(r.read_image(premultiplied=True), want_cover) == (0, 0), (size, "cover")
        r.upload_edges(*build_on_host(without))
        r.render_resident(1)
        got = r.read_image(premultiplied=True)
        assert not (got == cover).all(-1).any(), (size, "a pixel of the old cover remains")
        assert diff_stats(got, want_plain) == (0, 0), (size, "plain")
        r.upload_edges(*build_on_host(with_cover))                    # ... and the record is filled again
        r.render_resident(2)
        assert diff_stats(r.read_image(premultiplied=True), want_cover) == (0, 0), (size, "cover again")
    finally:
        r.close()
