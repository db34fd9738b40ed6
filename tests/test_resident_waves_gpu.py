"""What the loads moved for six resident wavefronts touch: k2_tiles reads the launch list (`strips`) and the strips' records
(`strip_top`) where it uses them -- the descriptor prefetch of the strip after next, the next strip's record, the record's clear.
The row-header table (`rows`) that k2_rows stores to and k2_tiles reads through a held pointer is covered too: a variant of k2_rows
that read it at its header stores was measured with this change and not shipped (profiles/w6_tables.md), the cases stay.  Every
frame is compared with the oracle, zero differing bytes, at the smallest shapes where those reads can go wrong:

* frames of 192x24 and 130x20 (three tile columns, two tile-rows, the last column and the last row cut by the frame) with one
  wavefront per strip, two strips per wavefront and seven persistent wavefronts (slots past the list's end, the prefetch of a strip
  two grids ahead), through render, render_resident with 1 and 4 frames in flight, and render_batch;
* a StripTop record read, cleared and filled again: an opaque cover of every strip, three frames in a row on ONE frame set, then a
  scene without the cover on the same handle -- no pixel of the cover may remain;
* row headers of every kind: FULL rows, rows of one to three sample passes, a queued row (a ninth active edge, and every row with
  SWFR_FAST_LIMIT=0) and another rank's rows (two handles, band_count = 2), with SWFR_CHUNK_ROWS 8, 16, 32 and 64.

Runs on the GPU (-m gpu) and under tools/emu/run.py."""
import functools
import os

import numpy as np
import pytest

from helpers import diff_stats, oracle_render
from host_frames import build_on_host
from test_row_pass_slots import comb_rows, kinked_box, scene as row_scene, sliver
from test_tile_walk_gpu import _cover, _paired_grid, _shape, store_scene

pytestmark = pytest.mark.gpu

KNOBS = ("SWFR_TILES_GRID", "SWFR_TILES_SHADERS", "SWFR_FRAMES_IN_FLIGHT", "SWFR_CHUNK_ROWS", "SWFR_FAST_LIMIT", "SWFR_ROWS_WIDE", "SWFR_BATCH_FRAMES", "SWFR_STRIP_ORDER")
SIZES = [(192, 24), (130, 20)]
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


def _grid(monkeypatch, grid, W, H):
    monkeypatch.setenv("SWFR_TILES_GRID", {"one_per_strip": "100000", "paired": _paired_grid(W, H), "seven": "7"}[grid])


@functools.lru_cache(maxsize=None)
def _store(size):
    sc = store_scene(*size)
    return sc, oracle_render(sc)


def _through(route, sc, **kw):
    """the frame of `sc` by one route (resident_N: N frames in flight, one frame more than that rendered: a frame set is used again)"""
    import swf_renderer_amd as S
    r = S.Renderer(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")), **kw)
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


# ---- 1. frames and grids: the launch list read where it is used
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("size", SIZES, ids=["192x24", "130x20"])
def test_frames_and_grids(size, grid, route, monkeypatch):
    sc, want = _store(size)
    _grid(monkeypatch, grid, *size)
    if route.startswith("resident"):
        monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
    assert diff_stats(_through(route, sc), want) == (0, 0), (size, grid, route)


# ---- 2. a StripTop record read, cleared and refilled
def _covered(W, H, with_cover):
    kids = [_shape([(3.3, 1.2), (W - 2.6, 0.4 * H), (0.35 * W, H - 0.7)], (230, 120, 10, 255))]
    if with_cover:
        kids.append(_cover(W, H, COVER))
    kids.append(_shape([(0.2 * W + 0.35, 2.25), (W - 9.0, 3.25), (W - 30.0, H - 1.4)], (10, 200, 90, 77)))
    return dict(width=W, height=H, stage={"children": kids})


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("size", SIZES, ids=["192x24", "130x20"])
def test_strip_record_is_cleared_and_refilled(size, grid, monkeypatch):
    import swf_renderer_amd as S
    W, H = size
    with_cover, without = _covered(W, H, True), _covered(W, H, False)
    want_cover, want_plain = oracle_render(with_cover), oracle_render(without)
    cover = np.array(COVER, np.uint8)
    assert (want_cover == cover).all(-1).any() and not (want_plain == cover).all(-1).any()       # the cover shows, and only where it is
    _grid(monkeypatch, grid, W, H)
    monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", "1")                  # ONE frame set: every frame reads the records the last one cleared
    r = S.Renderer(W, H)
    try:
        r.upload_edges(*build_on_host(with_cover))
        r.render_resident(3)
        assert diff_stats(r.read_image(premultiplied=True), want_cover) == (0, 0), (size, grid, "cover")
        r.upload_edges(*build_on_host(without))
        r.render_resident(1)
        got = r.read_image(premultiplied=True)
        assert not (got == cover).all(-1).any(), (size, grid, "a pixel of the old cover remains")
        assert diff_stats(got, want_plain) == (0, 0), (size, grid, "plain")
        r.upload_edges(*build_on_host(with_cover))                    # ... and the record is filled again
        r.render_resident(2)
        assert diff_stats(r.read_image(premultiplied=True), want_cover) == (0, 0), (size, grid, "cover again")
    finally:
        r.close()


# ---- 3. row headers of every kind through the `rows` table
ROWS_W, ROWS_H = 192, 72                                              # five tile-rows (the last cut by the frame), three tile columns


@functools.lru_cache(maxsize=None)
def _rows_case():
    polys = [[sliver(8.0, 3.0, 2, rows=20), sliver(8.0 + 1.5 * 20, 3.0, 2, rows=20, lean=-1)],      # FULL rows, four active edges where they cross
             kinked_box(70.3, 2.0, 1, 14, width=20.0),                                              # one sample pass
             kinked_box(100.3, 18.0, 5, 14, width=20.0),                                            # two
             kinked_box(130.3, 30.0, 9, 30, width=25.0),                                            # three
             comb_rows(9, x0=20.0, y_top=36.0, y_bottom=66.0),                                      # a row with a ninth active edge: queued
             sliver(150.0, 50.0, 17, rows=3)]                                                       # FULL rows over 17 and 18 columns, cut at x = width
    sc = row_scene(ROWS_W, ROWS_H, polys)
    return sc, oracle_render(sc)


def test_the_rows_case_has_a_ninth_edge():
    from test_row_pass_slots import active_counts
    sc, want = _rows_case()
    seen = set()
    for counts in active_counts(sc):
        seen |= set(counts)
    assert {3, 4, 9} <= seen, sorted(seen)
    assert ((want[..., 3] > 0) & (want[..., 3] < 255)).any()


@pytest.mark.parametrize("fast_limit", [None, "0"], ids=["fast", "queued"])
@pytest.mark.parametrize("chunk_rows", ["8", "16", "32", "64"])
def test_row_headers(chunk_rows, fast_limit, monkeypatch):
    sc, want = _rows_case()
    monkeypatch.setenv("SWFR_CHUNK_ROWS", chunk_rows)
    if fast_limit is not None:
        monkeypatch.setenv("SWFR_FAST_LIMIT", fast_limit)
    for route in ("render", "resident_1"):
        if route.startswith("resident"):
            monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
        assert diff_stats(_through(route, sc), want) == (0, 0), (chunk_rows, fast_limit, route)


@pytest.mark.parametrize("chunk_rows", ["8", "16", "32", "64"])
def test_row_headers_of_another_ranks_rows(chunk_rows, monkeypatch):
    """two handles, the tile-rows dealt between them: each writes 'not known here' headers for the other's rows"""
    from swf_renderer_amd import distributed as D
    sc, want = _rows_case()
    monkeypatch.setenv("SWFR_CHUNK_ROWS", chunk_rows)
    slabs = [D.extract_slab(_through("render", sc, band_index=rank, band_count=2), rank, 2) for rank in range(2)]
    assert diff_stats(np.asarray(D.assemble(slabs, ROWS_W, ROWS_H)), want) == (0, 0), chunk_rows
