"""Sampled rows whose cells k2_rows merges per (walk position, pixel column), pixel for pixel against the oracle.

A row that Cairo converts by sampling gives one cell of height +-1 per (boundary, sample row).  k2_tiles only ever adds a row's cells
per pixel column, so the sample pass of k2_rows adds the cells of neighbouring sample rows that fall into one column -- after the
clamping to the path's x_min / x_max -- into one cell before it stores them.  The frames here put sampled rows where that matters:
runs of fifteen (steep edges), runs of one or two over several tile columns (shallow edges), a merged cell left of the tile that
carries its height to the right, tips that share a pixel (runs that change edge and sign), crossings inside a row, cells clamped at
x_min and dropped at x_max, paths wider than 32 tile columns, rows of 9 .. 16 active edges (the sixteen-slot row kernel), rows that
keep more than sixteen cells (k2_tiles' tail rounds), a frame whose width is no multiple of 4 and whose last tile-row is cut.
Every geometry runs in both fill rules with opaque colours, translucent colours blended OVER and a translucent colour lerped onto
the clear surface, under every tile kernel instance and both row kernel instances; then a batch of random polygon frames through
render_batch.  The oracle alone says what a frame is; no tolerance: (0 pixels, 0 LSB)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import helpers  # noqa: E402
import scenarios  # noqa: E402
import test_tile_coverage as T  # noqa: E402
from helpers import diff_stats  # noqa: E402
from oracle import oracle_backend as ob  # noqa: E402

pytestmark = pytest.mark.gpu
EMU = bool(os.environ.get("SWFR_EMULATOR"))

poly = T.poly
W, H = 150, 40           # three tile columns, the last one cut at 150 (no multiple of 4); three tile rows, the last one cut at 40
WIDE_W, WIDE_H = 2118, 24  # 34 tile columns: a path over all of them is wider than the 32 the row kernel keeps masks for


def sawtooth(x, y0, n, dx=3.0, width=9.0):
    """a strip whose left and right sides have a vertex in every pixel row from y0 on: every row it touches is sampled"""
    left = [(x + dx * (k % 2), y0 + k + 0.45) for k in range(n)]
    right = [(x + width + dx * (k % 2), y0 + k + 0.55) for k in range(n)]
    return poly(left + right[::-1])


def frame_rect(w, h):
    return (0, 0, w, h)


FULL = frame_rect(W, H)
_spike_tips = [(70.3, 10.2), (70.6, 10.7), (70.1, 10.9), (70.8, 10.4), (70.5, 10.6), (70.2, 10.5), (70.7, 10.3), (70.4, 10.8)]

# name -> (width, height, [(edge rows, rectangle)])
GEOMETRIES = {
    # vertical and near-vertical sides through rows that the sawtooth makes sampled: runs of fifteen, merged heights +-15, between
    # analytic rows above and below  (a frame whose paths all have at most 32 edges runs the eight-slot row kernel unless the sixteen-slot
    # one is asked for: the sawtooths are short)
    "vertical": (W, H, [(poly([(20.3, 1.2), (60.5, 2.7), (60.5, 38.6), (21.1, 37.4)]) + sawtooth(100.2, 6, 12), FULL),
                        (poly([(30.0, 4.5), (31.0, 4.5), (31.0, 35.5), (30.0, 35.5)]) + sawtooth(40.6, 11, 13, dx=0.4, width=0.7), FULL)]),
    # shallow edges that start and end inside rows: runs of one or two cells over two and three tile columns, up to the frame's
    # last column and last row
    "shallow": (W, H, [(poly([(5.2, 10.3), (149.7, 12.1), (149.7, 12.9), (5.2, 11.2)]), FULL),
                       (poly([(50.4, 20.6), (140.3, 21.4), (58.8, 22.7)]), FULL),
                       (poly([(2.6, 37.3), (148.2, 38.2), (120.5, 39.8), (30.1, 39.4)]), FULL)]),
    # steep sides in the first tile column, sampled in every row, whose merged heights carry into the tiles to their right
    "left_carry": (W, H, [(poly([(10.4, 3.3), (140.2, 4.6), (138.8, 35.2), (12.9, 33.7)]) + sawtooth(30.3, 5, 13, dx=0.8, width=12.0), FULL),
                          (poly([(3.7, 8.1), (3.9, 30.8), (149.2, 29.6), (147.4, 9.2)]) + sawtooth(16.1, 13, 12, dx=5.0, width=2.0), FULL)]),
    # spikes whose tips share pixel (70, 10), up and down, wound both ways: at one walk position the runs change edge and sign
    "spikes": (W, H, [(sum((poly([t, (70.0 + 12 * (i - 3.5), 0.3 + 0.1 * i), (70.9 + 12 * (i - 3.5), 0.2)]) if i % 2 == 0 else
                            poly([t, (70.9 + 11 * (i - 3.5), 30.2), (70.0 + 11 * (i - 3.5), 30.4 + 0.1 * i)])
                            for i, t in enumerate(_spike_tips)), []) +
                       poly([(70.45, 10.1), (70.25, 0.4), (70.65, 0.6)]) + poly([(70.45, 10.9), (70.65, 25.2), (70.25, 25.4)]), FULL),
                      (poly([(60.2, 5.3), (80.9, 6.1), (70.45, 14.7)]) + poly([(65.1, 8.2), (70.2, 12.4), (75.7, 8.9)]) +
                       poly([(70.15, 10.35), (70.85, 10.45), (70.5, 10.95)]) + poly([(70.2, 10.6), (70.55, 10.15), (70.8, 10.7)]), FULL)]),
    # edges that cross inside pixel rows: the order of a row's cells changes between its sample rows
    "self_intersections": (W, H, [(poly([(10.2, 3.1), (90.7, 30.4), (92.3, 3.6), (8.8, 31.2)]), FULL),
                                  (poly([(75.0, 2.2), (95.3, 37.6), (44.1, 15.4), (106.2, 14.9), (55.6, 38.1)]), FULL),
                                  (poly([(100.3, 20.2), (145.6, 20.9), (100.9, 21.6), (146.1, 20.1), (146.3, 22.4), (100.1, 22.0)]), FULL)]),
    # rectangles that cut the path inside a tile and a strip: cells clamped to x_min, cells at and beyond x_max
    "clamped": (W, H, [(poly([(20.3, 1.2), (60.5, 2.7), (60.5, 38.6), (21.1, 37.4)]) + sawtooth(44.2, 4, 13), (25, 5, 58, 21)),
                       (poly([(5.2, 10.3), (149.7, 12.1), (149.7, 16.9), (5.2, 15.2)]) + sawtooth(61.2, 8, 10, dx=2.5, width=4.0), (0, 0, 64, H)),
                       (poly([(18.4, 2.5), (110.7, 6.3), (104.6, 38.2), (23.3, 36.1)]) + sawtooth(95.5, 12, 13, dx=4.0, width=8.0), (21, 3, 101, 37)),
                       (poly([(70.3, 22.2), (149.9, 24.1), (149.6, 39.7), (66.1, 38.3)]) + sawtooth(125.2, 25, 13, dx=1.0, width=6.0), (66, 22, 127, 38))]),
    # a sampled row that keeps more than sixteen cells after the merge: six shallow edges, each in another column per sample row
    "many_cells": (W, H, [(poly([(3.2, 10.3), (148.7, 12.1), (148.7, 12.6), (3.2, 10.8)]) + poly([(4.1, 12.2), (147.3, 10.4), (147.3, 10.9), (4.1, 12.7)]) +
                           poly([(2.5, 11.1), (149.4, 11.6), (149.4, 12.3), (2.5, 11.9)]), FULL),
                          (poly([(6.2, 30.4), (140.8, 33.3), (6.2, 33.9)]) + poly([(143.6, 30.2), (8.9, 31.7), (143.6, 32.8)]), FULL)]),
    # fourteen active edges in sampled rows: five leaning stripes and the sawtooth's four (two of its edges meet in every row), every
    # row sampled (the sixteen-slot instance of the row kernel where it is asked for; the queued-row kernels otherwise)
    "many_edges": (W, H, [(sum((poly([(8.3 + 25 * i, 2.4 + 0.3 * i), (14.6 + 25 * i, 2.9), (16.2 + 25 * i, 37.1), (9.9 + 25 * i, 36.6 - 0.2 * i)])
                                for i in range(5)), []) + sawtooth(141.3, 1, 37, dx=1.5, width=4.0), FULL)]),
    # a path wider than 32 tile columns, sampled in every row
    "wide": (WIDE_W, WIDE_H, [(poly([(3.3, 2.2), (2110.6, 3.7), (2105.2, 20.9), (9.1, 18.4)]) + sawtooth(1000.4, 1, 21, dx=2.0, width=30.0) +
                               sawtooth(2080.7, 1, 21, dx=0.5, width=3.0), frame_rect(WIDE_W, WIDE_H)),
                              (poly([(40.5, 5.5), (2100.5, 9.4), (2100.5, 10.2), (40.5, 6.6)]), (33, 0, 2090, WIDE_H))]),
}

COLOURS = T.COLOURS


def groups_of(geometry, colour, even_odd):
    w, h, paths = GEOMETRIES[geometry]
    back, argb = COLOURS[colour]
    out = [(poly([(0, 0), (w, 0), (w, h), (0, h)]), False, back, frame_rect(w, h))] if back is not None else []
    return out + [(edges, even_odd, argb, rect) for edges, rect in paths]


@functools.lru_cache(maxsize=None)
def oracle(geometry, colour, even_odd):
    w, h, _ = GEOMETRIES[geometry]
    be = ob.OracleBackend(w, h)
    try:
        for edges, eo, argb, rect in groups_of(geometry, colour, even_odd):
            be.fill_edges(np.array([r + (0,) for r in edges], dtype=np.int32), rect, eo, argb)
        return be.premultiplied_rgba()
    finally:
        be.close()


def product(geometry, colour, even_odd):
    import swf_renderer_amd as S
    w, h, _ = GEOMETRIES[geometry]
    r = S.Renderer(w, h)
    try:
        r.render_edges(*T.frame(groups_of(geometry, colour, even_odd)))
        st = r.stats()
        assert all(st[k] == 0 for k in ("pairtest_limit", "start_group_limit", "history_limit")), st
        return r.read_image(premultiplied=True)
    finally:
        r.close()


@pytest.mark.parametrize("rows", ["narrow", "wide"])
@pytest.mark.parametrize("tiles", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("colour", sorted(COLOURS))
@pytest.mark.parametrize("even_odd", [False, True], ids=["nonzero", "evenodd"])
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_merged_sampled_rows_vs_oracle(gpu, monkeypatch, geometry, even_odd, colour, tiles, rows):
    monkeypatch.setenv("SWFR_TILES_SHADERS", str(tiles))          # the tile kernel instance (solid, + bitmaps, + gradients, + operators, + groups)
    monkeypatch.setenv("SWFR_ROWS_WIDE", "1" if rows == "wide" else "0")     # the row kernel instance (eight / sixteen slots)
    want = oracle(geometry, colour, even_odd)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 8          # (edge pixels: many partial coverages)
    got = product(geometry, colour, even_odd)
    assert diff_stats(got, want) == (0, 0), (geometry, even_odd, colour, tiles, rows)


def test_the_two_fill_rules_differ_on_the_overlapping_geometries(gpu):
    for name in ("spikes", "self_intersections", "left_carry"):
        assert (oracle(name, "lerp", False) != oracle(name, "lerp", True)).any(), name


# ---------------------------------------------------------------------------------------------------------------- random frames
BW, BH = 90, 40          # (two tile columns, the second cut; the last tile-row cut)


def rand_frame(rng):
    """a few small polygons -- triangles to heptagons, thin slivers and spikes among them -- with vertices anywhere inside rows"""
    kids = []
    for _ in range(int(rng.integers(2, 6))):
        n = int(rng.integers(3, 8))
        cx, cy = rng.uniform(-5, BW + 5), rng.uniform(-5, BH + 5)
        sx, sy = rng.choice([0.6, 3.0, 12.0, 40.0]), rng.choice([0.6, 3.0, 12.0, 40.0])
        pts = np.stack([cx + rng.normal(0, sx, n), cy + rng.normal(0, sy, n)], axis=1)
        rgba = (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.choice([255, 255, 160, 60])))
        kids.append({"type": "shape", "definition": scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": scenarios._rgba(*rgba)})})
    return {"children": kids}


@pytest.mark.parametrize("even_odd", [False, True], ids=["nonzero", "evenodd"])
def test_random_polygon_frames_through_render_batch(gpu, monkeypatch, even_odd):
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    monkeypatch.delenv("SWFR_ROWS_WIDE", raising=False)
    rng = np.random.default_rng(20240 + int(even_odd))
    n = 12 if EMU else 300
    stages = [rand_frame(rng) for _ in range(n)]
    wants = [helpers.oracle_render(dict(width=BW, height=BH, even_odd=even_odd, stage=st)) for st in stages]
    assert sum(int(((w[..., 3] > 0) & (w[..., 3] < 255)).any()) for w in wants) > n // 2
    import swf_renderer_amd as S
    r = S.Renderer(BW, BH, even_odd=even_odd)
    try:
        if not EMU:                                               # (device tensors need the GPU)
            import torch
            out = torch.zeros((n, BH, BW, 4), dtype=torch.uint8, device="cuda")
            r.render_batch(stages, out.data_ptr(), BH * BW * 4)
            got = out.cpu().numpy()
            bad = [(k, diff_stats(got[k], wants[k])) for k in range(n) if diff_stats(got[k], wants[k]) != (0, 0)]
            assert not bad, bad[:8]
        for cut in (1, n // 2, n):                                # the per-frame route leaves the last frame in the handle
            r.render_batch(stages[:cut])
            assert diff_stats(r.read_image(premultiplied=True), wants[cut - 1]) == (0, 0), cut
    finally:
        r.close()
