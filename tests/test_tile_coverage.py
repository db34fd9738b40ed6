"""The coverage arithmetic of k2_tiles' partial tor paths, pixel for pixel against the oracle.

A partial (path, strip) pair accumulates each cell of a row into `acc` as two deltas of Cairo's coverage numerator
N(x) = 512 * H(x) - ua(x): 17 * (512 h - ua) at the cell's column, 17 * ua one column to the right (dropped beyond the tile's last
column), and a cell left of the tile as 17 * 512 h in column 0.  One scan per pixel row, alpha = bits 9 .. 16 of 17 N + 256.
Rows outside the path's rectangle get no cells; columns at or beyond its x_max are masked.  The frames here put cells where those
rules matter: many edges through one pixel, heights carried in from the tile to the left, cells in a tile's last column, x_max and
row limits inside a tile or strip.  Each geometry is drawn in both fill rules with opaque colours, translucent colours blended OVER
and a translucent colour lerped onto the clear surface, under all three tile kernel instances; then once in the aliased mode
(against tests/mono_model.py) and once under colour transforms (against the lowered oracle)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mono_model as M  # noqa: E402
import scenarios  # noqa: E402
from helpers import diff_stats  # noqa: E402
from oracle import oracle_backend as ob  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 150, 24          # three tile columns (the last one cut at 150, not a multiple of 4), two tile rows (the last one cut at 24)


def poly(pts):
    """edge rows (x1, y1, x2, y2, top, bottom, dir) in 24.8 of the closed polygon through `pts` (pixels)"""
    q = [(int(round(x * 256)), int(round(y * 256))) for x, y in pts]
    rows = []
    for a, b in zip(q, q[1:] + q[:1]):
        if a[1] < b[1]:
            rows.append((a[0], a[1], b[0], b[1], a[1], b[1], 1))
        elif a[1] > b[1]:
            rows.append((b[0], b[1], a[0], a[1], b[1], a[1], -1))
    return rows


FULL = (0, 0, W, H)

# geometry: a list of paths, each (edge rows, rectangle (x_min, y_min, x_max, y_max))
GEOMETRIES = {
    # thin spikes whose tips share pixel (70, 10), one tip in each neighbouring row and a spike through the pixel column; a triangle
    # over the tips wound the same way (winding 2 there) and one wound the other way (winding 0)
    "crossings": [(poly([(70.3, 10.2), (40.5, 1.5), (44.7, 2.1)]) + poly([(70.6, 10.7), (100.2, 3.3), (96.1, 1.2)]) +
                   poly([(70.1, 10.9), (45.2, 22.8), (52.9, 23.5)]) + poly([(70.8, 10.4), (110.5, 21.7), (104.3, 23.9)]) +
                   poly([(70.5, 11.6), (20.2, 12.3), (22.8, 15.9)]) + poly([(71.2, 9.3), (130.7, 8.6), (128.1, 4.4)]) +
                   poly([(70.4, 10.5), (70.9, 0.2), (69.6, 0.4)]) +
                   poly([(60.2, 5.3), (80.9, 6.1), (70.45, 14.7)]) + poly([(65.1, 8.2), (70.2, 12.4), (75.7, 8.9)]), FULL)],
    # slanted sides left of a tile whose heights reach the tiles to their right; a long shallow band (more than sixteen cells per row)
    "left_carry": [(poly([(10.3, 2.2), (140.6, 5.1), (146.9, 21.4), (30.7, 19.8)]), FULL),
                   (poly([(50.2, 1.0), (90.8, 22.6), (20.1, 23.0)]), FULL),
                   (poly([(5.5, 12.2), (145.5, 13.9), (145.5, 16.0), (5.5, 15.1)]), FULL)],
    # edges inside a tile's last column (63, 127) and the frame's last column (149): their uncovered area would land one column on
    "last_column": [(poly([(40.2, 1.3), (63.37, 1.3), (63.81, 22.7), (40.2, 22.7)]), FULL),
                    (poly([(63.55, 4.4), (120.3, 4.4), (120.3, 12.8), (63.2, 12.8)]), FULL),
                    (poly([(100.5, 3.2), (127.6, 2.9), (127.2, 20.1), (110.1, 19.5)]), FULL),
                    (poly([(120.0, 6.5), (149.7, 6.5), (149.4, 17.5), (120.0, 17.5)]), FULL)],
    # rectangles that cut the polygon inside a tile: x_max at 100, 64 and 127 where the coverage is still non-zero, x_min at 30
    "x_limits": [(poly([(20.7, 2.6), (140.2, 4.1), (135.5, 21.2), (15.3, 20.4)]), (30, 0, 100, H)),
                 (poly([(2.4, 5.5), (90.6, 3.3), (80.2, 9.7)]), (0, 0, 64, H)),
                 (poly([(60.3, 14.2), (149.6, 12.8), (140.1, 23.6), (70.9, 22.9)]), (45, 0, 127, H))],
    # rows that start and end inside strips: by the rectangle (rows 3 .. 12, row 9 alone) and by the polygon itself (rows 4 .. 19)
    "row_limits": [(poly([(10.2, 2.3), (140.1, 3.4), (130.6, 21.7), (5.9, 20.1)]), (0, 3, W, 13)),
                   (poly([(30.4, 5.6), (90.2, 4.7), (80.3, 19.4)]), FULL),
                   (poly([(95.5, 0.5), (148.2, 7.3), (120.1, 23.8)]), (0, 9, W, 10))],
}

BACKDROP = poly([(0, 0), (W, 0), (W, H), (0, H)])
# (backdrop colour or None, path colour) as premultiplied ARGB: the first path on the clear surface blends with the lerp rule
COLOURS = {"opaque": (0x80402010, 0xff1f6fbf), "translucent": (0xff204080, 0x9a5a3a1a), "lerp": (None, 0x60301806)}


def groups_of(geometry, colour, even_odd):
    back, argb = COLOURS[colour]
    out = [(BACKDROP, False, back, FULL)] if back is not None else []
    return out + [(edges, even_odd, argb, rect) for edges, rect in GEOMETRIES[geometry]]


def frame(groups):
    """(edges, paths, styles) for Renderer.render_edges: one tor path per group, painted in order; the first path and opaque ones
    blend with the lerp rule"""
    from swf_renderer_amd import api
    rows, paths, styles = [], np.zeros(len(groups), api.PATH_DTYPE), []
    for i, (edges, eo, argb, rect) in enumerate(groups):
        e = np.zeros(len(edges), api.EDGE_DTYPE)
        for k, name in enumerate(("x1", "y1", "x2", "y2", "top", "bottom", "dir")):
            e[name] = [r[k] for r in edges]
        e["reserved"] = i
        paths[i] = (sum(len(r) for r in rows), len(e), api.PATH_TOR, int(eo), i, int((argb >> 24) == 255 or i == 0)) + tuple(rect)
        rows.append(e)
        styles.append(api.solid_style(argb))
    return np.concatenate(rows), paths, styles


def oracle(groups):
    be = ob.OracleBackend(W, H)
    try:
        for edges, eo, argb, rect in groups:
            e = np.array([r + (0,) for r in edges], dtype=np.int32)
            be.fill_edges(e, rect, eo, argb)
        return be.premultiplied_rgba()
    finally:
        be.close()


def product(groups, **kw):
    import swf_renderer_amd as S
    r = S.Renderer(W, H, **kw)
    try:
        r.render_edges(*frame(groups))
        return r.read_image(premultiplied=True)
    finally:
        r.close()


@pytest.mark.parametrize("tiles", [0, 1, 2])
@pytest.mark.parametrize("colour", sorted(COLOURS))
@pytest.mark.parametrize("even_odd", [False, True], ids=["nonzero", "evenodd"])
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_partial_coverage_vs_oracle(gpu, monkeypatch, geometry, even_odd, colour, tiles):
    monkeypatch.setenv("SWFR_TILES_SHADERS", str(tiles))          # the tile kernel instance (solid, + bitmaps, + gradients)
    groups = groups_of(geometry, colour, even_odd)
    want = oracle(groups)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 8          # (edge pixels: many partial coverages)
    got = product(groups)
    assert diff_stats(got, want) == (0, 0), (geometry, even_odd, colour, tiles)


def test_fill_rules_differ_where_the_spikes_cross(gpu):
    """the crossing geometry has pixels of winding 2: the two rules must not draw the same frame"""
    a, b = (oracle(groups_of("crossings", "lerp", eo)) for eo in (False, True))
    assert (a != b).any()


@pytest.mark.parametrize("even_odd", [False, True], ids=["nonzero", "evenodd"])
def test_aliased_geometries_vs_model(gpu, even_odd):
    groups = []
    for i, name in enumerate(("crossings", "last_column", "x_limits", "row_limits")):
        argb = (0xff1f6fbf, 0x9a5a3a1a, 0x60301806, 0xff80c040)[i]
        groups += [(edges, even_odd, argb, rect) for edges, rect in GEOMETRIES[name]]
    fr = frame(groups)
    want = M.render(*fr, W, H)
    assert (want[..., 3] > 0).any()
    got = product(groups, antialias="none")
    assert diff_stats(got, want) == (0, 0)


@pytest.mark.parametrize("transform", ["tint", "fade"])
@pytest.mark.parametrize("even_odd", [False, True], ids=["nonzero", "evenodd"])
def test_colour_transform_vs_lowered_oracle(gpu, even_odd, transform):
    import make_cxform_goldens as G
    kids = []
    shapes = [([(40.2, 1.3), (63.37, 1.3), (63.81, 22.7), (40.2, 22.7)], (31, 97, 191, 255)),
              ([(20.7, 2.6), (140.2, 4.1), (135.5, 21.2), (15.3, 20.4)], (200, 90, 40, 160)),
              ([(70.3, 10.2), (40.5, 1.5), (130.7, 8.6), (60.2, 5.3), (80.9, 6.1), (45.2, 22.8)], (20, 180, 60, 255))]
    for pts, rgba in shapes:
        twips = np.rint(np.array(pts) * 20)
        kids.append({"type": "shape", "definition": scenarios._poly_shape(twips, {"type": "solid", "color": scenarios._rgba(*rgba)})})
    sc = dict(width=W, height=H, even_odd=even_odd, stage={"children": kids})
    stage = G.apply_transform(sc["stage"], transform)
    want = G.oracle_cxform(sc, stage)
    assert ((want[..., 3] > 0) & (want[..., 3] < 255)).any()
    import swf_renderer_amd as S
    r = S.Renderer(W, H, even_odd=even_odd)
    try:
        r.render(stage)
        got = r.read_image(premultiplied=True)
    finally:
        r.close()
    assert diff_stats(got, want) == (0, 0)
