"""The walk of k2_tiles over a strip's band entries, at the places its code branches: the order of the kinds of entry, the staging
round, the class-byte chunk, the two framebuffer store routes, and the rounded products of the compacted blend.

Every frame is compared with the oracle, zero differing bytes.  The frames are the smallest at which the code can go wrong:

* store routes: 192x24 (three tile columns, every strip inside the frame: two 16-byte stores per lane) and 130x20 (a width that is
  no multiple of 4: per-pixel stores; the last tile column and the last strip cut by the frame);
* entry order: one tile-row whose strips hold 1, 16, 17, 33 and 70 non-empty entries above the opaque cover of the whole frame --
  across the staging round (T3_LIST = 16) and, the band list of the tile-row being some 140 paths long, across the class-byte chunks
  (64 entries) and the two chunks fetched up front.  The lists are built from three kinds of entry -- rectilinear boxes (CLS_BOX),
  partial tor paths, full covers (a translucent one over all eight rows: coverage 255 through the blend; an opaque or translucent one
  that the path's rectangle cuts inside the strip: the row tests; boxes in one half of the strip's rows only) -- in the cyclic order
  B B P P F F B F P, in which each of the nine ordered pairs of kinds is adjacent, box after box included;
* rounding: slivers one pixel column wide whose coverage runs through every value 1 .. 254, in colours and over backgrounds whose
  channels are 0, 1, 127, 128, 254 and 255, opaque (Cairo's SOURCE lerp, 0x7f rounding) and translucent (pixman's OVER, 0x80).

Run modes: every instance of the kernel (SWFR_TILES_SHADERS 0 .. 4), one wavefront per strip, two strips per wavefront (the paired
shape of large frames) and a handful of persistent wavefronts (SWFR_TILES_GRID), through render, render_resident and render_batch.
The file also passes under the emulator (tools/emu/run.py tests/test_tile_walk_gpu.py)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import scenarios  # noqa: E402
from helpers import diff_stats, oracle_render, product_render  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_W, TILE_H, STRIP_H, XCDS = 64, 16, 8, 8
ORDER = "BBPPFFBFP"                      # cyclic: BB BP PP PF FF FB BF FP PB
LIST_LENGTHS = (1, 16, 17, 33, 70)
CHANNELS = (0, 1, 127, 128, 254, 255)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


def _shape(pts_px, rgba):
    return {"type": "shape", "definition": scenarios._poly_shape(np.rint(np.asarray(pts_px, float) * 20), {"type": "solid", "color": scenarios._rgba(*rgba)})}


def _cover(W, H, rgba):
    """an opaque or translucent tor path that covers every pixel of a W x H frame"""
    return _shape([(-0.6 * W - 9, -7.0), (1.9 * W, -5.0), (0.5 * W, 3.3 * H + 40)], rgba)


def _paired_grid(W, H):
    """SWFR_TILES_GRID that makes every wavefront of a W x H frame paint two slots of the launch list"""
    tiles_x, tile_rows = (W + TILE_W - 1) // TILE_W, (H + TILE_H - 1) // TILE_H
    slots = XCDS * ((tile_rows + XCDS - 1) // XCDS) * (TILE_H // STRIP_H) * tiles_x
    return str((slots + 1) // 2)


# ---- scenes
def store_scene(W, H):
    """Pixels that differ everywhere: a translucent cover on the clear frame, an opaque triangle, a translucent box, a sliver."""
    kids = [_cover(W, H, (40, 90, 200, 150)),
            _shape([(3.3, 1.2), (W - 2.6, 0.4 * H), (0.35 * W, H - 0.7)], (230, 120, 10, 255)),
            _shape([(0.2 * W + 0.35, 2.25), (W + 3.0, 2.25), (W + 3.0, H - 1.4), (0.2 * W + 0.35, H - 1.4)], (10, 200, 90, 77)),
            _shape([(-2.0, H - 6.1), (W + 1.0, H - 9.0), (W + 1.0, H - 7.8)], (255, 255, 255, 254))]
    return dict(width=W, height=H, stage={"children": kids})


def _entry(kind, k, x0, ty0):
    """Entry number k of a list, of kind B, P or F, inside the strip of rows ty0 .. ty0 + 7 of the tile column at x0.  Full covers reach
    22 .. 40 pixels into the neighbouring (spacer) columns on slanted sides, so that they are tor paths; nothing leaves the strip's rows."""
    alpha = (255, 140, 255, 31, 254, 1)[k % 6]
    col = ((37 * k) % 256, (91 * k + 50) % 256, (17 * k + 200) % 256, alpha)
    if kind == "B":
        xa, xb = x0 + (5 * k) % 40 + 0.35, x0 + 22 + (7 * k) % 42 + 0.6
        rows = [(0.25, 7.5), (0.0, 3.75), (4.3, 7.6), (2.0, 6.0), (0.0, 8.0)][k % 5]        # (1: the rows g only; 2: the rows g + 4 only)
        return _shape([(xa, ty0 + rows[0]), (xb, ty0 + rows[0]), (xb, ty0 + rows[1]), (xa, ty0 + rows[1])], col)
    if kind == "P":
        p = x0 + 4 + (11 * k) % 48
        return _shape([(p + 0.4, ty0 + 0.3 + (k % 3)), (p + 9.0 + (k % 7), ty0 + 7.6), (p - 3.3, ty0 + 5.1)], col)
    top = (0, 2, 4, 0, 5)[k % 5]                       # 0: all eight rows; else the path's rectangle starts inside the strip
    if alpha == 255 and top == 0:
        top = 3                                        # (an opaque cover of all eight rows would be the strip's StripTop cover: a shorter list)
    bottom = 8 if k % 4 else 6
    return _shape([(x0 - 30, ty0 + top), (x0 + TILE_W + 25, ty0 + top), (x0 + TILE_W + 40, ty0 + bottom), (x0 - 22, ty0 + bottom)], col)


def walk_scene():
    """Five lists (LIST_LENGTHS) in the tile columns 0, 2, 4, 6, 8 of the strip of rows 8 .. 15, over an opaque cover of the frame."""
    W, H = 9 * TILE_W, 24
    kids = [_cover(W, H, (200, 60, 120, 90)), _cover(W, H, (12, 34, 56, 255))]
    k = 0
    for c, n in enumerate(LIST_LENGTHS):
        for i in range(n):
            kids.append(_entry(ORDER[(i + c) % len(ORDER)], k, 2 * c * TILE_W, STRIP_H))
            k += 1
    return dict(width=W, height=H, stage={"children": kids})


def sliver_columns(x0, y0):
    """three slivers one pixel column wide and 256 rows long, on steep edges (the coverage of a pixel is the width left of the edge,
    in 1 / 256 of a pixel, averaged over the row's fifteen sample rows): 255 .. 0 falling, rising, and falling from half a step"""
    return [[(x0, y0), (x0 + 1, y0), (x0, y0 + 256)],
            [(x0 + 2, y0), (x0 + 2, y0 + 256), (x0 + 1, y0 + 256)],
            [(x0 + 2, y0 + 0.5), (x0 + 3, y0 + 0.5), (x0 + 2, y0 + 256.5)]]


def rounding_scene(alpha):
    """36 bands of three columns: the background of band (b, f) is CHANNELS rotated by b (none in the bands of b = 0: the clear frame),
    the slivers' colour CHANNELS rotated by f with alpha `alpha`."""
    W, H = 36 * 3, 260
    kids = []
    for b in range(6):
        for f in range(6):
            x0 = 3 * (6 * b + f)
            if b:
                kids.append(_shape([(x0, 0), (x0 + 3, 0), (x0 + 3, H), (x0, H)], (CHANNELS[b], CHANNELS[(b + 2) % 6], CHANNELS[(b + 4) % 6], 255)))
            for tri in sliver_columns(x0, 2):
                kids.append(_shape(tri, (CHANNELS[f], CHANNELS[(f + 1) % 6], CHANNELS[(f + 3) % 6], alpha)))
    return dict(width=W, height=H, stage={"children": kids})


_WANT = {}


def _want(key, sc):
    if key not in _WANT:
        _WANT[key] = oracle_render(sc)
    return _WANT[key]


def _exact(got, want, msg):
    assert diff_stats(got, want) == (0, 0), msg


GRIDS = ["default", "one_per_strip", "paired", "seven"]


def _use(monkeypatch, shaders, grid, sc):
    monkeypatch.setenv("SWFR_TILES_SHADERS", str(shaders))
    if grid == "default":
        monkeypatch.delenv("SWFR_TILES_GRID", raising=False)
    else:
        monkeypatch.setenv("SWFR_TILES_GRID", {"one_per_strip": "100000", "paired": _paired_grid(sc["width"], sc["height"]), "seven": "7"}[grid])


def _all_routes(sc, want, msg):
    """render, render_resident (two frames in flight, then one more) and render_batch (three frames, the per-frame target)"""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    _exact(product_render(sc), want, ("render",) + msg)
    host = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
    scene = host.build_frame(sc["stage"])
    host.close()
    r = S.Renderer(sc["width"], sc["height"])
    try:
        r.upload_edges(*scene)
        for frames in (3, 1):
            r.render_resident(frames)
            _exact(r.read_image(premultiplied=True), want, ("resident", frames) + msg)
        r.render_batch([sc["stage"]] * 3)
        _exact(r.read_image(premultiplied=True), want, ("batch",) + msg)
    finally:
        r.close()


# ---- 1. the store routes
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shaders", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("size", [(192, 24), (130, 20)], ids=["192x24", "130x20"])
def test_store_routes(size, shaders, grid, monkeypatch):
    sc = store_scene(*size)
    _use(monkeypatch, shaders, grid, sc)
    _all_routes(sc, _want(("store", size), sc), (size, shaders, grid))


# ---- 2. the order of the kinds of entry
def test_walk_scene_is_what_it_is_for():
    """The oracle's frame shows the lists: in the strip of rows 8 .. 15 the columns of the lists differ from the cover below them, the
    other strips are the cover's colour; the order string holds the nine ordered pairs."""
    assert {ORDER[i] + ORDER[(i + 1) % len(ORDER)] for i in range(len(ORDER))} == {a + b for a in "BPF" for b in "BPF"}
    sc = walk_scene()
    want = _want("walk", sc)
    cover = np.array([12, 34, 56, 255], np.uint8)
    assert (want[:STRIP_H] == cover).all() and (want[2 * STRIP_H:] == cover).all()
    for c in range(len(LIST_LENGTHS)):
        assert (want[STRIP_H:2 * STRIP_H, 2 * c * TILE_W:(2 * c + 1) * TILE_W] != cover).any(), c


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shaders", [0, 1, 2, 3, 4])
def test_entry_order(shaders, grid, monkeypatch):
    sc = walk_scene()
    _use(monkeypatch, shaders, grid, sc)
    _all_routes(sc, _want("walk", sc), (shaders, grid))


# ---- 3. the rounded products
def test_slivers_reach_every_coverage():
    """Opaque white slivers on the clear frame: the alpha channel is the coverage itself."""
    kids = [_shape(tri, (255, 255, 255, 255)) for tri in sliver_columns(0, 2)]
    want = oracle_render(dict(width=3, height=260, stage={"children": kids}))
    assert set(range(1, 255)) <= set(np.unique(want[..., 3]).tolist())


@pytest.mark.parametrize("shaders", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("alpha", [255, 254, 128, 1])
def test_rounding(alpha, shaders, monkeypatch):
    sc = rounding_scene(alpha)
    _use(monkeypatch, shaders, "default", sc)
    _exact(product_render(sc), _want(("rounding", alpha), sc), (alpha, shaders))
