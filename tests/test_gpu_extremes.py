"""The HIP path at the limits of its 24.8 coordinate range (end points up to +-32768 px = +-2^23): whole scenes against the oracle,
raw edge lists (swfr_render_edges) against the oracle's raw-edge entry swfo_fill_edges, the refusal just past the range, and
bitmap and gradient fills on geometry far off the frame.  Every case is bit-exact.

What reaches the magnitude claims of raster_common.hip (ex = 256 dx, dy = 7680 (y2 - y1); DX = dx, D = 30 (y2 - y1)):
- floor_div_inv's int32 quotient estimate (|a / b| < 2^31).  In edge_x_at the quotient is the edge's x offset from x1 in 24.8
  units, at most |dx| <= 2^24; reached by diagonal_limits and many_parallel_long_edges (|dx| near 2^24 over the whole range).
- make_dev_edge's fq (dy < 2^37, |ex| >= 256: below 2^28): largest for an edge 2^24 tall and 1/256 px wide -- steep_1_256.
- make_dev_edge's q15 (|ex| <= 2^32, dy >= 200 * 7680: below 2^25): largest for the shortest stepped edge, 200 units tall, about
  2^24 wide -- wide_q15.
- make_fast_edge's dqf / hq (512 DX / D): largest for D = 30, an edge 1 unit tall and about 2^24 wide -- wide_flat; its q15
  (7680 DX / D) -- wide_q15; its fq (256 D / 512 |DX|) -- steep_1_256.
- fast_x_at's A * DX < 2^53 (A = 512 s + 256 - 30 y1): largest with y1 = -2^23 and |DX| near 2^24 -- diagonal_limits.
Each raw case runs under the default route, the 64-bit DevEdge route (SWFR_FAST_LIMIT=0) and 8-row chunks (SWFR_CHUNK_ROWS=8);
the scene fuzz (test_extreme_scenes_vs_oracle) reaches the same helpers through the frame builder."""
import os
import zlib

import numpy as np
import pytest

import scenarios
from helpers import LARGE_MODES, diff_stats, extreme_scene, oracle_render, product_render, rand_raw_frame, raw_oracle, raw_product
from helpers import random_raw_pair as _random_pair  # noqa: F401  (tests/test_mono_gpu.py draws its raw edges with it)
from oracle import oracle_backend as ob

pytestmark = pytest.mark.gpu

L = 1 << 23                                   # +-32768 px in 24.8
ROUTES = [{}, {"SWFR_FAST_LIMIT": "0"}, {"SWFR_CHUNK_ROWS": "8"}]
ROUTE_IDS = ["default", "devedge", "chunk8"]
EMU = bool(os.environ.get("SWFR_EMULATOR"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


def _route(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _kind(img):
    a = img[..., 3]
    return "empty" if not a.any() else ("full" if (a == 255).all() else "partial")


# ---- a. whole scenes: fills, curves, strokes and box strokes whose geometry reaches the limits, HIP against the oracle
@pytest.mark.parametrize("env", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("mode", LARGE_MODES)
def test_extreme_scenes_vs_oracle(mode, env, monkeypatch):
    _route(monkeypatch, env)
    rng = np.random.default_rng(zlib.crc32(("gpu" + mode).encode()) % 1000)
    sizes = [(64, 48), (333, 97)] * 6 + ([] if EMU else [(1920, 1080)])
    kinds = {"empty": 0, "full": 0, "partial": 0}
    for it, (W, H) in enumerate(sizes):
        sc = extreme_scene(rng, W, H, mode)
        want = oracle_render(sc)
        assert diff_stats(product_render(sc), want) == (0, 0), (mode, env, it)
        kinds[_kind(want)] += 1
    assert kinds["partial"] >= len(sizes) // 2, kinds        # not only empty or fully covered frames


def test_extreme_scene_at_4k():
    if EMU:
        pytest.skip("a 4K frame is only a matter of time on the emulator")
    rng = np.random.default_rng(4096)
    for mode in LARGE_MODES:
        sc = extreme_scene(rng, 3840, 2160, mode)
        want = oracle_render(sc)
        assert diff_stats(product_render(sc), want) == (0, 0), mode


def test_rectilinear_stroke_near_the_limit_renders():
    """The square outline of tests/test_host.py::test_rectilinear_stroke_near_the_limit_stays_inside_the_range: it used to be refused
    (SWFR_ERR_INVALID, a box end point past 2^23).  Fully covered frame, and the partly covered one with the right side in the frame."""
    from test_host import _square_outline
    for sc, covered in ((_square_outline(), 64 * 48), (_square_outline(tx=-(32760 - 32) * 20, width=20), 34 * 48)):
        got = product_render(sc)
        assert diff_stats(got, oracle_render(sc)) == (0, 0)
        assert int((got[..., 3] > 0).sum()) == covered


# ---- b. raw edges through Renderer.render_edges against swfo_fill_edges
def _render_raw(W, H, groups):
    """groups: [(edge rows (x1, y1, x2, y2, top, bottom, dir), even_odd, premultiplied ARGB)], one path each with the frame as its
    rectangle.  Returns (HIP image, oracle image)."""
    return raw_product(W, H, groups), raw_oracle(W, H, groups)


FLAT_S = 14 + 15 * 10                         # sample rows s = 14 (mod 15) are centred 7/15 of a unit below an integer y (24.8)


def _flat_edge(s, dy, target, width=15_600_000):
    """An edge `width` units wide and `dy` units tall, active over [y1, y2), whose x at the centre of sample row s
    ((2 s + 1) * 128 / 15 in 24.8) is `target`: the centre lies in (y1, y2), about half way."""
    from fractions import Fraction
    import math
    c = Fraction((2 * s + 1) * 128, 15)
    y1 = math.floor(c - Fraction(dy, 2)) if dy > 1 else math.floor(c)
    x1 = round(target - (c - y1) / dy * width)
    assert -L <= x1 and x1 + width <= L and y1 < c < y1 + dy
    return (x1, y1, x1 + width, y1 + dy)


def _band(W, H, dy):
    """A closed band: its top edge (dy units tall, about 2^24 wide) crosses sample row FLAT_S at 0.4 W, its bottom edge crosses a
    sample row near the frame's bottom at 0.7 W; the sides join their ends far left and far right of the frame."""
    t = _flat_edge(FLAT_S, dy, int(0.4 * W * 256) + 37)
    b = _flat_edge(14 + 15 * (H - 6), dy, int(0.7 * W * 256) + 11)
    return [t + (t[1], t[3], 1), (t[2], t[3], b[2], b[3], t[3], b[3], 1), b + (b[1], b[3], -1), (t[0], t[1], b[0], b[1], t[1], b[1], -1)]


def _raw_cases(W, H):
    px = 256
    diag = (-L, -L, L, L)
    cases = {
        # end points exactly at +-2^23: the diagonal through the frame closed by the vertical at x = +2^23 (covered right of y = x)
        "diagonal_limits": [([diag + (-L, L, 1), (L, -L, L, L, -L, L, -1)], False, 0xff2080c0)],
        # vertical edges at x = -2^23 and x = +2^23 (alone: a fully covered frame), and one at -2^23 with the diagonal (left of y = x)
        "verticals_at_the_limits": [([(-L, -L, -L, L, -L, L, 1), (L, -L, L, L, -L, L, -1)], False, 0x80402010),
                                    ([(-L, -L, -L, L, -L, L, 1), diag + (-L, L, -1)], False, 0xc0c00000)],
        # a 1/256 px slope over 2^24 in y through the frame, closed at +2^23
        "steep_1_256": [([(int(W * 0.37 * px) + 3, -L, int(W * 0.37 * px) + 4, L, -L, L, 1), (L, -L, L, L, -L, L, -1)], False, 0xff00ff00),
                        ([(int(W * 0.61 * px), -L, int(W * 0.61 * px) - 1, L, -L, L, 1), (L, -L, L, L, -L, L, -1)], True, 0x60006000)],
        # a band whose top and bottom are edges about 2^24 wide and 1 unit (1/256 px) tall, each active in exactly one sample row and
        # crossing it inside the frame (dy = 1: the largest per-row steps dqf / hq of the fast route, D = 30)
        "wide_flat": [(_band(W, H, 1), False, 0xffa0a000)],
        # the same with edges 200 units tall: the shortest edge whose 15-sample-row step q15 is computed, |ex| near 2^32
        "wide_q15": [(_band(W, H, 200), True, 0xc0a000a0)],
        # active only over [top, bottom) strictly inside (y1, y2)
        "top_bottom_inside": [([(-L, -L, L, L, 5 * px + 3, (H - 7) * px - 11, 1),
                                (W * px - 700, -L, W * px - 700, L, 5 * px + 3, (H - 7) * px - 11, -1)], False, 0xff3060ff)],
        # never-active edges (top == bottom) beside an active pair: they change nothing
        "never_active": [([(0, 0, W * px, H * px, 9 * px, 9 * px, 1), (-L, -L, L, L, 0, 0, -1),
                           (3 * px, 0, 3 * px, H * px, 0, H * px, 1), (W * px - 5 * px + 17, 0, W * px - 5 * px + 17, H * px, 0, H * px, -1),
                           (7 * px, -L, 7 * px, L, 20 * px, 20 * px, 1)], False, 0xff777777)],
        # edges entirely left of the frame (their winding folds into column 0) closed inside it; entirely right of it, closed inside
        "left_and_right_of_the_frame": [([(-L, -L, -5 * px - 3, L, -L, L, 1), (int(W * 0.5 * px) + 9, 0, 11 * px, H * px, 0, H * px, -1)], False, 0xff00c0c0),
                                        ([(W * px + 1, -L, L, L, -L, L, -1), (int(W * 0.8 * px), 0, W * px - 3, H * px, 0, H * px, 1)], False, 0x9f5f0000)],
    }
    # 96 long parallel edges (slope about 1) crossing row 0 spread over the frame, directions alternating: more active edges per row
    # than the generic routine of k2_rows_slow holds (ROWS_BIG_MAXA = 64), with end points near +-2^23; stripes, partly covered
    many = []
    for k in range(96):
        x0, d = (2 * k + 1) * W * 128 // 96, L - W * 256 - 1000 * k
        many.append((x0 - d, -L, x0 + d, L, -L, L, 1 if k % 2 == 0 else -1))
    cases["many_parallel_long_edges"] = [(many, False, 0xff1090f0), (many, True, 0x80800080)]
    return cases


RAW_NAMES = sorted(_raw_cases(64, 48))


@pytest.mark.parametrize("env", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("name", RAW_NAMES)
def test_raw_edges_at_the_limits(name, env, monkeypatch):
    _route(monkeypatch, env)
    for W, H in ((64, 48), (333, 97)):
        got, want = _render_raw(W, H, _raw_cases(W, H)[name])
        assert diff_stats(got, want) == (0, 0), (name, W, H)
        # no case is an empty or a fully covered frame ("verticals_at_the_limits": its first path alone covers the frame, the
        # second makes it partial)
        assert _kind(want) == "partial", name
        if name.startswith("wide_"):
            # the flat top edge is active in sample row FLAT_S and crosses it inside the frame: that pixel row changes at its x
            e = _raw_cases(W, H)[name][0][0][0]
            assert (15 * e[4] + 128) >> 8 <= FLAT_S < (15 * e[5] + 128) >> 8
            row = want[FLAT_S // 15, :, 3].astype(int)
            x = int(0.4 * W)
            assert row[x - 2] != row[x + 2], (name, row)


@pytest.mark.parametrize("env", ROUTES, ids=ROUTE_IDS)
def test_random_raw_edges_anywhere_in_the_range(env, monkeypatch):
    """Seeded fuzz of raw edge lists that meet the validation rule (y1 < y2, y1 <= top < bottom <= y2, or never active) with end
    points anywhere in +-2^23, both fill rules, opaque and translucent paths painted in order."""
    _route(monkeypatch, env)
    rng = np.random.default_rng(2 ** 23)
    partial = 0
    for it in range(20 if EMU else 40):
        W, H, groups = rand_raw_frame(rng, it)
        got, want = _render_raw(W, H, groups)
        assert diff_stats(got, want) == (0, 0), (env, it)
        partial += _kind(want) == "partial"
    assert partial >= 10


# ---- c. the refusal boundary of swfr_upload_edges
def test_refusal_just_past_the_range_then_a_valid_frame():
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    W, H = 64, 48
    good = [(-L, -L, L, L, -L, L, 1), (L, -L, L, L, -L, L, -1)]
    bad_cases = {
        "x past 2^23": [(-L, -L, L + 1, L, -L, L, 1), (L, -L, L, L, -L, L, -1)],
        "x below -2^23": [(-L - 1, -L, L, L, -L, L, 1), (L, -L, L, L, -L, L, -1)],
        "y past 2^23": [(-L, -L, L, L + 1, -L, L, 1), (L, -L, L, L, -L, L, -1)],
        "top above y1": [(-L, 0, L, L, -1, L, 1), (L, -L, L, L, -L, L, -1)],
        "bottom below y2": [(-L, -L, L, H * 256, -L, H * 256 + 1, 1), (L, -L, L, L, -L, L, -1)],
    }
    r = S.Renderer(W, H)
    try:
        for name, edges in bad_cases.items():
            e = np.zeros(len(edges), api.EDGE_DTYPE)
            for k, f in enumerate(("x1", "y1", "x2", "y2", "top", "bottom", "dir")):
                e[f] = [row[k] for row in edges]
            paths = np.zeros(1, api.PATH_DTYPE)
            paths[0] = (0, len(e), api.PATH_TOR, 0, 0, 1, 0, 0, W, H)
            with pytest.raises(S.SwfrError) as ex:
                r.render_edges(e, paths, [api.solid_style(0xff102030)])
            assert ex.value.code == api.ERR_INVALID, name
        # the same handle: the last valid edges exactly at the limit, then a scene, bit-exact
        e = np.zeros(2, api.EDGE_DTYPE)
        for k, f in enumerate(("x1", "y1", "x2", "y2", "top", "bottom", "dir")):
            e[f] = [row[k] for row in good]
        paths = np.zeros(1, api.PATH_DTYPE)
        paths[0] = (0, 2, api.PATH_TOR, 0, 0, 1, 0, 0, W, H)
        r.render_edges(e, paths, [api.solid_style(0xff102030)])
        be = ob.OracleBackend(W, H)
        be.fill_edges(e, (0, 0, W, H), False, 0xff102030)
        want = be.premultiplied_rgba()
        be.close()
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0) and _kind(want) == "partial"
        sc = dict(extreme_scene(np.random.default_rng(1), W, H, "far"), even_odd=False)
        r.render(sc["stage"])
        assert diff_stats(r.read_image(premultiplied=True), oracle_render(sc)) == (0, 0)
    finally:
        r.close()


def test_open_finding_polygon_stroke_past_the_limit_is_currently_refused():
    """Pins the CURRENT behaviour of an open finding, not the intended one (tests/test_host.py::
    test_polygon_stroke_near_the_limit_stays_inside_the_range, a strict xfail): a stroke whose path lies inside +-32768 px gets clipped
    edges with end points past 2^23, and the device handle refuses the frame (SWFR_ERR_INVALID) rather than paint something else.
    The stroke should render; whoever fixes the frame builder replaces this test with a comparison against the oracle."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    from helpers import _fine_shape
    tag = _fine_shape([(20.0, 10.0), (32766.0, 32760.0)], None, None, line=scenarios._rgba(9, 99, 199), line_width_px=20.0, closed=False)
    sc = dict(width=64, height=48, stage={"children": [{"type": "shape", "definition": tag, "matrix": scenarios._m(1 / 256, 1 / 256)}]})
    with pytest.raises(S.SwfrError) as ex:
        product_render(sc)
    assert ex.value.code == api.ERR_INVALID


# ---- d. bitmap and radial gradient fills on geometry far off the frame
def _far_fill_scene(rng, W, H, kind):
    from helpers import large_pts, make_bitmap_tag
    mode = LARGE_MODES[int(rng.integers(0, len(LARGE_MODES)))]
    pts = np.array(large_pts(rng, W, H, int(rng.integers(3, 7)), mode)) * 20
    pts = np.clip(np.rint(pts), -32767 * 20, 32767 * 20)
    if kind == "bitmap":
        k = float(rng.uniform(0.3, 6.0))
        t = float(rng.uniform(-3.2, 3.2))
        c, s = np.cos(t), np.sin(t)
        fill = {"type": "bitmap", "bitmap_id": 3, "repeating": bool(rng.integers(0, 2)), "smoothed": True,
                "matrix": scenarios._m(20 * k * c, 20 * k * c, int(rng.integers(-200, W * 20)), int(rng.integers(-200, H * 20)), 20 * k * s, -20 * k * s)}
        bitmaps = [make_bitmap_tag(3, int(rng.integers(1, 40)), int(rng.integers(1, 40)), rng)]
    else:
        # the gradient circle centred in the frame and at least 0.6 frame diagonals wide (pixman's 16.16 range, README)
        sc_ = float(rng.uniform(0.6, 3.0)) * 20 / 16384 * float(np.hypot(W, H))
        t = float(rng.uniform(-3.2, 3.2))
        c, s = np.cos(t), np.sin(t)
        n = int(rng.integers(2, 6))
        cols = [(int(v), (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.choice([255, 128]))))
                for v in sorted(rng.integers(0, 256, n))]
        fill = {"type": "radial-gradient", "gradient": scenarios._grad(cols),
                "matrix": scenarios._m(sc_ * c, sc_ * c, int(rng.integers(0, W * 20)), int(rng.integers(0, H * 20)), sc_ * s, -sc_ * s)}
        bitmaps = []
    return dict(width=W, height=H, bitmaps=bitmaps, stage={"children": [{"type": "shape", "definition": scenarios._poly_shape(pts, fill)}]})


@pytest.mark.parametrize("kind", ["bitmap", "radial"])
def test_fills_on_geometry_far_off_the_frame(kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) % 1000)
    painted = 0
    for it in range(24):
        W, H = [(64, 48), (333, 97)][it % 2]
        sc = _far_fill_scene(rng, W, H, kind)
        want = oracle_render(sc)
        assert diff_stats(product_render(sc), want) == (0, 0), (kind, it)
        painted += int((want[..., 3] > 0).sum())
    assert painted > 20000
