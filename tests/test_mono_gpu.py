"""The aliased row pass (csrc/mono.hip: k2_rows_mono, and k2_rows_mono_huge for rows of more than MONO_NS = 16 crossings) against the
exact model of tests/mono_model.py, where kernels go wrong: end points at +-2^23, the 16-crossing route boundary, the columns next to a
path's x_min and x_max (k2_rows_mono_huge's bin 0 and bin W + 1), the 8 192-edge capacity, a full queue of huge rows and paths split at
8 192 columns.  Every comparison is bit-exact.  Also runs on the CPU emulator: `python tools/emu/run.py tests/test_mono_gpu.py -q`.

Padding: a pair of vertical edges at one x with opposite directions changes no winding, but its crossings count towards a row's 16, so
it moves the row to k2_rows_mono_huge.  It can still change the picture next to it (a span that closes one pixel before it is
continued), which the model knows; at pixel x_min - 1 or further left, or x_max + 1 or further right, it changes nothing inside
the path's columns."""
import os
import zlib

import numpy as np
import pytest

import mono_model as M
from helpers import GOLD, LARGE_MODES, diff_stats, extreme_scene
from test_gpu_extremes import _random_pair, _raw_cases
from test_mono_model import host_frame

pytestmark = pytest.mark.gpu

L = 1 << 23
U = 256
ROUTES = [{}, {"SWFR_CHUNK_ROWS": "8"}, {"SWFR_CHUNK_ROWS": "64"}]
ROUTE_IDS = ["default", "chunk8", "chunk64"]
EMU = bool(os.environ.get("SWFR_EMULATOR"))
FIELDS = ("x1", "y1", "x2", "y2", "top", "bottom", "dir")


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


def frame(W, H, groups):
    """groups: [(edge rows (x1, y1, x2, y2, top, bottom, dir), even_odd, premultiplied ARGB[, rect (x_min, y_min, x_max, y_max)])],
    one tor path each (the frame its rectangle unless given), painted in order: the first path and opaque ones blend with the lerp
    rule.  Returns (edges, paths, styles) as render_edges takes them."""
    from swf_renderer_amd import api
    rows, paths, styles = [], np.zeros(len(groups), api.PATH_DTYPE), []
    for i, g in enumerate(groups):
        edges, eo, argb = g[:3]
        rect = g[3] if len(g) > 3 else (0, 0, W, H)
        e = np.zeros(len(edges), api.EDGE_DTYPE)
        for k, name in enumerate(FIELDS):
            e[name] = [r[k] for r in edges]
        paths[i] = (sum(len(r) for r in rows), len(e), api.PATH_TOR, int(eo), i, int((argb >> 24) == 255 or i == 0)) + tuple(rect)
        rows.append(e)
        styles.append(api.solid_style(argb))
    return np.concatenate(rows), paths, styles


def gpu_render(W, H, fr, antialias="none", stats=None):
    import swf_renderer_amd as S
    r = S.Renderer(W, H, antialias=antialias)
    try:
        r.render_edges(*fr)
        if stats is not None:
            stats.update(r.stats())
        return r.read_image(premultiplied=True)
    finally:
        r.close()


def check(W, H, fr, stats=None):
    """the aliased GPU frame equals the model; returns it"""
    want = M.render(*fr, W, H)
    got = gpu_render(W, H, fr, stats=stats)
    assert diff_stats(got, want) == (0, 0)
    return got


def vpair(x, rows=(-L, L)):
    """a zero-winding pair of vertical edges at x (24.8), active over rows [rows[0], rows[1]) in 24.8"""
    return [(x, rows[0], x, rows[1], rows[0], rows[1], 1), (x, rows[0], x, rows[1], rows[0], rows[1], -1)]


def limit_pads(x_min, x_max):
    """padding at -2^23, x_min - 1, x_min, x_min + 1/2 (the 127/128 tie both ways), x_max - 1, x_max, x_max + 1 and +2^23: 18 crossings"""
    xs = (-L, (x_min - 1) * U, x_min * U, x_min * U + 128, x_min * U + 129, (x_max - 1) * U, x_max * U, (x_max + 1) * U, L)
    return [e for x in xs for e in vpair(x)]


def inert_pads(x_min, x_max):
    """padding that changes nothing inside [x_min, x_max): at -2^23, pixel x_min - 1 (also as the 1/2 px tie that rounds down to it),
    pixel x_max + 1 (also as the tie x_max + 1/2 + 1/256 that rounds up to it) and +2^23, the far ones twice: 18 crossings"""
    xs = (-L, -L, (x_min - 1) * U, (x_min - 1) * U + 128, x_max * U + 129, (x_max + 1) * U, L, L, L)
    return [e for x in xs for e in vpair(x)]


# ---- a. the raw limit cases of tests/test_gpu_extremes.py, aliased
@pytest.mark.parametrize("env", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("name", sorted(_raw_cases(64, 48)))
def test_raw_limit_cases(name, env, monkeypatch):
    _route(monkeypatch, env)
    for W, H in ((64, 48), (333, 97)):
        groups = _raw_cases(W, H)[name]
        got = check(W, H, frame(W, H, groups))
        assert _kind(got) != "empty" or name == "wide_flat", (name, W, H)


# ---- b. seeded fuzz of raw edges anywhere in +-2^23, half of the frames padded into k2_rows_mono_huge
def _fuzz_groups(rng, W, H, pads):
    groups = []
    for _ in range(int(rng.integers(1, 4))):
        edges = []
        for _ in range(int(rng.integers(1, 12))):
            edges += _random_pair(rng, W, H)
        argb = int(rng.choice([0xff000000 | int(rng.integers(0, 1 << 24)), 0x80402010, 0x20101000]))
        if rng.integers(0, 3) == 0:                   # a path rectangle inside the frame
            x0, y0 = int(rng.integers(0, W // 3)), int(rng.integers(0, H // 3))
            rect = (x0, y0, int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1)))
        else:
            rect = (0, 0, W, H)
        groups.append((edges + (pads(rect[0], rect[2]) if pads else []), bool(rng.integers(0, 2)), argb, rect))
    return groups


@pytest.mark.parametrize("env", ROUTES, ids=ROUTE_IDS)
def test_random_raw_edges_vs_model(env, monkeypatch):
    _route(monkeypatch, env)
    rng = np.random.default_rng(zlib.crc32(b"mono fuzz"))
    partial = crowded = 0
    n = 10 if EMU else 48
    for it in range(n):
        W, H = [(64, 48), (333, 97), (97, 333)][it % 3]
        stats = {}
        got = check(W, H, frame(W, H, _fuzz_groups(rng, W, H, limit_pads if it % 2 else None)), stats)
        partial += _kind(got) == "partial"
        crowded += stats["crowded_rows"] > 0
        assert (stats["crowded_rows"] > 0) == bool(it % 2), (it, stats)
    assert partial >= n // 3 and crowded == n // 2


# ---- c. padding changes the route, not the picture
@pytest.mark.parametrize("env", ROUTES[:2], ids=ROUTE_IDS[:2])
def test_padding_into_the_huge_route_changes_nothing(env, monkeypatch):
    _route(monkeypatch, env)
    rng = np.random.default_rng(zlib.crc32(b"mono padding"))
    for it in range(6 if EMU else 30):
        W, H = [(64, 48), (333, 97)][it % 2]
        groups = _fuzz_groups(rng, W, H, None)
        s0, s1 = {}, {}
        plain = check(W, H, frame(W, H, groups), s0)
        padded = check(W, H, frame(W, H, [(g[0] + inert_pads(g[3][0], g[3][2]),) + g[1:] for g in groups]), s1)
        assert diff_stats(plain, padded) == (0, 0), it
        assert s1["crowded_rows"] > s0["crowded_rows"], (s0, s1)
    # a span that starts exactly at x_min (a vertical edge there, a slanted one and one from far left) beside padding at x_min - 1
    W, H, rect = 64, 24, (9, 2, 50, 22)
    content = [(9 * U, -L, 9 * U, L, -L, L, 1), (30 * U + 77, 0, 20 * U, H * U, 0, H * U, -1),
               (-L, -L, 9 * U + 127, 12 * U, 4 * U, 12 * U, 1), (40 * U, 4 * U, 40 * U, 12 * U, 4 * U, 12 * U, -1)]
    for eo in (False, True):
        plain = check(W, H, frame(W, H, [(content, eo, 0xff2040c0, rect)]))
        for pads in (inert_pads(9, 50), vpair(8 * U) * 9, vpair(8 * U + 128) * 9):
            s = {}
            padded = check(W, H, frame(W, H, [(content + pads, eo, 0xff2040c0, rect)]), s)
            assert s["crowded_rows"] == 20 and diff_stats(plain, padded) == (0, 0), eo
        assert plain[2:4, 9, 3].all() and not plain[:, 8, 3].any()


# ---- d. 16 crossings against 18 (a closed polygon crosses a row an even number of times: 16 is the largest row k2_rows_mono keeps,
#      18 the smallest one it hands to k2_rows_mono_huge)
X_MIN, X_MAX = 8, 40
PATTERNS = {                                  # (pixel, direction); the path's columns are [8, 40)
    "touch": [(10, 1), (16, -1), (16, 1), (22, -1)],
    "gap_one": [(10, 1), (16, -1), (17, 1), (22, -1)],
    "gap_two": [(10, 1), (16, -1), (18, 1), (22, -1)],
    "overlap": [(10, 1), (20, -1), (14, 1), (24, -1)],
    "hole_one": [(10, 1), (17, 1), (18, -1), (24, -1)],
    "hole_two": [(10, 1), (17, 1), (19, -1), (24, -1)],
    "gap_one_at_x_min": [(4, 1), (8, -1), (9, 1), (14, -1)],
    "gap_two_at_x_min": [(4, 1), (8, -1), (10, 1), (14, -1)],
    "gap_one_before_x_min": [(3, 1), (7, -1), (8, 1), (12, -1)],
    "from_x_min_less_one": [(7, 1), (12, -1)],
    "closes_at_x_min_plus_one": [(2, 1), (9, -1), (11, 1), (14, -1)],
    "gap_one_at_x_max": [(30, 1), (39, -1), (40, 1), (44, -1)],
    "gap_two_at_x_max": [(30, 1), (38, -1), (40, 1), (44, -1)],
    "to_x_max": [(30, 1), (40, -1)],
    "beyond_x_max": [(30, 1), (39, -1), (41, 1), (44, -1)],
    "pairs_everywhere": [(11, 1), (13, -1), (14, 1), (16, -1), (19, 1), (20, -1), (20, 1), (21, -1)],
}
OFFSETS = (0, 1, 128, -127)                  # within the pixel: I(p * 256 + f) = p for each


def _pattern_frame(count, eo, offset_seed):
    """one path per pattern on its own pixel row, each row exactly `count` crossings: the pattern and far padding"""
    rng = np.random.default_rng(offset_seed)
    W, H = 48, len(PATTERNS)
    groups = []
    for i, (name, pat) in enumerate(PATTERNS.items()):
        edges = []
        for p, d in pat:
            x = p * U + int(rng.choice(OFFSETS))
            edges.append((x, -L, x, L, -L, L, d))
        k = (count - len(pat)) // 2
        edges += [e for j in range(k) for e in vpair(-L if j % 2 else L)]
        groups.append((edges, eo, 0xff000000 | (40 * i + 1) << 8, (X_MIN, i, X_MAX, i + 1)))
    return W, H, frame(W, H, groups)


@pytest.mark.parametrize("eo", [False, True], ids=["nonzero", "evenodd"])
def test_sixteen_and_eighteen_crossings(eo):
    for seed in range(3):
        imgs = {}
        for count in (16, 18):
            W, H, fr = _pattern_frame(count, eo, seed)
            s = {}
            imgs[count] = check(W, H, fr, s)
            assert s["crowded_rows"] == (H if count > 16 else 0), (count, s)
        assert diff_stats(imgs[16], imgs[18]) == (0, 0), seed
    cov = imgs[16][..., 3] > 0
    rows = {name: "".join(".#"[int(v)] for v in cov[i]) for i, name in enumerate(PATTERNS)}
    assert rows["gap_one"][10:22] == "#" * 12 and rows["gap_two"][16:18] == ".."
    assert rows["gap_one_at_x_max"][30:] == "#" * 10 + "." * 8 and rows["to_x_max"][39] == "#"
    assert rows["from_x_min_less_one"][:12] == "." * 8 + "#" * 4


# ---- e. the capacity: 8 192 active edges in a row render, 8 193 are refused, in both modes
def _capacity_edges(n, rng, W):
    """n vertical edges active in pixel row 1 only, at distinct x (1/256 px apart at the closest) over the frame and a little past it,
    directions balanced (an odd n has one more upward edge)"""
    xs = np.sort(rng.choice(np.arange(-3 * U, (W + 3) * U), n, replace=False))
    dirs = rng.permutation(np.concatenate([np.ones((n + 1) // 2, int), -np.ones(n // 2, int)]))
    return [(int(x), U, int(x), 2 * U, U, 2 * U, int(d)) for x, d in zip(xs, dirs)]


@pytest.mark.parametrize("antialias", ["none", "default"])
def test_8192_active_edges_render_and_8193_are_refused(antialias):
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    from oracle import oracle_backend as ob
    W, H = 64, 4
    rng = np.random.default_rng(8193)
    ok = {eo: frame(W, H, [(_capacity_edges(8192, rng, W), eo, 0xff30a050)]) for eo in (False, True)}
    bad = frame(W, H, [(_capacity_edges(8193, rng, W), False, 0xff30a050)])
    want = {}
    for eo, fr in ok.items():
        if antialias == "none":
            want[eo] = M.render(*fr, W, H)
        else:
            be = ob.OracleBackend(W, H)
            be.fill_edges(fr[0], (0, 0, W, H), eo, 0xff30a050)
            want[eo] = be.premultiplied_rgba()
            be.close()
    r = S.Renderer(W, H, antialias=antialias)
    try:
        for eo, fr in ok.items():
            r.render_edges(*fr)
            got = r.read_image(premultiplied=True)
            assert diff_stats(got, want[eo]) == (0, 0), eo
            assert _kind(got) == "partial" and got[1, :, 3].any() and not got[0, :, 3].any()
        assert r.stats()["start_group_limit"] == 0
        with pytest.raises(api.SwfrError) as ex:
            r.render_edges(*bad)
        assert ex.value.code == api.ERR_CAPACITY
        assert r.stats()["start_group_limit"] == 1
        r.render_edges(*ok[True])                                  # the same handle afterwards
        assert diff_stats(r.read_image(premultiplied=True), want[True]) == (0, 0)
    finally:
        r.close()


# ---- f. whole extreme scenes (tests/helpers.extreme_scene) through render(), aliased
def _aliased_render(sc):
    from helpers import product_render
    return product_render(sc, antialias="none")


@pytest.mark.parametrize("mode", LARGE_MODES)
def test_extreme_scenes_vs_model(mode):
    rng = np.random.default_rng(zlib.crc32(("gpu mono" + mode).encode()) % 1000)
    sizes = [(64, 48), (333, 97)] * 6 + ([] if EMU else [(1920, 1080)])
    kinds = {"empty": 0, "full": 0, "partial": 0}
    for it, (W, H) in enumerate(sizes):
        sc = extreme_scene(rng, W, H, mode)
        want = M.render(*host_frame(sc), W, H)
        assert diff_stats(_aliased_render(sc), want) == (0, 0), (mode, it)
        kinds[_kind(want)] += 1
    assert kinds["partial"] >= len(sizes) // 3, kinds


def test_extreme_scenes_vs_libcairo_goldens():
    import make_aliased_goldens as G
    g = np.load(os.path.join(GOLD, "cairo_aliased_extreme.npz"))
    scenes = G.extreme_scenes()
    assert sorted(g.files) == sorted(scenes)
    for k, sc in scenes.items():
        assert diff_stats(_aliased_render(sc), g[k]) == (0, 0), k


def test_extreme_scene_at_4k_vs_model():
    if EMU:
        pytest.skip("a 4K frame is only a matter of time on the emulator")
    rng = np.random.default_rng(2160)
    for mode in LARGE_MODES:
        sc = extreme_scene(rng, 3840, 2160, mode)
        assert diff_stats(_aliased_render(sc), M.render(*host_frame(sc), 3840, 2160)) == (0, 0), mode


# ---- g. a full queue of huge rows, and huge rows of a path split at 8 192 columns
def test_every_row_of_a_tall_path_is_queued():
    """2 160 rows, each with 20 crossings: every row goes to k2_rows_mono_huge, whose 64 workgroups walk the whole queue"""
    W, H = 96, 2160
    edges = []
    for k in range(5):                         # five slanted bands across the full height, alternately nonzero / crossing
        a, b = (k * 19 + 2) * U + 37 * k, (k * 19 + 9) * U + 11 * k
        edges += [(a, 0, a + 60 * U, H * U, 0, H * U, 1), (b + 3 * U, 0, b - 40 * U, H * U, 0, H * U, -1)]
    edges += [e for x in (-L, 200 * U, L, 97 * U, 95 * U + 64) for e in vpair(x, (0, H * U))]
    for eo in (False, True):
        s = {}
        got = check(W, H, frame(W, H, [(edges, eo, 0xff8040c0)]), s)
        assert s["crowded_rows"] == H and s["start_group_limit"] == 0, s
        assert _kind(got) == "partial"


def test_huge_rows_across_the_8192_column_split():
    """a 9 600 px wide frame: its path is split at 8 192 columns; crossings of huge-route rows on both sides of the split and at
    columns 8 191 / 8 192 (x_max - 1 / x_max of the left piece, x_min - 1 / x_min of the right one)"""
    W, H = 9600, 6
    rows = []
    for y in range(H):                         # one path row each: the crossings move across the split row by row
        c = 8188 + y
        xs = [(40, 1), (c, -1), (c + 2, 1), (9300, -1), (8191, 1), (8191, -1), (8192, 1), (8192, -1), (8190 - y, 1), (8195 + y, -1)]
        edges = [(x * U + (64 if k % 3 == 0 else 0), -L, x * U + (64 if k % 3 == 0 else 0), L, -L, L, d) for k, (x, d) in enumerate(xs)]
        edges += [e for x in (-L, L, 5000 * U, 9599 * U) for e in vpair(x)]
        rows.append((edges, y % 2 == 1, 0xff000000 | (30 * y + 20), (0, y, W, y + 1)))
    # a slanted path over all rows, crossing the split
    slant = [(8000 * U, 0, 8400 * U, H * U, 0, H * U, 1), (8300 * U + 5, 0, 8100 * U, H * U, 0, H * U, -1)] + vpair(-L) * 9
    rows.append((slant, False, 0x80402000))
    s = {}
    got = check(W, H, frame(W, H, rows), s)
    assert s["crowded_rows"] >= 2 * H, s
    assert got[:, 8180:8200, 3].any() and got[:, :8192, 3].any() and got[:, 8192:, 3].any()
