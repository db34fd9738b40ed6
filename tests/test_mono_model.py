"""tests/mono_model.py, the exact model of the aliased mode, pinned to live libcairo under CAIRO_ANTIALIAS_NONE on the host frames that
swfr_build_frame makes for an aliased handle; and the host contract of aliased frames whose geometry reaches the +-2^23 limits of the
24.8 range.  Without a GPU.  tests/test_mono_gpu.py holds the row pass of csrc/mono.hip to this model."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_aliased_goldens as G  # noqa: E402
import mono_model as M  # noqa: E402
from helpers import LARGE_MODES, extreme_scene  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402

L = 1 << 23
needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
EDGE_FIELDS = ["x1", "y1", "x2", "y2", "top", "bottom", "dir"]


def host_frame(sc, antialias="none"):
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    r = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY, even_odd=bool(sc.get("even_odd")), antialias=antialias)
    try:
        for b in sc.get("bitmaps", []):
            r.add_bitmap(b)
        return r.build_frame(sc["stage"])
    finally:
        r.close()


def model_render(sc):
    return M.render(*host_frame(sc), sc["width"], sc["height"])


def extreme_scenes(mode, n=10):
    """n seeded extreme_scene frames of one LARGE_MODES entry, alternately 64 x 48 and 333 x 97"""
    rng = np.random.default_rng(zlib.crc32(("mono" + mode).encode()) % 1000)
    return [extreme_scene(rng, *[(64, 48), (333, 97)][it % 2], mode) for it in range(n)]


def _kind(img):
    a = img[..., 3]
    return "empty" if not a.any() else ("full" if (a == 255).all() else "partial")


@needs_cairo
def test_model_matches_libcairo_on_the_probes():
    for k, sc in G.probe_scenarios().items():
        assert (model_render(sc) == G.cairo_aliased(sc)).all(), k


@needs_cairo
def test_model_matches_libcairo_on_the_random_scenes():
    from swf_renderer_amd import api
    n = 0
    for s in G.RANDOM_SEEDS:
        sc = G.random_scene(s)
        frame = host_frame(sc)
        if any(st.kind != api.STYLE_SOLID for st in frame[2]):
            continue                                   # (the model draws solid styles only)
        assert (M.render(*frame, sc["width"], sc["height"]) == G.cairo_aliased(sc)).all(), s
        n += 1
    assert n >= len(G.RANDOM_SEEDS) // 2


@needs_cairo
@pytest.mark.parametrize("mode", LARGE_MODES)
def test_model_matches_libcairo_on_extreme_scenes(mode):
    kinds = {"empty": 0, "full": 0, "partial": 0}
    for it, sc in enumerate(extreme_scenes(mode, 12)):
        want = G.cairo_aliased(sc)
        assert (model_render(sc) == want).all(), (mode, it)
        kinds[_kind(want)] += 1
    assert kinds["partial"] >= 4, kinds                  # not only empty or fully covered frames


def test_model_refuses_what_it_does_not_model():
    from swf_renderer_amd import api
    e = np.zeros(2, api.EDGE_DTYPE)
    e[["x1", "y1", "x2", "y2", "top", "bottom"]] = [(256, 0, 256, 2560, 0, 2560), (2560, 0, 2560, 2560, 0, 2560)]
    e["dir"] = [1, 1]                                    # one direction only: no closed polygon
    paths = np.zeros(1, api.PATH_DTYPE)
    paths[0] = (0, 2, api.PATH_TOR, 0, 0, 1, 0, 0, 16, 16)
    with pytest.raises(ValueError):
        M.render(e, paths, [api.solid_style(0xff000000)], 16, 16)
    e["dir"] = [1, -1]
    assert M.render(e, paths, [api.solid_style(0xff000000)], 16, 16)[:10, 1:10, 3].all()
    st = api.solid_style(0xff000000)
    st.kind = api.STYLE_RADIAL
    with pytest.raises(NotImplementedError):
        M.render(e, paths, [st], 16, 16)


def _walk(pairs, eo, x_min, x_max):
    """The rule of csrc/mono.hip's header walked crossing by crossing in plain Python: pairs (pixel, direction) of one row -> spans"""
    pairs = sorted(pairs)
    zero = (lambda w: w % 2 == 0) if eo else (lambda w: w == 0)
    out, w, xs = [], 0, None
    for i, (x, d) in enumerate(pairs):
        xp = pairs[i - 1][0] if i else None
        xn = pairs[i + 1][0] if i + 1 < len(pairs) else None
        wb, w = w, w + (1 if d > 0 else -1)
        if zero(wb) and (xp is None or x > xp + 1):
            xs = x
        if zero(w) and (xn is None or xn > x + 1):
            a, b = max(xs, x_min), min(x, x_max)
            if b > a:
                out.append((a, b))
    return out


def _row_of(spans, W=24):
    s = ["."] * W
    for a, b in spans:
        s[a:b] = "#" * (b - a)
    return "".join(s)


def test_model_rule_by_hand():
    """The rule on rows written out by hand: the 127/128 tie of a crossing, one-pixel gaps filled, two-pixel gaps kept, spans clipped
    to the path's columns, both fill rules."""
    from swf_renderer_amd import api

    def row(xs_dirs, eo=False, rect=(0, 0, 24, 1)):
        e = np.zeros(len(xs_dirs), api.EDGE_DTYPE)
        for i, (x, d) in enumerate(xs_dirs):
            e[i] = (x, 0, x, 256, 0, 256, d, 0)
        paths = np.zeros(1, api.PATH_DTYPE)
        paths[0] = (0, len(e), api.PATH_TOR, int(eo), 0, 1) + tuple(rect)
        return "".join(".#"[int(v)] for v in M.render(e, paths, [api.solid_style(0xffffffff)], 24, 1)[0, :, 3] > 0)

    U = 256
    assert row([(2 * U + 128, 1), (6 * U + 128, -1)]) == _row_of([(2, 6)])                 # 1/2 px ties go left
    assert row([(2 * U + 129, 1), (6 * U + 129, -1)]) == _row_of([(3, 7)])
    assert row([(2 * U, 1), (6 * U, -1), (7 * U, 1), (10 * U, -1)]) == _row_of([(2, 10)])   # one-pixel gap: filled
    assert row([(2 * U, 1), (6 * U, -1), (8 * U, 1), (10 * U, -1)]) == _row_of([(2, 6), (8, 10)])   # two pixels: kept
    assert row([(2 * U, 1), (12 * U, -1), (8 * U, 1), (16 * U, -1)]) == _row_of([(2, 16)])  # winding 2, nonzero
    assert row([(2 * U, 1), (12 * U, -1), (8 * U, 1), (16 * U, -1)], eo=True) == _row_of([(2, 8), (12, 16)])
    assert row([(2 * U, 1), (9 * U, 1), (10 * U, -1), (16 * U, -1)], eo=True) == _row_of([(2, 16)])  # one-pixel hole: filled
    assert row([(-L, 1), (6 * U, -1), (20 * U, 1), (L, -1)], rect=(3, 0, 22, 1)) == _row_of([(3, 6), (20, 22)])


def test_model_is_exact_and_fast_on_8192_edges_per_row():
    """8 192 active edges in every one of 100 rows (slanted, end points anywhere in +-2^23): the vectorised model against the rule
    walked crossing by crossing with Python integers, in a few seconds."""
    import time
    from swf_renderer_amd import api
    rng = np.random.default_rng(8192)
    n, W, H = 8192, 64, 100
    e = np.zeros(n, api.EDGE_DTYPE)
    e["x1"] = rng.integers(-L, L + 1, n)
    e["x2"] = rng.integers(-2 * W * 256, 3 * W * 256, n)
    e["y1"], e["y2"], e["top"], e["bottom"] = -L, L, -L, L
    e["dir"] = rng.permutation(np.repeat([1, -1], n // 2))
    for eo in (False, True):
        paths = np.zeros(1, api.PATH_DTYPE)
        paths[0] = (0, n, api.PATH_TOR, int(eo), 0, 1, 5, 0, W - 3, H)
        t = time.perf_counter()
        img = M.render(e, paths, [api.solid_style(0xff102030)], W, H)
        assert time.perf_counter() - t < 20.0
        assert _kind(img) == "partial"
        for y in (0, 37, H - 1):
            pairs = [((int(a["x1"]) + (256 * y + 127 - int(a["y1"])) * (int(a["x2"]) - int(a["x1"])) // (int(a["y2"]) - int(a["y1"])) + 127) >> 8,
                      int(a["dir"])) for a in e]
            assert "".join(".#"[int(v)] for v in img[y, :, 3] > 0) == _row_of(_walk(pairs, eo, 5, W - 3), W), (eo, y)


# ---- the host half of aliased extreme scenes
@pytest.mark.parametrize("mode", LARGE_MODES)
def test_aliased_host_frame_of_extreme_scenes(mode):
    """swfr_build_frame on a flagged handle, for geometry at the limits: every edge end point within +-2^23; every box rounded by
    (v + 127) & ~255 and clamped to its path's rectangle; tor paths and their edges exactly as without the flag."""
    from swf_renderer_amd import api
    tors = 0
    for it, sc in enumerate(extreme_scenes(mode)):
        e1, p1, s1 = host_frame(sc)
        e0, p0, s0 = host_frame(sc, "default")
        assert len(s0) == len(s1)
        for f in ("x1", "y1", "x2", "y2", "top", "bottom"):
            assert (np.abs(e1[f].astype(np.int64)) <= L).all(), (mode, it, f)
        k1 = 0
        for q0 in p0:
            lo0, hi0 = int(q0["first_edge"]), int(q0["first_edge"] + q0["n_edges"])
            if q0["kind"] == api.PATH_TOR:
                q1 = p1[k1]
                k1 += 1
                assert tuple(q0)[2:] == tuple(q1)[2:]
                assert (e0[lo0:hi0][EDGE_FIELDS] == e1[int(q1["first_edge"]):int(q1["first_edge"] + q1["n_edges"])][EDGE_FIELDS]).all()
                tors += 1
                continue
            bx = e0[lo0:hi0]
            rnd = lambda v: (v.astype(np.int64) + 127) & ~np.int64(255)          # noqa: E731
            x1, x2 = np.maximum(rnd(bx["x1"]), q0["x_min"] * 256), np.minimum(rnd(bx["x2"]), q0["x_max"] * 256)
            y1, y2 = np.maximum(rnd(bx["y1"]), q0["y_min"] * 256), np.minimum(rnd(bx["y2"]), q0["y_max"] * 256)
            keep = (x1 < x2) & (y1 < y2)
            if not keep.any():
                continue
            q1 = p1[k1]
            k1 += 1
            assert q1["kind"] == api.PATH_BOXES and tuple(q0)[2:] == tuple(q1)[2:]
            got = e1[int(q1["first_edge"]):int(q1["first_edge"] + q1["n_edges"])]
            want = np.stack([x1[keep], y1[keep], x2[keep], y2[keep]], 1)
            assert (np.stack([got["x1"], got["y1"], got["x2"], got["y2"]], 1) == want).all(), (mode, it)
            assert ((got["x1"] & 255) == 0).all() and ((got["y2"] & 255) == 0).all()
        assert k1 == len(p1)
    assert tors > 0
