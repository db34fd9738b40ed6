"""Renderer(antialias="none") / SWFR_FLAG_ANTIALIAS_NONE: Cairo's CAIRO_ANTIALIAS_NONE (node-canvas's ctx.antialias = 'none').

Goldens: tests/golden/cairo_aliased_*.npz, rendered by libcairo 1.16.0 under CAIRO_ANTIALIAS_NONE (tools/make_aliased_goldens.py, whose
scene builders these tests share).  Without a GPU: the argument, the host half (tor edges untouched, boxes rounded to whole pixels) and
the goldens against live libcairo.  On the GPU (or `python tools/emu/run.py tests/test_aliased.py`): the mono row pass against the
goldens and against live libcairo, through every render route."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_aliased_goldens as G  # noqa: E402
import scenarios  # noqa: E402
from helpers import GOLD, diff_stats, golden, product_render  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402

SC = scenarios.scenarios()
LINEAR = {name for name, sc in SC.items() if not sc["exact"]}      # linear gradients: the documented +-1 LSB extension
EMU = bool(os.environ.get("SWFR_EMULATOR"))
needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")


def aliased(sc, **kw):
    return product_render(sc, antialias="none", **kw)


def assert_matches(got, want, exact=True):
    n, mx = diff_stats(got, want)
    if exact:
        assert (n, mx) == (0, 0)
    else:
        assert mx <= 1, (n, mx)


# ---------------------------------------------------------------------------------------------------------- without a GPU
def test_antialias_argument_is_validated():
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    for bad in ("None", "gray", "subpixel", "", None, 0):
        with pytest.raises(ValueError):
            S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY, antialias=bad)
    for good in ("default", "none"):
        r = S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY, antialias=good)
        assert r.antialias == good
        r.close()


def _host_frames(sc):
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    out = []
    for mode in ("default", "none"):
        r = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY, even_odd=bool(sc.get("even_odd")), antialias=mode)
        try:
            for b in sc.get("bitmaps", []):
                r.add_bitmap(b)
            out.append(r.build_frame(sc["stage"]))
        finally:
            r.close()
    return out


def _round(v):
    return (v.astype(np.int64) + 127) & ~np.int64(255)


@pytest.mark.parametrize("name", sorted(G.probe_scenarios()) + ["stroke_rectilinear_open", "stroke_rectilinear_loop_scaled", "fixture_squares",
                                                                 "config2_squares", "nonzero_pentagram", "stroke_curves", "offframe_fill_stroke"])
def test_host_frame_keeps_tor_edges_and_rounds_boxes(name):
    """swfr_build_frame on a flagged host-only handle: every tor path and its edges exactly as without the flag; every box of a box path
    rounded as _cairo_boxes_add rounds under CAIRO_ANTIALIAS_NONE ((v + 127) & ~255), clamped to the converter rectangle, empty ones
    dropped -- the same pixels the frame builder hands swfr_upload_edges and swfr_render."""
    from swf_renderer_amd import api
    sc = G.probe_scenarios()[name] if name in G.probe_scenarios() else SC[name]
    (e0, p0, s0), (e1, p1, s1) = _host_frames(sc)
    assert len(s0) == len(s1)
    k1 = 0
    tor = boxes = 0
    for q0 in p0:
        if q0["kind"] == api.PATH_TOR:
            q1 = p1[k1]; k1 += 1
            assert tuple(q0)[2:] == tuple(q1)[2:]
            a = e0[q0["first_edge"]:q0["first_edge"] + q0["n_edges"]]
            b = e1[q1["first_edge"]:q1["first_edge"] + q1["n_edges"]]
            assert (a[["x1", "y1", "x2", "y2", "top", "bottom", "dir"]] == b[["x1", "y1", "x2", "y2", "top", "bottom", "dir"]]).all()
            tor += 1
            continue
        bx = e0[q0["first_edge"]:q0["first_edge"] + q0["n_edges"]]
        x1, x2 = np.maximum(_round(bx["x1"]), q0["x_min"] * 256), np.minimum(_round(bx["x2"]), q0["x_max"] * 256)
        y1, y2 = np.maximum(_round(bx["y1"]), q0["y_min"] * 256), np.minimum(_round(bx["y2"]), q0["y_max"] * 256)
        keep = (x1 < x2) & (y1 < y2)
        if not keep.any():
            continue                                               # every box rounded away: the path is not emitted
        q1 = p1[k1]; k1 += 1
        assert q1["kind"] == api.PATH_BOXES and tuple(q0)[2:] == tuple(q1)[2:]
        got = e1[q1["first_edge"]:q1["first_edge"] + q1["n_edges"]]
        want = np.stack([x1[keep], y1[keep], x2[keep], y2[keep]], 1)
        assert (np.stack([got["x1"], got["y1"], got["x2"], got["y2"]], 1) == want).all()
        assert (got["top"] == got["y1"]).all() and (got["bottom"] == got["y2"]).all()
        boxes += 1
    assert k1 == len(p1) and tor + boxes > 0


def test_probe_goldens_pin_the_rule():
    """What the probes of libcairo showed, read off the committed goldens: half-pixel boundaries (left / top side inclusive), the
    one-pixel gap of a polygon filled, a two-pixel gap and a box path's gap kept."""
    g = np.load(os.path.join(GOLD, "cairo_aliased_probes.npz"))
    cov = {k: g[k][..., 3] > 0 for k in g.files}
    assert cov["vleft_128"][3, 5] and not cov["vleft_129"][3, 5]
    assert not cov["vright_128"][3, 5] and cov["vright_129"][3, 5]
    assert cov["top_128"][0].any() and not cov["top_129"][0].any()
    assert cov["gap_one"][3, 2:20].all()
    assert not cov["gap_two"][3, 10:12].any() and cov["gap_two"][3, 12]
    assert not cov["gap_boxes"][3, 10] and cov["gap_boxes"][3, 9] and cov["gap_boxes"][3, 11]
    assert (cov["box_L_127"] == cov["box_L_128"]).all() and not (cov["box_L_128"] == cov["box_L_129"]).all()


@needs_cairo
def test_goldens_regenerate_byte_for_byte():
    """A sample of the committed goldens, rendered again by live libcairo under CAIRO_ANTIALIAS_NONE."""
    for name in ("nonzero_pentagram", "evenodd_pentagram", "stroke_curves", "stroke_rectilinear_loop_scaled", "morph_037", "translucent_stack"):
        assert (G.cairo_aliased(SC[name]) == golden("cairo_aliased_" + name, "rgba_premul")).all(), name
    probes = np.load(os.path.join(GOLD, "cairo_aliased_probes.npz"))
    for k, sc in G.probe_scenarios().items():
        assert (G.cairo_aliased(sc) == probes[k]).all(), k
    rnd = np.load(os.path.join(GOLD, "cairo_aliased_random.npz"))
    for s in list(G.RANDOM_SEEDS)[:8]:
        assert (G.cairo_aliased(G.random_scene(s)) == rnd["mixed_%d" % s]).all(), s
    ext = np.load(os.path.join(GOLD, "cairo_aliased_extreme.npz"))
    for k, sc in list(G.extreme_scenes().items())[::2]:
        assert (G.cairo_aliased(sc) == ext[k]).all(), k


# ---------------------------------------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC))
def test_scenario_vs_aliased_golden(gpu, name):
    assert_matches(aliased(SC[name]), golden("cairo_aliased_" + name, "rgba_premul"), exact=name not in LINEAR)


@pytest.mark.gpu
def test_antialiased_render_differs_from_the_aliased_golden(gpu):
    """The aliased goldens are not what the default mode draws: an antialiased pentagram differs at its edge pixels."""
    sc = SC["nonzero_pentagram"]
    want = golden("cairo_aliased_nonzero_pentagram", "rgba_premul")
    n, _ = diff_stats(product_render(sc), want)
    assert n > 50
    assert diff_stats(aliased(sc), want) == (0, 0)


@pytest.mark.gpu
def test_probes_random_scenes_and_wide_frames(gpu):
    probes = np.load(os.path.join(GOLD, "cairo_aliased_probes.npz"))
    for k, sc in G.probe_scenarios().items():
        assert diff_stats(aliased(sc), probes[k]) == (0, 0), k
    rnd = np.load(os.path.join(GOLD, "cairo_aliased_random.npz"))
    for s in G.RANDOM_SEEDS:
        assert diff_stats(aliased(G.random_scene(s)), rnd["mixed_%d" % s]) == (0, 0), s
    wide = np.load(os.path.join(GOLD, "cairo_aliased_wide.npz"))
    for k, sc in G.wide_scenes().items():
        assert diff_stats(aliased(sc), wide[k]) == (0, 0), k


def _s1():
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    return synth.S1["width"], synth.S1["height"], api.stars_to_stage(pts, cols)


def _check_s1(img):
    g = np.load(os.path.join(GOLD, "cairo_aliased_s1.npz"))
    for (x, y) in G.S1_CROPS:
        assert (img[y:y + 256, x:x + 256] == g["%d_%d" % (x, y)]).all(), (x, y)
    assert hashlib.sha256(img.tobytes()).hexdigest() == str(g["sha256"])


@pytest.mark.gpu
def test_s1_4k_known_answer(gpu):
    import swf_renderer_amd as S
    W, H, stage = _s1()
    r = S.Renderer(W, H, antialias="none")
    try:
        r.render(stage)
        _check_s1(r.read_image(premultiplied=True))
    finally:
        r.close()


@pytest.mark.gpu
def test_every_route_gives_the_same_frame(gpu):
    """render, render_batch (into a device tensor, and the per-frame route), build_frame -> upload_edges -> render_resident (+ the
    batched resident entry) and render_sequence_readback: one stage, one frame, equal to the golden."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    name = "config2_homestuck-beta-1"
    sc = SC[name]
    want = golden("cairo_aliased_" + name, "rgba_premul")
    w, h = sc["width"], sc["height"]
    r = S.Renderer(w, h, antialias="none")
    try:
        r.render(sc["stage"])
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        if not EMU:                                                 # (device tensors need the GPU)
            import torch
            out = torch.zeros((3, h, w, 4), dtype=torch.uint8, device="cuda")
            r.render_batch([sc["stage"]] * 3, out.data_ptr(), h * w * 4)
            for f in range(3):
                assert diff_stats(out[f].cpu().numpy(), want) == (0, 0), f
        r.render_batch([sc["stage"], sc["stage"]])
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        r.render_sequence_readback([sc["stage"]], repeat=2, premultiplied=True)
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
    finally:
        r.close()
    host = S.Renderer(w, h, device=api.DEVICE_HOST_ONLY, antialias="none")
    frame = host.build_frame(sc["stage"])
    host.close()
    r = S.Renderer(w, h, antialias="none")
    try:
        r.upload_edges(*frame)
        r.render_resident(3)
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        r.render_resident_batched(2, 1)
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        r.render_edges(*frame)
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
    finally:
        r.close()


@pytest.mark.gpu
def test_frames_per_launch_with_queued_rows(gpu, monkeypatch):
    """The two routes that launch several frames per kernel -- render_resident_batched and render_resident in groups of frame sets
    (SWFR_RESIDENT_BATCH=2, no per-kernel events) -- on an aliased handle whose scene has queued rows (a comb of 80 edges per row):
    every read-back equals the blocking render_edges frame of the same handle, and no capacity limit was reached."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    from helpers import crowded_rows_scene
    monkeypatch.setenv("SWFR_RESIDENT_BATCH", "2")
    monkeypatch.setenv("SWFR_EVENT_STRIDE", "1000")
    sc = crowded_rows_scene(40, False)
    w, h = sc["width"], sc["height"]
    assert w <= 256 and h <= 192
    host = S.Renderer(w, h, device=api.DEVICE_HOST_ONLY, antialias="none")
    frame = host.build_frame(sc["stage"])
    host.close()
    r = S.Renderer(w, h, antialias="none")
    try:
        r.render_edges(*frame)
        want = r.read_image(premultiplied=True).copy()
        assert want[..., 3].any()
        r.render_resident_batched(3, 2)
        assert (r.read_image(premultiplied=True) == want).all()
        r.render_resident(6)
        assert (r.read_image(premultiplied=True) == want).all()
        st = r.stats()
        assert st["queued_rows"] > 0
        assert (st["pairtest_limit"], st["start_group_limit"], st["history_limit"]) == (0, 0, 0)
    finally:
        r.close()


def _owned(h, rank, world, contiguous):
    tile_rows = (h + 15) // 16
    t = np.arange(h) // 16
    if contiguous:
        n = -(-tile_rows // world)
        return (t >= rank * n) & (t < (rank + 1) * n)
    return t % world == rank


@pytest.mark.gpu
@pytest.mark.parametrize("contiguous", [False, True])
def test_eight_banded_handles_assemble_to_the_golden(gpu, contiguous):
    import swf_renderer_amd as S
    name = "config2_homestuck-beta-1"
    sc = SC[name]
    want = golden("cairo_aliased_" + name, "rgba_premul")
    w, h = sc["width"], sc["height"]
    out = np.zeros_like(want)
    for rank in range(8):
        r = S.Renderer(w, h, band_index=rank, band_count=8, contiguous_bands=contiguous, antialias="none")
        try:
            r.render(sc["stage"])
            img = r.read_image(premultiplied=True)
        finally:
            r.close()
        rows = _owned(h, rank, 8, contiguous)
        out[rows] = img[rows]
    assert diff_stats(out, want) == (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("teeth", G.COMB_TEETH)
def test_combs_of_thousands_of_active_edges(gpu, teeth):
    """2 200 and 6 000 active edges in every row (k2_rows_mono_huge), both fill rules."""
    g = np.load(os.path.join(GOLD, "cairo_aliased_combs.npz"))
    for eo in (False, True):
        stats = {}
        got = aliased(G.comb_scene(teeth, eo), stats=stats)
        assert diff_stats(got, g["comb_%d_%s" % (teeth, "evenodd" if eo else "nonzero")]) == (0, 0), eo
        assert stats["crowded_rows"] > 0 and stats["start_group_limit"] == 0, stats


@pytest.mark.gpu
def test_more_than_8192_active_edges_is_refused_and_counted(gpu):
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    sc = G.comb_scene(4200, False, width_twips=6000)           # 8 400 active edges in a row
    r = S.Renderer(sc["width"], sc["height"], antialias="none")
    try:
        with pytest.raises(api.SwfrError) as e:
            r.render(sc["stage"])
        assert e.value.code == api.ERR_CAPACITY
        assert r.stats()["start_group_limit"] >= 1
    finally:
        r.close()


@pytest.mark.gpu
def test_antialiased_and_aliased_handles_alternate(gpu):
    """One process, an antialiased and an aliased handle used in turn: each keeps matching its own goldens."""
    import swf_renderer_amd as S
    names = ("nonzero_pentagram", "translucent_stack", "offframe_fill_stroke")         # (100 x 100 each)
    aa, mono = S.Renderer(100, 100), S.Renderer(100, 100, antialias="none")
    try:
        for _ in range(2):
            for name in names:
                for r, prefix in ((aa, "cairo_"), (mono, "cairo_aliased_")):
                    r.render(SC[name]["stage"])
                    assert diff_stats(r.read_image(premultiplied=True), golden(prefix + name, "rgba_premul")) == (0, 0), (name, prefix)
    finally:
        aa.close()
        mono.close()


def _fuzz_scene(seed):
    rng = np.random.default_rng(77000 + seed)
    if seed % 3:
        from helpers import rand_mixed_scene
        return rand_mixed_scene(rng)
    # small polygons with vertices on the 1/256 px grid near pixel centres and boundaries: the rule's ties
    W, H = int(rng.integers(16, 64)), int(rng.integers(12, 48))
    polys = []
    for _ in range(int(rng.integers(1, 4))):
        n = int(rng.integers(3, 9))
        px = rng.integers(-4, max(W, H) + 4, (n, 2)) * 256 + rng.choice([0, 127, 128, 129, 255, 1, 64], (n, 2))
        polys.append([(int(x), int(y)) for x, y in px])
    return G._fine(W, H, polys, color=(int(rng.integers(0, 256)), 90, 200, int(rng.choice([255, 140]))), even_odd=bool(rng.integers(0, 2)))


@pytest.mark.gpu
@needs_cairo
def test_fuzz_against_live_libcairo(gpu):
    """300 seeded scenes (random solid / stroked / morph scenes, and polygons with vertices at 1/256 px ties) against libcairo under
    CAIRO_ANTIALIAS_NONE, bit for bit."""
    bad = []
    for seed in range(300):
        sc = _fuzz_scene(seed)
        if diff_stats(aliased(sc), G.cairo_aliased(sc)) != (0, 0):
            bad.append(seed)
    assert not bad, bad
