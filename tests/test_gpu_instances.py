"""The corpus under every compiled instance of the tile and row kernels.

A frame runs one of three k2_tiles instances (solid colours; + bitmaps; + gradients) and one of two k2_rows instances (8 edge slots
and 32 staged edges; k2_rows_wide: 16 and 64), picked by its heaviest style and its longest path.  The test knobs SWFR_TILES_SHADERS
(the lowest tile instance) and SWFR_ROWS_WIDE=1 (the wide row kernel for every frame) send any frame through any instance, so the
structural scenes -- almost all of them solid -- and the small-path scenes reach the instances their content never picks.  Every
frame is compared with the oracle (bit-exact; linear gradients within +-1 LSB).  Then: dense frames of every kind of path and style
(tests/helpers.py rand_dense_scene) under each launch shape of the tile pass, and gradients at their edges (focal points on and
beyond the circle, 16 stops) with the refusal of a 17th stop."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import helpers  # noqa: E402
import scenarios  # noqa: E402
from helpers import diff_stats, golden, oracle_render, product_render  # noqa: E402

pytestmark = pytest.mark.gpu
SC = scenarios.scenarios()
EMU = bool(os.environ.get("SWFR_EMULATOR"))

INSTANCES = [(rows, tiles) for rows in ("narrow", "wide") for tiles in (0, 1, 2)]
INSTANCE_IDS = ["%s-t%d" % i for i in INSTANCES]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


def _use(monkeypatch, inst):
    """Handles created from here on run the row / tile kernel instance `inst` (or the one the frame needs, if that is higher)."""
    rows, tiles = inst
    monkeypatch.setenv("SWFR_TILES_SHADERS", str(tiles))
    if rows == "wide":
        monkeypatch.setenv("SWFR_ROWS_WIDE", "1")
    else:
        monkeypatch.delenv("SWFR_ROWS_WIDE", raising=False)


_WANT = {}


def _want(key, make):
    """The oracle's frame for `key`, computed once per module and shared by the instances."""
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def _oracle(key, sc):
    return _want(key, lambda: oracle_render(sc))


def _exact(got, want, msg):
    assert diff_stats(got, want) == (0, 0), msg


# ---- the knobs reach the launches: without them, a solid frame never runs the shaded instances
def test_knobs_are_read_and_default_off(monkeypatch):
    from swf_renderer_amd import api
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    monkeypatch.delenv("SWFR_ROWS_WIDE", raising=False)
    sc = SC["translucent_stack"]
    _exact(product_render(sc), _oracle("translucent_stack", sc), "default")
    # out-of-range values are clamped to the three instances
    for v in ("-1", "3", "99"):
        monkeypatch.setenv("SWFR_TILES_SHADERS", v)
        _exact(product_render(sc), _oracle("translucent_stack", sc), v)
    # (host-only handles read them too and build the same frame)
    import swf_renderer_amd as S
    monkeypatch.setenv("SWFR_TILES_SHADERS", "2")
    monkeypatch.setenv("SWFR_ROWS_WIDE", "1")
    host = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
    e, p, s = host.build_frame(sc["stage"])
    host.close()
    assert len(p) == 3 and all(x.kind == api.STYLE_SOLID for x in s)


# ---- 1. every scenario of tests/scenarios.py
@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
@pytest.mark.parametrize("name", sorted(SC))
def test_scenario(name, inst, monkeypatch):
    _use(monkeypatch, inst)
    sc = SC[name]
    n, mx = diff_stats(product_render(sc), _oracle(name, sc))
    if sc["exact"]:
        assert (n, mx) == (0, 0), (name, inst)
    else:
        assert mx <= 1, (name, inst, n, mx)


# ---- 2. the aliased scenarios against their libcairo goldens (the rows knob does not apply: aliased frames have their own row kernel)
@pytest.mark.parametrize("tiles", [1, 2])
def test_aliased_scenarios_vs_golden(tiles, monkeypatch):
    _use(monkeypatch, ("wide", tiles))
    for name, sc in sorted(SC.items()):
        n, mx = diff_stats(product_render(sc, antialias="none"), golden("cairo_aliased_" + name, "rgba_premul"))
        if sc["exact"]:
            assert (n, mx) == (0, 0), (name, tiles)
        else:
            assert mx <= 1, (name, tiles, n, mx)


# ---- 3. fixed-seed subsets of the fuzzes of tests/test_gpu_parity.py (the same seeds: their first frames)
@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_fuzz_subsets(inst, monkeypatch):
    _use(monkeypatch, inst)
    rng = np.random.default_rng(5)
    for it in range(40):
        sc, info = helpers.rand_polygon_scene(rng, it)
        _exact(product_render(sc), _oracle(("poly", it), sc), ("poly", it, inst, info))
    rng = np.random.default_rng(11)
    for it in range(20):
        sc = helpers.rand_layered_translucent_scene(rng)
        _exact(product_render(sc), _oracle(("layered", it), sc), ("layered", it, inst))
    rng = np.random.default_rng(78)
    for it in range(30):
        sc = helpers.rand_stroked_scene(rng)
        _exact(product_render(sc), _oracle(("stroked", it), sc), ("stroked", it, inst))


# ---- 4. structural scenes
@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
@pytest.mark.parametrize("teeth", [12, 40, 140, 1100, 3000])
def test_crowded_rows(teeth, inst, monkeypatch):
    if teeth > 1100 and EMU:
        pytest.skip("thousands of edges per row: quadratic work per row, hours on the emulator")
    _use(monkeypatch, inst)
    for eo in (False, True):
        sc = helpers.crowded_rows_scene(teeth, eo)
        _exact(product_render(sc), _oracle(("comb", teeth, eo), sc), (teeth, eo, inst))


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_edges_arriving_together_at_the_frame_top(inst, monkeypatch):
    _use(monkeypatch, inst)
    for teeth in (9, 13, 16):
        for y_top in (0, -7, -300):
            for eo in (False, True):
                sc = helpers.frame_top_scene(teeth, y_top, eo)
                stats = {}
                _exact(product_render(sc, stats=stats), _oracle(("top", teeth, y_top, eo), sc), (teeth, y_top, eo, inst))
                assert stats["pairtest_limit"] == stats["start_group_limit"] == stats["history_limit"] == 0


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_soak_tie_regressions(inst, monkeypatch):
    import json
    _use(monkeypatch, inst)
    for case in helpers.SOAK_TIE_CASES:
        sc = helpers.soak_scene(*case)
        _exact(product_render(sc), _oracle(("soak",) + case, sc), (case, inst))
    for name in ("soak_big_7000_2285_child3", "soak_mixed_7100_2196_child0_1"):
        sc = json.load(open(os.path.join(helpers.GOLD, name + ".json")))
        _exact(product_render(sc), _oracle(name, sc), (name, inst))


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_uncovered_path_row(inst, monkeypatch):
    _use(monkeypatch, inst)
    for key, sc in helpers.uncovered_path_row_scenes():
        _exact(product_render(sc), _oracle(("uncovered", key), sc), (key, inst))


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_wide_frame(inst, monkeypatch):
    _use(monkeypatch, inst)
    for key, sc in helpers.wide_frame_scenes().items():
        _exact(product_render(sc), _oracle(("wide", key), sc), (key, inst))


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_twenty_thousand_paths_in_three_tile_rows(inst, monkeypatch):
    import swf_renderer_amd as S
    _use(monkeypatch, inst)
    W, H, fx, cols, scene = helpers.synth_scene(helpers.TWENTY_THOUSAND_PATHS)
    r = S.Renderer(W, H)
    try:
        r.render_edges(*scene)
        _exact(r.read_image(premultiplied=True), _want("20k", lambda: helpers.oracle_polys(fx, cols, W, H)), inst)
    finally:
        r.close()


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_s1_4k_known_answer(inst, monkeypatch):
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    import swf_renderer_amd as S
    from swf_renderer_amd import synth
    _use(monkeypatch, inst)
    W, H, _, _, scene = helpers.synth_scene(synth.S1)
    r = S.Renderer(W, H)
    try:
        r.render_edges(*scene)
        img = r.read_image(premultiplied=True)
        assert hashlib.sha256(img.tobytes()).hexdigest() == synth.S1_SHA256_PREMUL, inst      # libcairo known answer
        r.render_resident(3)                                  # (overlapped frames: the tile pass in its paired launch shape)
        assert hashlib.sha256(r.read_image(premultiplied=True).tobytes()).hexdigest() == synth.S1_SHA256_PREMUL, inst
    finally:
        r.close()


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_raw_edge_fuzz(inst, monkeypatch):
    """The raw-edge fuzz of tests/test_gpu_extremes.py (same seed, its first frames): end points anywhere in +-2^23."""
    _use(monkeypatch, inst)
    rng = np.random.default_rng(2 ** 23)
    for it in range(20):
        W, H, groups = helpers.rand_raw_frame(rng, it)
        want = _want(("raw", it), lambda: helpers.raw_oracle(W, H, groups))
        _exact(helpers.raw_product(W, H, groups), want, (it, inst))


@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_batch_and_resident(inst, monkeypatch):
    """One scene through swfr_render_batch (into a device tensor, and the per-frame route) and one through swfr_render_resident."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    _use(monkeypatch, inst)
    sc = SC["stroke_curves"]
    want = _oracle("stroke_curves", sc)
    h, w = want.shape[:2]
    r = S.Renderer(w, h)
    try:
        if not EMU:                                           # (device tensors need the GPU)
            import torch
            out = torch.zeros((3, h, w, 4), dtype=torch.uint8, device="cuda")
            r.render_batch([sc["stage"]] * 3, out.data_ptr(), h * w * 4)
            got = out.cpu().numpy()
            for k in range(3):
                _exact(got[k], want, ("batch", k, inst))
        r.render_batch([sc["stage"]] * 2)
        _exact(r.read_image(premultiplied=True), want, ("batch, per-frame route", inst))
    finally:
        r.close()
    sc = SC["morph_round_stroke_090"]
    host = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
    scene = host.build_frame(sc["stage"])
    host.close()
    r = S.Renderer(sc["width"], sc["height"])
    try:
        r.upload_edges(*scene)
        for frames in (3, 2):
            r.render_resident(frames)
            _exact(r.read_image(premultiplied=True), _oracle("morph_round_stroke_090", sc), ("resident", frames, inst))
    finally:
        r.close()


# ---- 5. dense frames of every kind of path and style, under each launch shape of the tile pass
DENSE_SEED, DENSE_FRAMES = 4040, 40
DENSE_ROUTES = [{}, {"SWFR_TILES_GRID": "7"}, {"SWFR_TILES_GRID": "100000"}, {"SWFR_STRIP_ORDER": "0"}, {"SWFR_FAST_LIMIT": "0"}, {"SWFR_ROWS_WIDE": "1"}]
DENSE_ROUTE_IDS = ["default", "grid7", "grid_all", "row_major", "fast0", "rows_wide"]


def _dense_scenes():
    rng = np.random.default_rng(DENSE_SEED)
    return [helpers.rand_dense_scene(rng) for _ in range(DENSE_FRAMES)]


@pytest.mark.parametrize("env", DENSE_ROUTES, ids=DENSE_ROUTE_IDS)
def test_dense_scenes(env, monkeypatch):
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scenes = _want("dense_scenes", _dense_scenes)
    for i, sc in enumerate(scenes[:8] if EMU else scenes):              # (the emulator: about ten seconds a frame)
        if env.get("SWFR_TILES_GRID") == "100000":
            assert 100000 >= ((sc["width"] + 63) // 64) * ((sc["height"] + 7) // 8)
        _exact(product_render(sc), _oracle(("dense", i), sc), (env, i))


def test_dense_scenes_with_linear_gradients():
    rng = np.random.default_rng(DENSE_SEED + 1)
    for i in range(4 if EMU else 10):
        sc = helpers.rand_dense_scene(rng, linear=True)
        n, mx = diff_stats(product_render(sc), oracle_render(sc))
        assert mx <= 1, (i, n, mx)


def test_dense_scene_under_colour_transforms():
    """The texel pass's variants of both bitmaps in a dense frame, under each transform of the colour-transform goldens."""
    import make_cxform_goldens as G
    sc = _want("dense_scenes", _dense_scenes)[0]
    for name in sorted(G.TRANSFORMS):
        stage = G.apply_transform(sc["stage"], name)
        _exact(product_render(dict(sc, stage=stage)), G.oracle_cxform(sc, stage), name)


@pytest.mark.parametrize("seed", [1, 2])
def test_dense_scene_at_4k(seed):
    """A dense 3840x2160 frame: 16 200 strips, above T3_PAIR_FROM, so that resident frames run the shaded instance in its paired launch
    shape; the blocking render runs it one strip per wavefront."""
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    sc = helpers.rand_dense_scene(np.random.default_rng(DENSE_SEED + 10 * seed), width=3840, height=2160, shapes=60)
    want = oracle_render(sc)
    _exact(product_render(sc), want, ("render", seed))
    host = S.Renderer(3840, 2160, device=api.DEVICE_HOST_ONLY)
    r = S.Renderer(3840, 2160)
    try:
        for b in sc["bitmaps"]:
            host.add_bitmap(b)
            r.add_bitmap(b)
        r.upload_edges(*host.build_frame(sc["stage"]))
        r.render_resident(4)
        _exact(r.read_image(premultiplied=True), want, ("resident", seed))
    finally:
        host.close()
        r.close()


# ---- 6. gradients at their edges
GRADIENT_EDGES = helpers.gradient_edge_scenes()


@pytest.mark.parametrize("inst", [("narrow", 0), ("wide", 2)], ids=["default", "wide"])
def test_gradient_edges(inst, monkeypatch):
    _use(monkeypatch, inst)
    for key, sc in sorted(GRADIENT_EDGES.items()):
        _exact(product_render(sc), _oracle(("grad", key), sc), (key, inst))


def _gradient_stage(n_stops):
    fill = {"type": "radial-gradient", "matrix": scenarios._m(0.004, 0.004, 600, 500),
            "gradient": scenarios._grad([(int(k * 255 / max(n_stops - 1, 1)), (10 * k, 255 - 10 * k, 40, 255 - 5 * k)) for k in range(n_stops)])}
    return {"children": [{"type": "shape", "definition": scenarios._poly_shape([(100, 100), (1100, 150), (900, 950), (150, 800)], fill)}]}


def test_seventeen_stops_are_refused_then_a_valid_frame():
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    W, H = 60, 50
    valid = dict(width=W, height=H, stage=_gradient_stage(16))
    want = oracle_render(valid)
    assert (want[..., 3] > 0).sum() > 500
    r = S.Renderer(W, H)
    try:
        with pytest.raises(S.SwfrError) as e:
            r.render(_gradient_stage(17))
        assert e.value.code == api.ERR_CAPACITY
        r.render(valid["stage"])
        _exact(r.read_image(premultiplied=True), want, "after the refused stage")
        # a raw style of 17 stops: refused by the scene's validation
        host = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY)
        edges, paths, styles = host.build_frame(valid["stage"])
        host.close()
        assert styles[0].n_stops == 16
        styles[0].n_stops = 17
        with pytest.raises(S.SwfrError) as e:
            r.render_edges(edges, paths, styles)
        assert e.value.code == api.ERR_INVALID
        styles[0].n_stops = 16
        r.render_edges(edges, paths, styles)
        _exact(r.read_image(premultiplied=True), want, "after the refused raw style")
    finally:
        r.close()
