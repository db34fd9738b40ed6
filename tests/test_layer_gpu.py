"""Isolated layers on the device: every libcairo golden of tests/layer_scenes.py -- every file, every scene -- through render,
swfr_render_edges (+ resident frames), SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and render_batch with layered and
plain frames in one group, zero differing bytes (linear-gradient scenes: LINEAR_BOUND, see layer_scenes.py); the plain frames of a
batch are held against the oracle, the aliased ones against tests/frame_model.py's render(..., aliased=True).  Under the emulator the
routes other than render take every fourth scene of a file.  One 4K frame, S1 with its stars in layers.  And the existing corpus through
the layer instance of the tile kernel (SWFR_TILES_SHADERS=4), byte-identical to what instances 0-2 give.  Runs on an MI355X (-m gpu) and
under tools/emu/run.py.

Observed on an MI355X: every exact scene 0 differing bytes; the linear-gradient scenes at most 2 LSB (bound 3).
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import frame_model  # noqa: E402
import layer_scenes as bs  # noqa: E402
import helpers  # noqa: E402
import scenarios  # noqa: E402
from helpers import diff_stats, golden, oracle_render, product_render  # noqa: E402

pytestmark = pytest.mark.gpu
EMU = bool(os.environ.get("SWFR_EMULATOR"))
SC = scenarios.scenarios()
FILES = bs.files()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


def _check(got, want, sc, msg):
    n, mx = diff_stats(got, want)
    print("layer", msg, "differing pixels", n, "max", mx)
    if sc["exact"]:
        assert (n, mx) == (0, 0), msg
    else:
        assert mx <= bs.LINEAR_BOUND, (msg, n, mx)


# ---- 1. every golden through render
@pytest.mark.parametrize("fname", sorted(FILES))
def test_goldens_through_render(fname):
    make, aliased = FILES[fname]
    gold = np.load(bs.golden_path(fname))
    scenes = make()
    assert sorted(scenes) == sorted(gold.files)
    for name, sc in sorted(scenes.items()):
        _check(product_render(sc, **({"antialias": "none"} if aliased else {})), gold[name], sc, (fname, name))


# ---- 2. the same through the other routes: every golden file, every scene (under the emulator, where a frame takes seconds, every
#         fourth scene of a file, the offset moving with the route so that the routes together still see most scenes)
ROUTE_FILES = sorted(FILES)


def _scenes(fname, route):
    make, aliased = FILES[fname]
    items = sorted(make().items())
    if EMU:
        items = items[route % 4::4]
    return items, aliased, np.load(bs.golden_path(fname))


def _renderer(sc, aliased, **kw):
    import swf_renderer_amd as S
    r = S.Renderer(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")), antialias="none" if aliased else "default", **kw)
    for b in sc.get("bitmaps", []):
        r.add_bitmap(b)
    return r


def _built_on_a_host_handle(sc, aliased):
    """swfr_build_frame's arrays for the scene.  They must not name colour-transformed textures: those belong to the handle that walked
    the stage, so such a frame could not be handed to another handle (a cxform_* scene with a bitmap -- there is none today)"""
    from swf_renderer_amd import api
    host = _renderer(sc, aliased, device=api.DEVICE_HOST_ONLY)
    try:
        e, p, s = host.build_frame(sc["stage"])
    finally:
        host.close()
    assert not any(st.kind == api.STYLE_BITMAP and st.bitmap >= api.VARIANT_BASE for st in s)
    return e, p, s


@pytest.mark.parametrize("fname", ROUTE_FILES)
def test_goldens_through_render_edges(fname):
    """swfr_build_frame on one handle, swfr_render_edges on another: the groups travel as marker paths"""
    items, aliased, gold = _scenes(fname, 0)
    for name, sc in items:
        e, p, s = _built_on_a_host_handle(sc, aliased)
        r = _renderer(sc, aliased)
        try:
            r.render_edges(e, p, s)
            _check(r.read_image(premultiplied=True), gold[name], sc, (fname, name, "render_edges"))
            r.render_resident(3)
            _check(r.read_image(premultiplied=True), gold[name], sc, (fname, name, "resident"))
        finally:
            r.close()


@pytest.mark.parametrize("fname", ROUTE_FILES)
def test_goldens_with_graphs(fname, monkeypatch):
    monkeypatch.setenv("SWFR_GRAPHS", "1")
    items, aliased, gold = _scenes(fname, 1)
    for name, sc in items:
        e, p, s = _built_on_a_host_handle(sc, aliased)
        r = _renderer(sc, aliased)
        try:
            r.upload_edges(e, p, s)
            r.render_resident(3)
            _check(r.read_image(premultiplied=True), gold[name], sc, (fname, name, "graphs"))
        finally:
            r.close()


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("fname", ROUTE_FILES)
def test_goldens_through_two_band_handles(fname, contiguous):
    items, aliased, gold = _scenes(fname, 2)
    for name, sc in items:
        h = sc["height"]
        out = np.zeros_like(gold[name])
        n = -(-((h + 15) // 16) // 2)                             # tile-rows per handle
        for rank in range(2):
            r = _renderer(sc, aliased, band_index=rank, band_count=2, contiguous_bands=contiguous)
            try:
                r.render(sc["stage"])
                img = r.read_image(premultiplied=True)
            finally:
                r.close()
            t = np.arange(h) // 16
            rows = ((t >= rank * n) & (t < (rank + 1) * n)) if contiguous else (t % 2 == rank)
            out[rows] = img[rows]
        _check(out, gold[name], sc, (fname, name, "bands", contiguous))


@pytest.mark.parametrize("fname", ROUTE_FILES)
def test_goldens_through_render_batch_with_unlike_frames(fname):
    """The file's scenes of one frame size as ONE batch, a plain frame (no group, no blended path: no operator table) after every third
    of them: layered and plain frames, solid, bitmap and gradient frames in one group, so in one launch of the layer instance.  Into a device
    tensor where there is a device for it (every frame checked), and by the per-frame route (the last frame is what stays)."""
    import swf_renderer_amd as S
    items, aliased, gold = _scenes(fname, 3)
    sizes = sorted({(sc["width"], sc["height"]) for _, sc in items})
    for w, h in sizes:
        group = [(name, sc) for name, sc in items if (sc["width"], sc["height"]) == (w, h)]
        plain = dict(width=w, height=h, exact=True, stage={"children": bs._with_ground(dict(width=w, height=h))})
        # (the plain frame's expected pixels: the oracle's; aliased, where there is no oracle, tests/frame_model.py's -- the exact
        #  model of the aliased rule over the frame builder's arrays, pinned against libcairo by tests/test_frame_model.py; the layered
        #  frames are checked against libcairo)
        plain_want = frame_model.render(*_built_on_a_host_handle(plain, True), w, h, aliased=True) if aliased else oracle_render(plain)
        frames = []                                               # (message, scenario, expected pixels)
        for k, (name, sc) in enumerate(group):
            frames.append((name, sc, gold[name]))
            if k % 3 == 0:
                frames.append(("plain", plain, plain_want))
        r = S.Renderer(w, h, antialias="none" if aliased else "default")
        try:
            seen = set()
            for _, sc, _ in frames:
                for b in sc.get("bitmaps", []):
                    if b["id"] not in seen:
                        seen.add(b["id"])
                        r.add_bitmap(b)
            stages = [sc["stage"] for _, sc, _ in frames]
            if not EMU:                                           # (device tensors need the GPU)
                import torch
                out = torch.zeros((len(stages), h, w, 4), dtype=torch.uint8, device="cuda")
                r.render_batch(stages, out.data_ptr(), h * w * 4)
                got = out.cpu().numpy()
                for k, (name, sc, want) in enumerate(frames):
                    _check(got[k], want, sc, (fname, name, "batch", k))
            for cut in sorted({1, 2, len(frames) // 2, len(frames)}):
                if 0 < cut <= len(frames):
                    r.render_batch(stages[:cut])
                    name, sc, want = frames[cut - 1]
                    _check(r.read_image(premultiplied=True), want, sc, (fname, name, "per-frame route", cut))
        finally:
            r.close()


def test_s1_4k_stars_in_layers():
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    sc = bs.s1_stage()
    gold = np.load(bs.golden_path("cairo_layer_s1_crops"))
    img = product_render(sc)
    for key in gold.files:
        if key == "sha256":
            continue
        x, y = map(int, key.split("_"))
        assert (img[y:y + 256, x:x + 256] == gold[key]).all(), key
    assert hashlib.sha256(img.tobytes()).digest() == gold["sha256"].tobytes()


# ---- 3. the culling rules
@pytest.mark.parametrize("mode", ["normal", "multiply", "add", "overlay"])
def test_cover_inside_a_group_does_not_cull_and_an_opaque_cover_above_does(mode):
    gold = np.load(bs.golden_path("cairo_layer_structure_" + mode))
    scenes = bs.structure_scenes([mode])
    for name in ("cover_inside_" + mode, "cover_above_" + mode):
        assert diff_stats(product_render(scenes[name]), gold[name]) == (0, 0), name
    # what is below a group that holds an opaque full cover shows through it wherever the composite lets it: the frame differs from
    # the one without the inner rectangle below the groups
    inside = scenes["cover_inside_" + mode]
    kids = inside["stage"]["children"]
    if mode != "normal":                                         # (an opaque group pixel composited with OVER does hide what is below)
        assert (product_render(dict(inside, stage={"children": kids[:1] + kids[2:]})) != gold["cover_inside_" + mode]).any()
    # what is below an opaque cover does not: in the cover's columns the frame is the one without the group
    above = scenes["cover_above_" + mode]
    kids = above["stage"]["children"]
    assert (product_render(dict(above, stage={"children": kids[:1] + kids[2:]}))[:, :100] == gold["cover_above_" + mode][:, :100]).all()


def test_a_layer_is_not_the_per_path_rule():
    """the feature is visible: overlapping translucent children as one layer and each on its own differ under every operator"""
    scenes = bs.overlap_scenes()
    gold = np.load(bs.golden_path("cairo_layer_overlap"))
    for mode in bs.MODES:
        sc = scenes[mode + "_opaque"]
        kids = sc["stage"]["children"]
        per_path = dict(sc, stage={"children": kids[:-1] + [dict({k: v for k, v in kids[-1].items() if k != "layer"}, blend_mode=mode)]})
        assert (product_render(per_path) != gold[mode + "_opaque"]).any(), mode


# ---- 4. the existing corpus through the layer instance: byte-identical to what instances 0-2 give
def _use4(monkeypatch, rows="narrow"):
    monkeypatch.setenv("SWFR_TILES_SHADERS", "4")
    if rows == "wide":
        monkeypatch.setenv("SWFR_ROWS_WIDE", "1")
    else:
        monkeypatch.delenv("SWFR_ROWS_WIDE", raising=False)


@pytest.mark.parametrize("rows", ["narrow", "wide"])
@pytest.mark.parametrize("name", sorted(SC))
def test_scenario_through_instance_4(name, rows, monkeypatch):
    sc = SC[name]
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    base = product_render(sc)
    _use4(monkeypatch, rows)
    got = product_render(sc)
    assert diff_stats(got, base) == (0, 0), name
    n, mx = diff_stats(got, golden("cairo_" + name, "rgba_premul"))
    assert ((n, mx) == (0, 0)) if sc["exact"] else mx <= 1, (name, n, mx)


def test_aliased_scenarios_through_instance_4(monkeypatch):
    _use4(monkeypatch)
    for name, sc in sorted(SC.items()):
        n, mx = diff_stats(product_render(sc, antialias="none"), golden("cairo_aliased_" + name, "rgba_premul"))
        assert ((n, mx) == (0, 0)) if sc["exact"] else mx <= 1, (name, n, mx)


@pytest.mark.parametrize("rows", ["narrow", "wide"])
def test_structural_scenes_through_instance_4(rows, monkeypatch):
    """the tests/helpers.py scenes that tests/test_gpu_instances.py runs per instance"""
    import json
    import swf_renderer_amd as S
    _use4(monkeypatch, rows)
    rng = np.random.default_rng(5)
    for it in range(12 if EMU else 40):
        sc, info = helpers.rand_polygon_scene(rng, it)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), ("poly", it, info)
    rng = np.random.default_rng(11)
    for it in range(6 if EMU else 20):
        sc = helpers.rand_layered_translucent_scene(rng)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), ("layered", it)
    rng = np.random.default_rng(78)
    for it in range(8 if EMU else 30):
        sc = helpers.rand_stroked_scene(rng)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), ("stroked", it)
    for teeth in (12, 40, 140):
        for eo in (False, True):
            sc = helpers.crowded_rows_scene(teeth, eo)
            assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), ("comb", teeth, eo)
    for teeth in (9, 16):
        for y_top in (0, -7):
            sc = helpers.frame_top_scene(teeth, y_top, False)
            assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), ("top", teeth, y_top)
    for case in helpers.SOAK_TIE_CASES:
        sc = helpers.soak_scene(*case)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), case
    for name in ("soak_big_7000_2285_child3", "soak_mixed_7100_2196_child0_1"):
        sc = json.load(open(os.path.join(helpers.GOLD, name + ".json")))
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), name
    for key, sc in helpers.uncovered_path_row_scenes():
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), key
    for key, sc in helpers.wide_frame_scenes().items():
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), key
    rng = np.random.default_rng(4040)
    for i in range(3 if EMU else 12):
        sc = helpers.rand_dense_scene(rng)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), ("dense", i)
    if not EMU:
        W, H, fx, cols, scene = helpers.synth_scene(helpers.TWENTY_THOUSAND_PATHS)
        r = S.Renderer(W, H)
        try:
            r.render_edges(*scene)
            assert diff_stats(r.read_image(premultiplied=True), helpers.oracle_polys(fx, cols, W, H)) == (0, 0)
        finally:
            r.close()


def test_s1_4k_known_answer_through_instance_4(monkeypatch):
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    import swf_renderer_amd as S
    from swf_renderer_amd import synth
    _use4(monkeypatch)
    W, H, _, _, scene = helpers.synth_scene(synth.S1)
    r = S.Renderer(W, H)
    try:
        r.render_edges(*scene)
        assert hashlib.sha256(r.read_image(premultiplied=True).tobytes()).hexdigest() == synth.S1_SHA256_PREMUL
        r.render_resident(3)                                      # (overlapped frames: the tile pass in its paired launch shape)
        assert hashlib.sha256(r.read_image(premultiplied=True).tobytes()).hexdigest() == synth.S1_SHA256_PREMUL
    finally:
        r.close()
