"""Host logic of the product without a GPU: the C-ABI library loads and exports every symbol of
include/swfr.h, decode matches the reference goldens, and the frame builder's edge lists equal the
oracle's polygons edge for edge."""
import ctypes
import os
import re

import numpy as np
import pytest

import scenarios
import swf_renderer_amd as S
from helpers import fixture, fixture_text
from oracle import canvas_replay as cr, oracle_backend as ob
from swf_renderer_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = scenarios.scenarios()


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "swfr.h")).read()
    declared = set(re.findall(r"^(?:int|long|void|const char \*|uint32_t|size_t|void \*)\s*\*?(swfr_[a-z_]+)\s*\(", header, re.M))
    assert declared == set(api.EXPORTS), declared ^ set(api.EXPORTS)
    L = S.load_library()
    for name in declared:
        assert hasattr(L, name), name
    assert L.swfr_abi_version() == 1


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(S.SwfrError) as e:
        S.Renderer(32, 32)
    assert e.value.code == api.ERR_NO_DEVICE
    r = S.Renderer(32, 32, device=api.DEVICE_HOST_ONLY)
    with pytest.raises(S.SwfrError) as e:
        r.render({"children": []})
    assert e.value.code == api.ERR_NO_DEVICE     # no CPU rasterization fallback exists


@pytest.mark.parametrize("name", ["squares", "triangle", "homestuck-beta-1", "homestuck-beta-4"])
def test_decode_shape_json_golden(name):
    r = S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY)
    sid = r.register_shape(fixture(name))
    assert r.shape_json(sid) == fixture_text(name + ".shape.ts.json")


@pytest.mark.parametrize("name", ["squares", "triangle", "homestuck-beta-1"])
def test_decode_shape_rust_golden(name):
    """The reference's Rust decoder golden (tests/flat-shapes/*/shape.rs.log, rs/src/lib.rs:26-71), string-exact."""
    import json
    from helpers import shape_to_rs_log
    r = S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY)
    sid = r.register_shape(fixture(name))
    assert shape_to_rs_log(json.loads(r.shape_json(sid)), fixture(name)) == fixture_text(name + ".shape.rs.log")


def test_decode_morph_shape_json_golden():
    r = S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY)
    sid = r.register_morph_shape(fixture("homestuck-beta-29"))
    assert r.shape_json(sid, morph=True) == fixture_text("homestuck-beta-29.shape.ts.json")


def test_bitmap_decode_matches_reference_pam():
    tag = fixture("homestuck-beta-3.bitmap")
    w, h, rgba = api.decode_x_swf_bmp(bytes.fromhex(tag["data"]))
    with open(os.path.join(ROOT, "tests", "golden", "fixtures", "homestuck-beta-3.pam"), "rb") as f:
        want = f.read()
    assert cr.image_to_pam(w, h, rgba) == want
    assert api.image_to_pam(w, h, rgba) == want        # the product's own PAM writer (rs/src/pam.rs format)


def _xswfbmp(width, height, palette, indices, level=6, strategy=0):
    """An image/x-swf-bmp tag body (format 3) as the SWF parser hands it over: header, zlib(palette RGB + rows padded to 4)."""
    import zlib
    padded = width + ((4 - width % 4) % 4)
    rows = np.zeros((height, padded), dtype=np.uint8)
    rows[:, :width] = indices
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    body = co.compress(bytes(np.asarray(palette, dtype=np.uint8).tobytes()) + rows.tobytes()) + co.flush()
    return bytes([3, width & 255, width >> 8, height & 255, height >> 8, len(palette) - 1]) + body


def test_bitmap_decoder_of_the_library_against_zlib_and_numpy():
    """swfr_decode_x_swf_bmp (csrc/bitmap_decode.cpp: its own inflater) on stored, fixed-Huffman and dynamic-Huffman streams of random
    and of compressible images, ragged widths (row padding), a full and a short palette (indices past it are opaque black)."""
    import zlib
    rng = np.random.default_rng(7)
    cases = 0
    for (w, h, ncol) in [(1, 1, 1), (3, 5, 2), (139, 208, 256), (64, 64, 17), (257, 3, 255), (5, 300, 4)]:
        for level, strategy in [(0, 0), (1, zlib.Z_FIXED), (6, 0), (9, zlib.Z_FILTERED)]:
            pal = rng.integers(0, 256, (ncol, 3), dtype=np.uint8)
            idx = rng.integers(0, 256 if ncol < 200 else ncol, (h, w), dtype=np.uint8)
            if level == 9:
                idx = np.repeat(np.repeat(idx[:(h + 7) // 8, :(w + 7) // 8], 8, axis=0), 8, axis=1)[:h, :w]      # long matches, far back
            gw, gh, rgba = api.decode_x_swf_bmp(_xswfbmp(w, h, pal, idx, level, strategy))
            want = np.zeros((h, w, 4), dtype=np.uint8)
            want[..., 3] = 255
            ok = idx < ncol
            want[ok, :3] = pal[idx[ok]]
            assert (gw, gh) == (w, h) and rgba == want.tobytes(), (w, h, ncol, level)
            cases += 1
    assert cases == 24


def test_bitmap_tag_errors_like_the_reference():
    """Another format id: UnsupportedXSwfBmpFormatId (decode-x-swf-bmp.ts:12-14); another media type: NotImplemented
    (node-canvas-bitmap-service.ts:34-35); a damaged stream is refused, never decoded into something else."""
    good = _xswfbmp(4, 4, [[1, 2, 3]], np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(S.SwfrError) as e:
        api.decode_x_swf_bmp(bytes([5]) + good[1:])
    assert e.value.code == api.ERR_NOT_IMPLEMENTED
    for bad in (good[:-3], good[:8] + bytes([good[8] ^ 0x55]) + good[9:], good[:6]):
        with pytest.raises(S.SwfrError) as e:
            api.decode_x_swf_bmp(bad)
        assert e.value.code == api.ERR_INVALID
    r = S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY)
    try:
        with pytest.raises(S.SwfrError) as e:
            r.add_bitmap({"id": 1, "media_type": "image/jpeg", "data": good})
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplemented: Support for image/jpeg images" in str(e.value)
        with pytest.raises(S.SwfrError) as e:
            r.add_bitmap({"id": 1, "media_type": "image/x-swf-bmp", "data": bytes([7]) + good[1:]})
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "UnsupportedXSwfBmpFormatId: 7" in str(e.value)
        r.add_bitmap({"id": 1, "media_type": "image/x-swf-bmp", "data": good})          # (a host-only handle keeps the dimensions)
    finally:
        r.close()


def test_clear_state_after_a_rectilinear_stroke_outside_the_frame():
    """The host half of test_rectilinear_stroke_outside_the_frame_leaves_the_surface_clear (no GPU): after the off-frame box stroke
    the oracle's surface is still clear, and the frame builder marks the next translucent path as a SOURCE lerp, not an OVER."""
    import json
    sc = json.load(open(os.path.join(ROOT, "tests", "golden", "soak_mixed_7100_2196_child0_1.json")))
    be = ob.OracleBackend(sc["width"], sc["height"])
    be.set_fill_rule(True)
    cr.CanvasReplay(be, linear_extension=True).render({"children": sc["stage"]["children"][:1]})
    assert be.L.swfo_is_clear(be.ctx) == 1
    r = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY, even_odd=True)
    try:
        edges, paths, styles = r.build_frame(sc["stage"])
        assert len(paths) == 1 and int(paths[0]["lerp"]) == 1
    finally:
        r.close()


class _Tap(ob.OracleBackend):
    """Oracle backend that records the polygon of every fill()/stroke()."""

    def __init__(self, w, h):
        super().__init__(w, h)
        self.polys = []
        self.L.swfo_last_polygon.restype = ctypes.c_int
        self.L.swfo_last_polygon.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), ctypes.POINTER(ctypes.c_int)]

    def _grab(self):
        p, rect = ctypes.POINTER(ctypes.c_int32)(), ctypes.c_int()
        n = self.L.swfo_last_polygon(self.ctx, ctypes.byref(p), ctypes.byref(rect))
        if n:
            self.polys.append((np.ctypeslib.as_array(p, shape=(n, 7)).copy(), rect.value))

    def fill(self):
        super().fill()
        self._grab()

    def stroke(self):
        super().stroke()
        self._grab()


@pytest.mark.parametrize("name", sorted(SC))
def test_frame_edges_equal_oracle_polygons(name):
    sc = SC[name]
    r = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY, even_odd=bool(sc.get("even_odd")))
    for b in sc.get("bitmaps", []):
        r.add_bitmap(b)
    edges, paths, styles = r.build_frame(sc["stage"])
    tap = _Tap(sc["width"], sc["height"])
    rp = cr.CanvasReplay(tap, linear_extension=True)
    for b in sc.get("bitmaps", []):
        rp.add_bitmap(b)
    rp.render(sc["stage"])
    assert len(paths) == len(tap.polys)
    for pth, (pe, rect) in zip(paths, tap.polys):
        e = edges[pth["first_edge"]: pth["first_edge"] + pth["n_edges"]]
        if rect:
            assert pth["kind"] == api.PATH_BOXES
            continue
        assert pth["kind"] == api.PATH_TOR
        got = np.stack([e[k] for k in ("x1", "y1", "x2", "y2", "top", "bottom", "dir")], 1)
        assert got.shape == pe.shape and (got == pe).all()
    tap.close()


def test_png_writer_round_trips_through_a_png_decoder():
    """image_to_png: the reference's golden images are PNGs; ours decode to the same straight RGBA bytes."""
    import io
    from PIL import Image
    rng = np.random.default_rng(3)
    for w, h in ((1, 1), (7, 3), (54, 81)):
        px = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        back = np.asarray(Image.open(io.BytesIO(api.image_to_png(w, h, px.tobytes()))).convert("RGBA"))
        assert np.array_equal(back, px)
    with pytest.raises(ValueError):
        api.image_to_png(2, 2, b"\x00" * 15)


def test_fuzz_bitmap_scenes_edges_equal_oracle():
    """Bitmap fills: a non-repeating bitmap bounds its fill by its own device-space extents, which become the polygon limits --
    the frame builder must clip exactly as the oracle (and Cairo) does."""
    from helpers import rand_bitmap_scene
    rng = np.random.default_rng(99)
    for it in range(150):
        sc = rand_bitmap_scene(rng)
        r = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
        for b in sc["bitmaps"]:
            r.add_bitmap(b)
        edges, paths, styles = r.build_frame(sc["stage"])
        tap = _Tap(sc["width"], sc["height"])
        rp = cr.CanvasReplay(tap, linear_extension=True)
        for b in sc["bitmaps"]:
            rp.add_bitmap(b)
        rp.render(sc["stage"])
        tor = [(pe, rect) for pe, rect in tap.polys if not rect]
        got = [p for p in paths if p["kind"] == api.PATH_TOR]
        # the oracle also records polygons whose pixel rectangle is empty; the frame builder drops those
        tor = [(pe, rect) for pe, rect in tor if len(pe)]
        for pth in got:
            e = edges[pth["first_edge"]: pth["first_edge"] + pth["n_edges"]]
            g = np.stack([e[k] for k in ("x1", "y1", "x2", "y2", "top", "bottom", "dir")], 1)
            assert any(g.shape == pe.shape and (g == pe).all() for pe, _ in tor), it
        tap.close(); r.close()


def test_synthetic_scene_builder_equals_host_api():
    pts, cols = synth.scene(seed=synth.S1["seed"], n_shapes=300, width=3840, height=2160)
    e1, p1, s1 = api.polygons_to_scene(synth.twips_to_fixed(pts), cols, 3840, 2160)
    r = S.Renderer(3840, 2160, device=api.DEVICE_HOST_ONLY)
    e2, p2, s2 = r.build_frame(api.stars_to_stage(pts, cols))
    assert e1.tobytes() == e2.tobytes() and p1.tobytes() == p2.tobytes()
    assert [s.pixel for s in s1] == [s.pixel for s in s2]


def test_reference_error_behaviour():
    r = S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY)
    bad = fixture("triangle")
    bad["shape"]["records"][0]["left_fill"] = 9
    with pytest.raises(S.SwfrError) as e:          # decode-swf-shape.ts:410-421 "Invalid fill ID"
        r.register_shape(bad)
    assert e.value.code == api.ERR_INVALID and "Invalid fill ID" in str(e.value)
    tag = fixture("homestuck-beta-4")              # bitmap 3 never added: node-canvas-bitmap-service.ts:39-45
    with pytest.raises(S.SwfrError) as e:
        r.build_frame(cr.stage_for_shape(tag)[2])
    assert e.value.code == api.ERR_NOT_FOUND and "BitmapNotFound" in str(e.value)
    with pytest.raises(S.SwfrError) as e:          # unknown display object / id
        r.build_frame({"children": [{"type": "shape", "id": 77}]})
    assert e.value.code == api.ERR_NOT_FOUND
    morph = fixture("homestuck-beta-29")
    morph["shape"]["initial_styles"]["fill"][0] = {"type": "radial-gradient", "matrix": morph["shape"]["initial_styles"]["fill"][0].get("matrix", scenarios._m()), "gradient": scenarios._grad([(0, (0, 0, 0))])}
    with pytest.raises(S.SwfrError) as e:          # decode-swf-morph-shape.ts:94-106 "Unknown fill type"
        r.register_morph_shape(morph)
    assert "Unknown fill type" in str(e.value)


def test_empty_and_degenerate_inputs():
    r = S.Renderer(16, 16, device=api.DEVICE_HOST_ONLY)
    e, p, s = r.build_frame({"children": []})
    assert len(e) == 0 and len(p) == 0
    # a shape whose path is a single point / zero-area produces nothing
    tag = scenarios._poly_shape([(100, 100), (100, 100), (100, 100)], {"type": "solid", "color": scenarios._rgba(1, 2, 3)})
    e, p, s = r.build_frame({"children": [{"type": "shape", "definition": tag}]})
    assert len(p) == 0
    # fully off-frame geometry is dropped before it reaches the device
    tag = scenarios._poly_shape([(-5000, -5000), (-4000, -5000), (-4500, -4000)], {"type": "solid", "color": scenarios._rgba(1, 2, 3)})
    e, p, s = r.build_frame({"children": [{"type": "shape", "definition": tag}]})
    assert len(p) == 0


def _rand_path_shape(rng, line_width, morph=False, segments=(1, 8)):
    """A random open path of straight / quadratic / axis-aligned segments with a solid line style (and sometimes a fill)."""
    kind = rng.choice(["straight", "curved", "rectilinear", "mixed"])
    x, y = int(rng.integers(200, 1500)), int(rng.integers(200, 1200))
    sc = {"type": "style-change", "move_to": {"x": x, "y": y}, "line_style": 1}
    if morph:
        sc["morph_move_to"] = {"x": x + int(rng.integers(-100, 100)), "y": y + int(rng.integers(-100, 100))}
    fill = None
    if rng.integers(0, 3) == 0:
        fill = {"type": "solid", "color": {"r": 10, "g": 200, "b": 90, "a": int(rng.choice([255, 120]))}}
        if morph:
            fill["morph_color"] = fill["color"]
        sc["left_fill"] = 1
    recs = [sc]
    xs, ys = [x], [y]
    for k in range(int(rng.integers(*segments))):
        if kind == "rectilinear":
            d = (int(rng.integers(-600, 600)), 0) if k % 2 == 0 else (0, int(rng.integers(-600, 600)))
        else:
            d = (int(rng.integers(-700, 700)), int(rng.integers(-700, 700)))
        e = {"type": "edge", "delta": {"x": d[0], "y": d[1]}}
        if kind == "curved" or (kind == "mixed" and rng.integers(0, 2)):
            e["control_delta"] = {"x": int(rng.integers(-500, 500)), "y": int(rng.integers(-500, 500))}
        if morph:
            e["morph_delta"] = {"x": d[0] + int(rng.integers(-150, 150)), "y": d[1] + int(rng.integers(-150, 150))}
            if "control_delta" in e:
                e["morph_control_delta"] = {"x": e["control_delta"]["x"] + int(rng.integers(-80, 80)), "y": e["control_delta"]["y"] + int(rng.integers(-80, 80))}
        x += d[0]; y += d[1]
        xs.append(x); ys.append(y)
        recs.append(e)
    col = {"r": int(rng.integers(0, 256)), "g": 30, "b": 60, "a": int(rng.choice([255, 255, 100]))}
    line = {"width": line_width, "fill": {"type": "solid", "color": col}}
    if morph:
        line["morph_width"] = int(line_width * rng.uniform(0.5, 2.0)) + 1
        line["fill"]["morph_color"] = col
    b = {"x_min": min(xs) - 400, "x_max": max(xs) + 400, "y_min": min(ys) - 400, "y_max": max(ys) + 400}
    tag = {"id": 1, "bounds": b, "shape": {"initial_styles": {"fill": [fill] if fill else [], "line": [line]}, "records": recs}}
    if morph:
        tag["morph_bounds"] = b
        tag["type"] = "define-morph-shape"
    return tag


def test_fuzz_stroked_shapes_edges_equal_oracle():
    """Host stroker vs the oracle's, edge for edge, over random open paths (straight, curved, rectilinear), line widths down to
    hairlines, reflecting / scaling placement matrices that push parts off the frame, and morph shapes (round caps and joins)."""
    import scenarios
    rng = np.random.default_rng(77)
    W, H = 120, 100
    for it in range(800):
        morph = bool(rng.integers(0, 3) == 0)
        tag = _rand_path_shape(rng, int(rng.choice([1, 2, 5, 20, 45, 90, 200])), morph)
        sx, sy = float(rng.choice([1, 1, 0.6, 1.7, -1])), float(rng.choice([1, 1, 0.8, 1.3]))
        mat = scenarios._m(sx, sy, int(rng.integers(-300, 900)) + (2000 if sx < 0 else 0), int(rng.integers(-300, 500)),
                           float(rng.choice([0, 0, 0.2])), float(rng.choice([0, 0, -0.15])))
        child = {"type": "morph-shape", "definition": tag, "ratio": float(rng.uniform(0, 1)), "matrix": mat} if morph else \
                {"type": "shape", "definition": tag, "matrix": mat}
        stage = {"children": [child]}
        r = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY)
        edges, paths, styles = r.build_frame(stage)
        r.close()
        tap = _Tap(W, H)
        cr.CanvasReplay(tap, linear_extension=True).render(stage)
        assert not tap.unsupported

        def visible(pe):        # the host drops polygons whose pixel rectangle inside the frame is empty (nothing would be painted)
            x0 = min(pe[:, 0].min(), pe[:, 2].min()) >> 8
            x1 = (max(pe[:, 0].max(), pe[:, 2].max()) + 255) >> 8
            y0, y1 = pe[:, 4].min() >> 8, (pe[:, 5].max() + 255) >> 8
            return max(x0, 0) < min(x1, W) and max(y0, 0) < min(y1, H)

        polys = [(pe, rect) for pe, rect in tap.polys if visible(pe)]
        assert len(paths) == len(polys), it
        for pth, (pe, rect) in zip(paths, polys):
            e = edges[pth["first_edge"]: pth["first_edge"] + pth["n_edges"]]
            assert (pth["kind"] == api.PATH_BOXES) == bool(rect), it
            if rect:
                continue
            got = np.stack([e[k] for k in ("x1", "y1", "x2", "y2", "top", "bottom", "dir")], 1)
            assert got.shape == pe.shape and (got == pe).all(), it
        tap.close()

def test_frame_build_on_several_threads_equals_single_thread(monkeypatch):
    """A frame with many top-level display objects is built by several threads (contiguous ranges of children, joined in painter's
    order).  Same edge list, paths and styles as one thread -- including the one cross-object rule, the SOURCE-rule lerp of the first
    translucent paint on a still-clear surface: scenes whose first painted object lies in a later piece, scenes that start with
    objects entirely off the frame (they leave the surface clear), S1, and the error of the first bad display object."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth

    def build(stage, w, h, threads):
        monkeypatch.setenv("SWFR_BUILD_THREADS", str(threads))
        r = S.Renderer(w, h, device=api.DEVICE_HOST_ONLY)
        try:
            e, p, st = r.build_frame(stage)
            return e.tobytes(), p.tobytes(), b"".join(bytes(x) for x in st)
        finally:
            r.close()

    rng = np.random.default_rng(11)
    def tri(x, y, size, color):
        pts = [(x, y), (x + size, y + size * 0.3), (x + size * 0.4, y + size)]
        return {"type": "shape", "definition": scenarios._poly_shape(pts, {"type": "solid", "color": color})}
    w, h = 200, 160
    for case in range(6):
        kids = []
        n = 300 + 67 * case
        first_visible = [0, 70, 150, n - 1, 64, 128][case]
        for i in range(n):
            off_frame = i < first_visible
            x = -9000 if off_frame else int(rng.integers(0, w * 20 - 400))
            y = -9000 if off_frame else int(rng.integers(0, h * 20 - 400))
            a = 255 if rng.random() < 0.3 else int(rng.integers(1, 255))
            kids.append(tri(x, y, int(rng.integers(60, 900)), scenarios._rgba(int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), a)))
        stage = {"children": kids}
        one = build(stage, w, h, 1)
        for threads in (2, 3, 8):
            assert build(stage, w, h, threads) == one, (case, threads)
        assert any(p for p in np.frombuffer(one[1], dtype=api.PATH_DTYPE)["lerp"])          # the scenes do exercise the rule
    cfg = synth.S1
    pts, cols = synth.scene(**cfg)
    stage = api.stars_to_stage(pts, cols)
    assert build(stage, cfg["width"], cfg["height"], 8) == build(stage, cfg["width"], cfg["height"], 1)
    # errors: the first failing display object in painter's order decides, whichever thread meets it
    bad = {"children": [tri(100, 100, 300, scenarios._rgba(1, 2, 3))] * 200 + [{"type": "shape", "id": 12345}] + [tri(100, 100, 300, scenarios._rgba(1, 2, 3))] * 200}
    for threads in (1, 4):
        monkeypatch.setenv("SWFR_BUILD_THREADS", str(threads))
        r = S.Renderer(64, 64, device=api.DEVICE_HOST_ONLY)
        with pytest.raises(S.SwfrError) as e:
            r.build_frame(bad)
        r.close()


# ---- the limits of the 24.8 device range: geometry up to +-32768 px (+-2^23 in 24.8), what validate_scene accepts
LIM = 1 << 23


def _assert_within_contract(edges, paths, W, H):
    """What validate_scene (renderer.cpp) requires of a frame, plus the frame builder's own promise that boxes lie inside the frame."""
    assert len(edges) == int(paths["n_edges"].sum()) if len(paths) else len(edges) == 0
    for k in ("x1", "y1", "x2", "y2"):
        assert len(edges) == 0 or (np.abs(edges[k].astype(np.int64)) <= LIM).all(), k
    for pth in paths:
        assert 0 <= pth["x_min"] < pth["x_max"] <= W and 0 <= pth["y_min"] < pth["y_max"] <= H
        e = edges[pth["first_edge"]: pth["first_edge"] + pth["n_edges"]]
        assert len(e) and (e["reserved"] == e["reserved"][0]).all()
        if pth["kind"] == api.PATH_BOXES:
            assert (e["x1"] < e["x2"]).all() and (e["y1"] < e["y2"]).all()
            assert (e["x1"] >= pth["x_min"] * 256).all() and (e["x2"] <= pth["x_max"] * 256).all()
            assert (e["y1"] >= pth["y_min"] * 256).all() and (e["y2"] <= pth["y_max"] * 256).all()
        else:
            act = e["top"] < e["bottom"]
            assert (e["y1"][act] < e["y2"][act]).all()
            assert (e["y1"][act] <= e["top"][act]).all() and (e["bottom"][act] <= e["y2"][act]).all()


def _square_outline(W=64, H=48, scale=32.76, tx=-2000, ty=-2000, width=200):
    sq = [(0, 0), (20000, 0), (20000, 20000), (0, 20000)]
    tag = scenarios._poly_shape(sq, None, line=scenarios._rgba(200, 30, 60), line_width=width)
    return dict(width=W, height=H, stage={"children": [{"type": "shape", "definition": tag, "matrix": scenarios._m(scale, scale, tx, ty)}]})


def test_rectilinear_stroke_near_the_limit_stays_inside_the_range():
    """A 20 000-twip square outline 200 twips wide under a stage scale of 32.76: its path ends at 32 660 px, inside the device range,
    but the box stroker's boxes reached 32 823.8 px (8 402 892 in 24.8, past 2^23) and validate_scene refused the whole frame.  The
    boxes are now clamped to the frame: here the top and left boxes cover the whole 64 x 48 frame (as in the oracle: 3072 pixels),
    and with the right side moved into the frame and a 20-twip line only a 32.76 px wide band of it is covered."""
    from helpers import oracle_render
    sc = _square_outline()
    r = S.Renderer(64, 48, device=api.DEVICE_HOST_ONLY)
    try:
        edges, paths, _ = r.build_frame(sc["stage"])
    finally:
        r.close()
    _assert_within_contract(edges, paths, 64, 48)
    assert len(paths) == 1 and paths[0]["kind"] == api.PATH_BOXES
    assert edges[["x1", "y1", "x2", "y2"]].tolist() == [(0, 0, 64 * 256, 48 * 256)]
    assert int((oracle_render(sc)[..., 3] > 0).sum()) == 64 * 48
    # the right side at x = 20000 twips * 32.76 / 20 + tx lands at 32 px: a band from 15.62 to 48.38 px, every row
    sc = _square_outline(tx=-(32760 - 32) * 20, width=20)
    r = S.Renderer(64, 48, device=api.DEVICE_HOST_ONLY)
    try:
        edges, paths, _ = r.build_frame(sc["stage"])
    finally:
        r.close()
    _assert_within_contract(edges, paths, 64, 48)
    half = 20 * 32.76 / 20 / 2 * 256        # (the 16.16 scale and 24.8 rounding move the band by at most 1/256 px)
    (x1, y1, x2, y2), = edges[["x1", "y1", "x2", "y2"]].tolist()
    assert (y1, y2) == (0, 48 * 256) and abs(x1 - (32 * 256 - half)) < 2 and abs(x2 - (32 * 256 + half)) < 2
    img = oracle_render(sc)
    cov = (img[..., 3] > 0).sum(1)
    assert (cov == 34).all()              # columns 15 .. 48: two partly covered, 32 fully


def test_boxes_of_a_path_do_not_merge_into_the_previous_paths_edges():
    """rectilinear_to_boxes appends to the frame's edge list and merges a box with the box above it of the same x range.  It used
    to search the whole list: a triangle whose last edge runs from (0, 0) to (10, 10) px followed by the rectangle (0, 10)-(10, 20)
    px extended the triangle's edge to (10, 20) and lost the rectangle."""
    A = scenarios._poly_shape([(0, 200), (0, 0), (200, 200)], {"type": "solid", "color": scenarios._rgba(255, 0, 0)})
    B = scenarios._poly_shape([(0, 200), (200, 200), (200, 400), (0, 400)], {"type": "solid", "color": scenarios._rgba(0, 0, 255)})
    stage = {"children": [{"type": "shape", "definition": A}, {"type": "shape", "definition": B}]}
    r = S.Renderer(32, 32, device=api.DEVICE_HOST_ONLY)
    try:
        edges, paths, _ = r.build_frame(stage)
    finally:
        r.close()
    assert paths["kind"].tolist() == [api.PATH_TOR, api.PATH_BOXES]
    assert edges[["x1", "y1", "x2", "y2", "top", "bottom", "dir"]].tolist() == [
        (0, 0, 0, 2560, 0, 2560, -1), (0, 0, 2560, 2560, 0, 2560, 1), (0, 2560, 2560, 5120, 2560, 5120, 0)]
    _assert_within_contract(edges, paths, 32, 32)


@pytest.mark.parametrize("mode", ["far", "long_shallow", "long_steep", "boundary"])
def test_extreme_scenes_edges_equal_oracle_and_meet_the_contract(mode):
    """Scenes whose vertices lie thousands of pixels off the frame, whose edges are tens of thousands of pixels long or 1/256 px
    tall, or whose end points sit exactly on +-32768 px (helpers.extreme_scene): the frame builder's tor edges equal the oracle's
    polygons edge for edge, and every built frame meets what validate_scene requires."""
    import zlib
    from helpers import extreme_scene
    rng = np.random.default_rng(zlib.crc32(mode.encode()) % 1000)
    n_tor = 0
    for it in range(120):
        W, H = [(64, 48), (333, 97)][it % 2]
        sc = extreme_scene(rng, W, H, mode)
        r = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY, even_odd=sc["even_odd"])
        try:
            edges, paths, _ = r.build_frame(sc["stage"])
        finally:
            r.close()
        _assert_within_contract(edges, paths, W, H)
        tap = _Tap(W, H)
        if sc["even_odd"]:
            tap.set_fill_rule(True)
        cr.CanvasReplay(tap, linear_extension=True).render(sc["stage"])
        assert not tap.unsupported

        def visible(pe):
            x0 = min(pe[:, 0].min(), pe[:, 2].min()) >> 8
            x1 = (max(pe[:, 0].max(), pe[:, 2].max()) + 255) >> 8
            y0, y1 = pe[:, 4].min() >> 8, (pe[:, 5].max() + 255) >> 8
            return max(x0, 0) < min(x1, W) and max(y0, 0) < min(y1, H)

        want = [pe for pe, rect in tap.polys if not rect and visible(pe)]
        got = [p for p in paths if p["kind"] == api.PATH_TOR]
        assert len(got) == len(want), (mode, it)
        for pth, pe in zip(got, want):
            e = edges[pth["first_edge"]: pth["first_edge"] + pth["n_edges"]]
            g = np.stack([e[k] for k in ("x1", "y1", "x2", "y2", "top", "bottom", "dir")], 1)
            assert g.shape == pe.shape and (g == pe).all(), (mode, it)
        n_tor += len(got)
        tap.close()
    assert n_tor > 100


@pytest.mark.xfail(strict=True, reason="open: a clipped polygon-stroke edge keeps its line's end points, which may lie past 2^23")
def test_polygon_stroke_near_the_limit_stays_inside_the_range():
    """The polygon stroker's counterpart of test_rectilinear_stroke_near_the_limit_stays_inside_the_range, still open: a 20 px wide
    stroke of a diagonal line through the frame ending at (32 766, 32 760) px has outline corners near 32 773 px.  Clipping to the frame keeps the end points of
    every line it cuts (the scan converter steps along the exact line), so the frame carries end points past 2^23 and a device
    handle refuses it with SWFR_ERR_INVALID (tests/test_gpu_extremes.py checks that refusal).  Moving the end points would change
    the line; bringing such an edge into range exactly needs another representation of its line."""
    from helpers import _fine_shape
    tag = _fine_shape([(20.0, 10.0), (32766.0, 32760.0)], None, None, line=scenarios._rgba(9, 99, 199), line_width_px=20.0, closed=False)
    stage = {"children": [{"type": "shape", "definition": tag, "matrix": scenarios._m(1 / 256, 1 / 256)}]}
    r = S.Renderer(64, 48, device=api.DEVICE_HOST_ONLY)
    try:
        edges, paths, _ = r.build_frame(stage)
    finally:
        r.close()
    assert len(paths) == 1
    _assert_within_contract(edges, paths, 64, 48)


def test_oracle_raw_edge_entry_equals_its_polygon_fill():
    """swfo_fill_edges (the checker of swfr_render_edges) against swfo_fill_polygons_fixed: closed polygons inside the frame, both
    fill rules, opaque and translucent colours painted over each other -- the same pixels."""
    rng = np.random.default_rng(5)
    painted = 0
    for it in range(60):
        W, H = int(rng.integers(8, 90)), int(rng.integers(8, 70))
        n = int(rng.integers(1, 4))
        verts = int(rng.integers(3, 9))
        xy = np.stack([rng.integers(0, W * 256 + 1, (n, verts)), rng.integers(0, H * 256 + 1, (n, verts))], -1).astype(np.int32)
        if it % 3 == 0:
            xy &= ~255                      # pixel-aligned vertices
        cols = rng.integers(0, 256, (n, 4)).astype(np.uint8)
        cols[: n // 2 + 1, 3] = 255
        eo = bool(it % 2)
        edges, paths, styles = api.polygons_to_scene(xy, cols, W, H)
        a, b = ob.OracleBackend(W, H), ob.OracleBackend(W, H)
        argb = np.array([s.pixel for s in styles], dtype=np.uint32)
        a.L.swfo_fill_polygons_fixed(a.ctx, xy.ctypes.data, np.full(n, verts, np.int32).ctypes.data, argb.ctypes.data, n, int(eo))
        for p in paths:
            e = edges[p["first_edge"]: p["first_edge"] + p["n_edges"]]
            b.fill_edges(e, (p["x_min"], p["y_min"], p["x_max"], p["y_max"]), eo, argb[p["style"]])
        ia, ib = a.premultiplied_rgba(), b.premultiplied_rgba()
        a.close(); b.close()
        assert np.array_equal(ia, ib), it
        painted += int(((ia[..., 3] > 0) & (ia[..., 3] < 255)).sum())
    assert painted > 1000
    # edges whose directions do not balance in a row of the rectangle are no closed polygon: refused, not scan-converted (Cairo's
    # full-row pass would run off its active list); outside the rectangle's rows they do not matter
    b = ob.OracleBackend(16, 16)
    try:
        with pytest.raises(ValueError):
            b.fill_edges(np.array([[0, 0, 4096, 4096, 0, 4096, 1, 0], [256, 0, 256, 4096, 0, 2048, -1, 0]]), (0, 0, 16, 16), False, 0xff000000)
        b.fill_edges(np.array([[0, 0, 4096, 4096, 0, 4096, 1, 0], [256, 0, 256, 8192, 0, 8192, -1, 0]]), (0, 0, 16, 16), False, 0xff000000)
        assert b.premultiplied_rgba()[..., 3].any()
    finally:
        b.close()


def test_dense_generator_covers_every_kind():
    """tests/helpers.py rand_dense_scene is what pins the shaded tile instances' crowded strips (tests/test_gpu_instances.py): its
    frames must keep having strips of more than 16 and of more than 32 entries, every kind of path and of style, opaque covers
    of the whole frame, a translucent first draw, a width that is not a multiple of 64 and a tile-row count that is not a
    multiple of 8 -- checked on the frames the product builds, so that a change to the generator cannot quietly test less."""
    from helpers import rand_dense_scene, strip_path_counts
    rng = np.random.default_rng(4040)                  # (test_gpu_instances.py DENSE_SEED: the same frames)
    painted = crowded = over32 = 0
    path_kinds, style_kinds, fills = set(), set(), set()
    for it in range(40):
        sc = rand_dense_scene(rng)
        W, H = sc["width"], sc["height"]
        assert W % 64 != 0 and ((H + 15) // 16) % 8 != 0, (it, W, H)
        r = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY)
        try:
            for b in sc["bitmaps"]:
                r.add_bitmap(b)
            edges, paths, styles = r.build_frame(sc["stage"])
        finally:
            r.close()
        cnt = strip_path_counts(W, H, paths)
        painted += int((cnt > 0).sum())
        crowded += int((cnt > 16).sum())
        over32 += int((cnt > 32).sum())
        path_kinds |= set(int(k) for k in paths["kind"])
        style_kinds |= set(s.kind for s in styles)
        for p in paths:
            s = styles[p["style"]]
            a = s.pixel >> 24
            full = p["x_min"] == 0 and p["y_min"] == 0 and p["x_max"] == W and p["y_max"] == H
            if s.kind == api.STYLE_SOLID:
                fills.add("opaque" if a == 255 else "translucent")
                fills.add("alpha1" if a == 1 else ("alpha254" if a == 254 else "other"))
                if a == 255 and full:
                    fills.add("box cover" if p["kind"] == api.PATH_BOXES else "tor cover")
            if s.kind == api.STYLE_BITMAP:
                fills.add("repeat" if s.extend else "clamped")
                k = float(np.hypot(s.inv[0], s.inv[1]))   # texels per pixel along x
                fills.add("magnified" if k < 0.75 else ("minified" if k > 1.4 else "near 1"))
            if s.kind == api.STYLE_RADIAL:
                fills.add("focal" if s.c0x != 0 else "radial")
        first = paths[0]
        assert first["lerp"] == 1 and styles[first["style"]].pixel >> 24 < 255, it      # translucent onto the clear surface
    assert crowded * 4 >= painted and over32 > 0, (painted, crowded, over32)
    assert path_kinds == {api.PATH_TOR, api.PATH_BOXES}
    assert style_kinds == {api.STYLE_SOLID, api.STYLE_BITMAP, api.STYLE_RADIAL}      # (no linear gradient in the bit-exact corpus)
    assert {"opaque", "translucent", "alpha1", "alpha254", "box cover", "tor cover", "repeat", "clamped", "magnified", "minified",
            "focal", "radial"} <= fills, fills
    rng = np.random.default_rng(4041)
    assert any(s.kind == api.STYLE_LINEAR for _ in range(3) for s in _dense_styles(rand_dense_scene(rng, linear=True)))


def _dense_styles(sc):
    r = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
    try:
        for b in sc["bitmaps"]:
            r.add_bitmap(b)
        return r.build_frame(sc["stage"])[2]
    finally:
        r.close()


def test_batch_corpus_kinds_keep_their_properties():
    """tests/helpers.py batch_corpus is what mixes unlike frames in one batch group (tests/test_gpu_batches.py): every kind must keep
    the property it is in the corpus for -- checked on the frames the product builds, so that a change to a generator or a scenario
    cannot quietly empty a kind.  (Queued, crowded and tied rows are counted by the GPU test itself.)"""
    from helpers import BATCH_H, BATCH_W, batch_corpus
    corpus = batch_corpus()
    assert list(corpus) == ["empty", "boxes", "solid", "translucent", "bitmaps", "radial_focal", "linear", "round_strokes", "tie", "comb",
                            "long_path", "cxform", "morph"]
    built = {}
    for kind, sc in corpus.items():
        assert (sc["width"], sc["height"]) == (BATCH_W, BATCH_H), kind
        r = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
        try:
            for b in sc["bitmaps"]:
                r.add_bitmap(b)
            built[kind] = r.build_frame(sc["stage"])
        finally:
            r.close()
    ids = {}
    for sc in corpus.values():
        for b in sc["bitmaps"]:
            assert ids.setdefault(b["id"], b) is b, "one bitmap per id across the corpus"

    def kinds_of(kind):
        _, p, s = built[kind]
        return set(int(k) for k in p["kind"]), set(x.kind for x in s)

    e, p, s = built["empty"]
    assert len(e) == len(p) == 0
    # boxes only (no tor chunks): fills at whole and fractional pixels, and rectilinear strokes
    e, p, s = built["boxes"]
    assert kinds_of("boxes") == ({api.PATH_BOXES}, {api.STYLE_SOLID}) and len(p) >= 5
    xy = np.stack([e["x1"], e["y1"], e["x2"], e["y2"]], -1)
    assert (xy % 256 != 0).any() and (xy % 256 == 0).all(-1).any()
    # solid styles only (the compact style table) and tor paths
    for kind in ("solid", "translucent", "long_path", "round_strokes", "tie", "comb", "morph"):
        assert kinds_of(kind)[1] == {api.STYLE_SOLID}, kind
        assert api.PATH_TOR in kinds_of(kind)[0], kind
    alphas = [x.pixel >> 24 for x in built["translucent"][2]]
    assert sum(a < 255 for a in alphas) >= 2, alphas
    # bitmap fills: repeat and clamped, magnified and minified
    fills = set()
    for x in built["bitmaps"][2]:
        if x.kind == api.STYLE_BITMAP:
            fills.add("repeat" if x.extend else "clamped")
            k = float(np.hypot(x.inv[0], x.inv[1]))
            fills.add("magnified" if k < 0.75 else ("minified" if k > 1.4 else "near 1"))
    assert {"repeat", "clamped", "magnified", "minified"} <= fills, fills
    # radial and focal gradients; a linear gradient
    grads = [x for x in built["radial_focal"][2] if x.kind == api.STYLE_RADIAL]
    assert any(x.c0x != 0 for x in grads) and any(x.c0x == 0 for x in grads)
    assert api.STYLE_LINEAR in kinds_of("linear")[1]
    # a path of more than ROWS_STAGE (32) edges in a solid-only frame; a comb of more than 64 edges active in one row
    assert int(built["long_path"][1]["n_edges"].max()) > 32
    assert int(built["comb"][1]["n_edges"].max()) >= 120
    assert int(built["round_strokes"][1]["n_edges"].max()) > 32
    # the colour-transformed bitmap: a texture variant of the texel pass
    assert any(x.kind == api.STYLE_BITMAP and x.bitmap >= api.VARIANT_BASE for x in built["cxform"][2])
    # morph shapes: four placements at several ratios; the soak scene's shapes
    assert len(built["morph"][1]) >= 4 and len(built["tie"][1]) >= 2
