"""Colour transforms (swfr_set_color_transform, SWFR_OBJECT_COLOR_TRANSFORM, "color_transform" on display objects).

The rule is defined by a lowering (tools/make_cxform_goldens.py, imported here): a transformed stage renders exactly as the same
stage with the transforms removed, recoloured copies of its definitions and recoloured bitmaps under fresh ids.  Without a GPU: the
C-ABI, the host walk against the walk of the lowered stage, the clamp between nested transforms, the premultiply arithmetic of the
texel pass, and the goldens against live libcairo.  On the GPU (or `python tools/emu/run.py tests/test_color_transform.py`): every
scenario under every transform against its golden and the live lowered oracle, the bitmap texel pass, every render route, the texture
cache, and random transform trees."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_cxform_goldens as G  # noqa: E402
import scenarios  # noqa: E402
from helpers import GOLD, diff_stats, golden  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402

SC = scenarios.scenarios()
LINEAR = {name for name, sc in SC.items() if not sc["exact"]}      # linear gradients: the documented +-1 LSB extension
EMU = bool(os.environ.get("SWFR_EMULATOR"))
needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")


def _renderer(w, h, device=0, **kw):
    import swf_renderer_amd as S
    return S.Renderer(w, h, device=device, **kw)


def _host(sc):
    from swf_renderer_amd import api
    return _renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY, even_odd=bool(sc.get("even_odd")))


def _register(r, sc, low=None):
    for b in sc.get("bitmaps", []):
        r.add_bitmap(b)
    if low is not None:
        for bid, (w, h, px) in low.extra.items():
            r.register_bitmap(bid, w, h, px)


def assert_matches(got, want, exact=True):
    n, mx = diff_stats(got, want)
    if exact:
        assert (n, mx) == (0, 0)
    else:
        assert mx <= 1, (n, mx)


# ---------------------------------------------------------------------------------------------------------- without a GPU
def test_abi_export_and_version():
    from swf_renderer_amd import api
    L = api.load_library()
    assert hasattr(L, "swfr_set_color_transform")
    assert L.swfr_abi_version() == 1
    assert api.OBJECT_COLOR_TRANSFORM == 3


def test_slot_and_value_ranges_are_checked():
    from swf_renderer_amd import api
    r = _renderer(16, 16, device=api.DEVICE_HOST_ONLY)
    try:
        ok = api.ColorTransform((C.c_int32 * 4)(256, 256, 256, 256), (C.c_int32 * 4)(0, 0, 0, 0))
        assert r.L.swfr_set_color_transform(r.h, 65535, C.byref(ok)) == api.OK
        assert r.L.swfr_set_color_transform(r.h, 65536, C.byref(ok)) == api.ERR_INVALID
        assert r.L.swfr_set_color_transform(r.h, 0, None) == api.OK                    # clearing an unset slot
        for k in range(8):
            for bad in (32768, -32769):
                v = [256] * 4 + [0] * 4
                v[k] = bad
                ct = api.ColorTransform((C.c_int32 * 4)(*v[:4]), (C.c_int32 * 4)(*v[4:]))
                assert r.L.swfr_set_color_transform(r.h, 1, C.byref(ct)) == api.ERR_INVALID
            v = [256] * 4 + [0] * 4
            v[k] = 32767 if k % 2 else -32768
            ct = api.ColorTransform((C.c_int32 * 4)(*v[:4]), (C.c_int32 * 4)(*v[4:]))
            assert r.L.swfr_set_color_transform(r.h, 1, C.byref(ct)) == api.OK
    finally:
        r.close()


def _raw_stage(obj_type, slot, child_shape_id):
    from swf_renderer_amd import api
    kid = api.DisplayObject()
    kid.type, kid.id = api.OBJECT_SHAPE, child_shape_id
    kids = (api.DisplayObject * 1)(kid)
    d = api.DisplayObject()
    d.type, d.id = obj_type, slot
    d.n_children, d.children = 1, C.cast(kids, C.POINTER(api.DisplayObject))
    objs = (api.DisplayObject * 1)(d)
    s = api.Stage()
    s.width = s.height = 16
    s.n_children, s.children = 1, C.cast(objs, C.POINTER(api.DisplayObject))
    return s, (kids, objs)


def test_unset_slot_and_unknown_types():
    from swf_renderer_amd import api
    r = _renderer(16, 16, device=api.DEVICE_HOST_ONLY)
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": scenarios._rgba(9, 9, 9)}))
        s, keep = _raw_stage(api.OBJECT_COLOR_TRANSFORM, 7, sid)
        n = C.c_size_t()
        args = (C.byref(C.c_void_p()), C.byref(n), C.byref(C.c_void_p()), C.byref(C.c_size_t()), C.byref(C.c_void_p()), C.byref(C.c_size_t()))
        assert r.L.swfr_build_frame(r.h, C.byref(s), *args) == api.ERR_NOT_FOUND
        assert r.L.swfr_last_error(r.h).decode() == "ColorTransformNotFound"
        r.set_color_transform(7, G.cxform(mult=(0, 0, 0, 256), add=(255, 0, 0, 0)))
        assert r.L.swfr_build_frame(r.h, C.byref(s), *args) == api.OK and n.value > 0
        r.set_color_transform(7, None)                                                # cleared again
        assert r.L.swfr_build_frame(r.h, C.byref(s), *args) == api.ERR_NOT_FOUND
        s4, keep4 = _raw_stage(4, 7, sid)
        assert r.L.swfr_build_frame(r.h, C.byref(s4), *args) == api.ERR_INVALID
        assert r.L.swfr_last_error(r.h).decode() == "UnexpectedDisplayObjectType"
    finally:
        r.close()


def test_python_values():
    from swf_renderer_amd import api
    ct = {"red_mult": {"epsilons": -256}, "green_mult": 2, "blue_mult": 0.5, "alpha_mult": {"epsilons": 77},
          "red_add": 255, "green_add": -3, "blue_add": 0, "alpha_add": 1}
    assert api.color_transform_values(ct) == (-256, 512, 128, 77, 255, -3, 0, 1) == G.values(ct)
    assert api.color_transform_values({}) == (256, 256, 256, 256, 0, 0, 0, 0)


def _frame_key(frame, ignore_bitmap_field=True):
    edges, paths, styles = frame
    st = []
    for s in styles:
        b = bytes(s)
        if ignore_bitmap_field and s.kind == 3:
            off = type(s).bitmap.offset
            b = b[:off] + b[off + 4:]
        st.append(b)
    return edges.tobytes(), paths.tobytes(), st


def _host_pair(sc, stage):
    """swfr_build_frame of a transformed stage and of its lowered stage, on host-only handles"""
    low = G.Lowering(sc.get("bitmaps", []))
    lowered = low.lower(stage)
    r0, r1 = _host(sc), _host(sc)
    try:
        _register(r0, sc)
        _register(r1, sc, low)
        return r0.build_frame(stage), r1.build_frame(lowered)
    finally:
        r0.close()
        r1.close()


@pytest.mark.parametrize("transform", sorted(G.TRANSFORMS))
@pytest.mark.parametrize("name", sorted(SC))
def test_host_walk_equals_lowered_walk(name, transform):
    """the frame builder applies the chain to the straight colours before anything else: edges, paths and styles of a transformed
    stage are those of its lowered stage, except which texture a bitmap style names"""
    sc = SC[name]
    got, want = _host_pair(sc, G.apply_transform(sc["stage"], transform))
    assert _frame_key(got) == _frame_key(want)
    e, p, s = got
    n_var = sum(1 for x in s if x.kind == 3 and x.bitmap >= 65536)
    assert n_var == (0 if transform == "identity" or not sc.get("bitmaps") else sum(1 for x in s if x.kind == 3))


@pytest.mark.parametrize("name", sorted(SC))
def test_identity_wrapper_is_byte_identical(name):
    sc = SC[name]
    stages = [sc["stage"], G.apply_transform(sc["stage"], "identity"), G.apply_transform_value(G.apply_transform(sc["stage"], "identity"), G.cxform())]
    r = _host(sc)
    try:
        _register(r, sc)
        frames = [r.build_frame(st) for st in stages]
    finally:
        r.close()
    base = _frame_key(frames[0], ignore_bitmap_field=False)
    assert _frame_key(frames[1], ignore_bitmap_field=False) == base
    assert _frame_key(frames[2], ignore_bitmap_field=False) == base


def _solid_pixel(r, stage):
    e, p, s = r.build_frame(stage)
    assert len(s) == 1
    return s[0].pixel


def test_nested_clamp_innermost_first():
    """mult 512 inside mult 128: the inner x2 clamps at 255 before the outer x0.5 -- 200 -> 255 -> 127, not 200; swapped: 200 -> 100 -> 200"""
    from swf_renderer_amd import api
    shape = scenarios._poly_shape([(0, 0), (300, 0), (300, 300), (0, 300)], {"type": "solid", "color": scenarios._rgba(200, 100, 10, 255)})
    r = _renderer(20, 20, device=api.DEVICE_HOST_ONLY)
    try:
        def nested(outer, inner):
            return {"children": [{"type": "container", "color_transform": G.cxform(mult=(outer,) * 3 + (256,)),
                                  "children": [{"type": "shape", "definition": shape, "color_transform": G.cxform(mult=(inner,) * 3 + (256,))}]}]}
        px = _solid_pixel(r, nested(128, 512))
        assert (px >> 16) & 255 == 127 and (px >> 8) & 255 == 100 and px & 255 == 10
        px = _solid_pixel(r, nested(512, 128))
        assert (px >> 16) & 255 == 200 and (px >> 8) & 255 == 100 and px & 255 == 10
        # negative mult: an arithmetic (floor) shift -- (-1 * 1) >> 8 = -1, + 1 = 0 (a truncating shift would give 1)
        ct = G.cxform(mult=(1, 256, 256, 256), add=(1, 0, 0, 0))
        assert G.table(ct)[0][1] == 1 and G.table(G.cxform(mult=(-1, 256, 256, 256), add=(1, 0, 0, 0)))[0][1] == 0
        one = {"children": [{"type": "shape", "definition": scenarios._poly_shape([(0, 0), (300, 0), (300, 300)], {"type": "solid", "color": scenarios._rgba(1, 0, 0, 255)}),
                             "color_transform": G.cxform(mult=(-1, 256, 256, 256), add=(1, 0, 0, 0))}]}
        assert (_solid_pixel(r, one) >> 16) & 255 == 0
    finally:
        r.close()


def test_parallel_walk_equals_single_walk():
    """a stage with hundreds of top-level objects is built by several threads: same arrays, same texture numbering"""
    from swf_renderer_amd import api
    rng = np.random.default_rng(5)
    sc = SC["bitmap_repeat_over_solid"]
    kids = []
    for i in range(300):
        k = dict(sc["stage"]["children"][i % 2])
        k["matrix"] = scenarios._m(0.3, 0.3, int(rng.integers(0, 2000)), int(rng.integers(0, 1500)))
        if i % 3:
            k["color_transform"] = G.cxform(mult=(256, 256, 256, int(rng.choice([64, 128, 200]))), add=(int(rng.choice([0, 40])), 0, 0, 0))
        kids.append(k)
    _assert_parallel_walk_is_single_walk(sc, {"children": kids})


@pytest.mark.parametrize("wrap", ["fade", "nested_with_matrix", "missing_slot"])
def test_parallel_walk_inside_one_wrapper(wrap):
    """a whole clip under one fade: the children of the stage's single wrapper (through nested single wrappers) are cut into pieces
    and walked in the wrappers' state -- the same arrays and texture numbering as one walk, and the same error"""
    from swf_renderer_amd import api
    sc = SC["bitmap_repeat_over_solid"]
    kids = []
    for i in range(400):
        k = dict(sc["stage"]["children"][i % 2])
        k["matrix"] = scenarios._m(0.25, 0.25, (i * 37) % 2400, (i * 53) % 1800)
        if i % 5 == 0:
            k["color_transform"] = G.cxform(mult=(256, 128, 256, 256))
        kids.append(k)
    fade = G.cxform(mult=(256, 256, 256, 150), add=(20, 0, 0, 0))
    if wrap == "fade":
        stage = {"children": [{"type": "container", "color_transform": fade, "children": kids}]}
    else:
        stage = {"children": [{"type": "container", "color_transform": fade, "children": [
            {"type": "container", "matrix": scenarios._m(0.8, 0.9, 300, -200, 0.1, 0.05), "children": kids}]}]}
    if wrap != "missing_slot":
        _assert_parallel_walk_is_single_walk(sc, stage)
        return
    # a type-3 wrapper naming an unset slot, built from raw structs: every route reports ColorTransformNotFound
    for threads in ("1", "8"):
        os.environ["SWFR_BUILD_THREADS"] = threads
        try:
            r = _host(sc)
            _register(r, sc)
            arena = api._Arena()
            inner = r._stage(arena, {"children": kids})
            w = api.DisplayObject()
            w.type, w.id = api.OBJECT_COLOR_TRANSFORM, 999
            w.n_children, w.children = inner.n_children, inner.children
            objs = (api.DisplayObject * 1)(w)
            st = api.Stage()
            st.n_children, st.children = 1, C.cast(objs, C.POINTER(api.DisplayObject))
            r._apply_cxforms(arena)
            out = (C.c_void_p(), C.c_size_t())
            rc = r.L.swfr_build_frame(r.h, C.byref(st), C.byref(out[0]), C.byref(out[1]), C.byref(C.c_void_p()), C.byref(C.c_size_t()),
                                      C.byref(C.c_void_p()), C.byref(C.c_size_t()))
            assert rc == api.ERR_NOT_FOUND and r.L.swfr_last_error(r.h).decode() == "ColorTransformNotFound"
            r.close()
        finally:
            del os.environ["SWFR_BUILD_THREADS"]


def _assert_parallel_walk_is_single_walk(sc, stage):
    from swf_renderer_amd import api
    out = []
    for threads in ("1", "8"):
        os.environ["SWFR_BUILD_THREADS"] = threads
        try:
            r = _host(sc)
            _register(r, sc)
            out.append(r.build_frame(stage))
            r.close()
        finally:
            del os.environ["SWFR_BUILD_THREADS"]
    assert _frame_key(out[0], False) == _frame_key(out[1], False)
    assert any(s.kind == 3 and s.bitmap >= api.VARIANT_BASE for s in out[0][2])


def test_div255_multiply_shift_is_exact():
    """the formula the texel pass divides c * a by 255 with, (x + 1 + (x >> 8)) >> 8 (csrc/cxform.hip, cx_mul_div255), restated in numpy:
    exact for every c, a in 0..255.  (The device's own arithmetic: test_texel_pass_exhaustive.)"""
    c = np.arange(256, dtype=np.uint32)[:, None]
    a = np.arange(256, dtype=np.uint32)[None, :]
    x = c * a
    assert ((x + 1 + (x >> 8)) >> 8 == x // 255).all()


@needs_cairo
@pytest.mark.parametrize("transform", sorted(t for t in G.TRANSFORMS if t != "identity"))
def test_goldens_match_live_libcairo(transform):
    g = np.load(os.path.join(GOLD, "cairo_cxform_%s.npz" % transform))
    for name, sc in SC.items():
        assert (G.cairo_cxform(sc, G.apply_transform(sc["stage"], transform)) == g[name]).all(), name


# ---------------------------------------------------------------------------------------------------------- on the GPU
def _want(name, transform):
    return golden("cairo_" + name, "rgba_premul") if transform == "identity" else np.load(os.path.join(GOLD, "cairo_cxform_%s.npz" % transform))[name]


def _product(sc, stage, **kw):
    r = _renderer(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")), **kw)
    try:
        _register(r, sc)
        r.render(stage)
        return r.read_image(premultiplied=True)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("transform", sorted(G.TRANSFORMS))
@pytest.mark.parametrize("name", sorted(SC))
def test_scenario_under_transform(gpu, name, transform):
    sc = SC[name]
    stage = G.apply_transform(sc["stage"], transform)
    got = _product(sc, stage)
    assert_matches(got, _want(name, transform), exact=name not in LINEAR)
    assert_matches(got, G.oracle_cxform(sc, stage), exact=name not in LINEAR)


@pytest.mark.gpu
def test_one_bitmap_plain_and_under_two_transforms(gpu):
    sc = SC["bitmap_repeat_over_solid"]
    shape = sc["stage"]["children"][1]
    stage = {"children": [dict(shape, matrix=scenarios._m(0.5, 0.5, 0, 0)),
                          dict(shape, matrix=scenarios._m(0.5, 0.5, 1500, 0), color_transform=G.cxform(mult=(256, 0, 0, 256))),
                          dict(shape, matrix=scenarios._m(0.5, 0.5, 0, 1100), color_transform=G.cxform(mult=(256, 256, 256, 100), add=(0, 90, 0, 0)))]}
    got = _product(sc, stage)
    assert_matches(got, G.oracle_cxform(sc, stage))
    assert (got[..., 3] > 0).sum() > 1000


@pytest.mark.gpu
def test_texel_pass_exhaustive(gpu):
    """a 256 x 256 bitmap whose texel (x, y) is (x, 255 - x, x ^ 0x5a, y), mapped 1:1 onto the pixels (no filtering): every pixel is
    the premultiplied transformed texel, for every (channel value, alpha) pair"""
    W = 256
    x = np.arange(W, dtype=np.int64)[None, :].repeat(W, 0)
    y = np.arange(W, dtype=np.int64)[:, None].repeat(W, 1)
    tex = np.stack([x, 255 - x, x ^ 0x5A, y], -1).astype(np.uint8)
    square = scenarios._poly_shape([(0, 0), (W * 20, 0), (W * 20, W * 20), (0, W * 20)],
                                   {"type": "bitmap", "bitmap_id": 7, "repeating": False, "smoothed": False, "matrix": scenarios._m(20, 20)})
    cts = [G.cxform(), G.cxform(mult=(-256, -256, -256, 256), add=(255, 255, 255, 0)), G.cxform(mult=(300, 77, -20, 180), add=(-30, 60, 255, 40)),
           G.cxform(mult=(256, 256, 256, 0), add=(0, 0, 0, 128))]
    r = _renderer(W, W)
    try:
        r.register_bitmap(7, W, W, tex.tobytes())
        for ct in cts:
            r.render({"children": [{"type": "shape", "definition": square, "color_transform": ct}]})
            got = r.read_image(premultiplied=True).astype(np.int64)
            t = G.table(ct).astype(np.int64)
            s = np.stack([t[k][tex[..., k]] for k in range(4)], -1)
            want = np.concatenate([s[..., :3] * s[..., 3:] // 255, s[..., 3:]], -1)
            assert (got == want).all(), ct
    finally:
        r.close()


class _Dest:
    """n frames of device memory for render_batch (a torch tensor; under the emulator, whose device memory is host memory, numpy)"""

    def __init__(self, n, h, w):
        if EMU:
            self.a = np.zeros((n, h, w, 4), np.uint8)
            self.ptr = self.a.ctypes.data
        else:
            import torch
            self.t = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
            self.ptr = self.t.data_ptr()

    def numpy(self):
        if EMU:
            return self.a.copy()
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def _fade_stages(sc, n):
    return [G.apply_transform_value(sc["stage"], G.cxform(mult=(256, 256, 256, int(256 * (i + 1) / n)), add=(i % 3, 0, 0, 0))) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("antialias", ["default", "none"])
def test_routes_agree(gpu, antialias):
    """swfr_render, render_batch (device destination and none), render_sequence(_readback), build_frame + upload_edges, banded handles"""
    sc = SC["bitmap_no_repeat_magnified"]
    n = 6 if EMU else 64
    stages = _fade_stages(sc, n)
    W, H = sc["width"], sc["height"]
    singles = []
    r = _renderer(W, H, antialias=antialias)
    try:
        _register(r, sc)
        for st in stages:
            r.render(st)
            singles.append(r.read_image(premultiplied=True).copy())
        dst = _Dest(n, H, W)
        r.render_batch(stages, dst.ptr, W * H * 4)
        batch = dst.numpy()
        for i in range(n):
            assert (batch[i] == singles[i]).all(), i
        r.render_batch(stages)
        assert (r.read_image(premultiplied=True) == singles[-1]).all()
        r.render_sequence(stages[:3])
        assert (r.read_image(premultiplied=True) == singles[2]).all()
        r.render_sequence_readback(stages[:4], premultiplied=True)
        assert (r.read_image(premultiplied=True) == singles[3]).all()
        e, p, s = r.build_frame(stages[1])
        r.upload_edges(e, p, s)
        r.render_resident(3)
        assert (r.read_image(premultiplied=True) == singles[1]).all()
    finally:
        r.close()
    if antialias == "default":
        for i in (0, n - 1):
            assert_matches(singles[i], G.oracle_cxform(sc, stages[i]))
        # banded handles: every band's rows are the full frame's
        for bc in (2, 3):
            for bi in range(bc):
                rb = _renderer(W, H, band_index=bi, band_count=bc)
                try:
                    _register(rb, sc)
                    rb.render(stages[2])
                    img = rb.read_image(premultiplied=True)
                finally:
                    rb.close()
                for t in range(bi, (H + 15) // 16, bc):              # the band's own tile-rows
                    assert (img[t * 16:t * 16 + 16] == singles[2][t * 16:t * 16 + 16]).all()


@pytest.mark.gpu
def test_cache_steady_changed_and_reregistered(gpu):
    sc = SC["bitmap_minified_rotated"]
    W, H = sc["width"], sc["height"]
    a = G.apply_transform_value(sc["stage"], G.cxform(mult=(256, 128, 128, 256)))
    r = _renderer(W, H)
    try:
        _register(r, sc)
        r.render(a)
        first = r.read_image(premultiplied=True).copy()
        r.render(a)
        assert (r.read_image(premultiplied=True) == first).all()
        assert_matches(first, G.oracle_cxform(sc, a))
        # a type-3 object names slot 0: its value at the time of the call is used, never a stale texture
        for ct in (G.cxform(mult=(0, 256, 256, 256)), G.cxform(mult=(256, 256, 0, 256))):
            b = G.apply_transform_value(sc["stage"], ct)
            r.render(b)
            assert_matches(r.read_image(premultiplied=True), G.oracle_cxform(sc, b))
        # re-registering the bitmap (other texels, same id) invalidates its textures
        low = G.Lowering(sc["bitmaps"])
        w, h, px = low.straight[3]
        flipped = px[::-1].copy()
        r.register_bitmap(3, w, h, flipped.tobytes())
        r.render(a)
        got = r.read_image(premultiplied=True)
        r2 = _renderer(W, H)
        try:
            r2.register_bitmap(3, w, h, flipped.tobytes())
            r2.render(a)
            assert (got == r2.read_image(premultiplied=True)).all()
        finally:
            r2.close()
        assert not (got == first).all()
    finally:
        r.close()


@pytest.mark.gpu
def test_tiny_cache_budget_keeps_frames_right(gpu, monkeypatch):
    monkeypatch.setenv("SWFR_CXFORM_CACHE_MB", "0")
    sc = SC["bitmap_repeat_over_solid"]
    W, H = sc["width"], sc["height"]
    n = 5 if EMU else 40
    stages = [G.apply_transform_value(sc["stage"], G.cxform(mult=(256 - 5 * i, 256, 100 + 3 * i, 256), add=(0, i, 0, 0))) for i in range(n)]
    r = _renderer(W, H)
    try:
        _register(r, sc)
        dst = _Dest(n, H, W)
        for rep in range(2):
            r.render_batch(stages, dst.ptr, W * H * 4)
            out = dst.numpy()
            for i in (0, n // 2, n - 1):
                assert_matches(out[i], G.oracle_cxform(sc, stages[i]))
            for i, st in enumerate(stages[:3]):
                r.render(st)
                assert (r.read_image(premultiplied=True) == out[i]).all()
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch_frames", ["1", "2", "64"])
def test_first_use_inside_a_batch(gpu, monkeypatch, batch_frames):
    """a fresh handle whose first use of a bitmap under transforms is a render_batch with a distinct transform per frame: the frames run on
    several frame-set streams (SWFR_BATCH_FRAMES=1) or batch groups (2): each texel pass is ordered after the one-time upload of the
    bitmap's texels, wherever that upload was queued"""
    monkeypatch.setenv("SWFR_BATCH_FRAMES", batch_frames)
    sc = SC["bitmap_no_repeat_minified"]
    W, H = sc["width"], sc["height"]
    n = 4 if EMU else 12
    stages = [G.apply_transform_value(sc["stage"], G.cxform(mult=(256, 256 - 9 * i, 256, 256 - 7 * i), add=(3 * i, 0, 0, 0))) for i in range(n)]
    want = [G.oracle_cxform(sc, st) for st in stages]
    r = _renderer(W, H)
    try:
        _register(r, sc)
        dst = _Dest(n, H, W)
        r.render_batch(stages, dst.ptr, W * H * 4)
        out = dst.numpy()
        for i in range(n):
            assert_matches(out[i], want[i])
    finally:
        r.close()
    r = _renderer(W, H)
    try:
        _register(r, sc)
        r.render_batch(stages)                                       # (no destination: frame i on frame set i mod 4, the last one kept)
        assert_matches(r.read_image(premultiplied=True), want[-1])
    finally:
        r.close()


def _random_tree(rng, kids, depth=0):
    out = []
    for k in kids:
        k = dict(k)
        if rng.random() < 0.6:
            k["color_transform"] = G.cxform(mult=tuple(int(v) for v in rng.choice([-256, -100, 0, 77, 128, 256, 256, 300, 700], 4)),
                                            add=tuple(int(v) for v in rng.choice([-300, -40, 0, 0, 0, 30, 255], 4)))
        out.append(k)
    if depth < 2 and len(out) > 1 and rng.random() < 0.7:
        cut = int(rng.integers(1, len(out)))
        inner = {"type": "container", "children": _random_tree(rng, out[cut:], depth + 1)}
        if rng.random() < 0.8:
            inner["color_transform"] = G.cxform(mult=tuple(int(v) for v in rng.choice([0, 128, 256, 512], 4)), add=tuple(int(v) for v in rng.choice([-60, 0, 90], 4)))
        out = out[:cut] + [inner]
    return out


@pytest.mark.gpu
def test_random_transform_trees(gpu):
    import helpers
    rng = np.random.default_rng(2026)
    n = 12 if EMU else 300
    for i in range(n):
        kind = i % 3
        sc = helpers.rand_mixed_scene(rng) if kind == 0 else (helpers.rand_bitmap_scene(rng) if kind == 1 else helpers.rand_radial_scene(rng))
        stage = {"children": _random_tree(rng, sc["stage"]["children"])}
        assert_matches(_product(sc, stage), G.oracle_cxform(sc, stage)), i
