"""What the device tests of the compositing and filter features share (tests/test_{blend,layer,mask,fade}_gpu.py,
tests/test_composite_fuzz_gpu.py, tests/test_{blur,shadow,inner,filters,convolution}_gpu.py): handles, the routes a frame can take to
the device, the comparisons, every libcairo golden of a compositing family through every route, and what the filter families' tests
have in common ("the filter families", below).

A family is one row of FAMILIES: its scenes module (files(), golden_path(), LINEAR_BOUND), the SWFR_TILES_SHADERS value of its
k2_tiles instance, and what differs between the families' golden runs.  A new compositing feature adds a scenes module and a row.

The routes of a golden file, by their number (under the emulator, where a frame takes seconds, a route takes every fourth scene of a
file, the offset moving with the number so that the routes together still see most scenes): 0 swfr_build_frame on a host-only handle
and swfr_render_edges on another, then resident frames; 1 the same under SWFR_GRAPHS=1; 2 two band handles; 3 render_batch with
unlike frames; 4 render; 5 render with the family's instance forced.

Every comparison prints a line ending in "differing pixels N max M"; after every frame the handle's swfr_stats show no capacity
refusal.  Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import hashlib
import json
import os
from collections import namedtuple

import numpy as np
import pytest

import blend_scenes
import blur_scenes
import convolution_scenes
import fade_scenes
import filter_scenes
import frame_model
import helpers
import inner_scenes
import layer_scenes
import mask_scenes
import scenarios
import shadow_model
import shadow_scenes
from helpers import diff_stats, oracle_render
from host_frames import build_on_host

EMU = bool(os.environ.get("SWFR_EMULATOR"))
REFUSALS = ("pairtest_limit", "start_group_limit", "history_limit")

# forced_render: the goldens go through render with the instance forced too (under the emulator both runs then take every fourth scene,
# routes 4 and 5; blend and layer render every scene, and have the through_instance_N tests of their own files instead)
# layouts: the band layouts of route 2 (contiguous_bands of swfr_create)
Family = namedtuple("Family", "name scenes instance forced_render layouts")
FAMILIES = {f.name: f for f in (Family("blend", blend_scenes, "3", False, (True,)), Family("layer", layer_scenes, "4", False, (True, False)),
                                Family("mask", mask_scenes, "5", True, (True, False)), Family("fade", fade_scenes, "6", True, (True, False)),
                                # the filter families: the instance is the layers' (a filtered layer is composited as one bitmap path),
                                # never forced; no band layouts (filtered layers are refused on band handles)
                                Family("blur", blur_scenes, "4", False, ()), Family("shadow", shadow_scenes, "4", False, ()),
                                Family("inner", inner_scenes, "4", False, ()), Family("filters", filter_scenes, "4", False, ()),
                                Family("convolution", convolution_scenes, "4", False, ()))}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(gpu):
    """(imported by a device test module: its tests need a GPU and the built library)"""
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


# ---------------------------------------------------------------------------------------------------------------- comparisons
def check(family, got, want, sc, msg):
    """exact unless the scene says otherwise (a linear gradient: the family's LINEAR_BOUND)"""
    n, mx = diff_stats(got, want)
    print(family.name, msg, "differing pixels", n, "max", mx)
    if sc["exact"]:
        assert (n, mx) == (0, 0), msg
    else:
        assert mx <= family.scenes.LINEAR_BOUND, (msg, n, mx)


def zero(got, want, msg):
    n, mx = diff_stats(got, want)
    print("composite", msg, "differing pixels", n, "max", mx)
    assert (n, mx) == (0, 0), msg


def not_refused(r, msg):
    st = r.stats()
    assert st["frames"] >= 1 and all(st[k] == 0 for k in REFUSALS), (msg, st)


# ---------------------------------------------------------------------------------------------------------------- handles and routes
def handle(W, H, aliased=False, bitmaps=None, **kw):
    """bitmaps: {id: (width, height, straight RGBA bytes)} registered on the handle (a RawFrame's, a scene's "raw_bitmaps")"""
    import swf_renderer_amd as S
    r = S.Renderer(W, H, antialias="none" if aliased else "default", **kw)
    for bid, (w, h, px) in (bitmaps or {}).items():
        r.register_bitmap(bid, w, h, px)
    return r


def renderer_for(sc, aliased, **kw):
    """a handle of the scene's size and fill rule that holds the scene's bitmaps"""
    r = handle(sc["width"], sc["height"], aliased, bitmaps=sc.get("raw_bitmaps"), even_odd=bool(sc.get("even_odd")), **kw)
    for b in sc.get("bitmaps", []):
        r.add_bitmap(b)
    return r


def through_edges(W, H, arrays, aliased=False, resident=0, bitmaps=None, **kw):
    r = handle(W, H, aliased, bitmaps, **kw)
    try:
        r.render_edges(*arrays)
        img = r.read_image(premultiplied=True)
        if resident:
            r.render_resident(resident)
            assert (r.read_image(premultiplied=True) == img).all(), "resident frames differ from the first"
        not_refused(r, "render_edges")
        return img
    finally:
        r.close()


def through_render(sc, aliased=False, **kw):
    r = handle(sc["width"], sc["height"], aliased, sc.get("raw_bitmaps"), **kw)
    try:
        r.render(sc["stage"])
        not_refused(r, "render")
        return r.read_image(premultiplied=True)
    finally:
        r.close()


def two_bands(W, H, contiguous, draw, aliased=False, make=None, bitmaps=None):
    """the frame assembled from two handles, each drawing its own tile rows (`draw(handle)`; `make(**bands)`: the handle; `bitmaps`:
    registered on both)"""
    out = np.zeros((H, W, 4), np.uint8)
    n = -(-((H + 15) // 16) // 2)                                    # tile rows per handle
    for rank in range(2):
        bands = dict(band_index=rank, band_count=2, contiguous_bands=contiguous)
        r = make(**bands) if make else handle(W, H, aliased, bitmaps, **bands)
        try:
            draw(r)
            img = r.read_image(premultiplied=True)
            not_refused(r, "bands")
        finally:
            r.close()
        t = np.arange(H) // 16
        rows = ((t >= rank * n) & (t < (rank + 1) * n)) if contiguous else (t % 2 == rank)
        out[rows] = img[rows]
    return out


# ---------------------------------------------------------------------------------------------------------------- caller-owned frames
SENTINEL = 0xA5


class GuardedFrames:
    """n frames of h x w RGBA8 words in ONE allocation of device memory (a torch tensor; under the emulator, whose device memory is
    host memory, numpy) filled with SENTINEL bytes: frame i starts at base + pad + offset + i * (h * w * 4 + gap), where `base` is
    picked from the allocation's real address so that frame 0's address is `offset` modulo 16 -- `offset` 4, 8 or 12: a target that is
    word aligned only; 1, 2, 3: one no kernel may be given.  Every byte of the allocation outside the frames is a guard: the front pad,
    the gaps, the back pad.  The frames start as SENTINEL bytes too: a frame with clear pixels that equals its expected picture has
    had every pixel written.  All of it lies inside the one allocation: a store that strays by less than `pad` bytes is seen and
    harms nothing."""

    def __init__(self, n, h, w, offset=0, gap=0, pad=256):
        assert n >= 1 and 0 <= offset < 16 and gap >= 0 and pad >= 16
        self.n, self.h, self.w, self.offset, self.gap = n, h, w, offset, gap
        self.frame_bytes = h * w * 4
        self.stride = self.frame_bytes + gap
        size = 16 + pad + offset + (n - 1) * self.stride + self.frame_bytes + pad
        if EMU:
            self.a = np.full(size, SENTINEL, np.uint8)
            address = self.a.ctypes.data
        else:
            import torch
            self.t = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            address = self.t.data_ptr()
        self.first = (-(address + pad)) % 16 + pad + offset          # frame 0's place in the allocation
        self.ptr = address + self.first
        assert self.ptr % 16 == offset and self.first >= pad and self.first + (n - 1) * self.stride + self.frame_bytes + pad <= size

    def address(self, i):
        assert 0 <= i < self.n
        return self.ptr + i * self.stride

    def addresses(self):
        return [self.address(i) for i in range(self.n)]

    def _bytes(self, wait):
        if EMU:
            return self.a.copy()
        if wait:
            import torch
            torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def _frames_of(self, b):
        if self.gap == 0:
            return b[self.first:self.first + self.n * self.frame_bytes].reshape(self.n, self.h, self.w, 4)
        return np.stack([b[self.first + i * self.stride:][:self.frame_bytes].reshape(self.h, self.w, 4) for i in range(self.n)])

    def raw(self):
        """the n frames as they are, without waiting for anything"""
        return self._frames_of(self._bytes(False))

    def frames(self):
        """the n frames, [n, h, w, 4], once the device is idle"""
        return self._frames_of(self._bytes(True))

    def guards_intact(self):
        """every byte outside the frames is still SENTINEL; returns the frames (read in the same copy)"""
        b = self._bytes(True)
        at = 0
        for i in range(self.n + 1):
            end = self.first + i * self.stride if i < self.n else len(b)
            bad = np.flatnonzero(b[at:end] != SENTINEL)
            assert bad.size == 0, "guard bytes %d..%d overwritten (%d of them; frame %d begins at byte %d)" % (
                at + bad[0], at + bad[-1], bad.size, min(i, self.n - 1), self.first + min(i, self.n - 1) * self.stride)
            at = end + self.frame_bytes
        return self._frames_of(b)

    def refill(self):
        if EMU:
            self.a[:] = SENTINEL
        else:
            import torch
            torch.cuda.synchronize()
            self.t.fill_(SENTINEL)
            torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the goldens
def golden_scenes(family, fname, route, thin=True):
    """([(name, scene)], aliased, the golden file) of one route"""
    make, aliased = family.scenes.files()[fname]
    items = sorted(make().items())
    gold = np.load(family.scenes.golden_path(fname))
    if EMU and thin:
        items = items[route % 4::4]
    else:
        assert [n for n, _ in items] == sorted(gold.files)
    return items, aliased, gold


def built_for_another_handle(sc, aliased):
    """swfr_build_frame's arrays for the scene.  They must not name colour-transformed textures: those belong to the handle that walked
    the stage, so such a frame could not be handed to another handle (a cxform_* scene with a bitmap -- there is none today)"""
    from swf_renderer_amd import api
    e, p, s = build_on_host(sc, aliased)
    assert not any(st.kind == api.STYLE_BITMAP and st.bitmap >= api.VARIANT_BASE for st in s)
    return e, p, s


def goldens_through_render(family, fname, monkeypatch, forced=False):
    if forced:
        monkeypatch.setenv("SWFR_TILES_SHADERS", family.instance)
    else:
        monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    assert family.forced_render or not forced
    items, aliased, gold = golden_scenes(family, fname, 4 + forced, thin=family.forced_render)
    for name, sc in items:
        r = renderer_for(sc, aliased)
        try:
            r.render(sc["stage"])
            check(family, r.read_image(premultiplied=True), gold[name], sc, (fname, name, forced))
            not_refused(r, name)
        finally:
            r.close()


def goldens_through_render_edges(family, fname):
    """swfr_build_frame on one handle, swfr_render_edges on another: operators, fades and groups travel in the paths"""
    items, aliased, gold = golden_scenes(family, fname, 0)
    for name, sc in items:
        e, p, s = built_for_another_handle(sc, aliased)
        r = renderer_for(sc, aliased)
        try:
            r.render_edges(e, p, s)
            check(family, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "render_edges"))
            r.render_resident(3)
            check(family, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "resident"))
            not_refused(r, name)
        finally:
            r.close()


def goldens_with_graphs(family, fname, monkeypatch):
    monkeypatch.setenv("SWFR_GRAPHS", "1")
    items, aliased, gold = golden_scenes(family, fname, 1)
    for name, sc in items:
        e, p, s = built_for_another_handle(sc, aliased)
        r = renderer_for(sc, aliased)
        try:
            r.upload_edges(e, p, s)
            r.render_resident(3)
            check(family, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "graphs"))
        finally:
            r.close()


def goldens_through_two_band_handles(family, fname, contiguous):
    assert contiguous in family.layouts
    items, aliased, gold = golden_scenes(family, fname, 2)
    for name, sc in items:
        out = two_bands(sc["width"], sc["height"], contiguous, lambda r: r.render(sc["stage"]), make=lambda **kw: renderer_for(sc, aliased, **kw))
        check(family, out, gold[name], sc, (fname, name, "bands", contiguous))


def goldens_through_render_batch_with_unlike_frames(family, fname):
    """The file's scenes of one frame size as ONE batch, a plain frame (no group, no blended path: no operator table) after every third
    of them: composited and plain frames, solid, bitmap and gradient frames in one group, so in one launch of the family's instance.
    Into a device tensor where there is a device for it (every frame checked), and by the per-frame route (the last frame is what stays).
    The plain frame is held against the oracle; aliased, where there is no oracle, against tests/frame_model.py -- the exact model of
    the aliased rule over the frame builder's arrays; the other frames against libcairo."""
    items, aliased, gold = golden_scenes(family, fname, 3)
    for w, h in sorted({(sc["width"], sc["height"]) for _, sc in items}):
        group = [(name, sc) for name, sc in items if (sc["width"], sc["height"]) == (w, h)]
        plain = dict(width=w, height=h, exact=True, stage={"children": blend_scenes._with_ground(dict(width=w, height=h))})
        plain_want = frame_model.render(*built_for_another_handle(plain, True), w, h, aliased=True) if aliased else oracle_render(plain)
        frames = []                                                  # (message, scenario, expected pixels)
        for k, (name, sc) in enumerate(group):
            frames.append((name, sc, gold[name]))
            if k % 3 == 0:
                frames.append(("plain", plain, plain_want))
        r = handle(w, h, aliased)
        try:
            seen = set()
            for _, sc, _ in frames:
                for b in sc.get("bitmaps", []):
                    if b["id"] not in seen:
                        seen.add(b["id"])
                        r.add_bitmap(b)
            stages = [sc["stage"] for _, sc, _ in frames]
            if not EMU:                                              # (device tensors need the GPU)
                import torch
                out = torch.zeros((len(stages), h, w, 4), dtype=torch.uint8, device="cuda")
                r.render_batch(stages, out.data_ptr(), h * w * 4)
                got = out.cpu().numpy()
                for k, (name, sc, want) in enumerate(frames):
                    check(family, got[k], want, sc, (fname, name, "batch", k))
            for cut in sorted({1, 2, len(frames) // 2, len(frames)}):
                if 0 < cut <= len(frames):
                    r.render_batch(stages[:cut])
                    name, sc, want = frames[cut - 1]
                    check(family, r.read_image(premultiplied=True), want, sc, (fname, name, "per-frame route", cut))
            not_refused(r, fname)
        finally:
            r.close()


# ---------------------------------------------------------------------------------------------------------------- the corpus through an instance
def force_instance(monkeypatch, family, rows="narrow"):
    monkeypatch.setenv("SWFR_TILES_SHADERS", family.instance)
    if rows == "wide":
        monkeypatch.setenv("SWFR_ROWS_WIDE", "1")
    else:
        monkeypatch.delenv("SWFR_ROWS_WIDE", raising=False)


def scenario_through_instance(family, sc, name, rows, monkeypatch):
    """byte-identical to what the instance picked for the scenario gives, and its libcairo golden"""
    from helpers import golden, product_render
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    base = product_render(sc)
    force_instance(monkeypatch, family, rows)
    got = product_render(sc)
    assert diff_stats(got, base) == (0, 0), name
    n, mx = diff_stats(got, golden("cairo_" + name, "rgba_premul"))
    assert ((n, mx) == (0, 0)) if sc["exact"] else mx <= 1, (name, n, mx)


def aliased_scenarios_through_instance(family, scenarios, monkeypatch):
    from helpers import golden, product_render
    force_instance(monkeypatch, family)
    for name, sc in sorted(scenarios.items()):
        n, mx = diff_stats(product_render(sc, antialias="none"), golden("cairo_aliased_" + name, "rgba_premul"))
        assert ((n, mx) == (0, 0)) if sc["exact"] else mx <= 1, (name, n, mx)


def structural_scenes_through_instance(family, rows, monkeypatch):
    """the tests/helpers.py scenes that tests/test_gpu_instances.py runs per instance"""
    from helpers import product_render
    force_instance(monkeypatch, family, rows)
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
        r = handle(W, H)
        try:
            r.render_edges(*scene)
            assert diff_stats(r.read_image(premultiplied=True), helpers.oracle_polys(fx, cols, W, H)) == (0, 0)
        finally:
            r.close()


def s1_4k_known_answer_through_instance(family, monkeypatch):
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    from swf_renderer_amd import synth
    force_instance(monkeypatch, family)
    W, H, _, _, scene = helpers.synth_scene(synth.S1)
    r = handle(W, H)
    try:
        r.render_edges(*scene)
        assert hashlib.sha256(r.read_image(premultiplied=True).tobytes()).hexdigest() == synth.S1_SHA256_PREMUL
        r.render_resident(3)                                         # (overlapped frames: the tile pass in its paired launch shape)
        assert hashlib.sha256(r.read_image(premultiplied=True).tobytes()).hexdigest() == synth.S1_SHA256_PREMUL
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- the filter families
# What tests/test_{blur,shadow,inner,filters,convolution}_gpu.py share: a filtered layer is rendered as a sub-frame and composited as
# one bitmap path, so its goldens take render and the resident parent frame, and every other route refuses it by name.
#
# The image sizes at which the passes can go wrong.  blur.hip: the horizontal pass works on 1024 x 4 pixels a workgroup, the vertical
# one on 256 x 64 -- 2100 x 150 spans three segments of both on both axes and is a multiple of none.  shadow.hip: a lane takes four
# words -- 257 x 3 and 3 x 257 leave one and three words behind the groups of four and put a row's end inside a group; 2048 workgroups
# of 256 lanes stride over the image, 2 097 152 words a stride -- 2051 x 1029 is 2 110 479 words: both kernels' loops over groups of
# four run a second, partial time (3 331 groups), and three words are left for the word loop (which takes more than three only in a
# buffer that is not 16-byte aligned: none of the handle's own is).  On the emulator 2051 x 1029 is a matter of minutes and left out
SIZES = ((13, 11), (257, 3), (3, 257), (2100, 150))
LOOPS_TWICE = (2051, 1029)
SIZES_AND_LOOPS_TWICE = SIZES + (() if EMU else (LOOPS_TWICE,))


def content(w, h):
    """translucent and opaque shapes all over a w x h frame, some across its edges, clear pixels between them"""
    rng = np.random.default_rng(w * 1000 + h)
    kids = []
    for i in range(16):
        cx, cy = rng.uniform(-0.1, 1.1) * w, rng.uniform(-0.1, 1.1) * h
        pts = [(cx + rng.uniform(-0.25, 0.25) * w, cy + rng.uniform(-0.5, 0.5) * h) for _ in range(3)]
        a = 255 if i % 5 == 0 else int(rng.integers(30, 250))
        kids.append(blur_scenes._shape(pts, (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), a)))
    kids.append(blur_scenes._rect(0, 0, 1, h / 2, (255, 255, 255, 255)))       # opaque white against the left edge
    return kids


def whole_frame_bitmap(w, h, bitmap_id):
    """the bitmap drawn 1:1 over a w x h frame with a nearest fill: the frame is the bitmap's texels"""
    fill = {"type": "bitmap", "bitmap_id": bitmap_id, "repeating": False, "smoothed": False, "filter": "nearest",
            "matrix": scenarios._m(20, 20, 0, 0)}
    return {"type": "shape", "definition": scenarios._poly_shape([(0, 0), (w * 20, 0), (w * 20, h * 20), (0, h * 20)], fill)}


def goldens_through_render_and_resident(family, fname):
    """every scene of a libcairo + pixman golden file through render, zero differing bytes; the textures stay: the resident parent
    frame renders again to the same pixels"""
    items, aliased, gold = golden_scenes(family, fname, 4, thin=False)
    for name, sc in items:
        r = renderer_for(sc, aliased)
        try:
            r.render(sc["stage"])
            not_refused(r, name)
            zero(r.read_image(premultiplied=True), gold[name], (family.name, fname, name, "render"))
            r.render_resident(1)
            zero(r.read_image(premultiplied=True), gold[name], (family.name, fname, name, "resident"))
        finally:
            r.close()


def alpha_and_erase(family, golden_file, clear_name, opaque_name):
    """On a flagged handle the filtered surface is the source of DEST_OUT / DEST_IN (ERASE is the path's operator; ALPHA, a group's
    operator only, puts the path in a group of its own): against the frame model of the composite -- the surface from the goldens'
    normal scene over clear, where the frame IS that surface, applied to the ground of the scene over opaque"""
    final = np.load(family.scenes.golden_path(golden_file))[clear_name].astype(np.int64)
    sc = family.scenes.operator_scenes()[opaque_name]
    ground = through_render(dict(sc, stage={"children": sc["stage"]["children"][:-1]})).astype(np.int64)
    for mode, factor in (("erase", 255 - final[..., 3:]), ("alpha", final[..., 3:])):
        want = shadow_model.mul_un8(ground, factor).astype(np.uint8)
        assert (want != ground).any()
        kids = sc["stage"]["children"][:-1] + [dict(sc["stage"]["children"][-1], layer=mode)]
        zero(through_render(dict(sc, stage={"children": kids}), alpha_modes=True), want, (family.name, mode))


def refused_routes(family, sc, plain, want, want_plain):
    """the routes that do not draw filtered layers refuse `sc` by name, and the handle renders `plain` (sc without its filters)
    correctly afterwards; want, want_plain: the two frames"""
    from swf_renderer_amd import api
    r = renderer_for(sc, False)
    try:
        def refused(call, code, name):
            with pytest.raises(api.SwfrError) as e:
                call()
            assert e.value.code == code and name in str(e.value), (code, name, str(e.value))
            r.render(plain["stage"])
            zero(r.read_image(premultiplied=True), want_plain, (family.name, name, "the plain frame afterwards"))
        refused(lambda: r.render_batch([plain["stage"], sc["stage"], plain["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        refused(lambda: r.render_sequence([plain["stage"], sc["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        refused(lambda: r.render_sequence_readback([sc["stage"]]), api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        if not EMU:
            import torch
            dst = torch.zeros((3, sc["height"], sc["width"], 4), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            refused(lambda: r.render_batch([plain["stage"], sc["stage"], plain["stage"]], dst.data_ptr(), dst.stride(0)),
                    api.ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute")
        # the layer's texture named in a caller's scene: not found -- also right behind a render that made one
        r.render(sc["stage"])
        zero(r.read_image(premultiplied=True), want, (family.name, "render"))
        edges, paths, styles = r.build_frame(sc["stage"])
        assert any(s.kind == api.STYLE_BITMAP and s.bitmap == api.BLUR_BASE for s in styles)
        refused(lambda: r.upload_edges(edges, paths, styles), api.ERR_NOT_FOUND, "BitmapNotFound")
        r.render(sc["stage"])
        zero(r.read_image(premultiplied=True), want, (family.name, "render again"))
    finally:
        r.close()
    for contiguous in (False, True):
        b = renderer_for(sc, False, band_index=0, band_count=2, contiguous_bands=contiguous)
        try:
            with pytest.raises(api.SwfrError) as e:
                b.render(sc["stage"])
            assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedBlurBands" in str(e.value)
            b.render(plain["stage"])
        finally:
            b.close()


def plain_frame_after(family, names, golden_file):
    """a frame without filters behind a filtered one (the scenes `names` of the golden file) is the frame a fresh handle renders, also
    as resident frames; and the other way round: the filtered frame behind the plain one, then resident, is its golden"""
    scenes = family.scenes.files()[golden_file][0]()
    plain_sc = layer_scenes.overlap_scenes()["multiply_translucent"]
    assert (plain_sc["width"], plain_sc["height"]) == (family.scenes.W, family.scenes.H)
    fresh = through_render(plain_sc)
    gold = np.load(family.scenes.golden_path(golden_file))
    r = renderer_for(plain_sc, False)
    try:
        for name in names:
            r.render(scenes[name]["stage"])
            r.render(plain_sc["stage"])
            zero(r.read_image(premultiplied=True), fresh, (family.name, name))
            r.render_resident(3)
            zero(r.read_image(premultiplied=True), fresh, (family.name, name, "resident"))
            r.render(scenes[name]["stage"])
            r.render_resident(2)
            zero(r.read_image(premultiplied=True), gold[name], (family.name, name, "behind the plain one"))
    finally:
        r.close()


def s1_4k_crops(family, fname, aliased=False):
    """the family's S1 frame at 4K against its committed crops and the hash of the whole frame"""
    if EMU:
        pytest.skip("a 4K frame: minutes on the emulator")
    sc = family.scenes.s1_stage()
    gold = np.load(family.scenes.golden_path(fname))
    img = helpers.product_render(sc, **({"antialias": "none"} if aliased else {}))
    for key in gold.files:
        if key == "sha256":
            continue
        x, y = map(int, key.split("_"))
        assert (img[y:y + 256, x:x + 256] == gold[key]).all(), key
    assert hashlib.sha256(img.tobytes()).digest() == gold["sha256"].tobytes()
