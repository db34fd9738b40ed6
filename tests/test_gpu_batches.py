"""swfr_render_batch with unlike frames in one call.

With a device destination the frames are rendered in groups (SWFR_BATCH_FRAMES) by one launch per kernel and group: the tile
instance, the k2_bin grid, the row kernels and the queued-row passes come from the group's maximum, two groups alternate over two
sets of grow-only buffers.  tests/helpers.py batch_corpus holds one frame of every kind a group can mix (empty, boxes only, solids
only, translucent, bitmaps, gradients, queued rows, tied edges, a crowded comb, a long path, a colour transform, morph shapes); every
ordered pair of kinds shares a group, and every frame of every batch must be its oracle image, bit-exact (the linear gradient: the
frame of its own swfr_render, which is within +-1 LSB of the oracle).  Then the per-frame route, the routes without a destination,
both fill rules and the aliased mode, the test knobs, buffers that shrink and grow between the groups, a 4K batch, and the refusal of
a frame in the middle of a batch (swfr.h: nothing the call queued still runs when it returns).

Also `python tools/emu/run.py tests/test_gpu_batches.py` (fewer pairs and frames; the 4K batch is skipped)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import device_routes as dr  # noqa: E402
import helpers  # noqa: E402
import scenarios  # noqa: E402
from helpers import diff_stats, oracle_render  # noqa: E402
from oracle import cairo_backend as cb, oracle_backend as ob  # noqa: E402

pytestmark = pytest.mark.gpu
EMU = bool(os.environ.get("SWFR_EMULATOR"))
needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")

W, H = helpers.BATCH_W, helpers.BATCH_H
CORPUS = helpers.batch_corpus()
KINDS = list(CORPUS)
LINEAR = {"linear"}                          # the documented +-1 LSB extension against the oracle
SENTINEL = dr.SENTINEL


def _pairs(kinds):
    """frames 2k and 2k + 1 run through every ordered pair of `kinds`"""
    return [k for a in kinds for b in kinds for k in (a, b)]


# the emulator runs a frame in seconds: pairs chosen so that a group's first frame is the lighter one (no chunks, no edges, solid
# styles only) and the other needs more, then the reverse
EMU_PAIRS = ["solid", "bitmaps", "empty", "round_strokes", "boxes", "comb", "bitmaps", "solid", "empty", "tie", "solid", "cxform",
             "boxes", "radial_focal", "long_path", "morph", "translucent", "empty", "linear", "boxes"]
PAIRS = EMU_PAIRS if EMU else _pairs(KINDS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


_WANT = {}


def _scene(kind, mode):
    sc = CORPUS[kind]
    return dict(sc, even_odd=True) if mode == "evenodd" else sc


def _want(kind, mode="nonzero"):
    """the reference image of a corpus frame: the oracle (anti-aliased modes), live libcairo under ANTIALIAS_NONE (aliased mode);
    a colour-transformed frame by way of its lowered stage.  Computed once per module."""
    key = (kind, mode)
    if key not in _WANT:
        import make_aliased_goldens as GA
        import make_cxform_goldens as GC
        sc = _scene(kind, mode)
        if kind == "cxform":
            be = GA.aliased_backend(W, H) if mode == "aliased" else ob.OracleBackend(W, H)
            try:
                _WANT[key] = GC.render_lowered(be, sc, sc["stage"])
            finally:
                be.close()
        else:
            _WANT[key] = GA.cairo_aliased(sc) if mode == "aliased" else oracle_render(sc)
    return _WANT[key]


_SINGLE = {}


def _single(kind, mode):
    """a linear-gradient frame through swfr_render on a fresh handle: within +-1 LSB of the reference, and what every batch route
    must give bit for bit"""
    key = (kind, mode)
    if key not in _SINGLE:
        r = _renderer(mode)
        try:
            r.render(CORPUS[kind]["stage"])
            img = r.read_image(premultiplied=True)
        finally:
            r.close()
        n, mx = diff_stats(img, _want(kind, mode))
        assert mx <= 1, (kind, mode, n, mx)
        _SINGLE[key] = img
    return _SINGLE[key]


def _check(got, kind, mode, where):
    if kind in LINEAR:
        assert (got == _single(kind, mode)).all(), (where, kind)
    else:
        assert diff_stats(got, _want(kind, mode)) == (0, 0), (where, kind)


def _bitmaps():
    seen = {}
    for sc in CORPUS.values():
        for b in sc["bitmaps"]:
            assert seen.setdefault(b["id"], b) is b, "one id, one bitmap"
    return list(seen.values())


def _renderer(mode="nonzero", width=W, height=H, bitmaps=None):
    """a handle of `mode` with every corpus bitmap registered once (the knobs in the environment are read here)"""
    import swf_renderer_amd as S
    r = S.Renderer(width, height, even_odd=mode == "evenodd", antialias="none" if mode == "aliased" else "default")
    for b in (_bitmaps() if bitmaps is None else bitmaps):
        r.add_bitmap(b)
    return r


def _Dest(n, h=H, w=W):
    """n frames of device memory filled with SENTINEL bytes, guard bytes before and behind them (tests/device_routes.py)"""
    return dr.GuardedFrames(n, h, w, offset=0, gap=0)


def _batch(r, kinds, where, mode="nonzero"):
    """render_batch of the corpus frames `kinds` into a device destination; every frame checked"""
    d = _Dest(len(kinds))
    r.render_batch([CORPUS[k]["stage"] for k in kinds], d.ptr, d.stride)
    got = d.guards_intact()
    for i, k in enumerate(kinds):
        _check(got[i], k, mode, (where, i))


def _knobs(monkeypatch, **env):
    for k in ("SWFR_BATCH_FRAMES", "SWFR_FRAMES_IN_FLIGHT", "SWFR_ROWS_WIDE", "SWFR_TILES_SHADERS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


# ---- 1. every kind alone: its reference image, and the kernels it is in the corpus for
def test_every_kind_alone_reaches_its_kernels(monkeypatch):
    _knobs(monkeypatch)
    r = _renderer()
    try:
        for kind in KINDS:
            before = r.stats()
            r.render(CORPUS[kind]["stage"])
            _check(r.read_image(premultiplied=True), kind, "nonzero", "render")
            d = {k: v - before[k] for k, v in r.stats().items()}
            if kind in ("round_strokes", "tie", "comb"):
                assert d["queued_rows"] > 0, (kind, d)
            if kind == "comb":
                assert d["crowded_rows"] > 0, d
            if kind == "tie":
                assert d["tie_rows"] > 0, d
            if kind in ("empty", "boxes", "solid", "bitmaps", "cxform", "long_path"):
                assert d["queued_rows"] == 0, (kind, d)
    finally:
        r.close()


# ---- 2. the grouped route: every ordered pair in one group, groups of 3, the default group size, single frames
@pytest.mark.parametrize("group", [2, 3, None], ids=["B2", "B3", "default"])
def test_grouped_route_mixes_every_pair(group, monkeypatch):
    _knobs(monkeypatch, **({} if group is None else {"SWFR_BATCH_FRAMES": group}))
    seq = PAIRS[:-1] if group == 3 else PAIRS                       # (groups of 3: a short last group)
    assert group != 3 or len(seq) % 3
    r = _renderer()
    try:
        _batch(r, seq, ("batch", group))
        for kind in (KINDS if not EMU else ["round_strokes", "bitmaps"]):
            _batch(r, [kind], ("n=1", group))
    finally:
        r.close()


# ---- 3. the per-frame route into a device destination, over 1, 2 and 4 frame sets
@pytest.mark.parametrize("in_flight", [1, 2, 4])
def test_per_frame_route(in_flight, monkeypatch):
    _knobs(monkeypatch, SWFR_BATCH_FRAMES=1, SWFR_FRAMES_IN_FLIGHT=in_flight)
    r = _renderer()
    try:
        _batch(r, PAIRS if not EMU else PAIRS[:8], ("per-frame", in_flight))
    finally:
        r.close()


# ---- 4. without a destination, render_sequence, render_sequence_readback
def test_routes_without_a_destination(monkeypatch):
    _knobs(monkeypatch)
    lasts = KINDS if not EMU else ["comb", "bitmaps"]
    r = _renderer()
    try:
        for last in lasts:
            seq = [k for k in KINDS if k != last][:3 if EMU else None] + [last]
            stages = [CORPUS[k]["stage"] for k in seq]
            r.render_batch(stages)
            _check(r.read_image(premultiplied=True), last, "nonzero", ("no destination", seq))
            r.render_sequence(stages)
            _check(r.read_image(premultiplied=True), last, "nonzero", ("render_sequence", seq))
        seq = PAIRS if not EMU else PAIRS[:6]
        mid = (H // 2) * W + W // 2
        for premultiplied in (True, False):
            r.render_sequence_readback([CORPUS[k]["stage"] for k in seq], premultiplied=premultiplied, overlap=True)
            want = 0
            for k in seq:
                img = _single(k, "nonzero") if k in LINEAR else _want(k)
                px = img.reshape(-1, 4)[mid].astype(int)
                if not premultiplied and px[3]:                             # (the un-premultiply kernel: round(c * 255 / a))
                    px[0] = (px[0] * 255 + px[3] // 2) // px[3]
                want += int(px[0]) + int(px[3])
            assert r.readback_checksum == want, (premultiplied, r.readback_checksum, want)
    finally:
        r.close()


# ---- 5. the fill rules and the aliased mode; the test knobs that pick other kernel instances
@pytest.mark.parametrize("mode", ["evenodd", pytest.param("aliased", marks=needs_cairo)])
def test_modes(mode, monkeypatch):
    _knobs(monkeypatch, SWFR_BATCH_FRAMES=2)
    r = _renderer(mode)
    try:
        _batch(r, PAIRS, ("mode", mode), mode)
    finally:
        r.close()


@pytest.mark.parametrize("knob", ["SWFR_ROWS_WIDE", "SWFR_TILES_SHADERS"])
def test_knobs(knob, monkeypatch):
    _knobs(monkeypatch, SWFR_BATCH_FRAMES=3, **{knob: 1})
    r = _renderer()
    try:
        _batch(r, PAIRS[::-1], ("knob", knob))
    finally:
        r.close()


# ---- 6. buffers that shrink and grow: group g + 2 reuses group g's work buffer, cleared only when it grows
LIGHT, HEAVY = ["empty", "boxes", "solid"], ["comb", "tie", "round_strokes", "bitmaps", "morph", "radial_focal"]


def _light_heavy(n_groups, B):
    """groups of B frames: light, heavy, heavy, light, light, heavy, ... -- each of the two buffer sets sees small after big after small"""
    seq = []
    for g in range(n_groups):
        pool = HEAVY if (g // 2 + g) % 2 else LIGHT
        seq += [pool[(g * B + k) % len(pool)] for k in range(B)]
    return seq


@pytest.mark.parametrize("group", [2, 3])
def test_buffers_shrink_and_grow_between_groups(group, monkeypatch):
    _knobs(monkeypatch, SWFR_BATCH_FRAMES=group)
    r = _renderer()
    try:
        seq = _light_heavy(6 if EMU else 12, group)
        _batch(r, seq, ("light-heavy", group))
        _batch(r, seq[::-1], ("heavy-light", group))
    finally:
        r.close()


def _reid(sc, base):
    """the scene with its bitmaps under ids base, base + 1, ... (its bitmap fills renamed alike)"""
    ids = {b["id"]: base + i for i, b in enumerate(sc["bitmaps"])}

    def walk(v):
        if isinstance(v, list):
            return [walk(x) for x in v]
        if not isinstance(v, dict):
            return v
        d = {k: walk(x) for k, x in v.items()}
        if d.get("type") == "bitmap":
            d["bitmap_id"] = ids[d["bitmap_id"]]
        return d
    return dict(sc, stage=walk(sc["stage"]), bitmaps=[dict(b, id=ids[b["id"]]) for b in sc["bitmaps"]])


def test_dense_4k_frames_in_groups_of_two(monkeypatch):
    """Six dense 3840x2160 frames (each with bitmaps of its own) and two light ones in groups of two: four groups, so that each buffer
    set is reused, and frames above T3_PAIR_FROM strips (the paired tile launch)."""
    if EMU:
        pytest.skip("4K frames: minutes on the emulator")
    _knobs(monkeypatch, SWFR_BATCH_FRAMES=2)
    rng = np.random.default_rng(5150)
    dense = [_reid(helpers.rand_dense_scene(rng, width=3840, height=2160, shapes=40), 100 + 2 * i) for i in range(6)]
    light = dict(CORPUS["solid"], width=3840, height=2160), dict(width=3840, height=2160, stage={"children": []}, bitmaps=[])
    frames = [dense[0], dense[1], light[0], dense[2], dense[3], dense[4], light[1], dense[5]]
    r = _renderer(width=3840, height=2160, bitmaps=[b for sc in dense for b in sc["bitmaps"]])
    try:
        d = _Dest(len(frames), 2160, 3840)
        r.render_batch([sc["stage"] for sc in frames], d.ptr, d.stride)
        got = d.guards_intact()
    finally:
        r.close()
    for i, sc in enumerate(frames):
        assert diff_stats(got[i], oracle_render(sc)) == (0, 0), i


# ---- 7. a refused frame in the middle of a batch
def _refused(what):
    """(stage, error code) of a frame the frame builder refuses"""
    from swf_renderer_amd import api
    sq = [(200, 200), (2600, 300), (2400, 2000), (300, 1800)]
    if what == "unknown_shape":
        return {"children": [{"type": "shape", "id": 999999}]}, api.ERR_NOT_FOUND
    if what == "unregistered_bitmap":
        fill = {"type": "bitmap", "bitmap_id": 77, "repeating": True, "smoothed": True, "matrix": scenarios._m(20, 20)}
        return {"children": [{"type": "shape", "definition": scenarios._poly_shape(sq, fill)}]}, api.ERR_NOT_FOUND
    if what == "17_stops":
        fill = {"type": "radial-gradient", "matrix": scenarios._m(0.1, 0.1, 1400, 1100),
                "gradient": scenarios._grad([(15 * k, (10 * k, 255 - 10 * k, 40, 255)) for k in range(17)])}
        return {"children": [{"type": "shape", "definition": scenarios._poly_shape(sq, fill)}]}, api.ERR_CAPACITY
    assert what == "gradient_line"
    grad = {"type": "linear-gradient", "matrix": scenarios._m(0.1, 0.1, 1400, 1100), "gradient": scenarios._grad([(0, (255, 0, 0)), (255, (0, 0, 255))])}
    tag = scenarios._poly_shape(sq, {"type": "solid", "color": scenarios._rgba(9, 9, 9)}, line=scenarios._rgba(0, 0, 0), line_width=60)
    tag["shape"]["initial_styles"]["line"][0]["fill"] = grad
    return {"children": [{"type": "shape", "definition": tag}]}, api.ERR_NOT_IMPLEMENTED


REFUSALS = ["unknown_shape", "unregistered_bitmap", "17_stops", "gradient_line"]
# the frames around the refused one: queued rows, bitmaps, crowded rows, so that the groups before it are still running
VALID = ["round_strokes", "bitmaps", "comb", "solid", "tie", "boxes", "morph", "cxform", "translucent", "radial_focal"]


@pytest.mark.parametrize("route", ["grouped", "per_frame"])
@pytest.mark.parametrize("what", REFUSALS)
def test_refused_frame_ends_the_batch_after_its_work(what, route, monkeypatch):
    """The call returns the refused frame's code only after everything it queued has finished: read straight after the call, with no
    synchronisation, every slot is its frame or untouched; the frames of the groups before the refused frame's group are complete and
    nothing from that group on is written.  The handle then renders a batch and a frame correctly."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    B = 3
    _knobs(monkeypatch, **({"SWFR_BATCH_FRAMES": B} if route == "grouped" else {"SWFR_BATCH_FRAMES": 1, "SWFR_FRAMES_IN_FLIGHT": 4}))
    bad, code = _refused(what)
    n = 7 if EMU else len(VALID)
    positions = [0, 1, B, n - 1] if not EMU else ([B] if what != "unknown_shape" else [0, 1, B, n - 1])
    r = _renderer()
    try:
        for pos in positions:
            kinds = [VALID[i % len(VALID)] for i in range(n)]
            stages = [CORPUS[k]["stage"] for k in kinds]
            stages[pos] = bad
            d = _Dest(n)
            with pytest.raises(S.SwfrError) as e:
                r.render_batch(stages, d.ptr, d.stride)
            got = d.raw()                                               # (no synchronisation: the call itself must have waited)
            assert e.value.code == code, (pos, str(e.value))
            first_unwritten = (pos // B) * B if route == "grouped" else pos
            for i, k in enumerate(kinds):
                if i < first_unwritten:
                    _check(got[i], k, "nonzero", (what, route, pos, i))
                else:
                    assert (got[i] == SENTINEL).all(), (what, route, pos, i)
            d.guards_intact()
            with pytest.raises(S.SwfrError) as e:
                r.read_image(premultiplied=True)
            assert e.value.code == api.ERR_INVALID
            # the handle afterwards: a batch (the refused slot now a valid frame) and a frame
            kinds[pos] = "boxes"
            _batch(r, kinds, (what, route, pos, "after"))
            r.render(CORPUS["tie"]["stage"])
            _check(r.read_image(premultiplied=True), "tie", "nonzero", (what, route, pos, "render after"))
        # the route without a destination refuses alike, and leaves no image behind
        with pytest.raises(S.SwfrError) as e:
            r.render_batch([CORPUS["comb"]["stage"], CORPUS["round_strokes"]["stage"], bad, CORPUS["solid"]["stage"]])
        assert e.value.code == code
        with pytest.raises(S.SwfrError) as e:
            r.read_image(premultiplied=True)
        assert e.value.code == api.ERR_INVALID
        r.render(CORPUS["bitmaps"]["stage"])
        _check(r.read_image(premultiplied=True), "bitmaps", "nonzero", (what, "no destination", "render after"))
    finally:
        r.close()
