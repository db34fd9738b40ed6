"""The erase and alpha modes on the device (k2_tiles<7>: the fade instance plus the two combiners and the ALPHA END of a strip its
group never reached), on handles created with alpha_modes=True.  Every comparison is zero differing bytes.

a. Every libcairo golden of tests/alpha_modes_scenes.py through render, swfr_build_frame + swfr_render_edges (+ resident frames),
   SWFR_GRAPHS=1, two band handles (contiguous and interleaved) and render_batch with plain frames in the same group.
b. Raw frames of 128 x 32 (tests/alpha_modes_raw.py) against tests/alpha_modes_model.py, each aimed at one branch of the walk;
   test_the_raw_corpus_reaches_what_it_claims computes from the arrays what the strips of these frames see and asserts it.
c. Random display trees (alpha_modes_scenes.rand_alpha_mode_scene) through render and render_batch, both antialias modes, against
   the model over the host's own swfr_build_frame arrays; frames the host refuses for capacity are skipped, at most 5 % of them.

Observed on an MI355X: 83 passed, every comparison 0 differing bytes, 6 s.  Runs there (-m gpu) and, with smaller counts, under
tools/emu/run.py.
"""
import numpy as np
import pytest

import alpha_modes_model as am
import alpha_modes_raw as ar
import alpha_modes_scenes as scenes
import blend_scenes
import composite_scenes as cs
import frame_model
import host_frames as hf
from device_routes import EMU, handle, not_refused, two_bands, zero
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import oracle_render

pytestmark = pytest.mark.gpu
FILES = sorted(scenes.files())
FLAG = dict(alpha_modes=True)


def _handle(sc, aliased, **kw):
    r = handle(sc["width"], sc["height"], aliased, bitmaps=sc.get("raw_bitmaps"), even_odd=bool(sc.get("even_odd")), **FLAG, **kw)
    for b in sc.get("bitmaps", []):
        r.add_bitmap(b)
    return r


_built = scenes.build_flagged


def _items(fname, route):
    make, aliased = scenes.files()[fname]
    items = sorted(make().items())
    gold = np.load(scenes.golden_path(fname))
    assert [n for n, _ in items] == sorted(gold.files)
    return (items[route % 4::4] if EMU else items), aliased, gold


# ---------------------------------------------------------------------------------------------------------------- a. the goldens
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render(fname):
    items, aliased, gold = _items(fname, 0)
    for name, sc in items:
        r = _handle(sc, aliased)
        try:
            r.render(sc["stage"])
            zero(r.read_image(premultiplied=True), gold[name], (fname, name, "render"))
            not_refused(r, name)
        finally:
            r.close()


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_edges_and_resident_frames(fname):
    items, aliased, gold = _items(fname, 1)
    for name, sc in items:
        e, p, s = _built(sc, aliased)
        r = _handle(sc, aliased)
        try:
            r.render_edges(e, p, s)
            zero(r.read_image(premultiplied=True), gold[name], (fname, name, "render_edges"))
            r.render_resident(3)
            zero(r.read_image(premultiplied=True), gold[name], (fname, name, "resident"))
            not_refused(r, name)
        finally:
            r.close()


@pytest.mark.parametrize("fname", FILES)
def test_goldens_with_graphs(fname, monkeypatch):
    monkeypatch.setenv("SWFR_GRAPHS", "1")
    items, aliased, gold = _items(fname, 2)
    for name, sc in items:
        e, p, s = _built(sc, aliased)
        r = _handle(sc, aliased)
        try:
            r.upload_edges(e, p, s)
            r.render_resident(3)
            zero(r.read_image(premultiplied=True), gold[name], (fname, name, "graphs"))
        finally:
            r.close()


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_two_band_handles(fname, contiguous):
    items, aliased, gold = _items(fname, 3)
    for name, sc in items:
        out = two_bands(sc["width"], sc["height"], contiguous, lambda r: r.render(sc["stage"]), make=lambda **kw: _handle(sc, aliased, **kw))
        zero(out, gold[name], (fname, name, "bands", contiguous))


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_batch_with_unlike_frames(fname):
    """the file's scenes of one frame size as ONE batch, a plain frame (no operator table) after every third: frames with the new
    operators and frames without them in one group, so in one launch of instance 7 (the plan takes the group's highest instance)"""
    items, aliased, gold = _items(fname, 0)
    for w, h in sorted({(sc["width"], sc["height"]) for _, sc in items}):
        group = [(name, sc) for name, sc in items if (sc["width"], sc["height"]) == (w, h)]
        plain = dict(width=w, height=h, exact=True, stage={"children": blend_scenes._with_ground(dict(width=w, height=h))})
        plain_want = frame_model.render(*hf.build_on_host(plain, True), w, h, aliased=True) if aliased else oracle_render(plain)
        frames = []
        for k, (name, sc) in enumerate(group):
            frames.append((name, sc, gold[name]))
            if k % 3 == 0:
                frames.append(("plain", plain, plain_want))
        r = handle(w, h, aliased, **FLAG)
        try:
            seen = set()
            for _, sc, _ in frames:
                for b in sc.get("bitmaps", []):
                    if b["id"] not in seen:
                        seen.add(b["id"])
                        r.add_bitmap(b)
            stages = [sc["stage"] for _, sc, _ in frames]
            if not EMU:
                import torch
                out = torch.zeros((len(stages), h, w, 4), dtype=torch.uint8, device="cuda")
                r.render_batch(stages, out.data_ptr(), h * w * 4)
                got = out.cpu().numpy()
                for k, (name, sc, want) in enumerate(frames):
                    zero(got[k], want, (fname, name, "batch", k))
            for cut in sorted({1, 2, len(frames) // 2, len(frames)}):
                if 0 < cut <= len(frames):
                    r.render_batch(stages[:cut])
                    zero(r.read_image(premultiplied=True), frames[cut - 1][2], (fname, frames[cut - 1][0], "per-frame route", cut))
            not_refused(r, fname)
        finally:
            r.close()


# ---------------------------------------------------------------------------------------------------------------- b. raw frames
def _through(fr, arrays, resident=0, **kw):
    r = handle(fr.W, fr.H, **FLAG, **kw)
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


def _check_raw(fr, msg, **kw):
    arrays = fr.arrays()
    want = am.render(*arrays, fr.W, fr.H)
    zero(_through(fr, arrays, **kw), want, msg)
    return arrays, want


BOUNDARIES = (15, 16, 63, 64)                                      # list positions: the 16th and 17th staged entries, either side of a class chunk


def raw_corpus():
    """(name, frame) of every raw frame of this file"""
    out = []
    for mode in ("alpha", "erase"):
        for cut in (False, True):
            out.append(("cleared_%s_%d" % (mode, cut), ar.cleared_strips_frame(mode, cut, far=mode == "erase")))
        out.append(("masked_%s" % mode, ar.masked_reach_frame(mode)))
    for fade in (1, 128, 254, 255):
        out.append(("faded_%d" % fade, ar.cleared_strips_frame("alpha", False, 255 - fade, seed=fade)))
    for at in BOUNDARIES:
        out.append(("path_at_%d" % at, ar.sizes_frame("erase_path", at)))
        for what in ("erase", "alpha"):
            out.append(("%s_end_at_%d" % (what, at), ar.sizes_frame(what, at - 4, 3, seed=at)))
    out.append(("cover", ar.cover_frame()))
    out.append(("partial_rows", ar.partial_rows_frame()))
    for depth in range(1, 5):
        for where in ("outer", "inner"):
            out.append(("nesting_%d_%s" % (depth, where), ar.nesting_frame(depth, where)))
    return out


CORPUS = raw_corpus()


@pytest.mark.parametrize("name", [n for n, _ in CORPUS])
def test_raw_frame(name):
    fr = dict(CORPUS)[name]
    arrays, want = _check_raw(fr, name, resident=0 if EMU else 2)
    if name.startswith("cleared_alpha"):
        # the ALPHA END cleared what the ground had painted in the strips its group never reached; the same frame under ERASE did not
        erase = ar.cleared_strips_frame("erase", name.endswith("1"))
        assert (want[8:] != am.render(*erase.arrays(), fr.W, fr.H)[8:]).any()


def test_the_raw_corpus_reaches_what_it_claims():
    """from the arrays alone, no device"""
    ends, cleared, fades, end_pos, path_pos, band_pos, kinds, depths, cover = set(), set(), set(), set(), set(), set(), set(), set(), set()
    cut = False
    for name, fr in CORPUS:
        e, p, s = fr.arrays()
        rc = ar.strip_alpha_reach(fr.W, fr.H, p, s)
        ends |= rc["ends"]
        cleared |= rc["cleared"]
        cut = cut or rc["cut"]
        fades |= rc["fades"]
        end_pos |= rc["end_pos"]
        path_pos |= rc["path_pos"]
        band_pos |= rc["band_pos"]
        kinds |= rc["erase_kinds"]
        depths |= rc["depths"]
        cover |= rc["behind_cover"]
    A, E = am.OP_ALPHA, am.OP_ERASE
    # an ALPHA END where its group was set aside and where it never was: both tile columns, both strips of a tile, and a cut rectangle
    assert {(A, "plain", True), (A, "plain", False), (E, "plain", True), (E, "plain", False)} <= ends
    assert {(0, 1), (1, 0), (1, 1), (2, 0), (3, 1)} <= cleared and cut
    # masked: both halves, the content alone, the mask alone, neither
    assert {(A, "masked", (c, m)) for c in (True, False) for m in (True, False)} <= ends
    assert {(A, "faded", True), (A, "faded", False)} <= ends and {1, 128, 254, 255} <= fades
    for at in BOUNDARIES:
        assert at in path_pos and (E, at) in end_pos and (A, at) in end_pos and (E, at) in band_pos and (A, at) in band_pos, at
    assert cover == {"below", "above"}
    assert {(frame_model.PATH_BOXES, True), (frame_model.PATH_TOR, True)} <= kinds
    assert {(1, d) for d in range(4)} <= depths and {(d, 0) for d in range(1, 5)} <= depths


def test_a_batch_group_that_mixes_frames_with_and_without_the_operators():
    """one render_batch of raw-like stages: the group's plan takes instance 7 for all of them"""
    W, H = 128, 32
    rng = np.random.default_rng(4100)
    frames = []
    for k in range(2 if EMU else 6):
        frames.append(scenes.rand_alpha_mode_scene(rng, width=W, height=H))
        frames.append(cs.rand_composited_scene(rng, width=W, height=H, leaves=8))
    wants = [am.render(*_built(sc, False), W, H) for sc in frames]
    stages = [sc["stage"] for sc in frames]
    r = handle(W, H, **FLAG)
    try:
        if not EMU:
            import torch
            out = torch.zeros((len(stages), H, W, 4), dtype=torch.uint8, device="cuda")
            r.render_batch(stages, out.data_ptr(), H * W * 4)
            got = out.cpu().numpy()
            for k, want in enumerate(wants):
                zero(got[k], want, ("mixed batch", k))
        r.render_batch(stages)
        zero(r.read_image(premultiplied=True), wants[-1], "mixed batch, per-frame route")
        not_refused(r, "mixed batch")
    finally:
        r.close()


def test_random_raw_frames_and_band_handles():
    for seed in range(3 if EMU else 16):
        w, h = cs.EDGE_SIZES[seed % len(cs.EDGE_SIZES)]
        w, h = max(w, 128), max(h, 32)
        fr = ar.rand_frame(np.random.default_rng(9700 + seed), w, h, items=int(30 + 17 * (seed % 5)))
        arrays, want = _check_raw(fr, ("random raw", seed), resident=0 if EMU else 2)
        if seed % 4 == 0:
            for contiguous in (True, False):
                zero(two_bands(w, h, contiguous, lambda r: r.render_edges(*arrays), make=lambda **kw: handle(w, h, **FLAG, **kw)), want, ("random raw bands", seed, contiguous))


# ---------------------------------------------------------------------------------------------------------------- c. differential fuzz
fuzz_scene, _buildable = scenes.fuzz_scene, scenes.buildable        # (the seeds are chosen in tests/test_alpha_modes_host.py, on a host-only handle)


@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_stage_fuzz_through_render(aliased):
    n = 3 if EMU else 24
    skipped = 0
    for seed in range(n):
        sc = fuzz_scene(seed, aliased)
        arrays = _buildable(sc, aliased)
        if arrays is None:
            skipped += 1
            continue
        want = am.render(*arrays, sc["width"], sc["height"], aliased=aliased)
        r = _handle(sc, aliased)
        try:
            r.render(sc["stage"])
            zero(r.read_image(premultiplied=True), want, ("render", aliased, seed))
            not_refused(r, seed)
        finally:
            r.close()
    assert skipped * 20 <= n or EMU, skipped


@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_stage_fuzz_through_render_batch(aliased):
    W, H = 150, 90
    rng = np.random.default_rng(scenes.FUZZ_SEEDS + 500 + aliased)
    frames, wants, skipped = [], [], 0
    n = 3 if EMU else 12
    for k in range(n):
        sc = scenes.rand_alpha_mode_scene(rng, width=W, height=H, leaves=14)
        arrays = _buildable(sc, aliased)
        if arrays is None:
            skipped += 1
            continue
        frames.append(sc)
        wants.append(am.render(*arrays, W, H, aliased=aliased))
    assert skipped * 20 <= n or EMU, skipped
    stages = [sc["stage"] for sc in frames]
    r = handle(W, H, aliased, **FLAG)
    try:
        if not EMU:
            import torch
            out = torch.zeros((len(stages), H, W, 4), dtype=torch.uint8, device="cuda")
            r.render_batch(stages, out.data_ptr(), H * W * 4)
            got = out.cpu().numpy()
            for k, want in enumerate(wants):
                zero(got[k], want, ("batch", aliased, k))
        r.render_batch(stages)
        zero(r.read_image(premultiplied=True), wants[-1], ("per-frame route", aliased))
        not_refused(r, "batch")
    finally:
        r.close()
