"""Layer opacity on the device (k2_tiles<6>, the instance that fades: the mask instance plus the fade
step at a group's END).

a. Every libcairo golden of tests/fade_scenes.py -- every file, every scene -- through render, swfr_render_edges (+ resident frames),
   SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and render_batch with faded and plain frames in one group; and with
   SWFR_TILES_SHADERS forced to 6; frames WITHOUT a fade -- the scenario corpus, the layer and mask goldens, raw layer and mask frames
   -- forced through the instance that fades.  Zero differing bytes (linear-gradient scenes: LINEAR_BOUND of tests/test_layer_gpu.py;
   mul_un8 by the opacity has slope <= 1, so the bound carries over).
b. Raw frames of 70 x 13 up to 256 x 64 (tests/fade_raw.py) against tests/frame_model.py, zero differing bytes: a faded END in a
   strip its group reached and in one it reached by its rectangle alone, under all nine operators; a faded END as the last entry
   before and the first behind list positions 16, 64 and 128; four nested faded groups set aside by one path; a faded group around a
   masked one whose content misses the strip; opacities 0, 1, 254 and 255; random nesting of plain, faded and masked groups over
   several tile rows, through two-band handles too; a thousand small faded groups in one frame.  What the strips of these frames see
   is computed from the arrays (fade_raw.strip_fade_reach) and asserted.  After every frame the handle's swfr_stats show no capacity
   refusal.

Runs on an MI355X (-m gpu) and, with smaller counts, under tools/emu/run.py.  DESIGN.md, section 5 ("The fade model"), has the table of
kernel mutations this file catches.
"""
import numpy as np
import pytest

import composite_scenes as cs
import device_routes as dr
import fade_raw as fr_
import fade_scenes as ms
import frame_model
from composite_scenes import CHUNK, PREFETCH, ROUND
from device_routes import EMU, renderer_for, through_edges, two_bands, zero
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats

pytestmark = pytest.mark.gpu
FAMILY = dr.FAMILIES["fade"]
FILES = sorted(FAMILY.scenes.files())


# ---------------------------------------------------------------------------------------------------------------- a. the goldens
@pytest.mark.parametrize("forced", [False, True], ids=["picked", "forced"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render(fname, forced, monkeypatch):
    dr.goldens_through_render(FAMILY, fname, monkeypatch, forced)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_edges(fname):
    dr.goldens_through_render_edges(FAMILY, fname)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_with_graphs(fname, monkeypatch):
    dr.goldens_with_graphs(FAMILY, fname, monkeypatch)


@pytest.mark.parametrize("contiguous", FAMILY.layouts, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_two_band_handles(fname, contiguous):
    dr.goldens_through_two_band_handles(FAMILY, fname, contiguous)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_batch_with_unlike_frames(fname):
    dr.goldens_through_render_batch_with_unlike_frames(FAMILY, fname)


def test_a_fade_is_visible():
    """the feature is visible: every operator scene differs from the same scene drawn without its opacity (the plain layer), and the
    group faded as a whole from the same children under a colour transform with that alpha multiplier"""
    gold = np.load(ms.golden_path("cairo_fade_operators"))
    for name, sc in sorted(ms.operator_scenes().items())[:: 9 if EMU else 1]:
        r = renderer_for(sc, False)
        try:
            r.render({"children": ms.without_opacity(sc["stage"]["children"])})
            assert (r.read_image(premultiplied=True) != gold[name]).any(), name
        finally:
            r.close()
    gold = np.load(ms.golden_path("cairo_fade_sources"))
    assert (gold["whole_not_per_definition"] != gold["per_definition"]).any()


def test_frames_without_a_fade_through_the_instance_that_fades(monkeypatch):
    """for a frame without a fade the instance is what it was: the scenario corpus against its libcairo goldens, the layer structure
    goldens of two operators, every mask golden, and raw nested layer and mask frames against their models"""
    import layer_scenes as ls
    import mask_raw as mr
    import mask_scenes
    import scenarios
    from helpers import golden, product_render
    monkeypatch.setenv("SWFR_TILES_SHADERS", FAMILY.instance)
    SC = scenarios.scenarios()
    for name in sorted(SC)[:: 9 if EMU else 1]:
        sc = SC[name]
        n, mx = diff_stats(product_render(sc), golden("cairo_" + name, "rgba_premul"))
        assert ((n, mx) == (0, 0)) if sc["exact"] else mx <= 1, (name, n, mx)
    for mode in ("normal", "multiply"):
        gold = np.load(ls.golden_path("cairo_layer_structure_" + mode))
        for name, sc in sorted(ls.structure_scenes([mode]).items())[:: 7 if EMU else 1]:
            assert diff_stats(product_render(sc), gold[name]) == (0, 0), name
    for first, depth in cs.NESTINGS[:: 4 if EMU else 1]:
        fr = cs.raw_nesting_frame(first, depth)
        arrays = fr.arrays()
        zero(through_edges(fr.W, fr.H, arrays), frame_model.render(*arrays, fr.W, fr.H), ("layers through the fade instance", first, depth))
    for fname, (make, aliased) in sorted(mask_scenes.files().items()):
        gold = np.load(mask_scenes.golden_path(fname))
        for name, sc in sorted(make().items())[:: 11 if EMU else 1]:
            r = renderer_for(sc, aliased)
            try:
                r.render(sc["stage"])
                dr.check(FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "masks through the fade instance"))
            finally:
                r.close()
    for op in cs.MODES[:: 4 if EMU else 1]:
        fr = mr.reach_cases_frame(op, seed=cs.MODES.index(op))
        arrays = fr.arrays()
        zero(through_edges(fr.W, fr.H, arrays), frame_model.render(*arrays, fr.W, fr.H), ("mask reach through the fade instance", op))
    for which in ("four_by_one_path", "outer_survives", "in_content"):
        fr = mr.nested_masks_frame(which)
        arrays = fr.arrays()
        zero(through_edges(fr.W, fr.H, arrays), frame_model.render(*arrays, fr.W, fr.H), ("mask nesting through the fade instance", which))


# ---------------------------------------------------------------------------------------------------------------- b. raw frames
def _check_raw(fr, msg, **kw):
    arrays = fr.arrays()
    want = frame_model.render(*arrays, fr.W, fr.H)
    zero(through_edges(fr.W, fr.H, arrays, **kw), want, msg)
    return arrays, want


def _without_fades(arrays):
    e, p, s = arrays
    q = p.copy()
    q["lerp"] = (q["lerp"].astype(np.int64) & 0x00ffffff).astype(q["lerp"].dtype)
    return e, q, s


@pytest.mark.parametrize("op", cs.MODES)
def test_a_faded_end_where_the_group_reached_and_where_it_did_not(op):
    fr = fr_.reach_cases_frame(op, 128, seed=cs.MODES.index(op))
    arrays, want = _check_raw(fr, ("reach", op), resident=0 if EMU else 2)
    rc = fr_.strip_fade_reach(fr.W, fr.H, arrays[1])
    assert rc["cases"] == {True, False}, rc["cases"]
    # the fade does something where the group painted, and a strip the group reached by its rectangle alone shows the ground alone
    e, p, s = arrays
    plain = p[np.isin(np.arange(len(p)), [0, 1, len(p) - 1])]
    ground = frame_model.render(e, plain, s, fr.W, fr.H)
    unfaded = frame_model.render(*_without_fades(arrays), fr.W, fr.H)
    assert (want[:8, 64:128] == ground[:8, 64:128]).all() and (want[:8, 192:] == ground[:8, 192:]).all() and (want[8:, :192] == ground[8:, :192]).all()
    assert (want[:8, :64] != ground[:8, :64]).any() and (want[:8, :64] != unfaded[:8, :64]).any() and (want[8:, 192:] != unfaded[8:, 192:]).any()


SIZES = (3, 15, 16, 17, 63, 64, 65)


def _size_shapes(n):
    """(members, plain entries before BEGIN): the faded END (list position k + n + 1) as the last entry before and the first behind a
    staging round (16), a class-byte chunk (64) and the prefetched class bytes (128)"""
    shapes = [(n, 0), (n, 1)]
    for edge in (ROUND, CHUNK, PREFETCH):
        for at in (edge - 1, edge):
            if at - n - 1 >= 0:
                shapes.append((n, at - n - 1))
    return sorted(set(shapes))


def _size_frame(n, k):
    W, H = ((70, 13), (64, 16), (61, 9), (130, 12))[(n + k) % 4]
    return fr_.fade_sizes_frame(np.random.default_rng(9000 + 1000 * n + k), n, k, W=W, H=H)


@pytest.mark.parametrize("n", SIZES)
def test_a_faded_end_at_the_list_boundaries(n):
    shapes = _size_shapes(n)
    for members, k in shapes[::3] if EMU else shapes:
        _check_raw(_size_frame(members, k), ("sizes", members, k))


def test_the_size_frames_put_the_faded_end_where_they_claim():
    """from the arrays alone, no device: the faded END sits at 15, 16, 63, 64, 127 and 128 of a strip's list, and of its tile row's
    list (where a strip's class bytes are indexed)"""
    for which in (0, 1):
        pos = set()
        for n in SIZES:
            for members, k in _size_shapes(n):
                fr = _size_frame(members, k)
                pos |= {m[which] for m in fr_.strip_fade_reach(fr.W, fr.H, fr.arrays()[1])["markers"]}
        for edge in (ROUND, CHUNK, PREFETCH):
            assert edge - 1 in pos and edge in pos, (which, edge, sorted(pos))


@pytest.mark.parametrize("which", ["four_by_one_path", "around_masked_missing", "around_masked_alone"])
def test_nesting(which):
    fr = fr_.nested_fades_frame(which)
    arrays, want = _check_raw(fr, ("nested", which), resident=0 if EMU else 2)
    rc = fr_.strip_fade_reach(fr.W, fr.H, arrays[1])
    if which == "four_by_one_path":
        assert rc["together"] == 4, rc["together"]                   # four faded groups set aside by one path
    else:
        assert rc["after_dropped"]                                   # the faded END right behind a mask step that dropped its product
    assert (want != frame_model.render(*_without_fades(arrays), fr.W, fr.H)).any()


@pytest.mark.parametrize("opacity", [0, 1, 254, 255])
def test_the_opacities_at_both_ends(opacity):
    for k, op in enumerate(cs.MODES[:: 4 if EMU else 1]):
        fr = fr_.fade_sizes_frame(np.random.default_rng(9500 + k), 5 + k, 2, W=70, H=13, end_op=op, opacity=opacity)
        arrays, want = _check_raw(fr, ("opacity", opacity, op))
        e, p, s = arrays
        if opacity == 255:                                           # the plain layer, byte for byte
            assert not (p["lerp"].astype(np.int64) >> 24).any() and (want == frame_model.render(e, p, s, fr.W, fr.H)).all()
        if opacity == 0:                                             # the frame without the group
            kinds = p["kind"].tolist()
            without = np.concatenate([p[:kinds.index(cs.BEGIN)], p[kinds.index(cs.END) + 1:]])
            assert (want == frame_model.render(e, without, s, fr.W, fr.H)).all()


def test_random_nesting_across_tile_rows_and_band_boundaries():
    cases, fades = set(), 0
    for seed in range(3 if EMU else 16):
        W, H = cs.EDGE_SIZES[seed % len(cs.EDGE_SIZES)]
        W, H = max(W, 128), max(H, 32)
        fr = fr_.rand_raw_faded_frame(np.random.default_rng(9700 + seed), W=W, H=H, items=int(30 + 17 * (seed % 5)))
        arrays, want = _check_raw(fr, ("random raw", seed), resident=0 if EMU else 2)
        cases |= fr_.strip_fade_reach(W, H, arrays[1])["cases"]
        fades += int(((arrays[1]["lerp"].astype(np.int64) & 0xffffffff) >> 24 != 0).sum())
        if seed % 4 == 0:
            for contiguous in (True, False):
                zero(two_bands(W, H, contiguous, lambda r: r.render_edges(*arrays)), want, ("random raw bands", seed, contiguous))
    assert (cases == {True, False} and fades > 40) or EMU


def test_a_thousand_small_faded_groups():
    rng = np.random.default_rng(9900)
    fr = fr_.many_faded_groups_frame(rng, W=130, H=70, groups=60) if EMU else fr_.many_faded_groups_frame(rng, W=256, H=64, groups=1000)
    arrays, _ = _check_raw(fr, "many groups")
    assert int(((arrays[1]["lerp"].astype(np.int64) & 0xffffffff) >> 24 != 0).sum()) >= (60 if EMU else 1000)
