"""Masked layers on the device (k2_tiles<5>, the mask instance: the layer instance plus the mask step).

a. Every libcairo golden of tests/mask_scenes.py -- every file, every scene -- through render, swfr_render_edges (+ resident frames),
   SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and render_batch with masked and plain frames in one group; and with
   SWFR_TILES_SHADERS forced to 5; frames WITHOUT a mask -- the scenario corpus, layer goldens, raw layer frames -- forced through
   instance 5.  Zero differing bytes (linear-gradient scenes: LINEAR_BOUND of tests/test_layer_gpu.py).
b. Raw frames of 70 x 13 up to 256 x 64 (tests/mask_raw.py) against tests/frame_model.py, zero differing bytes: the four reach
   cases of a strip under all nine operators; MASK and the masked END as the last entry before and the first behind list positions
   16, 64 and 128; halves of 15 .. 65 members; masked inside masked with four levels set aside by one path; a masked group whose
   content never reaches a strip in which an outer group's pixels are set aside; random nesting over several tile rows, through
   two-band handles too; a thousand small masked groups in one frame.  What the strips of these frames see is computed from the arrays
   (mask_raw.strip_mask_reach) and asserted.  After every frame the handle's swfr_stats show no capacity refusal.

Runs on an MI355X (-m gpu) and, with smaller counts, under tools/emu/run.py.  DESIGN.md, section 5 ("The mask model"), has the table of
kernel mutations this file catches.
"""
import numpy as np
import pytest

import composite_scenes as cs
import device_routes as dr
import frame_model
import mask_raw as mr
import mask_scenes as ms
from composite_scenes import CHUNK, PREFETCH, ROUND
from device_routes import EMU, renderer_for, through_edges, two_bands, zero
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats

pytestmark = pytest.mark.gpu
MASK, END = mr.MASK, cs.END
FAMILY = dr.FAMILIES["mask"]
FILES = sorted(FAMILY.scenes.files())


# ---------------------------------------------------------------------------------------------------------------- a. the goldens
@pytest.mark.parametrize("forced", [False, True], ids=["picked", "forced_5"])
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


def test_a_mask_is_visible():
    """the feature is visible: every operator scene differs from the same scene drawn without its mask"""
    gold = np.load(ms.golden_path("cairo_mask_operators"))
    for name, sc in sorted(ms.operator_scenes().items())[:: 9 if EMU else 1]:
        r = renderer_for(sc, False)
        try:
            r.render({"children": ms.without_masks(sc["stage"]["children"])})
            assert (r.read_image(premultiplied=True) != gold[name]).any(), name
        finally:
            r.close()


def test_frames_without_a_mask_through_instance_5(monkeypatch):
    """the mask instance is the layer instance for a frame without a MASK: the scenario corpus against its libcairo goldens, the layer
    structure goldens of two operators, and raw nested layer frames against tests/frame_model.py"""
    import layer_scenes as ls
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
        zero(through_edges(fr.W, fr.H, arrays), frame_model.render(*arrays, fr.W, fr.H), ("layers through 5", first, depth))


# ---------------------------------------------------------------------------------------------------------------- b. raw frames
def _check_raw(fr, msg, **kw):
    arrays = fr.arrays()
    want = frame_model.render(*arrays, fr.W, fr.H)
    zero(through_edges(fr.W, fr.H, arrays, **kw), want, msg)
    return arrays, want


@pytest.mark.parametrize("op", cs.MODES)
def test_the_four_reach_cases_of_a_strip(op):
    fr = mr.reach_cases_frame(op, seed=cs.MODES.index(op))
    arrays, want = _check_raw(fr, ("reach", op), resident=0 if EMU else 2)
    rc = mr.strip_mask_reach(fr.W, fr.H, arrays[1])
    assert rc["cases"] == {(True, True), (True, False), (False, True), (False, False)}, rc["cases"]
    # the mask does something, and a strip the mask does not reach shows the ground alone
    e, p, s = arrays
    plain = p[np.isin(np.arange(len(p)), [0, 1, len(p) - 1])]
    ground = frame_model.render(e, plain, s, fr.W, fr.H)
    assert (want[:8, 64:128] == ground[:8, 64:128]).all() and (want[:8, 192:] == ground[:8, 192:]).all()
    assert (want[:8, :64] != ground[:8, :64]).any()


SIZES = (15, 16, 17, 63, 64, 65)
SMALL = 3


def _size_shapes(n):
    """(content members, mask members, plain entries before BEGIN): a half of n members beside one of SMALL, and both of n; k chosen
    so that MASK (list position k + content + 1) and the masked END (k + content + mask + 2) are the last entry before and the first
    behind a staging round (16), a class-byte chunk (64) and the prefetched class bytes (128)"""
    shapes = [(n, SMALL, 0), (SMALL, n, 1), (n, n, 0)]
    for edge in (ROUND, CHUNK, PREFETCH):
        for at in (edge - 1, edge):
            shapes.append((SMALL, n, at - SMALL - 1))                 # MASK at `at` (behind a short content half)
            shapes.append((SMALL + n % 3, SMALL, at - 2 * SMALL - n % 3 - 2))     # END at `at` (a short group behind many plain entries)
            if at - n - 1 >= 0:
                shapes.append((n, SMALL, at - n - 1))                # ... behind the long one
            if at - n - SMALL - 2 >= 0:
                shapes.append((n, SMALL, at - n - SMALL - 2))        # END at `at`
                shapes.append((SMALL, n, at - n - SMALL - 2))
    return sorted(set(shapes))


def _size_frame(content, mask, k):
    W, H = ((70, 13), (64, 16), (61, 9), (130, 12))[(content + mask + k) % 4]
    return mr.masked_sizes_frame(np.random.default_rng(7000 + 1000 * content + 10 * mask + k), content, mask, k, W=W, H=H)


@pytest.mark.parametrize("n", SIZES)
def test_halves_of_n_members_and_markers_at_the_list_boundaries(n):
    shapes = _size_shapes(n)
    for content, mask, k in shapes[::4] if EMU else shapes:
        _check_raw(_size_frame(content, mask, k), ("sizes", content, mask, k))


def test_the_size_frames_put_the_markers_where_they_claim():
    """from the arrays alone, no device: MASK and the masked END sit at 15, 16, 63, 64, 127 and 128 of a strip's list, and of its tile
    row's list (where a strip's class bytes are indexed)"""
    for which in (1, 2):
        pos = {MASK: set(), END: set()}
        for n in SIZES:
            for content, mask, k in _size_shapes(n):
                fr = _size_frame(content, mask, k)
                for m in mr.strip_mask_reach(fr.W, fr.H, fr.arrays()[1])["markers"]:
                    pos[m[0]].add(m[which])
        for kind in (MASK, END):
            for edge in (ROUND, CHUNK, PREFETCH):
                assert edge - 1 in pos[kind] and edge in pos[kind], (which, kind, edge, sorted(pos[kind]))


@pytest.mark.parametrize("which", ["four_by_one_path", "outer_survives", "in_content"])
def test_nesting(which):
    fr = mr.nested_masks_frame(which)
    arrays, want = _check_raw(fr, ("nested", which), resident=0 if EMU else 2)
    rc = mr.strip_mask_reach(fr.W, fr.H, arrays[1])
    if which == "four_by_one_path":
        assert rc["together"] == 4, rc["together"]                   # four levels set aside by one path
    if which == "outer_survives":
        assert rc["outer_kept"] and (False, True) in rc["cases"]
        # the outer group's pixels survived: strip (0, 0) is what the frame without the inner masked group gives there
        e, p, s = arrays
        kinds = p["kind"].tolist()
        b = [i for i, k in enumerate(kinds) if k == cs.BEGIN][1]
        en = [i for i, k in enumerate(kinds) if k == cs.END][0]
        without = np.concatenate([p[:b], p[en + 1:]])
        assert (want[:8, :64] == frame_model.render(e, without, s, fr.W, fr.H)[:8, :64]).all()


def test_random_nesting_across_tile_rows_and_band_boundaries():
    cases = set()
    for seed in range(3 if EMU else 16):
        W, H = cs.EDGE_SIZES[seed % len(cs.EDGE_SIZES)]
        W, H = max(W, 128), max(H, 32)
        fr = mr.rand_raw_masked_frame(np.random.default_rng(7700 + seed), W=W, H=H, items=int(30 + 17 * (seed % 5)))
        arrays, want = _check_raw(fr, ("random raw", seed), resident=0 if EMU else 2)
        cases |= mr.strip_mask_reach(W, H, arrays[1])["cases"]
        if seed % 4 == 0:
            for contiguous in (True, False):
                zero(two_bands(W, H, contiguous, lambda r: r.render_edges(*arrays)), want, ("random raw bands", seed, contiguous))
    assert len(cases) == 4 or EMU


def test_a_thousand_small_masked_groups():
    rng = np.random.default_rng(7900)
    fr = mr.many_masked_groups_frame(rng, W=130, H=70, groups=60) if EMU else mr.many_masked_groups_frame(rng, W=256, H=64, groups=1000)
    arrays, _ = _check_raw(fr, "many groups")
    assert int((arrays[1]["kind"] == MASK).sum()) >= (60 if EMU else 1000)
