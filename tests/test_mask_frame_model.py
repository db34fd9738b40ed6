"""tests/frame_model.py's masked groups pinned without a GPU: the committed libcairo goldens of the mask scenes whose styles are all solid
through the model over swfr_build_frame (host-only handles), byte for byte; and random composited trees with masks against live
libcairo -- which is also the random check of the frame builder's bookkeeping around masked groups.  Zero differing pixels."""
import numpy as np
import pytest

import composite_scenes as cs
import frame_model as fm
import mask_model as mk
import mask_scenes as ms
from helpers import diff_stats
from host_frames import build_on_host
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
MASK = mk.PATH_GROUP_MASK


def test_solid_goldens_through_the_model():
    from swf_renderer_amd import api
    checked = masks = 0
    for fname, name, sc, aliased in ms.solid_scenes():
        gold = np.load(ms.golden_path(fname))
        arrays = build_on_host(sc, aliased)
        assert all(int(st.kind) == api.STYLE_SOLID for st in arrays[2]), (fname, name)
        masks += int((arrays[1]["kind"] == MASK).sum())
        assert diff_stats(fm.render(*arrays, sc["width"], sc["height"], aliased=aliased), gold[name]) == (0, 0), (fname, name)
        checked += 1
    print("mask goldens through the model:", checked, "scenes,", masks, "MASK markers")
    assert checked >= 2 * (27 + 8 + 16 + 54) and masks > checked // 2


def test_the_model_refuses_what_the_header_refuses():
    fr = cs.RawFrame(32, 16)
    fr.begin().box(1, 1, 9, 9, 0x80402010, 1).mask().box(2, 2, 8, 8, 0x80000000, 1).end("add")
    e, p, s = fr.arrays()
    assert [int(k) for k in p["kind"]] == [2, 1, 4, 1, 3]
    fm.render(e, p, s, 32, 16)
    for edit in (lambda q: q["kind"].__setitem__(1, 4), lambda q: q["lerp"].__setitem__(2, 1), lambda q: q["n_edges"].__setitem__(2, 1),
                 lambda q: q["x_max"].__setitem__(2, 8), lambda q: q["kind"].__setitem__(0, 4), lambda q: q["kind"].__setitem__(4, 4)):
        q = p.copy()
        edit(q)
        with pytest.raises(ValueError):
            fm.render(e, q, s, 32, 16)
    deep = cs.RawFrame(32, 16)                                      # two masked groups nested plus one more group: five levels
    deep.begin().begin().box(1, 1, 9, 9, 1 << 24, 1).mask().begin().box(1, 1, 9, 9, 1 << 24, 1).mask().box(1, 1, 9, 9, 1 << 24, 1).end().end().mask().box(1, 1, 9, 9, 1 << 24, 1).end()
    e, p, s = deep.arrays()
    with pytest.raises(ValueError):
        fm.render(e, p, s, 32, 16)


@needs_cairo
@pytest.mark.parametrize("aliased,seeds", [(False, 120), (True, 60)], ids=["antialiased", "aliased"])
def test_random_masked_trees_equal_libcairo(aliased, seeds):
    differing = masks = deepest = nested = 0
    for seed in range(seeds):
        sc = ms.rand_masked_scene(np.random.default_rng(3000 + seed + 10000 * aliased))
        arrays = build_on_host(sc, aliased)
        depth, in_masked = 0, []
        for k in arrays[1]["kind"].tolist():
            if k == MASK and any(in_masked[:-1]):
                nested += 1
            if k == cs.BEGIN:
                in_masked.append(False)
            elif k == MASK:
                in_masked[-1] = True
            elif k == cs.END:
                in_masked.pop()
        levels = 0
        two = fm.masked_begins(arrays[1])
        stack = []
        for i, k in enumerate(arrays[1]["kind"].tolist()):
            if k == cs.BEGIN:
                stack.append(2 if i in two else 1)
                levels += stack[-1]
                deepest = max(deepest, levels)
            elif k == cs.END:
                levels -= stack.pop()
        masks += int((arrays[1]["kind"] == MASK).sum())
        n, _ = diff_stats(fm.render(*arrays, sc["width"], sc["height"], aliased=aliased), ms.cairo_render(sc, aliased))
        differing += n
        assert n == 0, (seed, aliased, sc["width"], sc["height"])
    print("random masked trees against libcairo:", seeds, "seeds, aliased" if aliased else "seeds,", masks, "masked groups,", nested,
          "of them inside a masked group, deepest", deepest, "differing pixels", differing)
    assert deepest == mk.MAX_DEPTH and masks > 3 * seeds and nested > seeds // 10


@needs_cairo
@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_threaded_build_of_masked_trees_is_the_single_walk_and_equals_libcairo(aliased, monkeypatch):
    for seed in range(4):
        sc = ms.rand_masked_scene(np.random.default_rng(4000 + seed), min_children=200 + 70 * (seed % 3), leaves=30)
        out = []
        for threads in ("1", "3"):
            monkeypatch.setenv("SWFR_BUILD_THREADS", threads)
            out.append(build_on_host(sc, aliased))
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
        assert (out[0][1]["kind"] == MASK).any()
        assert diff_stats(fm.render(*out[1], sc["width"], sc["height"], aliased=aliased), ms.cairo_render(sc, aliased)) == (0, 0), seed
