"""tests/frame_model.py's faded groups pinned without a GPU: the committed libcairo goldens of the fade scenes whose styles are all solid through
the model over swfr_build_frame (host-only handles), byte for byte; and random composited trees -- faded, masked and plain groups
nested up to the depth limit -- against live libcairo, which is also the random check of the frame builder's bookkeeping around faded
groups.  Zero differing pixels."""
import numpy as np
import pytest

import composite_scenes as cs
import fade_model as fd
import fade_scenes as fs
import frame_model as fm
from helpers import diff_stats
from host_frames import build_on_host
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
MASK = fd.PATH_GROUP_MASK


def _fades(paths):
    return int(((paths["lerp"].astype(np.int64) & 0xffffffff) >> 24 != 0).sum())


def test_solid_goldens_through_the_model():
    from swf_renderer_amd import api
    checked = fades = 0
    for fname, name, sc, aliased in fs.solid_scenes():
        gold = np.load(fs.golden_path(fname))
        arrays = build_on_host(sc, aliased)
        assert all(int(st.kind) == api.STYLE_SOLID for st in arrays[2]), (fname, name)
        fades += _fades(arrays[1])
        assert diff_stats(fm.render(*arrays, sc["width"], sc["height"], aliased=aliased), gold[name]) == (0, 0), (fname, name)
        checked += 1
    print("fade goldens through the model:", checked, "scenes,", fades, "faded ENDs")
    assert checked >= 2 * (63 + 8 + 16 + 81) and fades > checked // 3


def test_the_model_refuses_what_the_header_refuses():
    f = cs.RawFrame(32, 16)
    f.begin().box(1, 1, 9, 9, 0x80402010, 1).end("add", opacity=100)
    e, p, s = f.arrays()
    assert [int(k) for k in p["kind"]] == [2, 1, 3] and int(p["lerp"][2]) == fd.end_lerp(6, 100)
    fm.render(e, p, s, 32, 16)
    for edit in (lambda q: q["lerp"].__setitem__(0, 1 << 24), lambda q: q["lerp"].__setitem__(1, 1 | (1 << 24)),
                 lambda q: q["lerp"].__setitem__(2, int(q["lerp"][2]) | (1 << 16))):
        q = p.copy()
        edit(q)
        with pytest.raises(ValueError):
            fm.render(e, q, s, 32, 16)
    m = cs.RawFrame(32, 16)                                         # a fade on the END of a group that holds a MASK
    m.begin().box(1, 1, 9, 9, 0x80402010, 1).mask().box(2, 2, 8, 8, 0x80000000, 1).end("add", opacity=100)
    e, p, s = m.arrays()
    with pytest.raises(ValueError):
        fm.render(e, p, s, 32, 16)


@needs_cairo
@pytest.mark.parametrize("aliased,seeds", [(False, 120), (True, 60)], ids=["antialiased", "aliased"])
def test_random_faded_trees_equal_libcairo(aliased, seeds):
    differing = fades = masks = deepest = around_masked = 0
    for seed in range(seeds):
        sc = fs.rand_faded_scene(np.random.default_rng(7000 + seed + 10000 * aliased))
        assert max(fs._levels(k) for k in sc["stage"]["children"]) <= fd.MAX_DEPTH       # (no case is refused or skipped)
        arrays = build_on_host(sc, aliased)
        two = fm.masked_begins(arrays[1])
        levels, stack = 0, []
        for i, (k, v) in enumerate(zip(arrays[1]["kind"].tolist(), arrays[1]["lerp"].tolist())):
            if k == cs.BEGIN:
                stack.append(2 if i in two else 1)
                levels += stack[-1]
                deepest = max(deepest, levels)
                if i in two and i and arrays[1]["kind"][i - 1] == cs.BEGIN:
                    around_masked += 1
            elif k == cs.END:
                levels -= stack.pop()
        fades += _fades(arrays[1])
        masks += int((arrays[1]["kind"] == MASK).sum())
        n, _ = diff_stats(fm.render(*arrays, sc["width"], sc["height"], aliased=aliased), fs.cairo_render(sc, aliased))
        differing += n
        assert n == 0, (seed, aliased, sc["width"], sc["height"])
    print("random faded trees against libcairo:", seeds, "seeds, aliased" if aliased else "seeds,", fades, "faded groups,", masks,
          "masked groups, a group opening right around a masked one", around_masked, "deepest", deepest, "differing pixels", differing)
    assert deepest == fd.MAX_DEPTH and fades > 3 * seeds and masks > seeds


@needs_cairo
@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_threaded_build_of_faded_trees_is_the_single_walk_and_equals_libcairo(aliased, monkeypatch):
    for seed in range(4):
        sc = fs.rand_faded_scene(np.random.default_rng(8000 + seed), min_children=200 + 70 * (seed % 3), leaves=30)
        out = []
        for threads in ("1", "3"):
            monkeypatch.setenv("SWFR_BUILD_THREADS", threads)
            out.append(build_on_host(sc, aliased))
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
        assert _fades(out[0][1]) > 0
        assert diff_stats(fm.render(*out[1], sc["width"], sc["height"], aliased=aliased), fs.cairo_render(sc, aliased)) == (0, 0), seed
