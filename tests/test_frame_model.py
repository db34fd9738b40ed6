"""tests/frame_model.py pinned without a GPU: the committed libcairo goldens of the layer, blend, mask, fade, pad and spread scenes --
bitmap and radial sources included -- through the model over swfr_build_frame (host-only handles), random composited trees against live libcairo -- which is also the first random check of the frame
builder's clear-surface bookkeeping around groups, in single and threaded builds -- and the model against the oracle on plain frames,
where OVER and the lerp rule are the ones the rest of the suite already trusts.  Zero differing bytes everywhere.  And the reach of
the raw corpus of tests/test_composite_fuzz_gpu.py, computed from the arrays."""
import os

import numpy as np
import pytest

import blend_scenes as bs
import composite_scenes as cs
import frame_model as fm
import helpers
import layer_model as lm
import layer_scenes as ls
from helpers import diff_stats, oracle_render
from host_frames import build_on_host
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")

# golden files every scene of which is solid: all of them must go through the model
ALL_SOLID = (["cairo_layer_overlap", "cairo_layer_aliased_overlap", "cairo_blend_solids", "cairo_blend_aliased_solids", "cairo_blend_structure",
              "cairo_blend_aliased_structure"] + ["cairo_layer_%sstructure_%s" % (a, m) for a in ("", "aliased_") for m in ls.MODES])
GOLDEN_SCENES = 1667                                    # counted: every scene of the golden files below but those with a linear gradient (46 of them), and 13 run-start scenes
SOLID_GOLDEN_SCENES = 636                               # ... of them, the scenes of tests/layer_scenes.py and tests/blend_scenes.py whose built styles are all solid


def _model(sc, aliased=False):
    return fm.render(*build_on_host(sc, aliased), sc["width"], sc["height"], aliased=aliased)


def test_goldens_through_the_model():
    """Every committed libcairo golden of the layer, blend, mask, fade, pad and spread scenes through the model: zero differing bytes.
    A scene may be left out (NotImplementedError) for one reason only: a linear gradient -- a float ramp within 1 LSB by design -- or a
    colour-transformed (variant) texture, whose texels belong to the handle that walked the stage (the pad cxform files).  Padded
    radial gradients are drawn (tests/test_shaded_frame_model.py holds them against the oracle).  Of the run-start goldens of the
    spread scenes (tests/spread_scenes.py, runstart_cases) those go through whose case shows no caveat pixel -- every REPEAT one, and
    the REFLECT ones marked so; the others pin libcairo's covered-samples walker in their caveat pixels, not the every-sample rule,
    and there the model must differ from the golden, in those few pixels only."""
    import fade_scenes as fs
    import mask_scenes as ms
    import pad_scenes as ps
    import spread_scenes as ss
    from host_frames import bitmaps_of
    from swf_renderer_amd import api
    checked = solid = variants = 0
    per_file = {}
    files = [(mod, fname, v) for mod in (ls, bs, ms, fs, ps, ss) for fname, v in sorted(mod.files().items())]
    files += [(ps, fname, v) for fname, v in sorted(ps.cxform_files().items())]
    for mod, fname, (make, aliased) in files:
        gold = np.load(mod.golden_path(fname))
        for name, sc in sorted(make().items()):
            arrays = build_on_host(sc, aliased)
            styles = arrays[2]
            linear = any(int(st.kind) == api.STYLE_LINEAR for st in styles)
            variant = any(int(st.kind) == api.STYLE_BITMAP and int(st.bitmap) >= api.VARIANT_BASE for st in styles)
            if linear or variant:
                with pytest.raises(NotImplementedError):
                    fm.render(*arrays, sc["width"], sc["height"], aliased=aliased, bitmaps=bitmaps_of(sc))
                per_file.setdefault(fname, [0, 0])[1] += 1
                variants += variant
                continue
            assert diff_stats(fm.render(*arrays, sc["width"], sc["height"], aliased=aliased, bitmaps=bitmaps_of(sc)), gold[name]) == (0, 0), (fname, name)
            per_file.setdefault(fname, [0, 0])[0] += 1
            checked += 1
            solid += mod in (ls, bs) and all(int(st.kind) == api.STYLE_SOLID for st in styles)
    runstart = 0
    for fname, (_, aliased) in sorted(ss.runstart_files().items()):
        gold = np.load(ss.golden_path(fname))
        spread = "reflect" if "reflect" in fname else "repeat"
        for name, case in sorted(ss.runstart_cases(spread, aliased).items()):
            sc = case["scene"]
            n, _ = diff_stats(fm.render(*build_on_host(sc, aliased), sc["width"], sc["height"], aliased=aliased), gold[name])
            if spread == "reflect" and case["caveat"]:
                assert 0 < n <= 4, (fname, name, n)                  # (the golden is libcairo's side of the caveat)
            else:
                assert n == 0, (fname, name, n)
                runstart += 1
    checked += runstart
    for fname in ALL_SOLID:
        assert per_file[fname][0] > 0 and per_file[fname][1] == 0, (fname, per_file[fname])
    for fname, (ok, left_out) in per_file.items():                   # the files with bitmap and gradient sources: all but their linear scenes
        if "_sources" in fname:
            assert ok >= 8 and left_out <= 2, (fname, ok, left_out)
        if fname.startswith("cairo_pad_") and "cxform" not in fname:
            assert ok > 0 and left_out == 0, (fname, ok, left_out)
    layer_aa = sum(v[0] for k, v in per_file.items() if k.startswith("cairo_layer_") and "aliased" not in k)
    print("goldens through the model:", checked, "scenes,", solid, "of them solid layer and blend scenes,", layer_aa, "antialiased layer scenes;", variants, "left out for a variant texture")
    assert layer_aa >= 174 + 9 * 8 and solid >= SOLID_GOLDEN_SCENES and checked >= GOLDEN_SCENES, (layer_aa, solid, checked)
    assert variants > 0 and runstart >= 13


def test_a_transparent_group_pixel_leaves_the_destination_alone():
    """what lets the model composite inside the group's rectangle only"""
    d = np.random.default_rng(3).integers(0, 256, (4096, 4)).astype(np.uint8)
    d[:, :3] = np.minimum(d[:, :3], d[:, 3:])
    for mode in ls.MODES:
        assert (lm.composite(mode, np.zeros_like(d), d) == d).all(), mode


def test_the_model_refuses_what_the_header_refuses():
    fr = cs.RawFrame(32, 16)
    fr.begin().box(1, 1, 9, 9, 0x80402010, 1).end("add")
    e, p, s = fr.arrays()
    fm.render(e, p, s, 32, 16)
    for edit in (lambda q: q["kind"].__setitem__(2, 0), lambda q: q["kind"].__setitem__(0, 0), lambda q: q["lerp"].__setitem__(1, 1 | (3 << 8)),
                 lambda q: q["lerp"].__setitem__(1, 9 << 8), lambda q: q["x_max"].__setitem__(1, 20), lambda q: q["lerp"].__setitem__(2, 1)):
        q = p.copy()
        edit(q)
        with pytest.raises(ValueError):
            fm.render(e, q, s, 32, 16)


@needs_cairo
@pytest.mark.parametrize("aliased,seeds", [(False, 200), (True, 100)], ids=["antialiased", "aliased"])
def test_random_composited_trees_equal_libcairo(aliased, seeds):
    differing = groups = deepest = 0
    for seed in range(seeds):
        sc = cs.rand_composited_scene(np.random.default_rng(1000 + seed + 10000 * aliased))
        arrays = build_on_host(sc, aliased)
        depth = 0
        for k in arrays[1]["kind"].tolist():
            depth += (k == cs.BEGIN) - (k == cs.END)
            deepest = max(deepest, depth)
        groups += int((arrays[1]["kind"] == cs.BEGIN).sum())
        n, _ = diff_stats(fm.render(*arrays, sc["width"], sc["height"], aliased=aliased), ls.cairo_render(sc, aliased))
        differing += n
        assert n == 0, (seed, aliased, sc["width"], sc["height"])
    print("random trees against libcairo:", seeds, "seeds, aliased" if aliased else "seeds,", groups, "groups, deepest", deepest, "differing pixels", differing)
    assert deepest == lm.MAX_DEPTH and groups > 5 * seeds


@needs_cairo
@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_threaded_build_is_the_single_walk_and_equals_libcairo(aliased):
    """at least 200 children of the stage: FrameBuilder::build cuts two or three pieces of at least 64"""
    for seed in range(6):
        sc = cs.rand_composited_scene(np.random.default_rng(2000 + seed), min_children=200 + 70 * (seed % 3), leaves=30)
        assert len(sc["stage"]["children"]) >= 200
        built = []
        for threads in ("1", "2", "3", "8"):
            os.environ["SWFR_BUILD_THREADS"] = threads
            try:
                built.append(build_on_host(sc, aliased))
            finally:
                del os.environ["SWFR_BUILD_THREADS"]
        for other in built[1:]:
            assert other[0].tobytes() == built[0][0].tobytes() and other[1].tobytes() == built[0][1].tobytes(), seed
            assert [bytes(st) for st in other[2]] == [bytes(st) for st in built[0][2]], seed
        assert diff_stats(fm.render(*built[-1], sc["width"], sc["height"], aliased=aliased), ls.cairo_render(sc, aliased)) == (0, 0), seed


def test_the_model_equals_the_oracle_on_plain_frames(monkeypatch):
    rng = np.random.default_rng(5)
    for it in range(40):
        sc, info = helpers.rand_polygon_scene(rng, it)
        assert diff_stats(_model(sc), oracle_render(sc)) == (0, 0), ("poly", it, info)
    rng = np.random.default_rng(11)
    for it in range(20):
        sc = helpers.rand_layered_translucent_scene(rng)
        assert diff_stats(_model(sc), oracle_render(sc)) == (0, 0), ("layered", it)
    monkeypatch.setattr(helpers, "DENSE_KINDS", ("solid", "rect_fill", "rect_stroke", "stroke"))      # the solid kinds
    rng = np.random.default_rng(4040)
    for it in range(6):
        sc = helpers.rand_dense_scene(rng)
        assert diff_stats(_model(sc), oracle_render(sc)) == (0, 0), ("dense", it)


def test_the_raw_corpus_reaches_what_it_claims():
    """the frames of tests/test_composite_fuzz_gpu.py, checked here on the arrays: every frame is accepted by swfr_upload_edges' checks
    (a host-only handle answers NO_DEVICE only behind them), and together they reach the positions the tests are about"""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    rc = cs.raw_corpus_reach()
    print("raw corpus: most in-group entries of a strip", rc["in_group"], "markers", len(rc["markers"]), "first levels", sorted(rc["first_levels"]),
          "bare ENDs at depths", sorted(rc["bare_ends"]), "levels set aside together", rc["together"])
    cs.assert_reach(rc)
    frames = [fr for n in (17, 129, 200) for _, fr in cs.group_size_frames(n)] + [fr for _, fr in cs.late_group_frames()]
    frames += [cs.raw_nesting_frame(f, d) for f, d in cs.NESTINGS] + [fr for _, fr in cs.nested_frames()]
    frames += [cs.raw_cover_frame(p, k) for p in cs.COVER_PLACES for k in ("tor", "box")] + [cs.raw_many_groups_frame(np.random.default_rng(6900), 260, 120, 300)]
    for fr in frames:
        r = S.Renderer(fr.W, fr.H, device=api.DEVICE_HOST_ONLY)
        try:
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(*fr.arrays())
            assert ei.value.code == api.ERR_NO_DEVICE, ei.value
        finally:
            r.close()
