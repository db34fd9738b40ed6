"""The shaded sources of tests/frame_model.py -- bitmap fills by tests/pad_model.py, radial and focal gradients by tests/spread_model.py's
every-sample walker -- pinned without a GPU: the array form of the bitmap fetch against the scalar one, the padded radial source
against the oracle, random shaded trees and the lerp-bit rule against live libcairo, the refusals; and the reach of the raw frames of
tests/test_shaded_composite_fuzz_gpu.py, computed from the model's sample positions.  Zero differing bytes everywhere.  (The libcairo
goldens with bitmap and gradient sources go through the model in tests/test_frame_model.py, test_goldens_through_the_model.)"""
import hashlib
import json

import numpy as np
import pytest

import composite_scenes as cs
import frame_model as fm
import helpers
import pad_model as pm
import pad_scenes as ps
import scenarios
import spread_model as sm
from helpers import diff_stats, oracle_render
from host_frames import bitmaps_of, build_on_host
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")


def _model(sc, aliased=False):
    return fm.render(*build_on_host(sc, aliased), sc["width"], sc["height"], aliased=aliased, bitmaps=bitmaps_of(sc))


def test_the_array_fetch_is_the_scalar_fetch():
    """pad_model.source_pixels (bilinear_many, convolution_many) == pad_model.source (bilinear, convolution) on the whole
    random_box_case corpus of tests/test_pad_model.py, under all three edge rules"""
    from test_pad_model import CASES
    rng = np.random.default_rng(20261019)
    filters = {True: 0, False: 0}
    for it in range(CASES):
        md = ps.random_box_case(rng, minified=bool(it & 1))["model"]
        texels, m = pm.premultiply(md["bitmap"]), sm.pattern_matrix(md["matrices"])
        for extend in (pm.NONE, pm.REPEAT, pm.PAD):
            scalar = pm.source(md["matrices"], texels, md["rect"], extend)
            assert (pm.source_pixels(m, texels, md["rect"], extend) == scalar["pixels"]).all(), (it, extend, md["matrices"], md["rect"])
        filters[scalar["bilinear"]] += 1
    assert min(filters.values()) >= CASES // 3, filters


def test_the_padded_radial_source_is_the_oracle():
    """the device draws a padded radial gradient with shade_radial, which the suite holds against the oracle: the model's padded
    walker (spread_model.Walker, PAD) has to give the oracle's frame before the model may draw such a style at all"""
    assert fm.PAD_RADIAL
    rng = np.random.default_rng(31)
    differing = 0
    for it in range(60):
        sc = helpers.rand_radial_scene(rng)
        n, mx = diff_stats(_model(sc), oracle_render(sc))
        differing += n
        assert n == 0, (it, sc["width"], sc["height"], n, mx)
    print("padded radial scenes against the oracle: 60 scenes, differing pixels", differing)


@needs_cairo
@pytest.mark.parametrize("aliased,seeds", [(False, 160), (True, 80)], ids=["antialiased", "aliased"])
def test_random_shaded_trees_equal_libcairo(aliased, seeds):
    """Every pixel is compared.  libcairo's walker sees covered samples only, so the every-sample rule of the model may differ from
    it in the caveat pixels of spread_model.frame; these seeds have none -- the share printed is that of the pixels that had to be
    left out, and the bound on it 1 %."""
    kinds, compared, left_out = {}, 0, 0
    for seed in range(seeds):
        sc = cs.rand_composited_scene(np.random.default_rng(1000 + seed + 10000 * aliased), shaded=True)
        arrays = build_on_host(sc, aliased)
        for st in arrays[2]:
            kinds[int(st.kind), int(st.extend)] = kinds.get((int(st.kind), int(st.extend)), 0) + 1
        got = fm.render(*arrays, sc["width"], sc["height"], aliased=aliased, bitmaps=bitmaps_of(sc))
        n, mx = diff_stats(got, cs.cairo_render_shaded(sc, aliased))
        compared += sc["width"] * sc["height"]
        assert n == 0, (seed, aliased, sc["width"], sc["height"], n, mx)
    print("shaded trees against libcairo:", seeds, "seeds, styles by (kind, extend)", sorted(kinds.items()), "caveat share", left_out / compared)
    assert left_out < 0.01 * compared
    for kind in (fm.STYLE_RADIAL, fm.STYLE_BITMAP):
        for extend in (0, 1, 2):
            assert kinds.get((kind, extend), 0) >= seeds // 2, (kind, extend, kinds)


def _tri(fill, dx=0.0):
    return {"type": "shape", "definition": scenarios._poly_shape([(round((x + dx) * 20), round(y * 20)) for x, y in ((3.3, 2.4), (58.6, 7.7), (21.2, 41.9))], fill)}


def _lerp_fills():
    texels = cs.rand_texels(np.random.default_rng(9), 5, 3)
    bitmap = lambda extend: dict({"type": "bitmap", "bitmap_id": 7, "repeating": extend == "repeat", "smoothed": True,
                                  "matrix": ps._at(6.5, 9.25, 12.3, 6.1, 0.3, -0.2)}, **({"pad": True} if extend == "pad" else {}))
    import spread_scenes as ss
    fills = {"bitmap_" + e: bitmap(e) for e in ps.EXTENDS}
    for spread in ("pad", "reflect", "repeat"):
        fills["radial_" + spread] = ss._fill("focal+", ss._matrix(22, 30.4, 20.7), ss.STOPS["translucent"], spread)
    return {7: (5, 3, texels.tobytes())}, fills


@needs_cairo
@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_the_lerp_bit_of_a_shaded_first_paint_is_libcairo(aliased):
    """A shaded style as the first paint of the frame and of a group, partial coverage all along its outline: the frame builder sets
    the lerp bit, the model states mul_un8(source, coverage) with the destination ignored -- 0x80 rounding, where a solid's span lerp
    rounds with 0x7f -- and libcairo, which goes through a mask and pixman's IN and OVER there, gives the same bytes."""
    raw, fills = _lerp_fills()
    for name, fill in sorted(fills.items()):
        for where in ("frame", "group"):
            kid = _tri(fill)
            kids = [kid] if where == "frame" else [_tri({"type": "solid", "color": scenarios._rgba(40, 90, 200, 130)}, 30.0),
                                                   {"type": "container", "layer": "multiply", "children": [kid]}]
            sc = dict(width=96, height=48, raw_bitmaps=raw, stage={"children": kids})
            arrays = build_on_host(sc, aliased)
            shaded = [int(p["lerp"]) for p in arrays[1] if int(p["kind"]) < cs.BEGIN and int(arrays[2][int(p["style"])].kind) != fm.STYLE_SOLID]
            assert shaded == [1], (name, where, shaded)
            got = fm.render(*arrays, 96, 48, aliased=aliased, bitmaps=bitmaps_of(sc))
            assert diff_stats(got, cs.cairo_render_shaded(sc, aliased)) == (0, 0), (name, where)
            if not aliased:
                cov = fm.path_coverage(arrays[0], [p for p in arrays[1] if int(p["lerp"]) == 1 and int(arrays[2][int(p["style"])].kind)][0], 96, 48)[1]
                assert ((cov > 0) & (cov < 255)).sum() > 40, (name, where)


def test_the_lerp_bit_with_a_shaded_style_needs_a_clear_destination():
    fr = cs.RawFrame(70, 13)
    fr.rect_tor(0, 0, 70, 13, 0x80402010, 1)
    cs.add_shaded_member(fr, np.random.default_rng(1), "bitmap_rim_pad", "normal", 0, 0, lerp=1)
    with pytest.raises(ValueError):
        fm.render(*fr.arrays(), 70, 13, bitmaps=fr.model_bitmaps())
    fr = cs.RawFrame(70, 13)
    fr.rect_tor(0, 0, 70, 13, 0x80402010, 1)
    fr.begin()
    cs.add_shaded_member(fr, np.random.default_rng(1), "bitmap_rim_pad", "normal", 0, 0, lerp=1)
    fr.end("screen")
    fm.render(*fr.arrays(), 70, 13, bitmaps=fr.model_bitmaps())          # (inside a group the surface is the group's: clear)


def test_the_model_refuses_linear_gradients_and_variant_textures():
    from swf_renderer_amd import api
    fr = cs.RawFrame(70, 13)
    cs.add_shaded_member(fr, np.random.default_rng(2), "bitmap_rim_none", "normal", 0, 0)
    e, p, s = fr.arrays()
    fm.render(e, p, s, 70, 13, bitmaps=fr.model_bitmaps())
    with pytest.raises(ValueError):
        fm.render(e, p, s, 70, 13)                                       # (no texels given)
    s[0].bitmap = api.VARIANT_BASE + 1
    with pytest.raises(NotImplementedError):
        fm.render(e, p, s, 70, 13, bitmaps=fr.model_bitmaps())
    s[0].kind = api.STYLE_LINEAR
    with pytest.raises(NotImplementedError):
        fm.render(e, p, s, 70, 13, bitmaps=fr.model_bitmaps())


def _scene_hash(sc):
    return hashlib.sha256(json.dumps(sc, sort_keys=True).encode()).hexdigest()[:16]


def _frame_hash(fr):
    e, p, s = fr.arrays()
    return hashlib.sha256(e.tobytes() + p.tobytes() + b"".join(bytes(st) for st in s)).hexdigest()[:16]


def test_the_solid_corpora_are_what_they_were():
    """rand_composited_scene without `shaded` and the RawFrame corpora of tests/test_composite_fuzz_gpu.py, by their hashes from before
    shaded leaves and per-path styles were added"""
    scenes = ((1000, {}), (5003, {}), (11007, {}), (5600, dict(width=150, height=90, leaves=14)), (2001, dict(min_children=200, leaves=30)))
    assert [_scene_hash(cs.rand_composited_scene(np.random.default_rng(seed), **kw)) for seed, kw in scenes] == \
        ["3fc6a003a2f330f0", "ed692b57d46c0594", "4f7709cf198a8fbc", "b97a4c0bbdce77bc", "6f35adb17d017d18"]
    frames = (cs.raw_group_sizes_frame(np.random.default_rng(6017), 17, 3), cs.raw_nesting_frame(2, 4), cs.raw_cover_frame("inside", "box"),
              cs.rand_raw_nested_frame(np.random.default_rng(6701), W=61, H=20, items=47), cs.raw_many_groups_frame(np.random.default_rng(6900), 260, 120, 300))
    assert [_frame_hash(fr) for fr in frames] == ["a0b2ca863ab6b499", "2b42849062f3eed1", "51b7ec63c8bbb3a7", "78f951eafa92b0ca", "1d393e32a316207f"]


def test_the_shaded_raw_frames_reach_what_they_claim():
    """the frames of tests/test_shaded_composite_fuzz_gpu.py: every branch of the bitmap fetch, the lerp bit, every operator and every
    setting, counted from the model's positions; every frame is accepted by swfr_upload_edges' checks (a host-only handle answers
    NO_DEVICE only behind them) and drawn by the model"""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    frames = [fr for cls in cs.SHADED_CLASSES for _, fr in cs.shaded_frames(cls)]
    assert len(frames) == len(cs.SHADED_CLASSES) * len(cs.SHADED_MODES) * len(cs.SHADED_SETTINGS)
    rc = cs.shaded_reach(frames)
    print("shaded raw frames:", len(frames), "reach", sorted(rc.items(), key=str))
    cs.assert_shaded_reach(rc)
    for seed in range(12):                                           # the last texel column reached, and nothing beyond: under each edge rule
        fr, columns, bw = cs.last_column_frame(seed)
        assert columns == {bw - 2, bw - 1}, (seed, columns, bw)
        assert cs.shaded_reach([fr]).get(("general", seed % 3), 0) >= 2, seed            # (both row halves of the strip: never `inside`)
    for seed in range(12):                                           # a clear rectangle in a painted strip
        fr = cs.lerp_beside_painted_frame(seed)
        fm.render(*fr.arrays(), fr.W, fr.H, bitmaps=fr.model_bitmaps())
    sizes = {(w, h) for fr in frames for w, h, _ in fr.bitmaps.values()}
    assert sizes >= set(cs.RAW_BITMAP_SIZES), sizes
    for fr in frames[::5]:
        r = S.Renderer(fr.W, fr.H, device=api.DEVICE_HOST_ONLY)
        try:
            for bid, (w, h, px) in fr.bitmaps.items():
                r.register_bitmap(bid, w, h, px)
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(*fr.arrays())
            assert ei.value.code == api.ERR_NO_DEVICE, ei.value
        finally:
            r.close()
