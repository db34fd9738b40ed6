"""Unsmoothed bitmap fills on the host side (no GPU, host-only handles): swfr_fill_style::filter and swfr_style::filter in the structs'
tail padding; what an absent, "good" or zero filter builds (what was always built: the arrays of every bitmap scene of the scenario
corpus); a nearest fill that repeats or pads differs from the good one in swfr_style::filter alone; an EXTEND_NONE nearest fill is cut
to tests/nearest_model.py's rectangle, on the matrices of DESIGN.md's measured table; the refusals (UnknownBitmapFilter, a bad style at
upload); the fills that ignore the field; swfr_shape_json's keys."""
import ctypes as C
import json

import numpy as np
import pytest

import host_frames as hf
import nearest_model as nm
import nearest_scenes as ns
import scenarios
import spread_model as sm
from scenarios import _m, _poly_shape, _rgba

BID = 13                                                         # tests/pad_scenes.py: 3 x 5 texels
SHAPE = [(0, 0), (64, 0), (64, 48), (0, 48)]                     # the host handle's whole frame


def _bitmap_fill(**kw):
    return dict({"type": "bitmap", "bitmap_id": BID, "repeating": False, "smoothed": False, "matrix": _m(20 * 4, 20 * 4, 200, 80)}, **kw)


def _stage(fill):
    return {"children": [{"type": "shape", "definition": _poly_shape([(20 * x, 20 * y) for x, y in SHAPE], fill)}]}


def _host():
    r = hf.host()
    for b in ns.BITMAPS:
        r.add_bitmap(b)
    return r


def test_the_fields_lie_in_the_tail_padding():
    from swf_renderer_amd import api
    F, S = api.FillStyle, api.Style
    assert api.load_library().swfr_abi_version() == 1
    assert C.sizeof(F) == 64 and C.alignment(F) == 8
    assert [(n, getattr(F, n).offset) for n in ("bitmap_id", "repeating", "smoothed", "spread", "pad", "filter")] == \
        [("bitmap_id", 52), ("repeating", 56), ("smoothed", 57), ("spread", 58), ("pad", 59), ("filter", 60)]
    assert F.filter.size == 1
    assert C.sizeof(api.LineStyle) == 72 and api.LineStyle.fill.offset == 8
    assert C.sizeof(S) == 440 and S.extend.offset == 432 and S.filter.offset == 436 and S.filter.size == 4


def test_an_absent_good_or_zero_filter_builds_what_was_built():
    """every bitmap scene of the scenario corpus: the key absent, "good" and 0 give the same arrays, and no style carries a filter"""
    from swf_renderer_amd import api
    n = 0
    for name, sc in sorted(scenarios.scenarios().items()):
        if not sc.get("bitmaps"):
            continue
        for aliased in (False, True):
            a = hf.build_on_host(sc, aliased)
            assert all(st.filter == 0 for st in a[2]), name
            assert any(st.kind == api.STYLE_BITMAP for st in a[2]), name
            for value in ("good", 0):
                b = hf.build_on_host(dict(sc, stage=ns.with_filter(sc["stage"], value)), aliased)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
                assert len(a[2]) == len(b[2]) and all(bytes(x) == bytes(y) for x, y in zip(a[2], b[2])), name
        n += 1
    assert n >= 5
    arena = api._Arena()
    fills = ({}, {"filter": "good"}, {"filter": 0}, {"filter": "nearest"}, {"filter": "NEAREST"}, {"filter": 1}, {"filter": 7})
    assert [api._fill(arena, _bitmap_fill(**kw)).filter for kw in fills] == [0, 0, 0, 1, 1, 1, 7]
    for bad in ("bilinear", True, -1, 256, 1.0):
        with pytest.raises(api.SwfrError) as ei:
            api._fill(arena, _bitmap_fill(filter=bad))
        assert ei.value.code == api.ERR_INVALID and "UnknownBitmapFilter" in str(ei.value)


def test_smoothed_is_still_ignored():
    r = _host()
    try:
        built = [r.build_frame(_stage(_bitmap_fill(smoothed=v))) for v in (False, True)]
        assert built[0][0].tobytes() == built[1][0].tobytes() and built[0][1].tobytes() == built[1][1].tobytes()
        assert [bytes(s) for s in built[0][2]] == [bytes(s) for s in built[1][2]] and all(s.filter == 0 for s in built[0][2])
    finally:
        r.close()


@pytest.mark.parametrize("extend", ["repeat", "pad"])
def test_an_unbounded_nearest_fill_differs_in_the_filter_alone(extend):
    """for the scenario corpus' bitmap scenes and for every scene of tests/nearest_scenes.py: with "repeating" or "pad" the arrays of the
    nearest and of the good fill are the same bar swfr_style::filter of the bitmap styles"""
    from swf_renderer_amd import api
    corpus = {k: v for k, v in scenarios.scenarios().items() if v.get("bitmaps")}
    n = 0
    for name, sc in sorted(dict(corpus, **ns.all_scenes()).items()):
        stage = ns.with_extend(sc["stage"], extend)
        a = hf.build_on_host(dict(sc, stage=ns.with_filter(stage, "good")))
        b = hf.build_on_host(dict(sc, stage=ns.with_filter(stage, "nearest")))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
        assert len(a[2]) == len(b[2])
        for x, y in zip(a[2], b[2]):
            assert x.filter == 0 and y.filter == (1 if y.kind == api.STYLE_BITMAP else 0), name
            n += y.filter
            y.filter = 0
            assert bytes(x) == bytes(y), name
    assert n >= 40


TABLE = [  # k, off, GOOD, NEAREST: a 5 x 4 bitmap with device = k * texel + off (tests/test_nearest_model.py holds both against libcairo)
    (3, 10.3, (9, 9, 27, 24), (10, 10, 25, 22)),
    (3, 10.5, (9, 9, 27, 24), (10, 10, 26, 23)),
    (0.5, 10.3, (10, 10, 13, 13), (10, 10, 13, 12)),
    (1, 10.3, (10, 10, 16, 15), (10, 10, 15, 14)),
    (7.3, 4.9, (1, 1, 45, 38), (5, 5, 41, 34)),
]


@pytest.mark.parametrize("k,off,good,nearest", TABLE)
def test_the_path_rectangle_of_an_extend_none_fill_is_the_model_s_cut(k, off, good, nearest):
    from swf_renderer_amd import api
    matrix = _m(20 * k, 20 * k, round(20 * off), round(20 * off))
    assert matrix["scale_x"] == 20 * k * 65536 and matrix["translate_x"] == 20 * off        # (the table's matrices are exact in the format)
    r = hf.host()
    try:
        r.register_bitmap(5, 5, 4, bytes([255]) * (5 * 4 * 4))
        for name, want in (("nearest", nearest), ("good", good), (None, good)):
            fill = {"type": "bitmap", "bitmap_id": 5, "repeating": False, "smoothed": False, "matrix": matrix}
            if name:
                fill["filter"] = name
            e, p, s = r.build_frame(_stage(fill))
            assert len(p) == 1 and s[p["style"][0]].kind == api.STYLE_BITMAP and s[p["style"][0]].filter == (name == "nearest")
            assert hf.rects(p) == [want], (name, hf.rects(p))
            assert nm.cut_rect(sm.pattern_matrix([matrix]), 5, 4, nearest=name == "nearest") == want
    finally:
        r.close()


def test_the_cut_on_random_matrices_is_the_model_s():
    """rotated and skewed too: the frame builder's rectangle for a frame-filling shape is the model's cut within the frame"""
    rng = np.random.default_rng(60)
    r = hf.host(64, 48)
    seen = 0
    try:
        r.register_bitmap(5, 5, 4, bytes([255]) * (5 * 4 * 4))
        for it in range(120):
            kx, ky = float(rng.uniform(0.3, 9.0)), float(rng.uniform(0.3, 9.0))
            t = float(rng.uniform(-3.2, 3.2)) if it % 3 else 0.0
            matrix = _m(20 * kx * np.cos(t), 20 * ky * np.cos(t), int(rng.integers(0, 60 * 20)), int(rng.integers(0, 40 * 20)), 20 * kx * np.sin(t), -20 * ky * np.sin(t))
            fill = {"type": "bitmap", "bitmap_id": 5, "repeating": False, "smoothed": False, "matrix": matrix, "filter": "nearest"}
            want = nm.intersect((0, 0, 64, 48), nm.cut_rect(sm.pattern_matrix([matrix]), 5, 4))
            _, p, _ = r.build_frame(_stage(fill))
            assert hf.rects(p) == ([want] if want else []), (it, matrix)
            seen += want is not None
    finally:
        r.close()
    assert seen >= 100


def test_refusals():
    from swf_renderer_amd import api
    r = _host()
    try:
        for flt in (2, 255):                                         # (no name gives a filter above 1: a number, or set on the struct)
            with pytest.raises(api.SwfrError) as ei:
                r.build_frame(_stage(_bitmap_fill(filter=flt)))
            assert ei.value.code == api.ERR_INVALID and "UnknownBitmapFilter" in str(ei.value)
            for repeating, pad in ((0, 0), (1, 0), (0, 1)):
                arena = api._Arena()
                d = api._define_shape(arena, _stage(_bitmap_fill())["children"][0]["definition"])
                f = d.initial_styles.fill[0]
                f.filter, f.repeating, f.pad = flt, repeating, pad
                out = C.c_uint32()
                assert r.L.swfr_register_shape(r.h, C.byref(d), C.byref(out)) == api.ERR_INVALID, (flt, repeating, pad)
                assert "UnknownBitmapFilter" in r.L.swfr_last_error(r.h).decode(), (flt, repeating, pad)
        # a bad style at upload, on a host-only handle too: refused as invalid before the handle says it has no device
        e, p, s = r.build_frame(_stage(_bitmap_fill(filter="nearest")))
        k = int(p["style"][0])
        assert s[k].kind == api.STYLE_BITMAP and s[k].filter == 1
        with pytest.raises(api.SwfrError) as ei:
            r.upload_edges(e, p, s)
        assert ei.value.code == api.ERR_NO_DEVICE
        for flt in (2, 255, 2 ** 31):
            s[k].filter = flt
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, p, s)
            assert ei.value.code == api.ERR_INVALID and "filter" in str(ei.value), flt
        # a line style's bitmap fill and a morph shape's stay refused as they were
        line = _poly_shape([(0, 0), (600, 0), (600, 400)], None, line=_rgba(0, 0, 0), line_width=40)
        line["shape"]["initial_styles"]["line"][0]["fill"] = _bitmap_fill(filter="nearest")
        with pytest.raises(api.SwfrError) as ei:
            r.build_frame({"children": [{"type": "shape", "definition": line}]})
        assert ei.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedLineStyle" in str(ei.value)
    finally:
        r.close()


def test_solid_and_gradient_fills_and_styles_ignore_the_field():
    from swf_renderer_amd import api
    grad = {"type": "radial-gradient", "matrix": _m(0.01, 0.01, 300, 200),
            "gradient": {"color_space": "s-rgb", "colors": [{"ratio": 0, "color": _rgba(255, 0, 0)}, {"ratio": 255, "color": _rgba(0, 0, 255)}]}}
    r = _host()
    try:
        for fill, kind in (({"type": "solid", "color": _rgba(9, 9, 9, 100)}, api.STYLE_SOLID), (grad, api.STYLE_RADIAL)):
            built = []
            for flt in (0, 1, 9):                                    # (no key reaches a solid or a gradient through the JSON)
                arena = api._Arena()
                d = api._define_shape(arena, _stage(fill)["children"][0]["definition"])
                d.initial_styles.fill[0].filter = flt
                out = C.c_uint32()
                assert r.L.swfr_register_shape(r.h, C.byref(d), C.byref(out)) == api.OK, (kind, flt)
                e, p, s = r.build_frame({"children": [{"type": "shape", "id": out.value}]})
                assert len(p) == 1 and s[p["style"][0]].kind == kind and s[p["style"][0]].filter == 0
                built.append((e.tobytes(), p.tobytes(), bytes(s[p["style"][0]])))
            assert built[0] == built[1] == built[2]
            # the low-level scene: a filter on a style that is no bitmap's is not looked at (the handle has no device: that is all it says)
            s[p["style"][0]].filter = 77
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, p, s)
            assert ei.value.code == api.ERR_NO_DEVICE, kind
    finally:
        r.close()


def test_shape_json_has_no_new_key():
    """swfr_shape_json is held against the reference's decode goldens: a nearest fill prints as the good one does"""
    r = _host()
    try:
        texts = []
        for fill in (_bitmap_fill(), _bitmap_fill(filter="nearest")):
            sid = r.register_shape(_stage(fill)["children"][0]["definition"])
            texts.append(r.shape_json(sid))
        assert texts[0] == texts[1] and "filter" not in texts[1]
        fills = [p["fill"] for p in json.loads(texts[1])["paths"] if "fill" in p]
        assert fills and all(sorted(f) == sorted(["type", "bitmapId", "matrix", "repeating", "smoothed"]) for f in fills), fills
    finally:
        r.close()
