"""Padded bitmap fills on the host side (no GPU, host-only handles): swfr_fill_style::pad in the struct's tail padding, what an absent
or zero "pad" builds (what it built before: the arrays of every bitmap scene of the scenario corpus), swfr_style::extend == 2 and the
shape's own rectangle for a padded fill, the refusals (InvalidBitmapPad), the fills that ignore the field, and swfr_shape_json's keys."""
import ctypes as C
import json

import pytest

import host_frames as hf
import pad_scenes as ps
import scenarios
from scenarios import _m, _poly_shape, _rgba

BID = 13                                                         # tests/pad_scenes.py: 3 x 5 texels
BW, BH = ps.SIZES[BID]
K = 4                                                            # pixels per texel: the bitmap covers 12 x 20 pixels at (10, 4)
SHAPE = [(10, 4), (10 + 2 * K * BW, 4), (10 + 2 * K * BW, 4 + 2 * K * BH), (10, 4 + 2 * K * BH)]      # twice the bitmap's size


def _bitmap_fill(**kw):
    return dict({"type": "bitmap", "bitmap_id": BID, "repeating": False, "smoothed": True, "matrix": _m(20 * K, 20 * K, 200, 80)}, **kw)


def _stage(fill):
    return {"children": [{"type": "shape", "definition": _poly_shape([(20 * x, 20 * y) for x, y in SHAPE], fill)}]}


def _host():
    r = hf.host()
    for b in ps.BITMAPS:
        r.add_bitmap(b)
    return r


def test_the_field_lies_in_the_tail_padding():
    from swf_renderer_amd import api
    F = api.FillStyle
    assert api.load_library().swfr_abi_version() == 1
    assert C.sizeof(F) == 64 and C.alignment(F) == 8
    assert [(n, getattr(F, n).offset) for n in ("bitmap_id", "repeating", "smoothed", "spread", "pad")] == \
        [("bitmap_id", 52), ("repeating", 56), ("smoothed", 57), ("spread", 58), ("pad", 59)]
    assert C.sizeof(api.LineStyle) == 72 and api.LineStyle.fill.offset == 8


def test_an_absent_or_zero_pad_builds_what_it_built():
    """every bitmap scene of the scenario corpus: the key absent, False and 0 give the same arrays, and the styles' extend is what
    "repeating" says"""
    from swf_renderer_amd import api

    def with_pad(obj, value):
        if isinstance(obj, list):
            return [with_pad(o, value) for o in obj]
        if isinstance(obj, dict):
            out = {k: with_pad(v, value) for k, v in obj.items()}
            if out.get("type") == "bitmap":
                out["pad"] = value
            return out
        return obj
    n = 0
    for name, sc in sorted(scenarios.scenarios().items()):
        if not sc.get("bitmaps"):
            continue
        for aliased in (False, True):
            a = hf.build_on_host(sc, aliased)
            assert all(st.extend in (0, 1) for st in a[2] if st.kind == api.STYLE_BITMAP), name
            for value in (False, 0):
                b = hf.build_on_host(dict(sc, stage=with_pad(sc["stage"], value)), aliased)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
                assert len(a[2]) == len(b[2]) and all(bytes(x) == bytes(y) for x, y in zip(a[2], b[2])), name
        n += 1
    assert n >= 5
    arena = api._Arena()
    assert [api._fill(arena, _bitmap_fill(**kw)).pad for kw in ({}, {"pad": False}, {"pad": 0}, {"pad": True}, {"pad": 1}, {"pad": 7})] == [0, 0, 0, 1, 1, 1]


def test_a_padded_style_has_extend_2_and_the_shape_s_rectangle():
    """the unpadded fill is cut to the bitmap's rectangle (12 x 20 pixels at (10, 4), and half a texel -- 2 pixels -- more on the axes the
    filter magnifies); the padded one, like a repeating one, keeps the shape's (24 x 40)"""
    from swf_renderer_amd import api
    r = _host()
    try:
        want = {"none": (0, (10, 4, 10 + K * BW + K // 2, 4 + K * BH + K // 2)), "repeat": (1, (10, 4, 10 + 2 * K * BW, 4 + 2 * K * BH)), "pad": (2, (10, 4, 10 + 2 * K * BW, 4 + 2 * K * BH))}
        built = {}
        for extend, (number, rect) in want.items():
            e, p, s = r.build_frame(ps.with_extend(_stage(_bitmap_fill()), extend))
            assert len(p) == 1 and s[p["style"][0]].kind == api.STYLE_BITMAP
            assert s[p["style"][0]].extend == number, extend
            assert hf.rects(p) == [rect], extend
            built[extend] = (e, p, s)
        # everything but the extend is the repeating fill's: the polygon, the box / tor decision, the lerp flag
        (e1, p1, s1), (e2, p2, s2) = built["repeat"], built["pad"]
        assert e1.tobytes() == e2.tobytes() and p1.tobytes() == p2.tobytes()
        s2[p2["style"][0]].extend = 1
        assert bytes(s1[p1["style"][0]]) == bytes(s2[p2["style"][0]])
    finally:
        r.close()


def test_pad_reaches_every_bitmap_fill_of_a_scene():
    from swf_renderer_amd import api
    for name, sc in sorted(ps.all_scenes().items()):
        _, p, s = hf.build_on_host(sc)
        got = sorted(st.extend for st in s if st.kind == api.STYLE_BITMAP)
        assert got == ([0, 1, 2] if name.startswith("together") else [2] * len(got)) and got, (name, got)


def test_refusals():
    from swf_renderer_amd import api
    r = _host()
    try:
        for fill in (_bitmap_fill(pad=True, repeating=True), _bitmap_fill(pad=1, repeating=1)):
            with pytest.raises(api.SwfrError) as ei:
                r.build_frame(_stage(fill))
            assert ei.value.code == api.ERR_INVALID and "InvalidBitmapPad" in str(ei.value)
        for pad, repeating in ((2, 0), (255, 0), (2, 1), (1, 1), (1, 255)):            # (no key gives pad > 1 through the JSON: set on the struct)
            arena = api._Arena()
            d = api._define_shape(arena, _stage(_bitmap_fill())["children"][0]["definition"])
            d.initial_styles.fill[0].pad, d.initial_styles.fill[0].repeating = pad, repeating
            out = C.c_uint32()
            assert r.L.swfr_register_shape(r.h, C.byref(d), C.byref(out)) == api.ERR_INVALID, (pad, repeating)
            assert "InvalidBitmapPad" in r.L.swfr_last_error(r.h).decode(), (pad, repeating)
        # a line style's bitmap fill stays refused as it was
        line = _poly_shape([(0, 0), (600, 0), (600, 400)], None, line=_rgba(0, 0, 0), line_width=40)
        line["shape"]["initial_styles"]["line"][0]["fill"] = _bitmap_fill(pad=True)
        with pytest.raises(api.SwfrError) as ei:
            r.build_frame({"children": [{"type": "shape", "definition": line}]})
        assert ei.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedLineStyle" in str(ei.value)
    finally:
        r.close()


def test_solid_and_gradient_fills_ignore_the_field():
    from swf_renderer_amd import api
    grad = {"type": "radial-gradient", "matrix": _m(0.01, 0.01, 300, 200),
            "gradient": {"color_space": "s-rgb", "colors": [{"ratio": 0, "color": _rgba(255, 0, 0)}, {"ratio": 255, "color": _rgba(0, 0, 255)}]}}
    r = _host()
    try:
        for fill, kind in (({"type": "solid", "color": _rgba(9, 9, 9, 100)}, api.STYLE_SOLID), (grad, api.STYLE_RADIAL)):
            built = []
            for pad, repeating in ((0, 0), (9, 0), (1, 1)):                            # (no key reaches a solid or a gradient through the JSON)
                arena = api._Arena()
                d = api._define_shape(arena, _stage(fill)["children"][0]["definition"])
                d.initial_styles.fill[0].pad, d.initial_styles.fill[0].repeating = pad, repeating
                out = C.c_uint32()
                assert r.L.swfr_register_shape(r.h, C.byref(d), C.byref(out)) == api.OK, (kind, pad)
                e, p, s = r.build_frame({"children": [{"type": "shape", "id": out.value}]})
                assert len(p) == 1 and s[p["style"][0]].kind == kind and s[p["style"][0]].extend == 0
                built.append((e.tobytes(), p.tobytes(), bytes(s[p["style"][0]])))
            assert built[0] == built[1] == built[2]
    finally:
        r.close()


def test_shape_json_has_no_new_key():
    """swfr_shape_json is held against the reference's decode goldens: a padded fill prints as the unpadded one does"""
    r = _host()
    try:
        texts = []
        for fill in (_bitmap_fill(), _bitmap_fill(pad=True)):
            sid = r.register_shape(_stage(fill)["children"][0]["definition"])
            texts.append(r.shape_json(sid))
        assert texts[0] == texts[1] and "pad" not in texts[1]
        fills = [p["fill"] for p in json.loads(texts[1])["paths"] if "fill" in p]
        assert fills and all(sorted(f) == sorted(["type", "bitmapId", "matrix", "repeating", "smoothed"]) for f in fills), fills
    finally:
        r.close()
