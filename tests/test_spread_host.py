"""Gradient spread modes on the host side (no GPU, host-only handles): swfr_fill_style::spread in the struct's tail padding, the
spellings of fill["gradient"]["spread"], swfr_style::extend in swfr_build_frame's styles, "pad" byte for byte what an absent key
builds, and the refusals -- an unknown spread, an extend a gradient style cannot have at swfr_upload_edges, and a LINEAR gradient with
a spread other than pad (NotImplementedGradientSpread: refused, never approximated)."""
import ctypes as C

import numpy as np
import pytest

import host_frames as hf
import spread_scenes as ss
from scenarios import _m, _poly_shape, _rgba

BOX = [(0, 0), (600, 0), (600, 400), (0, 400)]
EXTEND = {"pad": 0, "repeat": 1, "reflect": 2}               # swfr_style::extend (bitmaps: 1 repeat, too)


def _fill(kind, spread=None, **kw):
    g = {"color_space": "s-rgb", "colors": [{"ratio": 0, "color": _rgba(255, 0, 0)}, {"ratio": 255, "color": _rgba(0, 0, 255)}]}
    if spread is not None:
        g["spread"] = spread
    return dict({"type": kind, "matrix": _m(0.01, 0.01, 300, 200), "gradient": g}, **kw)


def _stage(fill):
    return {"children": [{"type": "shape", "definition": _poly_shape(BOX, fill)}]}


def test_the_field_lies_in_the_tail_padding():
    from swf_renderer_amd import api
    F = api.FillStyle
    assert api.load_library().swfr_abi_version() == 1
    assert C.sizeof(F) == 64 and C.alignment(F) == 8
    assert [(n, getattr(F, n).offset) for n in ("type", "color", "morph_color", "matrix", "n_stops", "stops", "focal_point", "bitmap_id", "repeating",
                                                "smoothed", "spread")] == \
        [("type", 0), ("color", 4), ("morph_color", 8), ("matrix", 12), ("n_stops", 36), ("stops", 40), ("focal_point", 48), ("bitmap_id", 52),
         ("repeating", 56), ("smoothed", 57), ("spread", 58)]
    assert C.sizeof(api.LineStyle) == 72 and api.LineStyle.fill.offset == 8


@pytest.mark.parametrize("kind", ["radial-gradient", "focal-gradient"])
def test_spellings_and_extend(kind):
    from swf_renderer_amd import api
    kw = {"focal_point": {"epsilons": 100}} if kind == "focal-gradient" else {}
    r = hf.host()
    try:
        for spread, want in ((None, "pad"), ("pad", "pad"), ("reflect", "reflect"), ("repeat", "repeat"), ("Reflect", "reflect"), ("REPEAT", "repeat"),
                             (0, "pad"), (1, "reflect"), (2, "repeat")):
            _, p, s = r.build_frame(_stage(_fill(kind, spread, **kw)))
            assert len(p) == 1 and s[p["style"][0]].kind == api.STYLE_RADIAL
            assert s[p["style"][0]].extend == EXTEND[want], (spread, want)
        arena = api._Arena()
        assert [api._fill(arena, _fill(kind, sp, **kw)).spread for sp in (None, "pad", "reflect", "repeat", 0, 1, 2, 7)] == [0, 0, 1, 2, 0, 1, 2, 7]
    finally:
        r.close()


def test_solid_and_bitmap_fills_ignore_the_field():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        arena = api._Arena()
        d = api._define_shape(arena, _poly_shape(BOX, {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
        d.initial_styles.fill[0].spread = 9                          # (no key reaches it through the JSON: set on the struct)
        out = C.c_uint32()
        assert r.L.swfr_register_shape(r.h, C.byref(d), C.byref(out)) == api.OK
        _, p, s = r.build_frame({"children": [{"type": "shape", "id": out.value}]})
        assert len(p) == 1 and s[p["style"][0]].kind == api.STYLE_SOLID
    finally:
        r.close()


def test_pad_builds_what_an_absent_key_builds():
    """every padded scene of the spread files, the scenario corpus's gradients among them by way of tests/scenarios.py's "spread": "pad" """
    def without(obj):
        if isinstance(obj, list):
            return [without(o) for o in obj]
        if isinstance(obj, dict):
            return {k: without(v) for k, v in obj.items() if not (k == "spread" and "colors" in obj)}
        return obj
    n = 0
    for name, sc in sorted(ss.all_scenes("pad").items()):
        if any(k in name for k in ("blend_mode", "layer", "mask", "opacity", "cxform")):
            continue                                                 # (one plain scene per geometry is enough here)
        for aliased in (False, True):
            a, b = hf.build_on_host(sc, aliased), hf.build_on_host(dict(sc, stage=without(sc["stage"])), aliased)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
            assert len(a[2]) == len(b[2]) and all(bytes(x) == bytes(y) for x, y in zip(a[2], b[2])), name
            assert all(st.extend == 0 for st in a[2]), name
            n += 1
    assert n >= 40


def test_spread_reaches_every_gradient_of_a_scene():
    """under a colour transform, a blend mode, a layer, a mask and an opacity the style still carries the extend; the padded gradient
    beside a spread one keeps 0"""
    from swf_renderer_amd import api
    for spread in ss.SPREADS:
        for name, sc in sorted(ss.structure_scenes(spread).items()):
            _, p, s = hf.build_on_host(sc)
            got = sorted(st.extend for st in s if st.kind in (api.STYLE_RADIAL, api.STYLE_LINEAR))
            want = {"beside_pad": [0, EXTEND[spread]], "linear_pad": [0]}.get(name, [EXTEND[spread]])
            assert got == want, (spread, name, got)


def test_refusals():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        for bad in ("mirror", "", 2.0, True, -1, 256, [1]):
            with pytest.raises(api.SwfrError) as ei:
                r.build_frame(_stage(_fill("radial-gradient", bad)))
            assert ei.value.code == api.ERR_INVALID and "UnknownGradientSpread" in str(ei.value), bad
        for kind in ("radial-gradient", "focal-gradient", "linear-gradient"):
            for bad in (3, 4, 255):                                  # the library's own check
                with pytest.raises(api.SwfrError) as ei:
                    r.build_frame(_stage(_fill(kind, bad)))
                assert ei.value.code == api.ERR_INVALID and "UnknownGradientSpread" in str(ei.value), (kind, bad)
        # a linear gradient is the float64 extension: with a spread it is refused, padded it builds as ever
        for spread in ("reflect", "repeat", 1, 2):
            with pytest.raises(api.SwfrError) as ei:
                r.build_frame(_stage(_fill("linear-gradient", spread)))
            assert ei.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedGradientSpread" in str(ei.value), spread
        e, p, s = r.build_frame(_stage(_fill("linear-gradient", "pad")))
        assert s[p["style"][0]].kind == api.STYLE_LINEAR and s[p["style"][0]].extend == 0
        # line-style fills stay refused as they were
        line = _poly_shape(BOX, None, line=_rgba(0, 0, 0), line_width=40)
        line["shape"]["initial_styles"]["line"][0]["fill"] = _fill("radial-gradient", "reflect")
        with pytest.raises(api.SwfrError) as ei:
            r.build_frame({"children": [{"type": "shape", "definition": line}]})
        assert ei.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedLineStyle" in str(ei.value)
    finally:
        r.close()


def test_upload_refuses_an_extend_a_gradient_cannot_have():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        for kind in ("radial-gradient", "linear-gradient"):
            e, p, s = r.build_frame(_stage(_fill(kind, "pad")))
            i = int(p["style"][0])

            def refused(extend, code):
                s[i].extend = extend
                with pytest.raises(api.SwfrError) as ei:
                    r.upload_edges(e, p, s)
                assert ei.value.code == code, (kind, extend, ei.value)
                return str(ei.value)
            refused(0, api.ERR_NO_DEVICE)                            # the well-formed scene: a host-only handle cannot rasterize
            for extend in (3, 4, 0xffffffff):
                refused(extend, api.ERR_INVALID)
            for extend in (1, 2):
                if kind == "linear-gradient":
                    assert "NotImplementedGradientSpread" in refused(extend, api.ERR_NOT_IMPLEMENTED)
                else:
                    refused(extend, api.ERR_NO_DEVICE)
    finally:
        r.close()
