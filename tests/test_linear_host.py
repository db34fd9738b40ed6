"""Pixman-exact linear gradients on the host side (no GPU, host-only handles): without SWFR_FLAG_LINEAR_PIXMAN every array and every
refusal is what it was; with it a linear gradient fill becomes a SWFR_STYLE_LINEAR_PIXMAN style with the spread's extend; and what
swfr_create and swfr_upload_edges refuse by name -- kind 5, c0 == c1, an aliased handle, a rectilinear path of several boxes, a
rectangle outside pixman's range, a row step between 0 and one 16.16 unit.  Struct sizes, offsets and the ABI version are unchanged."""
import ctypes as C

import pytest

import host_frames as hf
import linear_scenes as ls
from scenarios import _m, _poly_shape, _rgba

EXTEND = {"pad": 0, "repeat": 1, "reflect": 2}


def _stage(matrix, spread, pts=((0, 0), (600, 0), (600, 400), (0, 400))):
    g = {"spread": spread, "color_space": "s-rgb", "colors": [{"ratio": 0, "color": _rgba(255, 0, 0)}, {"ratio": 255, "color": _rgba(0, 0, 255)}]}
    return {"children": [{"type": "shape", "definition": _poly_shape(list(pts), {"type": "linear-gradient", "matrix": matrix, "gradient": g})}]}


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[2]) == len(b[2]) and all(bytes(x) == bytes(y) for x, y in zip(a[2], b[2]))


def test_the_interface():
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    assert api.FLAG_LINEAR_PIXMAN == 8 and api.STYLE_LINEAR_PIXMAN == 4 and api.LINEAR_MODES == ("float64", "pixman")
    for bad in ("x", "", None, 1, "PIXMAN"):
        with pytest.raises(ValueError):
            S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY, linear=bad)
    r = S.Renderer(8, 8, device=api.DEVICE_HOST_ONLY)
    assert r.linear == "float64"
    r.close()


def test_sizes_and_offsets_are_unchanged():
    from swf_renderer_amd import api
    assert api.load_library().swfr_abi_version() == 1
    assert C.sizeof(api.Style) == 440 and api.Style.extend.offset == 432 and api.Style.filter.offset == 436 and api.Style.c0x.offset == 56
    assert C.sizeof(api.FillStyle) == 64 and api.FillStyle.spread.offset == 58
    assert C.sizeof(api.Config) == 16


def test_without_the_flag_nothing_changes():
    """the arrays of every padded linear scene from a default handle and from a linear="float64" one are the same bytes, the style is
    the float64 extension's, and reflect / repeat are refused as before"""
    from swf_renderer_amd import api
    n = 0
    for name, sc in sorted(ls.all_scenes("pad").items()):
        a = hf.build_on_host(sc)
        r = hf.host(sc["width"], sc["height"], linear="float64")
        try:
            b = r.build_frame(sc["stage"])
        finally:
            r.close()
        assert _same(a, b), name
        kinds = [st.kind for st in a[2]]
        assert api.STYLE_LINEAR in kinds and api.STYLE_LINEAR_PIXMAN not in kinds, name
        n += 1
    assert n >= 19
    for spread in ("reflect", "repeat"):
        for name, sc in sorted(ls.all_scenes(spread).items()):
            with pytest.raises(api.SwfrError) as ei:
                hf.build_on_host(sc)
            assert ei.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedGradientSpread" in str(ei.value), (spread, name)


def test_with_the_flag_every_spread_builds_a_pixman_style():
    """kind 4, the extend of the spread, the line (-16384, 0)-(16384, 0), and everything else of the frame as the float64 handle builds
    it: the same edges and paths, and the same styles bar kind and extend"""
    from swf_renderer_amd import api
    for spread in ls.SPREADS:
        for name, sc in sorted(ls.all_scenes(spread).items()):
            r = hf.host(sc["width"], sc["height"], linear="pixman")
            try:
                e, p, s = r.build_frame(sc["stage"])
            finally:
                r.close()
            lin = [st for st in s if st.kind == api.STYLE_LINEAR_PIXMAN]
            assert len(lin) == 1 and not any(st.kind == api.STYLE_LINEAR for st in s), (spread, name)
            assert lin[0].extend == EXTEND[spread] and (lin[0].c0x, lin[0].c0y, lin[0].c1x, lin[0].c1y) == (-16384.0, 0.0, 16384.0, 0.0)
            e0, p0, s0 = hf.build_on_host(ls.all_scenes("pad")[name])
            assert e.tobytes() == e0.tobytes() and p.tobytes() == p0.tobytes() and len(s) == len(s0), (spread, name)
            for x, y in zip(s, s0):
                if x.kind == api.STYLE_LINEAR_PIXMAN:
                    x.kind, x.extend = api.STYLE_LINEAR, 0
                assert bytes(x) == bytes(y), (spread, name)


def _built(spread="reflect", matrix=None, pts=((0, 0), (600, 0), (600, 400), (0, 400)), w=64, h=48):
    r = hf.host(w, h, linear="pixman")
    e, p, s = r.build_frame(_stage(matrix or _m(0.01, 0.01, 300, 200), spread, pts))
    return r, e, p, s


def _refused(r, e, p, s, code, text):
    from swf_renderer_amd import api
    with pytest.raises(api.SwfrError) as ei:
        r.upload_edges(e, p, s)
    assert ei.value.code == code and text in str(ei.value), ei.value


def test_upload_accepts_kind_4_and_refuses_kind_5_and_a_point():
    from swf_renderer_amd import api
    r, e, p, s = _built()
    try:
        i = int(p["style"][0])
        assert s[i].kind == 4
        _refused(r, e, p, s, api.ERR_NO_DEVICE, "host-only")         # well-formed: only the missing device stands in the way
        for extend in (0, 1, 2):
            s[i].extend = extend
            _refused(r, e, p, s, api.ERR_NO_DEVICE, "host-only")
        s[i].extend = 3
        _refused(r, e, p, s, api.ERR_INVALID, "extend")
        s[i].extend = 2
        for kind in (5, 6, 255):
            s[i].kind = kind
            _refused(r, e, p, s, api.ERR_INVALID, "unknown style kind")
        s[i].kind = 4
        s[i].c1x, s[i].c1y = s[i].c0x, s[i].c0y
        _refused(r, e, p, s, api.ERR_INVALID, "c0 == c1")
        s[i].c1x = 16384.0
        for line in ((-300.0, 0.0, 300.0, 0.0), (-16384.0, 0.0, 16384.0, 1.0), (16384.0, 0.0, -16384.0, 0.0)):     # only a SWF fill's line is drawn
            s[i].c0x, s[i].c0y, s[i].c1x, s[i].c1y = line
            _refused(r, e, p, s, api.ERR_NOT_IMPLEMENTED, "NotImplementedLinearLine")
        s[i].c0x, s[i].c0y, s[i].c1x, s[i].c1y = -16384.0, 0.0, 16384.0, 0.0
        _refused(r, e, p, s, api.ERR_NO_DEVICE, "host-only")
        s[i].kind, s[i].extend = api.STYLE_LINEAR, 2                 # kind 2 stays the float64 model and keeps refusing a spread
        _refused(r, e, p, s, api.ERR_NOT_IMPLEMENTED, "NotImplementedGradientSpread")
    finally:
        r.close()


def test_aliased_is_refused_at_create_and_at_upload():
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    with pytest.raises(api.SwfrError) as ei:
        S.Renderer(16, 16, device=api.DEVICE_HOST_ONLY, antialias="none", linear="pixman")
    assert ei.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedAliasedPixmanLinear" in str(ei.value)
    r, e, p, s = _built()
    r.close()
    a = hf.host(64, 48, antialias="none")
    try:
        _refused(a, e, p, s, api.ERR_NOT_IMPLEMENTED, "NotImplementedAliasedPixmanLinear")
    finally:
        a.close()


def test_pieces_range_and_row_step_are_refused_by_name():
    from swf_renderer_amd import api
    # a rectilinear outline of two boxes on whole pixels: libcairo composites box by box, each box starting the ramp anew
    steps = ((0, 0), (600, 0), (600, 800), (300, 800), (300, 400), (0, 400))
    r, e, p, s = _built(pts=steps)
    try:
        assert len(p) == 1 and p["kind"][0] == 1 and p["n_edges"][0] == 2
        _refused(r, e, p, s, api.ERR_NOT_IMPLEMENTED, "NotImplementedLinearPieces")
    finally:
        r.close()
    # one box is one piece
    r, e, p, s = _built()
    try:
        assert p["kind"][0] == 1 and p["n_edges"][0] == 1
        _refused(r, e, p, s, api.ERR_NO_DEVICE, "host-only")
    finally:
        r.close()
    # a gradient square of 2 pixels over a 60-pixel shape: the rectangle's corners leave pixman's 16.16 range
    r, e, p, s = _built(matrix=_m(0.002, 0.002, 300, 200))
    try:
        _refused(r, e, p, s, api.ERR_CAPACITY, "LinearGradientOutOfRange")
    finally:
        r.close()
    # turned by a hair: the position moves by less than one 16.16 unit a row, but moves
    r, e, p, s = _built(matrix=_m(0.2, 0.2, 300, 200, 0.0, 1 / 65536))
    try:
        _refused(r, e, p, s, api.ERR_NOT_IMPLEMENTED, "NotImplementedLinearRowStep")
    finally:
        r.close()
