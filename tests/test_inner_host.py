"""Inner shadows on host-only handles (no GPU; DESIGN.md, "Inner shadows"): SWFR_SHADOW_INNER = 8 is accepted alone and with KNOCKOUT by
swfr_set_shadow, swfr_set_filters and swfr_shadow_bitmap's argument check, every other value with bit 3 is refused by name, a blur entry
still carries no flag; a type-19 and a type-21 object with an inner shadow build what they build with the outer shadow of the same box;
the Python mirror takes and reports "inner" -- the key only where it is set -- and frames without it build what they built.
"""
import ctypes as C

import pytest

import blur_scenes as bl
import filter_model as fm
import filter_scenes as fsc
import host_frames as hf
import inner_model as im
import scenarios
import shadow_model as sm
import shadow_scenes as ss
from blend_scenes import _rgba
from swf_renderer_amd import api

W, H = 64, 48
DROP = {"color": (10, 20, 60, 200), "dx": 4, "dy": -3, "x": 5, "y": 0, "passes": 3, "strength": 2}
INNER = dict(DROP, inner=True)
INNER_KGLOW = {"color": (255, 220, 40, 255), "x": 6, "y": 7, "strength": 255, "knockout": True, "inner": True}
KIDS = [hf.tri((230, 40, 90, 150)), hf.tri((40, 200, 120, 119), dx=9.5), bl._rect(10.5, 8, 50, 40.25, (20, 60, 240, 255))]
ACCEPTED, REFUSED = (8, 10), (9, 11, 12, 16, 24)


def _same(a, b):
    ea, pa, sa = a[:3]
    eb, pb, sb = b[:3]
    return (ea.tobytes() == eb.tobytes() and pa.tobytes() == pb.tobytes() and len(sa) == len(sb) and all(bytes(x) == bytes(y) for x, y in zip(sa, sb)))


def _sid(r):
    return r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))


def _shadow_struct(flags):
    s = api._shadow_struct(api.shadow_values(DROP))
    s.flags = flags
    return s


def _list(place, entry, n=3):
    """a list of n entries, `entry` in place `place`, blurs around it"""
    arr = (api.Filter * n)(*[api._filter_structs(api.filter_values([fm.blur(2, 3, 1)]))[0]] * n)
    arr[place] = entry
    return arr


def test_the_flag_is_bit_3():
    assert api.SHADOW_INNER == 8 and api.SHADOW_INNER not in (api.SHADOW_HIDE_OBJECT, api.SHADOW_KNOCKOUT, 4)
    assert api.shadow_values(INNER)[-1] == 8 and api.shadow_values(INNER_KGLOW)[-1] == 10
    assert api.shadow_values(dict(DROP, inner=False)) == api.shadow_values(DROP)


def test_accepted_and_refused_flags_by_name():
    r = hf.host(W, H)
    try:
        def err():
            return r.L.swfr_last_error(r.h).decode()
        for flags in ACCEPTED:
            s = _shadow_struct(flags)
            assert r.L.swfr_set_shadow(r.h, 1, C.byref(s)) == api.OK, flags
            assert r.L.swfr_shadow_bitmap(r.h, 1, 1, C.byref(s)) == api.ERR_NO_DEVICE, flags       # (the arguments pass; the device is missing)
            entry = api.Filter(api.FILTER_SHADOW, s)
            for n in range(1, api.MAX_FILTERS + 1):
                for place in range(n):
                    assert r.L.swfr_set_filters(r.h, 1, _list(place, entry, n), n) == api.OK, (flags, n, place)
        r.set_shadow(1, DROP)
        r.set_filters(1, [fm.shadow(DROP)])
        for flags in REFUSED:
            s = _shadow_struct(flags)
            assert (r.L.swfr_set_shadow(r.h, 1, C.byref(s)), err()) == (api.ERR_INVALID, "InvalidShadow"), flags
            assert (r.L.swfr_shadow_bitmap(r.h, 1, 1, C.byref(s)), err()) == (api.ERR_INVALID, "InvalidShadow"), flags
            entry = api.Filter(api.FILTER_SHADOW, s)
            for place in range(3):
                assert (r.L.swfr_set_filters(r.h, 1, _list(place, entry), 3), err()) == (api.ERR_INVALID, "InvalidFilter"), (flags, place)
        # a blur entry carries no flag, the new one neither
        blur = api._filter_structs(api.filter_values([fm.blur(5, 4, 2)]))
        blur[0].shadow.flags = 8
        assert (r.L.swfr_set_filters(r.h, 1, blur, 1), err()) == (api.ERR_INVALID, "InvalidFilter")
        # the refused calls left both slots as they were
        sid = _sid(r)
        assert hf.build_raw(r, hf.raw_stage(api.OBJECT_SHADOWED_LAYER, 1 | 1 << 8, sid)[0])[0] == api.OK and r.built_layers()[0][4] == sm.as_dict(DROP)
        assert hf.build_raw(r, hf.raw_stage(api.OBJECT_FILTERED_LAYER, 1 | 1 << 8, sid)[0])[0] == api.OK
        assert r.built_filters() == [fm.as_dicts([fm.shadow(DROP)])]
        assert r.L.swfr_abi_version() == 1 and C.sizeof(api.Shadow) == 32 and C.sizeof(api.Filter) == 36
    finally:
        r.close()


def test_the_mirror_takes_inner_and_hands_inner_with_hide_to_the_library():
    r = hf.host(W, H)
    try:
        for bad in (1, None, 0, "yes"):
            for call in (lambda v: r.build_frame({"children": [ss._shadowed(KIDS, dict(DROP, inner=v))]}), lambda v: r.set_shadow(1, dict(DROP, inner=v)),
                         lambda v: r.shadow_bitmap(1, 1, dict(DROP, inner=v)), lambda v: r.build_frame({"children": [fsc._filtered(KIDS, [fm.shadow(DROP, inner=v)])]}),
                         lambda v: r.set_filters(1, [fm.shadow(DROP, inner=v)])):
                with pytest.raises(api.SwfrError) as e:
                    call(bad)
                assert e.value.code == api.ERR_INVALID and "InvalidShadow" in str(e.value), bad
        # inner with hide_object, alone and with knockout: the mirror builds the struct, the library refuses it by name
        for extra in ({}, {"knockout": True}):
            sh = dict(DROP, inner=True, hide_object=True, **extra)
            assert api.shadow_values(sh)[-1] == (9 | (2 if extra else 0))
            for call in (lambda: r.build_frame({"children": [ss._shadowed(KIDS, sh)]}), lambda: r.set_shadow(1, sh), lambda: r.shadow_bitmap(1, 1, sh)):
                with pytest.raises(api.SwfrError) as e:
                    call()
                assert e.value.code == api.ERR_INVALID and "InvalidShadow" in str(e.value), sh
            for call in (lambda: r.build_frame({"children": [fsc._filtered(KIDS, [fm.blur(2, 2), {"shadow": sh}])]}), lambda: r.set_filters(1, [{"shadow": sh}])):
                with pytest.raises(api.SwfrError) as e:
                    call()
                assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value), sh
        # accepted: through the mirror to the library; rendering needs the device
        r.set_shadow(1, INNER), r.set_shadow(2, INNER_KGLOW), r.set_filters(1, [fm.shadow(INNER), fm.blur(2, 2), fm.shadow(INNER_KGLOW)])
        with pytest.raises(api.SwfrError) as e:
            r.shadow_bitmap(1, 1, INNER)
        assert e.value.code == api.ERR_NO_DEVICE
        with pytest.raises(api.SwfrError) as e:
            r.render({"children": [ss._shadowed(KIDS, INNER)]})
        assert e.value.code == api.ERR_NO_DEVICE
    finally:
        r.close()


@pytest.mark.parametrize("aliased", (False, True), ids=("antialiased", "aliased"))
@pytest.mark.parametrize("mode", ("normal", "multiply", "add"))
def test_an_inner_shadow_builds_what_the_outer_one_builds(mode, aliased):
    r = hf.host(W, H, antialias="none" if aliased else "default")
    try:
        ground = [hf.tri((9, 9, 9, 255), dx=-1)]
        mat = scenarios._m(0.9, 1.1, 3, 2)
        # type 19
        outer = r.build_frame({"children": ground + [ss._shadowed(KIDS, DROP, mode, matrix=mat)] + ground})
        outer_layers = r.built_layers()
        assert outer_layers[0][4] == sm.as_dict(DROP) and "inner" not in outer_layers[0][4]
        inner = r.build_frame({"children": ground + [ss._shadowed(KIDS, INNER, mode, matrix=mat)] + ground})
        layers = r.built_layers()
        assert _same(inner, outer) and len(layers) == 1 and len(layers[0]) == 5 and _same(layers[0], outer_layers[0])
        assert layers[0][3] == (5, 0, 3) and layers[0][4] == im.as_dict(INNER) == dict(sm.as_dict(DROP), inner=True)
        assert r.built_filters() == [[{"shadow": im.as_dict(INNER)}]]
        has, out = C.c_int(-1), api.Shadow()
        assert r.L.swfr_built_layer_shadow(r.h, 0, C.byref(has), C.byref(out)) == api.OK and has.value == 1 and out.flags == api.SHADOW_INNER
        # type 21, the inner entries first, in the middle and last
        for chain, plain in (([fm.shadow(INNER), fm.blur(5, 0, 3)], [fm.shadow(DROP), fm.blur(5, 0, 3)]),
                             ([fm.blur(5, 0, 3), fm.shadow(INNER_KGLOW), fm.shadow(DROP)], [fm.blur(5, 0, 3), fm.shadow(im.outer_of(INNER_KGLOW)), fm.shadow(DROP)]),
                             ([fm.blur(5, 0, 3), fm.shadow(DROP), fm.shadow(INNER)], [fm.blur(5, 0, 3), fm.shadow(DROP), fm.shadow(DROP)])):
            outer = r.build_frame({"children": ground + [fsc._filtered(KIDS, plain, mode, matrix=mat)] + ground})
            outer_layers = r.built_layers()
            assert r.built_filters() == [fm.as_dicts(plain)]
            inner = r.build_frame({"children": ground + [fsc._filtered(KIDS, chain, mode, matrix=mat)] + ground})
            assert _same(inner, outer) and _same(r.built_layers()[0], outer_layers[0]) and len(r.built_layers()[0]) == 4
            assert r.built_filters() == [im.as_dicts(chain)]
            assert sum("inner" in e.get("shadow", {}) for e in r.built_filters()[0]) == sum(im.is_inner(e.get("shadow", {})) for e in chain) >= 1
        # the sub-frame is what the children build as a stage of their own
        own = r.build_frame({"children": [{"type": "container", "matrix": mat, "children": KIDS}]})
        assert r.built_layers() == [] and _same(layers[0], own)
    finally:
        r.close()


def test_raw_objects_report_the_flags_of_their_slots():
    r = hf.host(W, H)
    try:
        sid = _sid(r)
        r.set_shadow(7, INNER_KGLOW)
        assert hf.build_raw(r, hf.raw_stage(api.OBJECT_SHADOWED_LAYER, 4 | 7 << 8, sid)[0])[0] == api.OK
        assert r.built_layers()[0][4] == im.as_dict(INNER_KGLOW) and r.built_layers()[0][4]["knockout"] is True
        r.set_filters(9, [fm.blur(2, 0, 3), fm.shadow(INNER)])
        assert hf.build_raw(r, hf.raw_stage(api.OBJECT_FILTERED_LAYER, 1 | 9 << 8, sid)[0])[0] == api.OK
        n, arr = C.c_uint32(99), (api.Filter * api.MAX_FILTERS)()
        assert r.L.swfr_built_layer_filters(r.h, 0, C.byref(n), arr) == api.OK and n.value == 2
        assert (arr[0].kind, arr[0].shadow.flags, arr[1].kind, arr[1].shadow.flags) == (api.FILTER_BLUR, 0, api.FILTER_SHADOW, api.SHADOW_INNER)
        # distinct slots of a call: the flag is part of the value
        arena = api._Arena()
        r._object(arena, {"type": "container", "children": [dict(KIDS[0], shadow=DROP), dict(KIDS[1], shadow=INNER), dict(KIDS[2], shadow=dict(INNER))]})
        assert len(arena.shadows) == 2
    finally:
        r.close()


def test_an_unflagged_shadow_reports_the_nine_keys_and_stages_without_inner_are_unchanged():
    r = hf.host(W, H)
    try:
        for sh in (DROP, dict(DROP, knockout=True), dict(DROP, hide_object=True), dict(DROP, inner=False)):
            r.build_frame({"children": [ss._shadowed(KIDS, sh)]})
            got = r.built_layers()[0][4]
            assert got == sm.as_dict(im.outer_of(sh)) and sorted(got) == sorted(sm.KEYS)
            r.build_frame({"children": [fsc._filtered(KIDS, [fm.blur(2, 2), {"shadow": sh}])]})
            assert r.built_filters() == [fm.as_dicts([fm.blur(2, 2), {"shadow": im.outer_of(sh)}])]
        # a stage builds the same arrays whether or not another object of it carries "inner", and "inner": False is no key at all
        plain = r.build_frame({"children": KIDS})
        assert r.built_layers() == []
        with_inner = r.build_frame({"children": KIDS + [ss._shadowed(KIDS[:1], INNER)]})
        assert plain[0].tobytes() == with_inner[0][:-1].tobytes() and plain[1].tobytes() == with_inner[1][:-1].tobytes()
        a = r.build_frame({"children": [ss._shadowed(KIDS, DROP)]})
        la = r.built_layers()
        b = r.build_frame({"children": [ss._shadowed(KIDS, dict(DROP, inner=False))]})
        assert _same(a, b) and _same(la[0], r.built_layers()[0]) and la[0][4] == r.built_layers()[0][4]
    finally:
        r.close()
