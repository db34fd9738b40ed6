"""Filter lists on host-only handles (no GPU): what the frame builder makes of a SWFR_OBJECT_FILTERED_LAYER -- the parent's one box path and
its style, the sub-frame swfr_built_layer hands out, the list swfr_built_layer_filters reports for all three kinds of layer -- every
refusal by code and name, where the Python mirror puts the type-21 wrapper next to "mask" and "opacity", and that frames without
"filters" build what they built before.
"""
import ctypes as C

import pytest

import blur_scenes as bl
import fade_scenes as fs
import filter_model as fm
import filter_scenes as fsc
import host_frames as hf
import layer_scenes as ls
import mask_scenes as ms
import scenarios
import shadow_scenes as ss
from blend_scenes import _rgba
from swf_renderer_amd import api

W, H = 64, 48
OPS = {"normal": 0, "layer": 0, "multiply": 1, "screen": 2, "lighten": 3, "darken": 4, "difference": 5, "add": 6, "overlay": 7, "hardlight": 8}
DROP = {"color": (10, 20, 60, 200), "dx": 4, "dy": -3, "x": 5, "y": 0, "passes": 3, "strength": 2}
GLOW = {"color": (255, 220, 40, 255), "x": 6, "y": 7, "strength": 255, "knockout": True}
CHAIN = [fm.blur(5, 0, 3), fm.shadow(DROP), fm.shadow(GLOW)]
KIDS = [hf.tri((230, 40, 90, 150)), hf.tri((40, 200, 120, 119), dx=9.5), bl._rect(10.5, 8, 50, 40.25, (20, 60, 240, 255))]


def _same(a, b):
    ea, pa, sa = a[:3]
    eb, pb, sb = b[:3]
    return (ea.tobytes() == eb.tobytes() and pa.tobytes() == pb.tobytes() and len(sa) == len(sb) and all(bytes(x) == bytes(y) for x, y in zip(sa, sb)))


def _filtered(kids, filters=CHAIN, mode=None, **kw):
    return fsc._filtered(kids, filters, mode, **kw)


def _sid(r):
    return r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))


def _structs(filters):
    v = api.filter_values(filters)
    return api._filter_structs(v), len(v)


def _built(r, k):
    """swfr_built_layer_filters' answer for sub-frame k: (rc, count, [(kind, blur_x, blur_y, passes, dx, dy, rgba, strength, flags)])"""
    n, arr = C.c_uint32(99), (api.Filter * api.MAX_FILTERS)()
    rc = r.L.swfr_built_layer_filters(r.h, k, C.byref(n), arr)
    return rc, n.value, [(f.kind, f.shadow.blur_x, f.shadow.blur_y, f.shadow.passes, f.shadow.dx, f.shadow.dy,
                          (f.shadow.color.r, f.shadow.color.g, f.shadow.color.b, f.shadow.color.a), f.shadow.strength, f.shadow.flags)
                         for f in arr[:n.value if rc == api.OK else 0]]


@pytest.mark.parametrize("aliased", (False, True), ids=("antialiased", "aliased"))
@pytest.mark.parametrize("mode", sorted(OPS))
def test_parent_path_and_sub_frame(mode, aliased):
    r = hf.host(W, H, antialias="none" if aliased else "default")
    try:
        ground = [hf.tri((9, 9, 9, 255), dx=-1)]
        mat = scenarios._m(0.9, 1.1, 3, 2)
        edges, paths, styles = r.build_frame({"children": ground + [_filtered(KIDS, CHAIN, mode, matrix=mat)] + ground})
        layers = r.built_layers()
        # swfr_built_layer reports the first entry's box; the tuple has four members; built_filters() has the list, every key filled in
        assert len(layers) == 1 and len(layers[0]) == 4 and layers[0][3] == (5, 0, 3)
        assert r.built_filters() == [fm.as_dicts(CHAIN)]
        # the parent: ground, ONE box path over the whole frame, ground
        assert hf.kinds(paths) == [api.PATH_TOR, api.PATH_BOXES, api.PATH_TOR]
        p = paths[1]
        assert hf.rects(paths)[1] == (0, 0, W, H) and int(p["n_edges"]) == 1 and int(p["fill_rule"]) == 0
        assert int(p["lerp"]) == OPS[mode] << 8                      # lerp bits 0, the operator in bits 8..15
        e = edges[int(p["first_edge"])]
        assert [int(e[k]) for k in ("x1", "y1", "x2", "y2", "top", "bottom", "dir", "reserved")] == [0, 0, W * 256, H * 256, 0, H * 256, 1, 1]
        st = styles[int(p["style"])]
        assert (st.kind, st.bitmap, st.extend, st.filter) == (api.STYLE_BITMAP, api.BLUR_BASE, 0, 1) and list(st.inv) == [1, 0, 0, 1, 0, 0]
        # ... byte-equal to a blurred layer's, and so is the sub-frame
        blurred = r.build_frame({"children": ground + [bl._blurred(KIDS, 5, 0, 3, mode, matrix=mat)] + ground})
        assert _same((edges, paths, styles), blurred)
        assert _same(layers[0], r.built_layers()[0]) and layers[0][3] == r.built_layers()[0][3]
        # the sub-frame: what the same children build as a stage of their own, under the same matrix
        own = r.build_frame({"children": [{"type": "container", "matrix": mat, "children": KIDS}]})
        assert r.built_layers() == [] and r.built_filters() == []
        assert _same(layers[0], own)
        assert hf.lerps(layers[0][1])[0] == 1                        # the surface-is-clear state starts afresh
    finally:
        r.close()


def test_alpha_mode_puts_the_path_in_a_group_and_needs_the_flag():
    for alpha_modes in (False, True):
        r = hf.host(W, H, alpha_modes=alpha_modes)
        try:
            sid = _sid(r)
            r.set_filters(3, CHAIN)
            for mode in (11, 12):
                rc, err, n_paths = hf.build_raw(r, hf.raw_stage(api.OBJECT_FILTERED_LAYER, mode | 3 << 8, sid)[0])
                if not alpha_modes:
                    assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
                else:
                    assert rc == api.OK and n_paths == (3 if mode == 11 else 1), mode
        finally:
            r.close()
    # LayerDepth under ALPHA is shared, too: the group around the path is one level
    r = hf.host(W, H, alpha_modes=True)
    try:
        deep = _filtered(KIDS[:1], CHAIN, "alpha")
        for _ in range(api.MAX_LAYER_DEPTH):
            deep = ls._layer("normal", [deep])
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [deep]})
        assert e.value.code == api.ERR_CAPACITY and "LayerDepth" in str(e.value)
    finally:
        r.close()


def test_built_layer_filters_for_the_three_types_and_the_slot_at_the_walk():
    r = hf.host(W, H)
    try:
        sid = _sid(r)
        r.set_filters(65535, CHAIN)
        stage = hf.raw_stage(api.OBJECT_FILTERED_LAYER, 4 | 65535 << 8, sid)[0]
        assert hf.build_raw(r, stage)[0] == api.OK
        rc, n, got = _built(r, 0)
        assert (rc, n) == (api.OK, 3)
        assert got == [(api.FILTER_BLUR, 5, 0, 3, 0, 0, (0, 0, 0, 0), 0, 0), (api.FILTER_SHADOW, 5, 0, 3, 4, -3, (10, 20, 60, 200), 2, 0),
                       (api.FILTER_SHADOW, 6, 7, 1, 0, 0, (255, 220, 40, 255), 255, api.SHADOW_KNOCKOUT)]
        assert r.L.swfr_built_layer_filters(r.h, 0, None, None) == api.OK and r.L.swfr_built_layer_filters(r.h, 1, None, None) == api.ERR_NOT_FOUND
        assert r.built_filters() == [fm.as_dicts(CHAIN)]
        # swfr_built_layer: the first entry's box; swfr_built_layer_shadow: no shadow, whatever the list holds
        assert r.built_layers()[0][3] == (5, 0, 3) and len(r.built_layers()[0]) == 4
        has, out = C.c_int(-1), api.Shadow()
        assert r.L.swfr_built_layer_shadow(r.h, 0, C.byref(has), C.byref(out)) == api.OK and has.value == 0
        r.set_filters(7, [fm.shadow(GLOW), fm.blur(2, 2, 1)])
        assert hf.build_raw(r, hf.raw_stage(api.OBJECT_FILTERED_LAYER, 1 | 7 << 8, sid)[0])[0] == api.OK
        assert r.L.swfr_built_layer_shadow(r.h, 0, C.byref(has), None) == api.OK and has.value == 0 and r.built_layers()[0][3] == (6, 7, 1)
        # the slot's list is read at the walk: set anew, the next walk has the new one; the built frame keeps what it was built with
        assert hf.build_raw(r, stage)[0] == api.OK
        other = [fm.shadow(GLOW)]
        r.set_filters(65535, other)
        assert r.built_filters() == [fm.as_dicts(CHAIN)]
        assert hf.build_raw(r, stage)[0] == api.OK and r.built_filters() == [fm.as_dicts(other)]
        # cleared -- by None, by an empty list, by a count of 0 --: not found
        for clear in (lambda: r.set_filters(65535, None), lambda: r.set_filters(65535, []),
                      lambda: r._check(r.L.swfr_set_filters(r.h, 65535, _structs(CHAIN)[0], 0))):
            r.set_filters(65535, CHAIN)
            assert hf.build_raw(r, stage)[0] == api.OK
            clear()
            assert hf.build_raw(r, stage)[:2] == (api.ERR_NOT_FOUND, "FiltersNotFound")
        # a blurred layer reports its one blur entry, a shadowed layer its one shadow entry; what the older calls answer is unchanged
        r.build_frame({"children": [bl._blurred(KIDS, 2, 9, 4), ss._shadowed(KIDS, DROP), _filtered(KIDS)]})
        assert r.built_filters() == [[{"blur": {"x": 2, "y": 9, "passes": 4}}], fm.as_dicts([fm.shadow(DROP)]), fm.as_dicts(CHAIN)]
        assert _built(r, 0)[1:] == (1, [(api.FILTER_BLUR, 2, 9, 4, 0, 0, (0, 0, 0, 0), 0, 0)])
        assert _built(r, 1)[1:] == (1, [(api.FILTER_SHADOW, 5, 0, 3, 4, -3, (10, 20, 60, 200), 2, 0)])
        assert [len(l) for l in r.built_layers()] == [4, 5, 4] and [l[3] for l in r.built_layers()] == [(2, 9, 4), (5, 0, 3), (5, 0, 3)]
        assert [r.L.swfr_built_layer_shadow(r.h, k, C.byref(has), None) == api.OK and has.value for k in range(3)] == [0, 1, 0]
    finally:
        r.close()


def test_refusals_by_code_and_name():
    r = hf.host(W, H)
    try:
        sid = _sid(r)
        ok, n_ok = _structs(CHAIN)

        def one(base, **kw):
            """a list of one entry: the DROP shadow (or a 5 x 4 blur of 2 passes) with fields changed"""
            arr, _ = _structs([fm.shadow(DROP)] if base == api.FILTER_SHADOW else [fm.blur(5, 4, 2)])
            for k, v in kw.items():
                if k == "kind":
                    arr[0].kind = v
                elif k == "color":
                    arr[0].shadow.color = api.Rgba8(*v)
                else:
                    setattr(arr[0].shadow, k, v)
            return arr

        def set_one(arr, slot=1, count=1):
            return r.L.swfr_set_filters(r.h, slot, arr, count), r.L.swfr_last_error(r.h).decode()
        # swfr_set_filters: the slot, the count, the kind
        assert set_one(ok, 65535, n_ok)[0] == api.OK
        assert set_one(ok, 65536, n_ok) == (api.ERR_INVALID, "InvalidFilter")
        assert r.L.swfr_set_filters(r.h, 0, None, 0) == api.OK and r.L.swfr_set_filters(r.h, 0, None, 9) == api.OK      # clearing an unset slot
        five = (api.Filter * 5)(*[_structs([fm.blur(2, 2, 1)])[0][0]] * 5)
        assert set_one(five, 1, 4)[0] == api.OK
        assert set_one(five, 1, 5) == (api.ERR_CAPACITY, "FilterListLength")
        for kind in (2, 3, 255, 2 ** 32 - 1):
            assert set_one(one(api.FILTER_BLUR, kind=kind)) == (api.ERR_INVALID, "InvalidFilter"), kind
        # every field of both kinds at both ends of its range, and one past
        good_blur = [dict(blur_x=0), dict(blur_x=255), dict(blur_y=0), dict(blur_y=255), dict(passes=1), dict(passes=15)]
        bad_blur = [dict(blur_x=256), dict(blur_y=256), dict(blur_x=2 ** 32 - 1), dict(passes=0), dict(passes=16),
                    # the fields a blur entry does not use must be zero
                    dict(dx=1), dict(dy=-1), dict(color=(0, 0, 0, 1)), dict(color=(1, 0, 0, 0)), dict(color=(0, 1, 0, 0)), dict(color=(0, 0, 1, 0)),
                    dict(strength=1), dict(flags=1), dict(flags=2)]
        good_shadow = [dict(blur_x=0), dict(blur_x=255), dict(blur_y=0), dict(blur_y=255), dict(passes=1), dict(passes=15), dict(dx=-32768), dict(dx=32767),
                       dict(dy=-32768), dict(dy=32767), dict(strength=1), dict(strength=255), dict(flags=0), dict(flags=1), dict(flags=2)]
        bad_shadow = [dict(blur_x=256), dict(blur_y=256), dict(passes=0), dict(passes=16), dict(dx=-32769), dict(dx=32768), dict(dy=-32769), dict(dy=32768),
                      dict(strength=0), dict(strength=256), dict(flags=3), dict(flags=4), dict(flags=2 ** 31)]
        for kind, good, bad in ((api.FILTER_BLUR, good_blur, bad_blur), (api.FILTER_SHADOW, good_shadow, bad_shadow)):
            for kw in good:
                assert set_one(one(kind, **kw))[0] == api.OK, (kind, kw)
            r.set_filters(1, CHAIN)
            for kw in bad:
                assert set_one(one(kind, **kw)) == (api.ERR_INVALID, "InvalidFilter"), (kind, kw)
                # ... in any place of a list
                arr = (api.Filter * 3)(ok[0], ok[1], one(kind, **kw)[0])
                assert set_one(arr, 1, 3) == (api.ERR_INVALID, "InvalidFilter"), (kind, kw)

        def raw(mode, slot, t=api.OBJECT_FILTERED_LAYER):
            return hf.build_raw(r, hf.raw_stage(t, mode | slot << 8, sid)[0])
        # a refused list leaves the slot as it was
        assert raw(1, 1)[0] == api.OK and r.built_filters() == [fm.as_dicts(CHAIN)]
        for mode in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
            rc, _, n_paths = raw(mode, 1)
            assert rc == api.OK and n_paths == 1 and r.L.swfr_built_layers(r.h) == 1, mode
        for mode in (9, 10, 11, 12):
            assert raw(mode, 1)[:2] == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
        for mode in (15, 16, 255):
            assert raw(mode, 1)[0] == api.ERR_INVALID, mode
        assert raw(1, 2)[:2] == (api.ERR_NOT_FOUND, "FiltersNotFound")
        assert raw(1, 65536)[:2] == (api.ERR_INVALID, "InvalidFilter")                   # (the id has no room for such a slot)
        for t in (14, 15, 17, 18, 20, 22, 23, 255):                  # still not display-object types
            assert raw(1, 1, t=t)[:2] == (api.ERR_INVALID, "UnexpectedDisplayObjectType"), t
        # any of the three kinds below any of the three, however far below -- the mixes with a filtered layer
        kinds = {"filtered": _filtered, "blurred": lambda k: bl._blurred(k, 2, 2), "shadowed": lambda k: ss._shadowed(k, DROP)}
        for outer, inner in (("filtered", "filtered"), ("filtered", "blurred"), ("filtered", "shadowed"), ("blurred", "filtered"), ("shadowed", "filtered")):
            nested = {"children": [kinds[outer]([ls._layer("normal", [{"type": "container", "children": [kinds[inner](KIDS)]}])])]}
            with pytest.raises(api.SwfrError) as e:
                r.build_frame(nested)
            assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NestedBlur" in str(e.value), (outer, inner)
        # eight of the three kinds in a frame, whatever the lists' lengths, not nine
        mixed = [(_filtered(KIDS[:1], CHAIN + [fm.blur(2, 2, 1)]), ss._shadowed(KIDS[:1], DROP), bl._blurred(KIDS[:1], 2, 2))[i % 3] for i in range(api.MAX_BLUR_LAYERS + 1)]
        r.build_frame({"children": mixed[:api.MAX_BLUR_LAYERS]})
        assert [len(f) for f in r.built_filters()] == [4, 1, 1, 4, 1, 1, 4, 1]
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": mixed})
        assert e.value.code == api.ERR_CAPACITY and "BlurLayers" in str(e.value)
        # "filters" with either single key on one object
        for key, value in (("blur", {"x": 2, "y": 2}), ("shadow", DROP)):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [dict(_filtered(KIDS), **{key: value})]})
            assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedFilterChain" in str(e.value), key
        # rendering needs a device
        with pytest.raises(api.SwfrError) as e:
            r.render({"children": [_filtered(KIDS)]})
        assert e.value.code == api.ERR_NO_DEVICE
        # the Python mirror's own checks: an entry that is no dict of exactly one known key, a value that is no list
        for bad_value in (3, {"blur": {"x": 2}}, [3], [None], [[]], [{}], [{"blur": {"x": 2}, "shadow": DROP}], [{"glow": DROP}], [fm.blur(2, 2), "blur"]):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [dict(_filtered(KIDS), filters=bad_value)]})
            assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value), bad_value
            with pytest.raises(api.SwfrError) as e:
                r.set_filters(1, bad_value)
            assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value), bad_value
        # ... and what it hands to the library to refuse: values out of range, a list of five
        for bad_value in ([fm.blur(2, 2, 0)], [fm.blur(2, 2, 16)], [fm.shadow(DROP, strength=0)], [fm.shadow(DROP, dx=32768)],
                          [fm.blur(2, 2), fm.shadow(DROP, hide_object=True, knockout=True)]):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [_filtered(KIDS, bad_value)]})
            assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value), bad_value
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [_filtered(KIDS, [fm.blur(2, 2)] * 5)]})
        assert e.value.code == api.ERR_CAPACITY and "FilterListLength" in str(e.value)
        # an entry's own value is checked as the single key's is, and refused under that key's name
        for bad_value, name in (([{"shadow": {"color": (1, 2, 3)}}], "InvalidShadow"), ([fm.blur(256, 1)], "InvalidBlur"), ([{"blur": 3}], "InvalidBlur")):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [_filtered(KIDS, bad_value)]})
            assert e.value.code == api.ERR_INVALID and name in str(e.value), bad_value
        # the defaults
        r.build_frame({"children": [_filtered(KIDS, [{"blur": {}}, {"shadow": {"color": (1, 2, 3, 4)}}])]})
        assert r.built_filters() == [[{"blur": {"x": 0, "y": 0, "passes": 1}},
                                      {"shadow": {"color": (1, 2, 3, 4), "dx": 0, "dy": 0, "x": 0, "y": 0, "passes": 1, "strength": 1,
                                                  "hide_object": False, "knockout": False}}]]
    finally:
        r.close()


def _tree(r, obj):
    """(type, id, [children]) of the display object the mirror makes of `obj`, and the arena that holds the call's lists"""
    arena = api._Arena()
    d = r._object(arena, obj)

    def walk(d):
        return (d.type, d.id, [walk(d.children[i]) for i in range(d.n_children)])
    return walk(d), arena


def test_wrapper_order_next_to_mask_and_opacity_and_slots_per_call():
    r = hf.host(W, H)
    try:
        ct = {"red_mult": 0.5}
        shape = dict(KIDS[0], matrix=scenarios._m(1, 1, 2, 2), blend_mode="multiply", color_transform=ct)
        # alone: type 21 with the mode of "layer", the blend-mode and colour-transform wrappers and the matrix inside
        t, arena = _tree(r, dict(shape, filters=CHAIN, layer="screen"))
        assert t[:2] == (21, 4 | 0 << 8) and t[2][0][:2] == (5, 3) and t[2][0][2][0][0] == 3 and t[2][0][2][0][2][0][0] == 0
        assert list(arena.filters.items()) == [(api.filter_values(CHAIN), 0)] and not arena.shadows
        t, _ = _tree(r, dict(shape, filters=CHAIN))
        assert t[:2] == (21, 1)
        # an empty list is no filter at all: no wrapper, and what "layer" asks for stays
        t, arena = _tree(r, dict(shape, filters=[]))
        assert t[:2] == (5, 3) and not arena.filters
        assert _tree(r, dict(shape, filters=[], layer="screen"))[0] == _tree(r, dict(shape, layer="screen"))[0]
        assert _same(r.build_frame({"children": [dict(KIDS[0], filters=[]), KIDS[1]]}), r.build_frame({"children": KIDS[:2]})) and r.built_layers() == []
        # with "mask": type 11 takes the mode, the filtered layer is its content, composited normally
        t, _ = _tree(r, dict(shape, filters=CHAIN, layer="screen", mask=[KIDS[1]]))
        assert t[:2] == (11, 4) and t[2][0][0] == 2 and t[2][1][:2] == (21, 1) and t[2][1][2][0][:2] == (5, 3)
        # with "opacity": type 13 takes the mode
        t, _ = _tree(r, dict(shape, filters=CHAIN, layer="screen", opacity=77))
        assert t[:2] == (13, 4 | 77 << 8) and t[2][0][:2] == (21, 1)
        # with both: 13 around 11 around 21
        t, _ = _tree(r, dict(shape, filters=CHAIN, layer="add", opacity=77, mask=[KIDS[1]]))
        assert t[:2] == (13, 8 | 77 << 8) and t[2][0][:2] == (11, 1) and t[2][0][2][1][:2] == (21, 1)
        # slots by first appearance, one per distinct list of the call; the order of a list is part of it; shadows keep their own slots
        other = [CHAIN[1], CHAIN[0], CHAIN[2]]
        t, arena = _tree(r, {"type": "container", "children": [dict(KIDS[0], filters=CHAIN), dict(KIDS[1], filters=other), dict(KIDS[2], filters=list(CHAIN)),
                                                               dict(KIDS[0], shadow=DROP)]})
        assert [k[:2] for k in t[2]] == [(21, 1), (21, 1 | 1 << 8), (21, 1), (19, 1)] and len(arena.filters) == 2 and len(arena.shadows) == 1
        # the built frame says the same: BEGIN, the filtered layer's box, MASK, the mask, END
        edges, paths, styles = r.build_frame({"children": [dict(KIDS[0], filters=CHAIN, mask=[KIDS[1]])]})
        assert hf.kinds(paths) == [2, 1, 4, 0, 3] and len(r.built_layers()) == 1
        assert styles[int(paths[1]["style"])].bitmap == api.BLUR_BASE
        r.build_frame({"children": [dict(KIDS[0], filters=CHAIN), KIDS[2], dict(KIDS[1], filters=other), bl._blurred(KIDS, 3, 3)]})
        assert r.built_filters() == [fm.as_dicts(CHAIN), fm.as_dicts(other), [{"blur": {"x": 3, "y": 3, "passes": 1}}]]
        # on shapes and morph shapes alike
        morph = scenarios.scenarios()["morph_037"]["stage"]["children"][0]
        assert morph["type"] == "morph-shape"
        t, _ = _tree(r, dict(morph, filters=CHAIN))
        assert t[:2] == (21, 1) and t[2][0][0] == api.OBJECT_MORPH_SHAPE
    finally:
        r.close()


def test_a_stage_of_many_children_with_a_list_builds_in_one_walk(monkeypatch):
    monkeypatch.setenv("SWFR_BUILD_THREADS", "4")
    r = hf.host(W, H)
    try:
        many = [hf.tri((i % 250, 40, 90, 150), dx=(i % 7)) for i in range(300)]
        for _ in range(2):
            plain = r.build_frame({"children": many})
            assert r.built_layers() == []
            with_list = r.build_frame({"children": many + [_filtered(KIDS)]})
            assert len(r.built_layers()) == 1 and r.built_filters() == [fm.as_dicts(CHAIN)]
            assert plain[1].tobytes() == with_list[1][:-1].tobytes() and plain[0].tobytes() == with_list[0][:-1].tobytes()
    finally:
        r.close()


def test_frames_without_filters_build_what_they_built():
    """a sample of the existing scenes, the blurred and shadowed ones among them: the same children inside a filtered layer build, as the
    layer's sub-frame, exactly the arrays the scene builds as a frame.  (Not a comparison with arrays recorded before filter lists
    existed: the existing host tests of every family hold those.)"""
    sample = {}
    SC = scenarios.scenarios()
    for name in sorted(SC)[::6]:
        sample["scenario_" + name] = SC[name]
    for fam, scenes in (("layer", ls.overlap_scenes()), ("mask", ms.structure_scenes()), ("fade", fs.operator_scenes()), ("blur", bl.box_scenes()),
                        ("shadow", ss.structure_scenes())):
        for name in sorted(scenes)[::9]:
            sample["%s_%s" % (fam, name)] = scenes[name]
    assert len(sample) >= 16
    for name, sc in sample.items():
        r = hf.host(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")))
        try:
            for b in sc.get("bitmaps", []):
                r.add_bitmap(b)
            got = r.build_frame(sc["stage"])
            assert all(len(f) == 1 for f in r.built_filters()), name
            if name.startswith(("blur_", "shadow_")):
                # as a list of one entry: the same arrays, the same sub-frames
                subs = r.built_layers()
                again = r.build_frame({"children": fsc.as_filter_lists(sc["stage"]["children"])})
                assert _same(got, again) and len(subs) == len(r.built_layers()) and all(_same(a, b) for a, b in zip(subs, r.built_layers())), name
                continue
            assert r.built_layers() == [] and not any(s.kind == api.STYLE_BITMAP and s.bitmap >= api.BLUR_BASE for s in got[2]), name
            wrapped = r.build_frame({"children": [{"type": "container", "children": sc["stage"]["children"], "filters": CHAIN}]})
            assert len(wrapped[1]) == 1 and _same(r.built_layers()[0], got), name
        finally:
            r.close()
