"""Shadowed layers on host-only handles (no GPU): what the frame builder makes of a SWFR_OBJECT_SHADOWED_LAYER -- the parent's one box path
and its style, the sub-frame swfr_built_layer hands out, the shadow swfr_built_layer_shadow reports -- every refusal by code and name,
where the Python mirror puts the type-19 wrapper next to "mask" and "opacity", and that frames without a "shadow" build what they built
before.
"""
import ctypes as C

import pytest

import blur_scenes as bl
import fade_scenes as fs
import host_frames as hf
import layer_scenes as ls
import mask_scenes as ms
import scenarios
import shadow_model as sm
import shadow_scenes as ss
from blend_scenes import _rgba
from swf_renderer_amd import api

W, H = 64, 48
OPS = {"normal": 0, "layer": 0, "multiply": 1, "screen": 2, "lighten": 3, "darken": 4, "difference": 5, "add": 6, "overlay": 7, "hardlight": 8}
DROP = {"color": (10, 20, 60, 200), "dx": 4, "dy": -3, "x": 5, "y": 0, "passes": 3, "strength": 2}
KIDS = [hf.tri((230, 40, 90, 150)), hf.tri((40, 200, 120, 119), dx=9.5), bl._rect(10.5, 8, 50, 40.25, (20, 60, 240, 255))]


def _same(a, b):
    ea, pa, sa = a[:3]
    eb, pb, sb = b[:3]
    return (ea.tobytes() == eb.tobytes() and pa.tobytes() == pb.tobytes() and len(sa) == len(sb) and all(bytes(x) == bytes(y) for x, y in zip(sa, sb)))


def _shadowed(kids, shadow=DROP, mode=None, **kw):
    return ss._shadowed(kids, shadow, mode, **kw)


@pytest.mark.parametrize("aliased", (False, True), ids=("antialiased", "aliased"))
@pytest.mark.parametrize("mode", sorted(OPS))
def test_parent_path_and_sub_frame(mode, aliased):
    r = hf.host(W, H, antialias="none" if aliased else "default")
    try:
        ground = [hf.tri((9, 9, 9, 255), dx=-1)]
        mat = scenarios._m(0.9, 1.1, 3, 2)
        edges, paths, styles = r.build_frame({"children": ground + [_shadowed(KIDS, DROP, mode, matrix=mat)] + ground})
        layers = r.built_layers()
        # swfr_built_layer reports the shadow's box; the fifth member is the shadow, every key filled in
        assert len(layers) == 1 and len(layers[0]) == 5 and layers[0][3] == (5, 0, 3) and layers[0][4] == sm.as_dict(DROP)
        # the parent: ground, ONE box path over the whole frame, ground -- exactly a blurred layer's
        assert hf.kinds(paths) == [api.PATH_TOR, api.PATH_BOXES, api.PATH_TOR]
        p = paths[1]
        assert hf.rects(paths)[1] == (0, 0, W, H) and int(p["n_edges"]) == 1 and int(p["fill_rule"]) == 0
        assert int(p["lerp"]) == OPS[mode] << 8                      # lerp bits 0, the operator in bits 8..15
        e = edges[int(p["first_edge"])]
        assert [int(e[k]) for k in ("x1", "y1", "x2", "y2", "top", "bottom", "dir", "reserved")] == [0, 0, W * 256, H * 256, 0, H * 256, 1, 1]
        st = styles[int(p["style"])]
        assert (st.kind, st.bitmap, st.extend, st.filter) == (api.STYLE_BITMAP, api.BLUR_BASE, 0, 1) and list(st.inv) == [1, 0, 0, 1, 0, 0]
        blurred = r.build_frame({"children": ground + [bl._blurred(KIDS, 5, 0, 3, mode, matrix=mat)] + ground})
        assert _same((edges, paths, styles), blurred) and len(r.built_layers()[0]) == 4
        assert _same(layers[0], r.built_layers()[0])
        # the sub-frame: what the same children build as a stage of their own, under the same matrix
        own = r.build_frame({"children": [{"type": "container", "matrix": mat, "children": KIDS}]})
        assert r.built_layers() == []
        assert _same(layers[0], own)
        assert hf.lerps(layers[0][1])[0] == 1                        # the surface-is-clear state starts afresh
    finally:
        r.close()


def test_alpha_mode_puts_the_path_in_a_group_and_needs_the_flag():
    for alpha_modes in (False, True):
        r = hf.host(W, H, alpha_modes=alpha_modes)
        try:
            sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
            r.set_shadow(3, DROP)
            for mode in (11, 12):
                rc, err, n_paths = hf.build_raw(r, hf.raw_stage(api.OBJECT_SHADOWED_LAYER, mode | 3 << 8, sid)[0])
                if not alpha_modes:
                    assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
                else:
                    assert rc == api.OK and n_paths == (3 if mode == 11 else 1), mode
        finally:
            r.close()


def test_built_layer_shadow_and_the_slot_at_the_walk():
    r = hf.host(W, H)
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
        glow = {"color": (255, 220, 40, 255), "x": 6, "y": 7, "strength": 255, "knockout": True}
        r.set_shadow(65535, glow)
        stage = hf.raw_stage(api.OBJECT_SHADOWED_LAYER, 4 | 65535 << 8, sid)[0]
        assert hf.build_raw(r, stage)[0] == api.OK
        has, out = C.c_int(-1), api.Shadow()
        assert r.L.swfr_built_layer_shadow(r.h, 0, C.byref(has), C.byref(out)) == api.OK and has.value == 1
        assert (out.blur_x, out.blur_y, out.passes, out.dx, out.dy, out.strength, out.flags) == (6, 7, 1, 0, 0, 255, api.SHADOW_KNOCKOUT)
        assert (out.color.r, out.color.g, out.color.b, out.color.a) == (255, 220, 40, 255)
        assert r.L.swfr_built_layer_shadow(r.h, 0, None, None) == api.OK and r.L.swfr_built_layer_shadow(r.h, 1, None, None) == api.ERR_NOT_FOUND
        assert r.built_layers()[0][3] == (6, 7, 1) and r.built_layers()[0][4] == sm.as_dict(glow)
        # the slot's value is read at the walk: set anew, the next walk has the new one; the built frame keeps what it was built with
        r.set_shadow(65535, DROP)
        assert r.built_layers()[0][4] == sm.as_dict(glow)
        assert hf.build_raw(r, stage)[0] == api.OK and r.built_layers()[0][4] == sm.as_dict(DROP)
        # cleared: not found; a blurred layer has no shadow
        r.set_shadow(65535, None)
        assert hf.build_raw(r, stage)[:2] == (api.ERR_NOT_FOUND, "ShadowNotFound")
        r.build_frame({"children": [bl._blurred(KIDS, 2, 2)]})
        has.value = -1
        assert r.L.swfr_built_layer_shadow(r.h, 0, C.byref(has), C.byref(out)) == api.OK and has.value == 0
    finally:
        r.close()


def test_refusals_by_code_and_name():
    r = hf.host(W, H)
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
        ok = api._shadow_struct(api.shadow_values(DROP))

        def struct(**kw):
            s = api._shadow_struct(api.shadow_values(DROP))
            for k, v in kw.items():
                setattr(s, k, v)
            return s
        # swfr_set_shadow: the slot, then every field at both ends of its range and one past
        assert r.L.swfr_set_shadow(r.h, 65535, C.byref(ok)) == api.OK
        assert r.L.swfr_set_shadow(r.h, 65536, C.byref(ok)) == api.ERR_INVALID
        assert r.L.swfr_set_shadow(r.h, 0, None) == api.OK                               # clearing an unset slot
        good = [dict(blur_x=0), dict(blur_x=255), dict(blur_y=0), dict(blur_y=255), dict(passes=1), dict(passes=15), dict(dx=-32768), dict(dx=32767),
                dict(dy=-32768), dict(dy=32767), dict(strength=1), dict(strength=255), dict(flags=0), dict(flags=1), dict(flags=2)]
        bad = [dict(blur_x=256), dict(blur_y=256), dict(blur_x=2 ** 32 - 1), dict(passes=0), dict(passes=16), dict(dx=-32769), dict(dx=32768), dict(dy=-32769),
               dict(dy=32768), dict(dx=-2 ** 31), dict(strength=0), dict(strength=256), dict(flags=3), dict(flags=4), dict(flags=5), dict(flags=2 ** 31)]
        for kw in good:
            assert r.L.swfr_set_shadow(r.h, 1, C.byref(struct(**kw))) == api.OK, kw
        r.set_shadow(1, DROP)
        for kw in bad:
            assert r.L.swfr_set_shadow(r.h, 1, C.byref(struct(**kw))) == api.ERR_INVALID, kw
            assert r.L.swfr_last_error(r.h).decode() == "InvalidShadow", kw
            # swfr_shadow_bitmap checks its arguments before the device it needs
            assert r.L.swfr_shadow_bitmap(r.h, 1, 1, C.byref(struct(**kw))) == api.ERR_INVALID and r.L.swfr_last_error(r.h).decode() == "InvalidShadow", kw
        assert r.L.swfr_shadow_bitmap(r.h, 1, 1, None) == api.ERR_INVALID
        assert r.L.swfr_shadow_bitmap(r.h, 65536, 1, C.byref(ok)) == api.ERR_INVALID
        assert r.L.swfr_shadow_bitmap(r.h, 1, 1, C.byref(ok)) == api.ERR_NO_DEVICE
        # a refused value leaves the slot as it was
        assert hf.build_raw(r, hf.raw_stage(api.OBJECT_SHADOWED_LAYER, 1 | 1 << 8, sid)[0])[0] == api.OK and r.built_layers()[0][4] == sm.as_dict(DROP)

        def raw(mode, slot, t=api.OBJECT_SHADOWED_LAYER):
            return hf.build_raw(r, hf.raw_stage(t, mode | slot << 8, sid)[0])
        for mode in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
            rc, _, n_paths = raw(mode, 1)
            assert rc == api.OK and n_paths == 1 and r.L.swfr_built_layers(r.h) == 1, mode
        for mode in (9, 10, 11, 12):
            assert raw(mode, 1)[:2] == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
        for mode in (15, 16, 255):
            assert raw(mode, 1)[0] == api.ERR_INVALID, mode
        assert raw(1, 2)[:2] == (api.ERR_NOT_FOUND, "ShadowNotFound")
        assert raw(1, 65536)[:2] == (api.ERR_INVALID, "InvalidShadow")                   # (the id has no room for such a slot)
        for t in (14, 15, 17, 18, 20, 255):                          # still not display-object types
            assert raw(1, 1, t=t)[:2] == (api.ERR_INVALID, "UnexpectedDisplayObjectType"), t
        # either kind below either kind, however far below
        for outer, inner in ((_shadowed, _shadowed), (_shadowed, lambda k: bl._blurred(k, 2, 2)), (lambda k: bl._blurred(k, 3, 3), _shadowed)):
            nested = {"children": [outer([ls._layer("normal", [{"type": "container", "children": [inner(KIDS)]}])])]}
            with pytest.raises(api.SwfrError) as e:
                r.build_frame(nested)
            assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NestedBlur" in str(e.value)
        # eight of both kinds in a frame, not nine
        mixed = [_shadowed(KIDS[:1]) if i % 2 else bl._blurred(KIDS[:1], 2, 2) for i in range(api.MAX_BLUR_LAYERS + 1)]
        r.build_frame({"children": mixed[:api.MAX_BLUR_LAYERS]})
        assert [len(l) for l in r.built_layers()] == [4, 5] * (api.MAX_BLUR_LAYERS // 2)
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": mixed})
        assert e.value.code == api.ERR_CAPACITY and "BlurLayers" in str(e.value)
        # "blur" and "shadow" on one object
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [dict(_shadowed(KIDS), blur={"x": 2, "y": 2})]})
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedFilterChain" in str(e.value)
        # rendering needs a device
        with pytest.raises(api.SwfrError) as e:
            r.render({"children": [_shadowed(KIDS)]})
        assert e.value.code == api.ERR_NO_DEVICE
        # the Python mirror's own checks, and what it hands to the library to refuse
        for bad_value in (3, {}, {"color": (1, 2, 3)}, {"color": (1, 2, 3, 256)}, {"color": (1, 2, 3, 4), "dx": 1.5}, {"color": (1, 2, 3, 4), "x": -1},
                          {"color": (1, 2, 3, 4), "knockout": 1}, {"color": (1, 2, 3, 4), "angle": 45}, {"color": (1, 2, 3, 4), "strength": True}):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [dict(_shadowed(KIDS), shadow=bad_value)]})
            assert e.value.code == api.ERR_INVALID and "InvalidShadow" in str(e.value), bad_value
        for bad_value in ({"x": 256}, {"y": 256}, {"passes": 0}, {"passes": 16}, {"dx": 32768}, {"dy": -32769}, {"strength": 0}, {"strength": 256},
                          {"hide_object": True, "knockout": True}):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [_shadowed(KIDS, dict(DROP, **bad_value))]})
            assert e.value.code == api.ERR_INVALID and "InvalidShadow" in str(e.value), bad_value
            with pytest.raises(api.SwfrError) as e:
                r.shadow_bitmap(1, 1, dict(DROP, **bad_value))
            assert e.value.code == api.ERR_INVALID and "InvalidShadow" in str(e.value), bad_value
        # the defaults
        r.build_frame({"children": [_shadowed(KIDS, {"color": (1, 2, 3, 4)})]})
        assert r.built_layers()[0][3:] == ((0, 0, 1), {"color": (1, 2, 3, 4), "dx": 0, "dy": 0, "x": 0, "y": 0, "passes": 1, "strength": 1,
                                                       "hide_object": False, "knockout": False})
    finally:
        r.close()


def _tree(r, obj):
    """(type, id, [children]) of the display object the mirror makes of `obj`, and the arena that holds the call's shadows"""
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
        # alone: type 19 with the mode of "layer", the blend-mode and colour-transform wrappers and the matrix inside
        t, arena = _tree(r, dict(shape, shadow=DROP, layer="screen"))
        assert t[:2] == (19, 4 | 0 << 8) and t[2][0][:2] == (5, 3) and t[2][0][2][0][0] == 3 and t[2][0][2][0][2][0][0] == 0
        assert list(arena.shadows.items()) == [(api.shadow_values(DROP), 0)]
        t, _ = _tree(r, dict(shape, shadow=DROP))
        assert t[:2] == (19, 1)
        # with "mask": type 11 takes the mode, the shadowed layer is its content, composited normally
        t, _ = _tree(r, dict(shape, shadow=DROP, layer="screen", mask=[KIDS[1]]))
        assert t[:2] == (11, 4) and t[2][0][0] == 2 and t[2][1][:2] == (19, 1) and t[2][1][2][0][:2] == (5, 3)
        # with "opacity": type 13 takes the mode
        t, _ = _tree(r, dict(shape, shadow=DROP, layer="screen", opacity=77))
        assert t[:2] == (13, 4 | 77 << 8) and t[2][0][:2] == (19, 1)
        # with both: 13 around 11 around 19
        t, _ = _tree(r, dict(shape, shadow=DROP, layer="add", opacity=77, mask=[KIDS[1]]))
        assert t[:2] == (13, 8 | 77 << 8) and t[2][0][:2] == (11, 1) and t[2][0][2][1][:2] == (19, 1)
        # slots by first appearance, one per distinct shadow of the call
        other = dict(DROP, dx=0, dy=0)
        t, arena = _tree(r, {"type": "container", "children": [dict(KIDS[0], shadow=DROP), dict(KIDS[1], shadow=other), dict(KIDS[2], shadow=dict(DROP))]})
        assert [k[:2] for k in t[2]] == [(19, 1), (19, 1 | 1 << 8), (19, 1)] and len(arena.shadows) == 2
        # the built frame says the same: BEGIN, the shadowed layer's box, MASK, the mask, END
        edges, paths, styles = r.build_frame({"children": [dict(KIDS[0], shadow=DROP, mask=[KIDS[1]])]})
        assert hf.kinds(paths) == [2, 1, 4, 0, 3] and len(r.built_layers()) == 1
        assert styles[int(paths[1]["style"])].bitmap == api.BLUR_BASE
        r.build_frame({"children": [dict(KIDS[0], shadow=DROP), KIDS[2], dict(KIDS[1], shadow=other), bl._blurred(KIDS, 3, 3)]})
        assert [l[4] if len(l) == 5 else None for l in r.built_layers()] == [sm.as_dict(DROP), sm.as_dict(other), None]
    finally:
        r.close()


def test_a_stage_of_many_children_with_a_shadow_builds_in_one_walk(monkeypatch):
    monkeypatch.setenv("SWFR_BUILD_THREADS", "4")
    r = hf.host(W, H)
    try:
        many = [hf.tri((i % 250, 40, 90, 150), dx=(i % 7)) for i in range(300)]
        for _ in range(2):
            plain = r.build_frame({"children": many})
            assert r.built_layers() == []
            with_shadow = r.build_frame({"children": many + [_shadowed(KIDS)]})
            assert len(r.built_layers()) == 1 and r.built_layers()[0][4] == sm.as_dict(DROP)
            assert plain[1].tobytes() == with_shadow[1][:-1].tobytes() and plain[0].tobytes() == with_shadow[0][:-1].tobytes()
    finally:
        r.close()


def test_frames_without_a_shadow_build_what_they_built():
    """a sample of the existing scenes, the blurred ones among them: no shadow in what they build, and the same children inside a
    shadowed layer build, as the layer's sub-frame, exactly the arrays the scene builds as a frame.  (Not a comparison with arrays
    recorded before shadowed layers existed: the existing host tests of every family hold those.)"""
    sample = {}
    SC = scenarios.scenarios()
    for name in sorted(SC)[::6]:
        sample["scenario_" + name] = SC[name]
    for fam, scenes in (("layer", ls.overlap_scenes()), ("mask", ms.structure_scenes()), ("fade", fs.operator_scenes()), ("blur", bl.box_scenes())):
        for name in sorted(scenes)[::9]:
            sample["%s_%s" % (fam, name)] = scenes[name]
    assert len(sample) >= 14
    for name, sc in sample.items():
        r = hf.host(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")))
        try:
            for b in sc.get("bitmaps", []):
                r.add_bitmap(b)
            got = r.build_frame(sc["stage"])
            assert all(len(l) == 4 for l in r.built_layers()), name
            if name.startswith("blur_"):
                continue
            assert r.built_layers() == [] and not any(s.kind == api.STYLE_BITMAP and s.bitmap >= api.BLUR_BASE for s in got[2]), name
            wrapped = r.build_frame({"children": [{"type": "container", "children": sc["stage"]["children"], "shadow": DROP}]})
            assert len(wrapped[1]) == 1 and _same(r.built_layers()[0], got), name
        finally:
            r.close()
