"""Blurred layers on host-only handles (no GPU): what the frame builder makes of a SWFR_OBJECT_BLURRED_LAYER -- the parent's one box
path and its style, the sub-frame swfr_built_layer hands out -- every refusal by code and name, where the Python mirror puts the
type-16 wrapper next to "mask" and "opacity", and that frames without a "blur" build what they built before.
"""
import pytest

import blur_scenes as bl
import fade_scenes as fs
import host_frames as hf
import layer_scenes as ls
import mask_scenes as ms
import scenarios
from blend_scenes import _rgba
from swf_renderer_amd import api

W, H = 64, 48
OPS = {"normal": 0, "layer": 0, "multiply": 1, "screen": 2, "lighten": 3, "darken": 4, "difference": 5, "add": 6, "overlay": 7, "hardlight": 8}


def _same(a, b):
    ea, pa, sa = a[:3]
    eb, pb, sb = b[:3]
    return (ea.tobytes() == eb.tobytes() and pa.tobytes() == pb.tobytes() and len(sa) == len(sb) and all(bytes(x) == bytes(y) for x, y in zip(sa, sb)))


def _blurred(kids, x, y, passes=1, mode=None, **kw):
    return bl._blurred(kids, x, y, passes, mode, **kw)


KIDS = [hf.tri((230, 40, 90, 150)), hf.tri((40, 200, 120, 119), dx=9.5), bl._rect(10.5, 8, 50, 40.25, (20, 60, 240, 255))]


@pytest.mark.parametrize("aliased", (False, True), ids=("antialiased", "aliased"))
@pytest.mark.parametrize("mode", sorted(OPS))
def test_parent_path_and_sub_frame(mode, aliased):
    r = hf.host(W, H, antialias="none" if aliased else "default")
    try:
        ground = [hf.tri((9, 9, 9, 255), dx=-1)]
        mat = scenarios._m(0.9, 1.1, 3, 2)
        edges, paths, styles = r.build_frame({"children": ground + [_blurred(KIDS, 5, 0, 3, mode, matrix=mat)] + ground})
        layers = r.built_layers()
        assert len(layers) == 1 and layers[0][3] == (5, 0, 3)
        # the parent: ground, ONE box path over the whole frame, ground
        assert hf.kinds(paths) == [api.PATH_TOR, api.PATH_BOXES, api.PATH_TOR]
        p = paths[1]
        assert hf.rects(paths)[1] == (0, 0, W, H) and int(p["n_edges"]) == 1 and int(p["fill_rule"]) == 0
        assert int(p["lerp"]) == OPS[mode] << 8                      # lerp bits 0, the operator in bits 8..15
        e = edges[int(p["first_edge"])]
        assert [int(e[k]) for k in ("x1", "y1", "x2", "y2", "top", "bottom", "dir", "reserved")] == [0, 0, W * 256, H * 256, 0, H * 256, 1, 1]
        st = styles[int(p["style"])]
        assert (st.kind, st.bitmap, st.extend, st.filter) == (api.STYLE_BITMAP, api.BLUR_BASE, 0, 1) and list(st.inv) == [1, 0, 0, 1, 0, 0]
        assert hf.lerps(paths)[2] == 1                               # (an opaque triangle is a SOURCE lerp wherever it stands)
        # the sub-frame: what the same children build as a stage of their own, under the same matrix
        own = r.build_frame({"children": [{"type": "container", "matrix": mat, "children": KIDS}]})
        assert r.built_layers() == []
        assert _same(layers[0], own)
        assert hf.lerps(layers[0][1])[0] == 1                        # the surface-is-clear state starts afresh: the first translucent paint is a SOURCE lerp
    finally:
        r.close()


def test_sub_frame_inherits_colour_transform_and_blend_mode_and_counts_its_own_depth():
    r = hf.host(W, H)
    try:
        import make_cxform_goldens as mk
        ct = mk.cxform(mult=(256, 200, 128, 160), add=(0, 20, 60, 0))
        inner = [ls._layer("multiply", [ls._layer("screen", [ls._layer("add", [ls._layer("normal", KIDS)])])])]       # four levels inside
        stage = {"children": [{"type": "container", "color_transform": ct, "blend_mode": "darken", "children": [
            ls._layer("normal", [ls._layer("normal", [ls._layer("normal", [_blurred(inner, 3, 3)])])])]}]}              # three levels around
        edges, paths, styles = r.build_frame(stage)
        layers = r.built_layers()
        own = r.build_frame({"children": [{"type": "container", "color_transform": ct, "blend_mode": "darken", "children": inner}]})
        assert _same(layers[0], own)
        assert hf.kinds(paths) == [2, 2, 2, 1, 3, 3, 3]
    finally:
        r.close()


def test_two_layers_are_numbered_in_painters_order_and_many_children_build_alike():
    r = hf.host(W, H)
    try:
        a, b = _blurred(KIDS[:1], 2, 2), _blurred(KIDS[1:], 0, 9, 2, "screen")
        edges, paths, styles = r.build_frame({"children": [a, KIDS[0], b]})
        assert [styles[int(p["style"])].bitmap for p in paths if int(p["kind"]) == api.PATH_BOXES and int(p["x_max"]) == W][:2] == [api.BLUR_BASE, api.BLUR_BASE + 1]
        assert [l[3] for l in r.built_layers()] == [(2, 2, 1), (0, 9, 2)]
        # a stage of several hundred children is built in pieces by worker threads -- unless it holds a blurred layer: the same arrays
        many = [hf.tri((i % 250, 40, 90, 150), dx=(i % 7)) for i in range(300)]
        plain = r.build_frame({"children": many})
        with_blur = r.build_frame({"children": many + [a]})
        assert len(r.built_layers()) == 1
        assert plain[1].tobytes() == with_blur[1][:-1].tobytes() and plain[0].tobytes() == with_blur[0][:-1].tobytes()
    finally:
        r.close()


def test_a_frame_built_in_pieces_forgets_the_last_frames_layers(monkeypatch):
    """a plain stage of several hundred children is built by worker builders, never by a walk of the handle's own builder: the
    sub-frames of the frame before it are gone all the same"""
    monkeypatch.setenv("SWFR_BUILD_THREADS", "4")                     # (read at the handle's first build)
    r = hf.host(W, H)
    try:
        many = [hf.tri((i % 250, 40, 90, 150), dx=(i % 7)) for i in range(300)]
        for _ in range(2):
            r.build_frame({"children": [_blurred(KIDS, 3, 3), _blurred(KIDS[:1], 2, 2)]})
            assert len(r.built_layers()) == 2
            r.build_frame({"children": many})
            assert r.built_layers() == [] and r.L.swfr_built_layers(r.h) == 0
    finally:
        r.close()


def test_alpha_and_erase_modes_need_the_flag():
    for alpha_modes in (False, True):
        r = hf.host(W, H, alpha_modes=alpha_modes)
        try:
            sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
            for mode in (11, 12):
                rc, err, n_paths = hf.build_raw(r, hf.raw_stage(api.OBJECT_BLURRED_LAYER, mode | 3 << 8 | 3 << 16 | 1 << 24, sid)[0])
                if not alpha_modes:
                    assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
                else:
                    # erase is a path's operator; alpha is a group's only: the path sits in a group of its own over the whole frame
                    assert rc == api.OK and n_paths == (3 if mode == 11 else 1), mode
        finally:
            r.close()


def test_refusals_by_code_and_name():
    r = hf.host(W, H)
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))

        def raw(mode, bx, by, passes, t=api.OBJECT_BLURRED_LAYER):
            return hf.build_raw(r, hf.raw_stage(t, mode | bx << 8 | by << 16 | passes << 24, sid)[0])
        for mode in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
            rc, _, n_paths = raw(mode, 255, 0, 15)
            assert rc == api.OK and n_paths == 1 and r.L.swfr_built_layers(r.h) == 1, mode
        for mode in (9, 10, 11, 12):
            assert raw(mode, 3, 3, 1)[:2] == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
        for mode in (15, 16, 255):
            assert raw(mode, 3, 3, 1)[0] == api.ERR_INVALID, mode
        for passes in (0, 16, 255):
            assert raw(1, 3, 3, passes)[:2] == (api.ERR_INVALID, "InvalidBlur"), passes
        for t in (14, 15, 17, 18, 255):                              # still not display-object types
            assert raw(1, 3, 3, 1, t=t)[:2] == (api.ERR_INVALID, "UnexpectedDisplayObjectType"), t
        # a blurred layer below another, however far below
        nested = {"children": [_blurred([ls._layer("normal", [{"type": "container", "children": [_blurred(KIDS, 2, 2)]}])], 3, 3)]}
        with pytest.raises(api.SwfrError) as e:
            r.build_frame(nested)
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NestedBlur" in str(e.value)
        # eight in a frame, not nine
        r.build_frame({"children": [_blurred(KIDS[:1], 2, 2) for _ in range(api.MAX_BLUR_LAYERS)]})
        assert len(r.built_layers()) == api.MAX_BLUR_LAYERS
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [_blurred(KIDS[:1], 2, 2) for _ in range(api.MAX_BLUR_LAYERS + 1)]})
        assert e.value.code == api.ERR_CAPACITY and "BlurLayers" in str(e.value)
        # swfr_built_layer past the end
        r.build_frame({"children": [_blurred(KIDS, 2, 2)]})
        none = [None] * 9
        assert r.L.swfr_built_layer(r.h, 0, *none) == api.OK and r.L.swfr_built_layer(r.h, 1, *none) == api.ERR_NOT_FOUND
        # the two primitives: arguments first, then the device they need
        for bad in ((256, 0, 1), (0, 256, 1), (3, 3, 0), (3, 3, 16)):
            with pytest.raises(api.SwfrError) as e:
                r.blur_bitmap(1, *bad)
            assert e.value.code == api.ERR_INVALID and "InvalidBlur" in str(e.value), bad
        with pytest.raises(api.SwfrError) as e:
            r.blur_bitmap(1, 3, 3, 1)
        assert e.value.code == api.ERR_NO_DEVICE
        with pytest.raises(api.SwfrError) as e:
            r.capture_bitmap(1)
        assert e.value.code == api.ERR_NO_DEVICE
        with pytest.raises(api.SwfrError) as e:
            r.render({"children": [_blurred(KIDS, 2, 2)]})
        assert e.value.code == api.ERR_NO_DEVICE
        # the Python mirror's own checks
        for bad in ({"x": -1, "y": 0}, {"x": 256, "y": 0}, {"x": 1.5, "y": 0}, {"x": 1, "y": 1, "passes": 256}, 3):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [dict(_blurred(KIDS, 2, 2), blur=bad)]})
            assert e.value.code == api.ERR_INVALID and "InvalidBlur" in str(e.value), bad
        for passes in (0, 16):
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [_blurred(KIDS, 2, 2, passes)]})
            assert e.value.code == api.ERR_INVALID and "InvalidBlur" in str(e.value), passes
        assert r.build_frame({"children": [dict(_blurred(KIDS, 2, 2), blur={"x": 4})]}) and r.built_layers()[0][3] == (4, 0, 1)      # passes defaults to 1
    finally:
        r.close()


def _tree(r, obj):
    """(type, mode or id, [children]) of the display object the mirror makes of `obj`"""
    arena = api._Arena()
    d = r._object(arena, obj)

    def walk(d):
        return (d.type, d.id, [walk(d.children[i]) for i in range(d.n_children)])
    return walk(d), arena


def test_wrapper_order_next_to_mask_and_opacity():
    r = hf.host(W, H)
    try:
        blur = {"x": 3, "y": 4, "passes": 2}
        bid = 3 << 8 | 4 << 16 | 2 << 24
        ct = {"red_mult": 0.5}
        shape = dict(KIDS[0], matrix=scenarios._m(1, 1, 2, 2), blend_mode="multiply", color_transform=ct)
        # alone: type 16 with the mode of "layer", the blend-mode and colour-transform wrappers and the matrix inside
        t, _ = _tree(r, dict(shape, blur=blur, layer="screen"))
        assert t[:2] == (16, 4 | bid) and t[2][0][:2] == (5, 3) and t[2][0][2][0][0] == 3 and t[2][0][2][0][2][0][0] == 0
        t, _ = _tree(r, dict(shape, blur=blur))
        assert t[:2] == (16, 1 | bid)
        # with "mask": type 11 takes the mode, the blurred layer is its content, composited normally
        t, _ = _tree(r, dict(shape, blur=blur, layer="screen", mask=[KIDS[1]]))
        assert t[:2] == (11, 4) and t[2][0][0] == 2 and t[2][1][:2] == (16, 1 | bid) and t[2][1][2][0][:2] == (5, 3)
        # with "opacity": type 13 takes the mode
        t, _ = _tree(r, dict(shape, blur=blur, layer="screen", opacity=77))
        assert t[:2] == (13, 4 | 77 << 8) and t[2][0][:2] == (16, 1 | bid)
        # with both: 13 around 11 around 16
        t, _ = _tree(r, dict(shape, blur=blur, layer="add", opacity=77, mask=[KIDS[1]]))
        assert t[:2] == (13, 8 | 77 << 8) and t[2][0][:2] == (11, 1) and t[2][0][2][1][:2] == (16, 1 | bid)
        # the built frame says the same: BEGIN, the blurred layer's box, MASK, the mask, END
        edges, paths, styles = r.build_frame({"children": [dict(KIDS[0], blur=blur, mask=[KIDS[1]])]})
        assert hf.kinds(paths) == [2, 1, 4, 0, 3] and len(r.built_layers()) == 1
        assert styles[int(paths[1]["style"])].bitmap == api.BLUR_BASE
    finally:
        r.close()


def test_frames_without_a_blur_build_what_they_built():
    """a sample of the existing scenes: no blurred layers and no blur texture in what they build, and the same children inside a
    1 x 1 blurred layer build, as the layer's sub-frame, exactly the arrays the scene builds as a frame.  (Not a comparison with arrays
    recorded before blurred layers existed: the existing host tests of every family hold those.)"""
    sample = {}
    SC = scenarios.scenarios()
    for name in sorted(SC)[::6]:
        sample["scenario_" + name] = SC[name]
    for fam, scenes in (("layer", ls.overlap_scenes()), ("mask", ms.structure_scenes()), ("fade", fs.operator_scenes())):
        for name in sorted(scenes)[::9]:
            sample["%s_%s" % (fam, name)] = scenes[name]
    assert len(sample) >= 12
    for name, sc in sample.items():
        r = hf.host(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")))
        try:
            for b in sc.get("bitmaps", []):
                r.add_bitmap(b)
            got = r.build_frame(sc["stage"])
            assert r.built_layers() == [], name
            assert not any(s.kind == api.STYLE_BITMAP and s.bitmap >= api.BLUR_BASE for s in got[2]), name
            # the same children inside a 1 x 1 blurred layer: the sub-frame is the frame
            wrapped = r.build_frame({"children": [{"type": "container", "children": sc["stage"]["children"], "blur": {"x": 1, "y": 1}}]})
            assert len(wrapped[1]) == 1 and _same(r.built_layers()[0], got), name
        finally:
            r.close()
