"""Isolated layers on the host side (no GPU, host-only handles): the display-object type and its mode numbers, the refusals, the
marker paths swfr_build_frame emits (kinds, rectangles, balance), the lerp of the first and later paths inside a group, the parent's
"still clear" state behind each kind of group, threaded builds, and what swfr_upload_edges refuses."""
import os

import numpy as np
import pytest

import blend_model as bm
import blend_scenes as bs
import host_frames as hf
import layer_model as lm
import layer_scenes as ls
import scenarios
from scenarios import _rgba

BEGIN, END = lm.PATH_GROUP_BEGIN, lm.PATH_GROUP_END


def test_object_type_and_mode_numbers():
    from swf_renderer_amd import api
    assert api.OBJECT_LAYER == 8 and api.MAX_LAYER_DEPTH == lm.MAX_DEPTH and api.load_library().swfr_abi_version() == 1
    assert (api.PATH_GROUP_BEGIN, api.PATH_GROUP_END) == (BEGIN, END)
    assert api.layer_mode_number(True) == 1 and api.layer_mode_number("layer") == 2 and api.layer_mode_number("Multiply") == 3
    assert api.layer_mode_number(14) == 14
    r = hf.host()
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
        for mode in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
            rc, _, n_paths = hf.build_raw(r, hf.raw_stage(api.OBJECT_LAYER, mode, sid)[0])
            assert rc == api.OK and n_paths == 3, mode               # BEGIN, the triangle, END
        for mode in (9, 10, 11, 12):
            rc, err, _ = hf.build_raw(r, hf.raw_stage(api.OBJECT_LAYER, mode, sid)[0])
            assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
        for mode in (15, 16, 255, 0xffffffff):
            rc, _, _ = hf.build_raw(r, hf.raw_stage(api.OBJECT_LAYER, mode, sid)[0])
            assert rc == api.ERR_INVALID, mode
        for t in (4, 6, 7, 9, 10):                                   # not display-object types
            rc, err, _ = hf.build_raw(r, hf.raw_stage(t, 3, sid)[0])
            assert (rc, err) == (api.ERR_INVALID, "UnexpectedDisplayObjectType"), t
        rc, err, _ = hf.build_raw(r, hf.raw_stage(api.OBJECT_BLEND_MODE, 2, sid)[0])      # "layer" stays refused as a per-path blend mode
        assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode")
    finally:
        r.close()


def test_layer_key_lowers_to_a_type_8_wrapper_outside_the_others():
    """"layer" on a container, a shape and a morph shape; with "blend_mode" on the same object the paths carry the blend operator and
    the END marker the layer's"""
    SC = scenarios.scenarios()
    r = hf.host(100, 100)
    try:
        for layer, op in ((True, 0), ("normal", 0), ("layer", 0), (2, 0), ("screen", bm.OPERATORS["screen"]), (13, bm.OPERATORS["overlay"])):
            _, p, _ = r.build_frame({"children": [hf.tri((9, 9, 9, 200), layer=layer)]})
            assert hf.kinds(p) == [BEGIN, 0, END] and hf.lerps(p) == [0, 1, op << 8], layer
        _, p, _ = r.build_frame({"children": [hf.tri((1, 1, 1, 255)), {"type": "container", "layer": "add", "blend_mode": "multiply", "children": [
            hf.tri((9, 9, 9, 200)), hf.tri((9, 90, 9, 200), 7)]}]})
        mul = bm.OPERATORS["multiply"] << 8
        assert hf.kinds(p) == [0, BEGIN, 0, 0, END] and hf.lerps(p) == [1, 0, mul, mul, bm.OPERATORS["add"] << 8]
        morph = SC["morph_round_stroke_090"]["stage"]["children"][0]
        _, p, _ = r.build_frame({"children": [dict(morph, layer="darken")]})
        assert hf.kinds(p)[0] == BEGIN and hf.kinds(p)[-1] == END and len(p) > 3 and hf.lerps(p)[-1] == bm.OPERATORS["darken"] << 8
        assert r.build_frame({"children": [dict(morph, layer=False)]})[1].tobytes() == r.build_frame({"children": [morph]})[1].tobytes()
    finally:
        r.close()


def test_depth_limit():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        def nest(n):
            obj = hf.tri((9, 9, 9, 200))
            for k in range(n):
                obj = {"type": "container", "layer": ls.MODES[k % 9], "children": [hf.tri((k, 9, 9, 100), k), obj]}
            return {"children": [obj]}
        _, p, _ = r.build_frame(nest(4))
        assert hf.kinds(p) == [BEGIN, 0, BEGIN, 0, BEGIN, 0, BEGIN, 0, 0, END, END, END, END]
        with pytest.raises(api.SwfrError) as ei:
            r.build_frame(nest(5))
        assert ei.value.code == api.ERR_CAPACITY and "LayerDepth" in str(ei.value)
        # an empty fifth level is refused all the same: the limit is on the tree, not on what survives
        deep = nest(4)
        inner = deep["children"][0]
        for _ in range(3):
            inner = inner["children"][1]
        inner["children"][1] = {"type": "container", "layer": True, "children": []}
        with pytest.raises(api.SwfrError) as ei:
            r.build_frame(deep)
        assert ei.value.code == api.ERR_CAPACITY
    finally:
        r.close()


def test_marker_rectangles_and_balance():
    r = hf.host(64, 48)
    try:
        _, p, _ = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), ls._layer("multiply", [
            bs._rect(10, 12, 20, 30, (9, 9, 9, 100)), ls._layer("add", [bs._rect(40.5, 3.25, 70, 20, (9, 9, 9, 100)), bs._rect(90, 3, 99, 9, (1, 1, 1, 9))]),
            bs._rect(5, 40, 12, 60, (9, 9, 9, 100))])]})
        assert hf.kinds(p) == [0, BEGIN, 1, BEGIN, 1, END, 1, END]
        rects = hf.rects(p)
        assert rects[1] == rects[7] == (5, 3, 64, 48)                # the union of its members, clipped to the frame
        assert rects[3] == rects[5] == rects[4] == (40, 3, 64, 20)   # (the member off the frame left no path)
        assert all(int(p["n_edges"][i]) == 0 for i in (1, 3, 5, 7))
        assert hf.lerps(p) == [1, 0, 1, 0, 1, bm.OPERATORS["add"] << 8, 0, bm.OPERATORS["multiply"] << 8]
        # a group without surviving paths emits nothing
        _, p, _ = r.build_frame({"children": [ls._layer("screen", []), ls._layer("screen", [bs._rect(90, 3, 99, 9, (1, 1, 1, 9))]),
                                              ls._layer("normal", [hf.tri((255, 255, 255, 0))])]})
        assert len(p) == 0
    finally:
        r.close()


def test_lerp_of_the_first_and_later_paths_inside_a_group():
    """inside a group the surface is the group's: its first paint is a SOURCE lerp whatever lies below in the parent, later ones OVER,
    an opaque solid a lerp; ADD on the still-clear group surface is SOURCE; the other operators are never a lerp"""
    r = hf.host()
    try:
        ground = hf.tri((1, 2, 3, 255))
        _, p, _ = r.build_frame({"children": [ground, ls._layer("normal", [hf.tri((9, 9, 9, 100)), hf.tri((9, 9, 9, 100), 3), hf.tri((9, 9, 9, 255), 5)])]})
        assert hf.lerps(p) == [1, 0, 1, 0, 1, 0]
        add, mul = bm.OPERATORS["add"] << 8, bm.OPERATORS["multiply"] << 8
        _, p, _ = r.build_frame({"children": [ground, ls._layer("screen", [hf.tri((9, 9, 9, 100), blend_mode="add"), hf.tri((9, 9, 9, 255), 3, blend_mode="add")])]})
        assert hf.lerps(p) == [1, 0, 1, add, bm.OPERATORS["screen"] << 8]
        _, p, _ = r.build_frame({"children": [ground, ls._layer("screen", [hf.tri((9, 9, 9, 255), blend_mode="multiply"), hf.tri((9, 9, 9, 100), 3)])]})
        assert hf.lerps(p) == [1, 0, mul, 0, bm.OPERATORS["screen"] << 8]
        # a nested group starts clear again
        _, p, _ = r.build_frame({"children": [ls._layer("normal", [hf.tri((9, 9, 9, 100)), ls._layer("normal", [hf.tri((9, 9, 9, 100), 3)]), hf.tri((9, 9, 9, 100), 5)])]})
        assert hf.lerps(p) == [0, 1, 0, 1, 0, 0, 0]
    finally:
        r.close()


@pytest.mark.parametrize("mode", ls.MODES)
def test_parents_clear_state_after_each_kind_of_group(mode):
    """the lerp of a translucent path behind the group says what the group left of the parent's "still clear" state"""
    r = hf.host()
    try:
        after = hf.tri((200, 100, 50, 119), 9)
        clear_fill = hf.tri((255, 255, 255, 0))

        def following(group_kids):
            _, p, _ = r.build_frame({"children": [ls._layer(mode, group_kids), after]})
            return hf.lerps(p)[-1]
        for kids, still_clear in (([], True), ([bs._rect(90, 3, 99, 9, (1, 1, 1, 9))], True), ([clear_fill], True),
                                  ([dict(clear_fill, blend_mode="add")], True), ([dict(clear_fill, blend_mode="multiply")], False),
                                  ([ls._layer("normal", [])], True), ([ls._layer("screen", [])], False)):
            assert following(kids) == (1 if lm.parent_stays_clear(mode, still_clear) else 0), (mode, kids)
        assert following([hf.tri((9, 9, 9, 100))]) == 0                # a group that painted
        # a parent that was drawn on stays drawn on
        _, p, _ = r.build_frame({"children": [hf.tri((1, 1, 1, 9)), ls._layer(mode, []), after]})
        assert hf.lerps(p) == [1, 0]
    finally:
        r.close()


def _many(n=400):
    """n small objects, every fifth a layer of three overlapping triangles (enough display objects for a threaded build), the first
    object a layer without surviving paths"""
    rng = np.random.default_rng(7)
    kids = [ls._layer("add", [])]
    for i in range(n):
        x, y = rng.uniform(0, 50), rng.uniform(0, 36)
        col = (int(rng.integers(256)), 90, 200, int(rng.integers(1, 255)))
        t = bs._shape([(x, y), (x + 9.3, y + 2.1), (x + 3.2, y + 8.7)], col)
        if i % 5 == 0:
            kids.append(ls._layer(ls.MODES[(i // 5) % 9], [t, bs._shape([(x + 1, y), (x + 7.3, y + 4.1), (x + 2.2, y + 6.7)], col),
                                                           dict(t, blend_mode="multiply")]))
        else:
            kids.append(t)
    return {"children": [{"type": "container", "children": kids}]}


def test_threaded_build_is_the_single_walk():
    stage = _many()
    out = []
    for threads in ("1", "8"):
        os.environ["SWFR_BUILD_THREADS"] = threads
        try:
            r = hf.host()
            out.append(r.build_frame(stage))
            r.close()
        finally:
            del os.environ["SWFR_BUILD_THREADS"]
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    kinds, lerps = hf.kinds(out[0][1]), hf.lerps(out[0][1])
    assert kinds.count(BEGIN) == kinds.count(END) == 80
    assert kinds[0] == BEGIN and lerps[1] == 1                       # the empty ADD layer left the frame clear; the first group's first paint
    depth = 0
    for k, v in zip(kinds, lerps):
        depth += (k == BEGIN) - (k == END)
        assert 0 <= depth <= 1
    first_plain = next(i for i, k in enumerate(kinds) if k < BEGIN and i > 4)
    assert lerps[first_plain] == 0                                   # behind a group that painted nothing is a first paint any more


def test_upload_validates_the_markers():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        e, p, s = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), ls._layer("multiply", [
            hf.tri((9, 9, 9, 100)), ls._layer("add", [hf.tri((9, 9, 9, 100), 3)]), hf.tri((9, 9, 9, 100), 5)])]})
        assert hf.kinds(p) == [0, BEGIN, 0, BEGIN, 0, END, 0, END]

        def refused(edit, code=api.ERR_INVALID):
            q = p.copy()
            edit(q)
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, q, s)
            assert ei.value.code == code, ei.value
        refused(lambda q: None, api.ERR_NO_DEVICE)                   # the well-formed scene: a host-only handle cannot rasterize
        refused(lambda q: q["kind"].__setitem__(7, 0))               # BEGIN without END (and a path without edges is fine: still unbalanced)
        refused(lambda q: q["kind"].__setitem__(1, 0))               # END without BEGIN
        refused(lambda q: q["kind"].__setitem__(3, END))             # END, END: the inner pair reversed
        refused(lambda q: q["kind"].__setitem__(7, 4))               # unknown kind
        refused(lambda q: q["x_max"].__setitem__(7, int(q["x_max"][7]) - 1))      # the two rectangles differ
        refused(lambda q: q["y_min"].__setitem__(1, int(q["y_min"][1]) + 1))
        refused(lambda q: (q["x_max"].__setitem__(3, 30), q["x_max"].__setitem__(5, 30)))   # a member outside its group's rectangle

        def shrink_outer(q):                                         # the inner group outside the outer one's rectangle
            q["x_min"][1] = q["x_min"][7] = 4
        refused(shrink_outer)
        refused(lambda q: q["lerp"].__setitem__(5, (bm.OPERATORS["add"] << 8) | 1))         # bits 0..7 of END
        refused(lambda q: q["lerp"].__setitem__(1, 1))               # ... and of BEGIN
        refused(lambda q: q["lerp"].__setitem__(1, 3 << 8))          # BEGIN carries no operator
        refused(lambda q: q["lerp"].__setitem__(7, 9 << 8))          # no such operator
        refused(lambda q: q["lerp"].__setitem__(7, 1 << 16))
        refused(lambda q: q["n_edges"].__setitem__(1, 1))            # a marker has no edges
        # depth 5
        deep = np.concatenate([p[:1]] + [p[1:2]] * 5 + [p[2:3]] + [p[7:8]] * 5)
        for i in range(1, len(deep)):
            for k in ("x_min", "y_min", "x_max", "y_max"):
                deep[k][i] = p[k][2]
        with pytest.raises(api.SwfrError) as ei:
            r.upload_edges(e, deep, s)
        assert ei.value.code == api.ERR_INVALID
        with pytest.raises(api.SwfrError) as ei:                     # four deep passes the validation
            r.upload_edges(e, np.concatenate([deep[:5], deep[6:11]]), s)
        assert ei.value.code == api.ERR_NO_DEVICE
    finally:
        r.close()
