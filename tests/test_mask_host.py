"""Masked layers on the host side (no GPU, host-only handles): the display-object type, the path kind and the mode numbers, the
refusals, the three marker paths swfr_build_frame emits (order, shared rectangle), two levels per masked group at the depth limit, the
lerp of the first path of each half, the parent's "still clear" state behind each kind of masked group, threaded builds, and what
swfr_upload_edges refuses."""
import ctypes as C
import os

import numpy as np
import pytest

import blend_model as bm
import blend_scenes as bs
import host_frames as hf
import layer_scenes as ls
import mask_model as mk
import scenarios
from scenarios import _rgba

BEGIN, END, MASK = mk.PATH_GROUP_BEGIN, mk.PATH_GROUP_END, mk.PATH_GROUP_MASK


def _raw_masked_stage(mode, shape_ids, obj_type=11):
    """a stage holding one object of type 11 (or `obj_type`) whose children are plain shapes: the first is the mask"""
    from swf_renderer_amd import api
    kids = (api.DisplayObject * max(len(shape_ids), 1))()
    for k, sid in enumerate(shape_ids):
        kids[k].type, kids[k].id = api.OBJECT_SHAPE, sid
    d = api.DisplayObject()
    d.type, d.id = obj_type, mode
    d.n_children, d.children = len(shape_ids), C.cast(kids, C.POINTER(api.DisplayObject))
    objs = (api.DisplayObject * 1)(d)
    s = api.Stage()
    s.width = s.height = 16
    s.n_children, s.children = 1, C.cast(objs, C.POINTER(api.DisplayObject))
    return s, (kids, objs)


def test_type_kind_and_mode_numbers():
    from swf_renderer_amd import api
    assert api.OBJECT_MASKED_LAYER == mk.OBJECT_MASKED_LAYER == 11 and api.PATH_GROUP_MASK == MASK == 4
    assert api.MAX_LAYER_DEPTH == mk.MAX_DEPTH == 4 and api.load_library().swfr_abi_version() == 1
    r = hf.host()
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
        for mode in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
            rc, _, n_paths = hf.build_raw(r, _raw_masked_stage(mode, [sid, sid])[0])
            assert rc == api.OK and n_paths == 5, mode               # BEGIN, the content, MASK, the mask, END
        for mode in (9, 10, 11, 12):
            rc, err, _ = hf.build_raw(r, _raw_masked_stage(mode, [sid, sid])[0])
            assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
        for mode in (15, 16, 255, 0xffffffff):
            rc, _, _ = hf.build_raw(r, _raw_masked_stage(mode, [sid, sid])[0])
            assert rc == api.ERR_INVALID, mode
        rc, err, _ = hf.build_raw(r, _raw_masked_stage(1, [])[0])
        assert (rc, err) == (api.ERR_INVALID, "MaskedLayerWithoutMask")
        rc, _, n_paths = hf.build_raw(r, _raw_masked_stage(1, [sid])[0])           # a mask and no content: nothing to paint
        assert rc == api.OK and n_paths == 0
        for t in (4, 6, 7, 9, 10, 12):                               # not display-object types
            rc, err, _ = hf.build_raw(r, _raw_masked_stage(3, [sid, sid], obj_type=t)[0])
            assert (rc, err) == (api.ERR_INVALID, "UnexpectedDisplayObjectType"), t
    finally:
        r.close()


def test_mask_key_lowers_to_a_type_11_wrapper():
    """"mask" on a container, a shape and a morph shape; the mode comes from "layer" (absent: normal); the mask list is children[0],
    outside the object's own matrix, colour transform and blend mode"""
    from swf_renderer_amd import api
    SC = scenarios.scenarios()
    r = hf.host(100, 100)
    try:
        mask = [hf.tri((0, 0, 0, 255), 4)]
        for layer, op in ((None, 0), (True, 0), ("normal", 0), ("layer", 0), (False, 0), ("screen", bm.OPERATORS["screen"]), (13, bm.OPERATORS["overlay"])):
            obj = hf.tri((9, 9, 9, 200), mask=mask)
            if layer is not None:
                obj["layer"] = layer
            _, p, _ = r.build_frame({"children": [obj]})
            assert hf.kinds(p) == [BEGIN, 0, MASK, 0, END] and hf.lerps(p) == [0, 1, 0, 1, op << 8], layer
        # the wrapper's children: the mask container first, the object second; the object's blend mode stays with the object
        arena = api._Arena()
        w = r._object(arena, dict(hf.tri((9, 9, 9, 200), blend_mode="multiply", matrix=scenarios._m(1, 1, 600, 0)), mask=mask, layer="add"))
        assert (w.type, w.id, w.n_children, w.has_matrix) == (api.OBJECT_MASKED_LAYER, 8, 2, 0)
        assert (w.children[0].type, w.children[0].has_matrix, w.children[0].n_children) == (api.OBJECT_CONTAINER, 0, 1)
        assert w.children[1].type == api.OBJECT_BLEND_MODE
        _, p, _ = r.build_frame({"children": [hf.tri((1, 1, 1, 255)), dict(hf.tri((9, 9, 9, 200), blend_mode="multiply", matrix=scenarios._m(1, 1, 600, 0)), mask=mask, layer="add")]})
        mul = bm.OPERATORS["multiply"] << 8
        assert hf.kinds(p) == [0, BEGIN, 0, MASK, 0, END] and hf.lerps(p) == [1, 0, mul, 0, 1, bm.OPERATORS["add"] << 8]
        rects = hf.rects(p)
        assert rects[2][0] == rects[4][0] + 30 - 4                   # the matrix (30 px) moved the object, not the mask (drawn 4 px right)
        morph = SC["morph_round_stroke_090"]["stage"]["children"][0]
        _, p, _ = r.build_frame({"children": [dict(morph, mask=mask, layer="darken")]})
        k = hf.kinds(p)
        assert k[0] == BEGIN and k[-1] == END and k.count(MASK) == 1 and k[-3:] == [MASK, 0, END] and hf.lerps(p)[-1] == bm.OPERATORS["darken"] << 8
    finally:
        r.close()


def test_marker_order_and_shared_rectangles():
    r = hf.host(64, 48)
    try:
        _, p, _ = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), hf.masked("multiply", [
            bs._rect(10, 12, 20, 30, (9, 9, 9, 100)), ls._layer("add", [bs._rect(40.5, 3.25, 70, 20, (9, 9, 9, 100)), bs._rect(90, 3, 99, 9, (1, 1, 1, 9))])],
            [bs._rect(5, 40, 12, 60, (9, 9, 9, 100)), ls._layer("screen", [bs._rect(2, 1, 4, 3, (9, 9, 9, 100))])])]})
        assert hf.kinds(p) == [0, BEGIN, 1, BEGIN, 1, END, MASK, 1, BEGIN, 1, END, END]
        rects = hf.rects(p)
        assert rects[1] == rects[6] == rects[11] == (2, 1, 64, 48)   # the union of all members, content and mask, clipped to the frame
        assert rects[3] == rects[5] == (40, 3, 64, 20) and rects[8] == rects[10] == (2, 1, 4, 3)
        assert all(int(p["n_edges"][i]) == 0 for i in (1, 3, 5, 6, 8, 10, 11))
        assert hf.lerps(p) == [1, 0, 1, 0, 1, bm.OPERATORS["add"] << 8, 0, 1, 0, 1, bm.OPERATORS["screen"] << 8, bm.OPERATORS["multiply"] << 8]
        # a half without surviving paths: nothing at all is emitted, under any operator
        off = bs._rect(90, 3, 99, 9, (1, 1, 1, 9))
        for mode in ls.MODES:
            e, p, _ = r.build_frame({"children": [hf.masked(mode, [hf.tri((9, 9, 9, 100))], []), hf.masked(mode, [hf.tri((9, 9, 9, 100))], [off]),
                                                  hf.masked(mode, [], [hf.tri((9, 9, 9, 100))]), hf.masked(mode, [off], [hf.tri((9, 9, 9, 100))]),
                                                  hf.masked(mode, [hf.tri((255, 255, 255, 0))], [hf.tri((9, 9, 9, 100))]),
                                                  hf.masked(mode, [hf.tri((9, 9, 9, 100))], [hf.tri((255, 255, 255, 0))])]})
            assert len(p) == 0 and len(e) == 0, mode
        # ... and what follows is built as if the masked group were not there
        e0, p0, _ = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), hf.tri((9, 9, 9, 77), 3)]})
        e1, p1, _ = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), hf.masked("screen", [hf.tri((9, 9, 9, 100))], [off]), hf.tri((9, 9, 9, 77), 3)]})
        assert e0.tobytes() == e1.tobytes() and p0["first_edge"].tolist() == p1["first_edge"].tolist() and hf.rects(p0) == hf.rects(p1)
    finally:
        r.close()


def test_two_levels_per_masked_group_at_the_depth_limit():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        t = lambda k: hf.tri((k, 9, 9, 100), k)
        two = hf.masked("add", [t(1), hf.masked("screen", [t(2)], [t(3)])], [t(4)])                 # masked inside masked: four levels
        _, p, _ = r.build_frame({"children": [two]})
        assert hf.kinds(p) == [BEGIN, 0, BEGIN, 0, MASK, 0, END, MASK, 0, END]
        r2 = hf.masked("add", [t(1)], [t(2), hf.masked("screen", [t(3)], [t(4)])])                  # ... in the mask half
        assert hf.kinds(r.build_frame({"children": [r2]})[1]) == [BEGIN, 0, MASK, 0, BEGIN, 0, MASK, 0, END, END]
        _, p, _ = r.build_frame({"children": [ls._layer("normal", [ls._layer("multiply", [t(0), hf.masked("add", [t(1)], [t(2)])])])]})
        assert hf.kinds(p) == [BEGIN, BEGIN, 0, BEGIN, 0, MASK, 0, END, END, END]                 # a masked group inside two plain layers
        for tree in (ls._layer("normal", [two]),                                                # two masked groups nested plus one more group
                     hf.masked("add", [t(1), hf.masked("screen", [t(2), ls._layer("normal", [t(5)])], [t(3)])], [t(4)]),
                     hf.masked("add", [t(1), hf.masked("screen", [t(2)], [t(3), ls._layer("normal", [t(5)])])], [t(4)]),
                     hf.masked("add", [t(1)], [t(4), hf.masked("screen", [t(2)], [t(3), ls._layer("normal", [])])]),   # (an empty one counts: the limit is on the tree)
                     ls._layer("normal", [ls._layer("normal", [ls._layer("normal", [hf.masked("add", [t(1)], [t(2)])])])])):
            with pytest.raises(api.SwfrError) as ei:
                r.build_frame({"children": [tree]})
            assert ei.value.code == api.ERR_CAPACITY and "LayerDepth" in str(ei.value)
    finally:
        r.close()


def test_lerp_of_the_first_path_of_each_half():
    """both halves are group surfaces that start clear: the first paint in each is a SOURCE lerp whatever lies below, later ones OVER;
    ADD on the still-clear surface is SOURCE; the other operators are never a lerp"""
    r = hf.host()
    try:
        ground = hf.tri((1, 2, 3, 255))
        _, p, _ = r.build_frame({"children": [ground, hf.masked("normal", [hf.tri((9, 9, 9, 100)), hf.tri((9, 9, 9, 100), 3)],
                                                              [hf.tri((9, 9, 9, 100), 1), hf.tri((9, 9, 9, 100), 4), hf.tri((9, 9, 9, 255), 5)])]})
        assert hf.kinds(p) == [0, BEGIN, 0, 0, MASK, 0, 0, 0, END] and hf.lerps(p) == [1, 0, 1, 0, 0, 1, 0, 1, 0]
        add, mul = bm.OPERATORS["add"] << 8, bm.OPERATORS["multiply"] << 8
        _, p, _ = r.build_frame({"children": [ground, hf.masked("screen", [hf.tri((9, 9, 9, 100), blend_mode="add"), hf.tri((9, 9, 9, 255), 3, blend_mode="add")],
                                                              [hf.tri((9, 9, 9, 100), blend_mode="multiply"), hf.tri((9, 9, 9, 100), 3)])]})
        assert hf.lerps(p) == [1, 0, 1, add, 0, mul, 0, bm.OPERATORS["screen"] << 8]
    finally:
        r.close()


@pytest.mark.parametrize("mode", ls.MODES)
def test_parents_clear_state_after_each_kind_of_masked_group(mode):
    """the lerp of a translucent path behind the masked group says what it left of the parent's "still clear" state
    (mask_model.nothing_to_do, libcairo's rule: tests/test_mask_model.py)"""
    r = hf.host()
    try:
        after = hf.tri((200, 100, 50, 119), 9)
        paint = hf.tri((9, 9, 9, 100))
        clear_fill = hf.tri((255, 255, 255, 0))                        # OVER with a clear source: the surface stays clear
        drawn_zero = dict(clear_fill, blend_mode="multiply")         # drawn on, every pixel zero

        def following(content, mask):
            _, p, _ = r.build_frame({"children": [hf.masked(mode, content, mask), after]})
            return hf.lerps(p)[-1]
        halves = {True: ([], [clear_fill], [bs._rect(90, 3, 99, 9, (1, 1, 1, 9))], [ls._layer("normal", [])]),
                  False: ([paint], [drawn_zero], [ls._layer("screen", [])])}
        for content_clear in (True, False):
            for mask_clear in (True, False):
                for content in halves[content_clear]:
                    for mask in halves[mask_clear]:
                        want = 1 if mk.nothing_to_do(mode, content_clear, mask_clear) else 0
                        assert following(content, mask) == want, (mode, content, mask)
        # a parent that was drawn on stays drawn on
        _, p, _ = r.build_frame({"children": [hf.tri((1, 1, 1, 9)), hf.masked(mode, [], []), after]})
        assert hf.lerps(p) == [1, 0]
    finally:
        r.close()


def _many(n=400):
    """n small objects, every fifth a masked group (enough display objects for a threaded build), the first object a masked group
    that leaves the frame clear"""
    rng = np.random.default_rng(7)
    kids = [hf.masked("add", [], [hf.tri((9, 9, 9, 9))])]
    for i in range(n):
        x, y = rng.uniform(0, 50), rng.uniform(0, 36)
        col = (int(rng.integers(256)), 90, 200, int(rng.integers(1, 255)))
        t = bs._shape([(x, y), (x + 9.3, y + 2.1), (x + 3.2, y + 8.7)], col)
        if i % 5 == 0:
            kids.append(hf.masked(ls.MODES[(i // 5) % 9], [t, dict(t, blend_mode="multiply")],
                                [bs._shape([(x + 1, y), (x + 7.3, y + 4.1), (x + 2.2, y + 6.7)], col), ls._layer("screen", [t])]))
        else:
            kids.append(t)
    return {"children": [{"type": "container", "children": kids}]}


def test_threaded_builds_are_the_single_walk():
    stage = _many()
    out = []
    for threads in ("1", "2", "3", "8"):
        os.environ["SWFR_BUILD_THREADS"] = threads
        try:
            r = hf.host()
            out.append(r.build_frame(stage))
            r.close()
        finally:
            del os.environ["SWFR_BUILD_THREADS"]
    for o in out[1:]:
        assert out[0][0].tobytes() == o[0].tobytes() and out[0][1].tobytes() == o[1].tobytes()
        assert [bytes(s) for s in out[0][2]] == [bytes(s) for s in o[2]]
    kinds, lerps = hf.kinds(out[0][1]), hf.lerps(out[0][1])
    assert kinds.count(MASK) == 80 and kinds.count(BEGIN) == kinds.count(END) == 160
    assert kinds[:2] == [BEGIN, 0] and lerps[1] == 1                 # the first group left the frame clear and emitted nothing
    first_plain = next(i for i, k in enumerate(kinds) if k == 0 and i > kinds.index(END))
    assert lerps[first_plain] == 0                                   # behind a group that painted nothing is a first paint any more


def test_upload_validates_the_markers():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        t = lambda k: hf.tri((k, 9, 9, 100), k)
        e, p, s = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), hf.masked("multiply", [t(1), ls._layer("add", [t(2)])], [t(3), t(4)])]})
        assert hf.kinds(p) == [0, BEGIN, 0, BEGIN, 0, END, MASK, 0, 0, END]

        def refused(edit, code=api.ERR_INVALID, q=None):
            q = (p if q is None else q).copy()
            edit(q)
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, q, s)
            assert ei.value.code == code, ei.value
        refused(lambda q: None, api.ERR_NO_DEVICE)                   # the well-formed scene: a host-only handle cannot rasterize
        refused(lambda q: q["kind"].__setitem__(0, MASK))            # a MASK outside a group
        refused(lambda q: q["kind"].__setitem__(7, MASK))            # a second MASK in one group
        refused(lambda q: q["x_max"].__setitem__(6, int(q["x_max"][6]) - 1))       # its rectangle differs from its group's
        refused(lambda q: q["y_min"].__setitem__(6, int(q["y_min"][6]) + 1))
        refused(lambda q: q["n_edges"].__setitem__(6, 1))            # a MASK with edges
        refused(lambda q: q["lerp"].__setitem__(6, 1))               # ... with a lerp
        refused(lambda q: q["lerp"].__setitem__(6, 3 << 8))          # ... with an operator
        refused(lambda q: q["kind"].__setitem__(9, MASK))            # BEGIN without END (and a second MASK)
        refused(lambda q: q["kind"].__setitem__(6, 5))               # unknown kind
        # depth: a masked group takes two levels -- masked in masked passes, one more group around or inside is refused
        m = p[4:5]
        inner = np.concatenate([p[1:2], m, p[6:7], m, p[9:10]])      # BEGIN member MASK member END
        for i in range(len(inner)):
            for k in ("x_min", "y_min", "x_max", "y_max"):
                inner[k][i] = m[k][0]
        plain_b, plain_e, mask_m = inner[0:1], inner[4:5], inner[2:3]
        twice = np.concatenate([plain_b, m, plain_b, m, mask_m, m, plain_e, mask_m, m, plain_e])
        refused(lambda q: None, api.ERR_NO_DEVICE, twice)
        refused(lambda q: None, api.ERR_INVALID, np.concatenate([plain_b, twice, plain_e]))
        refused(lambda q: None, api.ERR_INVALID, np.concatenate([twice[:3], plain_b, m, plain_e, twice[3:]]))
        refused(lambda q: None, api.ERR_INVALID, np.concatenate([twice[:6], plain_b, m, plain_e, twice[6:]]))
        refused(lambda q: None, api.ERR_NO_DEVICE, np.concatenate([twice[:8], plain_b, m, plain_e, twice[8:]]))       # (behind the inner group: 2 + 1)
        refused(lambda q: None, api.ERR_NO_DEVICE, np.concatenate([plain_b, plain_b, inner, plain_e, plain_e]))
        refused(lambda q: None, api.ERR_INVALID, np.concatenate([plain_b, plain_b, plain_b, inner, plain_e, plain_e, plain_e]))
    finally:
        r.close()
