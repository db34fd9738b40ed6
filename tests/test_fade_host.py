"""Layer opacity on the host side (no GPU, host-only handles): the display-object type and its id (mode | opacity << 8), the
refusals, the markers swfr_build_frame emits and the fade in END's lerp, one level per faded group at the depth limit among the other
layer types, opacity 0 and 255, the parent's "still clear" state behind each kind of faded group, threaded builds, the Python lowering
of "opacity" (with "layer" and with "mask"), and what swfr_upload_edges refuses."""
import ctypes as C
import os

import numpy as np
import pytest

import blend_model as bm
import blend_scenes as bs
import fade_model as fd
import host_frames as hf
import layer_scenes as ls
import scenarios
from scenarios import _rgba

BEGIN, END, MASK = fd.PATH_GROUP_BEGIN, fd.PATH_GROUP_END, fd.PATH_GROUP_MASK


def _faded(mode, opacity, kids, **kw):
    obj = {"type": "container", "children": list(kids), "opacity": opacity, **kw}
    if mode is not None:
        obj["layer"] = mode
    return obj


def _ulerps(p):
    return [int(v) & 0xffffffff for v in p["lerp"]]


def test_type_and_id():
    from swf_renderer_amd import api
    assert api.OBJECT_FADED_LAYER == fd.OBJECT_FADED_LAYER == 13 and api.MAX_LAYER_DEPTH == fd.MAX_DEPTH == 4
    assert api.load_library().swfr_abi_version() == 1
    r = hf.host()
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
        for mode in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
            for opacity in (1, 128, 254, 255):
                rc, _, n_paths = hf.build_raw(r, hf.raw_stage(13, mode | opacity << 8, sid)[0])
                assert rc == api.OK and n_paths == 3, (mode, opacity)                      # BEGIN, the shape, END
            rc, _, n_paths = hf.build_raw(r, hf.raw_stage(13, mode, sid)[0])                  # opacity 0: nothing is emitted
            assert rc == api.OK and n_paths == 0, mode
        for mode in (9, 10, 11, 12):
            for opacity in (0, 128, 255):
                rc, err, _ = hf.build_raw(r, hf.raw_stage(13, mode | opacity << 8, sid)[0])
                assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), (mode, opacity)
        for mode in (15, 16, 255):
            for opacity in (0, 128, 255):
                rc, _, _ = hf.build_raw(r, hf.raw_stage(13, mode | opacity << 8, sid)[0])
                assert rc == api.ERR_INVALID, (mode, opacity)
        for bad in (0x10000, 0x10001, 0x1ff01, 0x01000001, 0xffffffff):
            rc, _, _ = hf.build_raw(r, hf.raw_stage(13, bad, sid)[0])
            assert rc == api.ERR_INVALID, bad
        for t in (4, 6, 7, 9, 10, 12, 14, 15):                       # still not display-object types
            rc, err, _ = hf.build_raw(r, hf.raw_stage(t, 1 | 128 << 8, sid)[0])
            assert (rc, err) == (api.ERR_INVALID, "UnexpectedDisplayObjectType"), t
    finally:
        r.close()


def test_opacity_key_lowers_to_a_type_13_wrapper():
    """"opacity" on a container, a shape and a morph shape; the mode comes from "layer" (absent: normal); with "mask" the type-13
    wrapper goes around the type-11 wrapper, which composites in normal mode; without "opacity" nothing changes"""
    from swf_renderer_amd import api
    SC = scenarios.scenarios()
    r = hf.host(100, 100)
    try:
        for layer, op in ((None, 0), (True, 0), ("normal", 0), ("layer", 0), (False, 0), ("screen", bm.OPERATORS["screen"]), (13, bm.OPERATORS["overlay"])):
            obj = hf.tri((9, 9, 9, 200), opacity=100)
            if layer is not None:
                obj["layer"] = layer
            _, p, _ = r.build_frame({"children": [obj]})
            assert hf.kinds(p) == [BEGIN, 0, END] and _ulerps(p) == [0, 1, fd.end_lerp(op, 100)], layer
        arena = api._Arena()
        w = r._object(arena, dict(hf.tri((9, 9, 9, 200), blend_mode="multiply", matrix=scenarios._m(1, 1, 600, 0)), opacity=7, layer="add"))
        assert (w.type, w.id, w.n_children, w.has_matrix) == (api.OBJECT_FADED_LAYER, 8 | 7 << 8, 1, 0)
        assert w.children[0].type == api.OBJECT_BLEND_MODE                       # the object's blend mode stays with the object, inside the group
        w = r._object(arena, _faded(None, 0, []))
        assert (w.type, w.id) == (api.OBJECT_FADED_LAYER, 1)
        w = r._object(arena, _faded(None, np.uint8(255), []))
        assert (w.type, w.id) == (api.OBJECT_FADED_LAYER, 1 | 255 << 8)
        # with "mask": type 13 (mode, opacity) around type 11 in normal mode around [the mask container, the object]
        mask = [hf.tri((0, 0, 0, 255), 4)]
        w = r._object(arena, dict(hf.tri((9, 9, 9, 200), blend_mode="multiply"), mask=mask, layer="screen", opacity=33))
        assert (w.type, w.id, w.n_children) == (api.OBJECT_FADED_LAYER, 4 | 33 << 8, 1)
        m = w.children[0]
        assert (m.type, m.id, m.n_children) == (api.OBJECT_MASKED_LAYER, 1, 2)
        assert m.children[0].type == api.OBJECT_CONTAINER and m.children[1].type == api.OBJECT_BLEND_MODE
        _, p, _ = r.build_frame({"children": [hf.tri((1, 1, 1, 255)), dict(hf.tri((9, 9, 9, 200)), mask=mask, layer="screen", opacity=33)]})
        assert hf.kinds(p) == [0, BEGIN, BEGIN, 0, MASK, 0, END, END]
        assert _ulerps(p) == [1, 0, 0, 1, 0, 1, 0, fd.end_lerp(bm.OPERATORS["screen"], 33)]
        # "layer" and "mask" without "opacity" lower as before
        w = r._object(arena, dict(hf.tri((9, 9, 9, 200)), mask=mask, layer="screen"))
        assert (w.type, w.id) == (api.OBJECT_MASKED_LAYER, 4)
        w = r._object(arena, dict(hf.tri((9, 9, 9, 200)), layer="screen"))
        assert (w.type, w.id) == (api.OBJECT_LAYER, 4)
        morph = SC["morph_round_stroke_090"]["stage"]["children"][0]
        _, p, _ = r.build_frame({"children": [dict(morph, opacity=200, layer="darken")]})
        assert hf.kinds(p)[0] == BEGIN and hf.kinds(p)[-1] == END and _ulerps(p)[-1] == fd.end_lerp(bm.OPERATORS["darken"], 200)
        for bad in (-1, 256, 0.5, 128.0, "128", True, [128], object()):
            with pytest.raises(api.SwfrError) as ei:
                r.build_frame({"children": [hf.tri((9, 9, 9, 200), opacity=bad)]})
            assert ei.value.code == api.ERR_INVALID, bad
    finally:
        r.close()


def test_markers_opacity_255_and_opacity_0():
    r = hf.host(64, 48)
    try:
        kids = [bs._rect(10, 12, 20, 30, (9, 9, 9, 100)), ls._layer("add", [bs._rect(40.5, 3.25, 70, 20, (9, 9, 9, 100)), bs._rect(90, 3, 99, 9, (1, 1, 1, 9))])]
        ground = hf.tri((1, 2, 3, 255))
        _, p, _ = r.build_frame({"children": [ground, _faded("multiply", 77, kids)]})
        assert hf.kinds(p) == [0, BEGIN, 1, BEGIN, 1, END, END]
        rects = hf.rects(p)
        assert rects[1] == rects[6] == (10, 3, 64, 30) and rects[3] == rects[5] == (40, 3, 64, 20)
        assert all(int(p["n_edges"][i]) == 0 for i in (1, 3, 5, 6))
        assert _ulerps(p) == [1, 0, 1, 0, 1, bm.OPERATORS["add"] << 8, fd.end_lerp(bm.OPERATORS["multiply"], 77)]
        for mode in ls.MODES:
            # opacity 255 emits exactly the paths of the type-8 layer
            a = r.build_frame({"children": [ground, _faded(mode, 255, kids), hf.tri((9, 9, 9, 77), 3)]})
            b = r.build_frame({"children": [ground, ls._layer(mode, kids), hf.tri((9, 9, 9, 77), 3)]})
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and [bytes(s) for s in a[2]] == [bytes(s) for s in b[2]], mode
            # opacity 0 emits nothing, and what follows is built as if the group were not there
            a = r.build_frame({"children": [ground, _faded(mode, 0, kids), hf.tri((9, 9, 9, 77), 3)]})
            b = r.build_frame({"children": [ground, hf.tri((9, 9, 9, 77), 3)]})
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and [bytes(s) for s in a[2]] == [bytes(s) for s in b[2]], mode
            # a faded group without surviving paths emits nothing either
            e, p, _ = r.build_frame({"children": [_faded(mode, 128, []), _faded(mode, 128, [bs._rect(90, 3, 99, 9, (1, 1, 1, 9))])]})
            assert len(p) == 0 and len(e) == 0, mode
    finally:
        r.close()


def test_one_level_per_faded_group_at_the_depth_limit():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        t = lambda k: hf.tri((k, 9, 9, 100), k)
        four = _faded("add", 10, [t(1), _faded("screen", 20, [t(2), _faded(None, 30, [t(3), _faded("multiply", 40, [t(4)])])])])
        _, p, _ = r.build_frame({"children": [four]})
        assert hf.kinds(p) == [BEGIN, 0, BEGIN, 0, BEGIN, 0, BEGIN, 0, END, END, END, END]
        assert [v >> 24 for v in _ulerps(p)[-4:]] == [255 - 40, 255 - 30, 255 - 20, 255 - 10]
        mixed = ls._layer("normal", [_faded("add", 9, [t(1), hf.masked("screen", [t(2)], [t(3)])])])                 # 1 + 1 + 2
        assert hf.kinds(r.build_frame({"children": [mixed]})[1]) == [BEGIN, BEGIN, 0, BEGIN, 0, MASK, 0, END, END, END]
        both = hf.masked("screen", [t(2)], [t(3)], opacity=9)                                                      # 1 + 2, inside one layer: 4
        assert hf.kinds(r.build_frame({"children": [ls._layer("add", [both])]})[1]) == [BEGIN, BEGIN, BEGIN, 0, MASK, 0, END, END, END]
        for tree in (_faded("normal", 50, [four]), ls._layer("normal", [four]), hf.masked("add", [four], [t(5)]),
                     _faded("add", 10, [_faded("add", 10, [hf.masked("screen", [t(2)], [t(3)], opacity=9)])]),       # 1 + 1 + 1 + 2
                     ls._layer("add", [ls._layer("add", [both])]),
                     _faded("add", 0, [four]),                                                                     # (opacity 0 counts: the limit is on the tree)
                     _faded("add", 10, [_faded("add", 10, [_faded("add", 10, [_faded("add", 10, [_faded("add", 10, [])])])])])):
            with pytest.raises(api.SwfrError) as ei:
                r.build_frame({"children": [tree]})
            assert ei.value.code == api.ERR_CAPACITY and "LayerDepth" in str(ei.value)
    finally:
        r.close()


@pytest.mark.parametrize("mode", ls.MODES)
def test_parents_clear_state_after_each_kind_of_faded_group(mode):
    """the lerp of a translucent path behind the faded group says what it left of the parent's "still clear" state
    (fade_model.parent_stays_clear, libcairo's rule: tests/test_fade_model.py)"""
    r = hf.host()
    try:
        after = hf.tri((200, 100, 50, 119), 9)
        paint = hf.tri((9, 9, 9, 100))
        clear_fill = hf.tri((255, 255, 255, 0))                        # OVER with a clear source: the surface stays clear
        drawn_zero = dict(clear_fill, blend_mode="multiply")         # drawn on, every pixel zero
        groups = {True: ([], [clear_fill], [bs._rect(90, 3, 99, 9, (1, 1, 1, 9))], [ls._layer("normal", [])], [_faded("multiply", 0, [paint])]),
                  False: ([drawn_zero], [ls._layer("screen", [])], [_faded("screen", 128, [])])}
        for group_clear in (True, False):
            for kids in groups[group_clear]:
                for opacity in (0, 1, 128, 254, 255):
                    _, p, _ = r.build_frame({"children": [_faded(mode, opacity, kids), after]})
                    want = 1 if fd.parent_stays_clear(mode, group_clear, opacity) else 0
                    assert hf.kinds(p)[-1] == 0 and hf.lerps(p)[-1] == want and (opacity or len(p) == 1), (mode, kids, opacity)
        # a painted group: drawn on whatever the opacity -- except at opacity 0, where nothing happens at all
        for opacity in (0, 1, 255):
            _, p, _ = r.build_frame({"children": [_faded(mode, opacity, [paint]), after]})
            assert hf.lerps(p)[-1] == (1 if opacity == 0 else 0) and len(p) == (1 if opacity == 0 else 4)
        # a parent that was drawn on stays drawn on
        _, p, _ = r.build_frame({"children": [hf.tri((1, 1, 1, 9)), _faded(mode, 0, [paint]), after]})
        assert hf.lerps(p) == [1, 0]
    finally:
        r.close()


def _many(n=400):
    """n small objects, every fifth a faded group (enough display objects for a threaded build), the first object a faded group at
    opacity 0 that leaves the frame clear"""
    rng = np.random.default_rng(7)
    kids = [_faded("multiply", 0, [hf.tri((9, 9, 9, 9))]), hf.tri((9, 9, 9, 9), 2)]
    for i in range(n):
        x, y = rng.uniform(0, 50), rng.uniform(0, 36)
        col = (int(rng.integers(256)), 90, 200, int(rng.integers(1, 255)))
        t = bs._shape([(x, y), (x + 9.3, y + 2.1), (x + 3.2, y + 8.7)], col)
        if i % 5 == 0:
            kids.append(_faded(ls.MODES[(i // 5) % 9], 1 + (i * 7) % 254, [t, dict(t, blend_mode="multiply"), ls._layer("screen", [t])]))
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
    kinds, lerps = hf.kinds(out[0][1]), _ulerps(out[0][1])
    assert kinds.count(BEGIN) == kinds.count(END) == 160 and sum(1 for v in lerps if v >> 24) == 80
    assert kinds[0] == 0 and lerps[0] == 1                           # the opacity-0 group emitted nothing and left the frame clear
    depth = np.cumsum([1 if k == BEGIN else (-1 if k == END else 0) for k in kinds])
    later = next(i for i in range(1, len(kinds)) if kinds[i] == 0 and depth[i] == 0)
    assert kinds[1] == BEGIN and lerps[later] == 0                   # behind a path and a painted group no first paint any more


def test_upload_validates_the_fade_bits():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        t = lambda k: hf.tri((k, 9, 9, 100), k)
        e, p, s = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), _faded("multiply", 100, [t(1), ls._layer("add", [t(2)])]), hf.masked("screen", [t(3)], [t(4)])]})
        assert hf.kinds(p) == [0, BEGIN, 0, BEGIN, 0, END, END, BEGIN, 0, MASK, 0, END]
        fade = 155 << 24
        assert _ulerps(p)[6] == (bm.OPERATORS["multiply"] << 8) | fade

        def refused(edit, code=api.ERR_INVALID):
            q = p.copy()
            edit(q)
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, q, s)
            assert ei.value.code == code, ei.value
        put = lambda i, v: (lambda q: q["lerp"].__setitem__(i, v))
        refused(lambda q: None, api.ERR_NO_DEVICE)                   # the well-formed scene: a host-only handle cannot rasterize
        refused(put(5, (bm.OPERATORS["add"] << 8) | (1 << 24)), api.ERR_NO_DEVICE)       # a fade on the inner END, too
        refused(put(6, bm.OPERATORS["multiply"] << 8 | (255 << 24)), api.ERR_NO_DEVICE)  # opacity 0
        refused(put(6, (bm.OPERATORS["multiply"] << 8) | fade | (1 << 16)))               # bits 16..23 stay 0
        refused(put(6, (bm.OPERATORS["multiply"] << 8) | fade | (0x80 << 16)))
        refused(put(6, (bm.OPERATORS["multiply"] << 8) | fade | 1))                        # ... and so do the lerp bits
        refused(put(6, (9 << 8) | fade))                                                   # no such operator
        refused(put(0, 1 | fade))                                    # a fade on a plain path
        refused(put(2, fade))
        refused(put(1, fade))                                        # ... on a BEGIN
        refused(put(9, fade))                                        # ... on a MASK
        refused(put(11, (bm.OPERATORS["screen"] << 8) | fade))       # ... on the END of a group that holds a MASK
        refused(put(11, (bm.OPERATORS["screen"] << 8) | (1 << 24)))
    finally:
        r.close()
