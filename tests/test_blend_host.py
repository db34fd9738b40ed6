"""Blend modes on the host side (no GPU, host-only handles): the display-object type, the refused modes, the operator field
swfr_build_frame emits -- ADD on a still-clear surface settling to a SOURCE lerp, in single and in threaded builds -- and what
swfr_upload_edges refuses."""
import os

import numpy as np
import pytest

import blend_model as bm
import blend_scenes as bs
import host_frames as hf
import scenarios
from scenarios import _rgba


def test_object_type_and_mode_numbers():
    from swf_renderer_amd import api
    assert api.OBJECT_BLEND_MODE == 5 and api.load_library().swfr_abi_version() == 1
    assert {k: api.BLEND_MODES[k] for k in bm.MODES} == bm.MODES and {k: api.BLEND_MODES[k] for k in bm.REFUSED} == bm.REFUSED
    assert api.PATH_OPERATORS == bm.OPERATORS
    assert api.blend_mode_number("Multiply") == 3 and api.blend_mode_number("HARDLIGHT") == 14 and api.blend_mode_number("hard-light") == 14
    assert api.blend_mode_number(8) == 8
    with pytest.raises(api.SwfrError):
        api.blend_mode_number("dodge")
    r = hf.host()
    try:
        sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))
        for mode in (0, 1, 3, 4, 5, 6, 7, 8, 13, 14):
            rc, _, n_paths = hf.build_raw(r, hf.raw_stage(api.OBJECT_BLEND_MODE, mode, sid)[0])
            assert rc == api.OK and n_paths == 1, mode
        for mode in (2, 9, 10, 11, 12):
            rc, err, _ = hf.build_raw(r, hf.raw_stage(api.OBJECT_BLEND_MODE, mode, sid)[0])
            assert (rc, err) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), mode
        for mode in (15, 16, 255, 0xffffffff):
            rc, _, _ = hf.build_raw(r, hf.raw_stage(api.OBJECT_BLEND_MODE, mode, sid)[0])
            assert rc == api.ERR_INVALID, mode
        for t in (4, 6, 7):                                          # not display-object types, before and after
            rc, err, _ = hf.build_raw(r, hf.raw_stage(t, 3, sid)[0])
            assert (rc, err) == (api.ERR_INVALID, "UnexpectedDisplayObjectType"), t
    finally:
        r.close()


def _tri(colour, **kw):
    return bs._shape([(2, 2), (60, 5), (30, 44)], colour, **kw)


@pytest.mark.parametrize("mode", sorted(bm.MODES))
def test_operator_field_of_built_paths(mode):
    op = bm.OPERATORS[mode]
    r = hf.host()
    try:
        for alpha in (255, 119):
            # first paint of the frame, then a later one
            _, p, _ = r.build_frame({"children": [_tri((200, 100, 50, alpha), blend_mode=mode), _tri((20, 100, 250, alpha), blend_mode=mode),
                                                  _tri((1, 2, 3, alpha))]})
            first = 1 if mode == "add" else op << 8                  # ADD on a clear surface is Cairo's SOURCE: an ordinary lerp path
            assert [int(v) for v in p["lerp"]] == [first, op << 8, 1 if alpha == 255 else 0], (mode, alpha)
        # under a container, numeric mode, inner normal; a stroke and its fill both carry the operator
        blob = scenarios.scenarios()["stroke_curves"]["stage"]["children"][0]
        _, p, _ = r.build_frame({"children": [_tri((9, 9, 9, 255)), {"type": "container", "blend_mode": bm.MODES[mode], "children": [
            blob, {"type": "container", "blend_mode": "normal", "children": [_tri((5, 5, 5, 255)), _tri((5, 5, 5, 9))]}]}]})
        assert [int(v) for v in p["lerp"]] == [1, op << 8, op << 8, 1, 0]
    finally:
        r.close()


def test_normal_wrapper_changes_nothing():
    sc = scenarios.scenarios()["translucent_stack"]
    r = hf.host(sc["width"], sc["height"])
    try:
        plain = r.build_frame(sc["stage"])
        for mode in ("normal", 0, 1):
            wrapped = r.build_frame({"children": [{"type": "container", "blend_mode": mode, "children": sc["stage"]["children"]}]})
            for a, b in zip(plain[:2], wrapped[:2]):
                assert a.tobytes() == b.tobytes()
            assert [bytes(st) for st in plain[2]] == [bytes(st) for st in wrapped[2]]
    finally:
        r.close()


def _many(mode, first_blended, n=400):
    """n small translucent triangles under one blend wrapper (enough display objects for a threaded build)"""
    rng = np.random.default_rng(7)
    kids = []
    for i in range(n):
        x, y = rng.uniform(0, 50), rng.uniform(0, 36)
        kids.append(bs._shape([(x, y), (x + 9.3, y + 2.1), (x + 3.2, y + 8.7)], (int(rng.integers(256)), 90, 200, int(rng.integers(1, 255)))))
    if first_blended:
        return {"children": [{"type": "container", "blend_mode": mode, "children": kids}]}
    return {"children": [{"type": "container", "children": [{"type": "container", "blend_mode": mode, "children": kids[:1]}] + kids[1:] + [
        {"type": "container", "blend_mode": mode, "children": kids[:40]}]}]}


@pytest.mark.parametrize("mode", ["add", "multiply"])
@pytest.mark.parametrize("first_blended", [True, False])
def test_threaded_build_is_the_single_walk(mode, first_blended):
    """the pieces of a threaded build each start as if the surface were clear; joined, only the frame's first paint may be a lerp"""
    stage = _many(mode, first_blended)
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
    lerp = [int(v) for v in out[0][1]["lerp"]]
    op = bm.OPERATORS[mode] << 8
    n_blended = 400 if first_blended else 41
    assert lerp[0] == (1 if mode == "add" else op)                   # the frame's first paint
    assert sum(1 for v in lerp if v == op) == n_blended - (1 if mode == "add" else 0)
    assert all(v in (0, op) for v in lerp[1:])                       # translucent colours: nothing else is a lerp


def test_clear_source_under_an_operator_still_counts_as_drawn():
    r = hf.host()
    try:
        for mode, lerps in (("multiply", [bm.OPERATORS["multiply"] << 8, 0]), ("add", [1]), ("normal", [1])):
            _, p, _ = r.build_frame({"children": [_tri((255, 255, 255, 0), blend_mode=mode), _tri((200, 100, 50, 119))]})
            assert [int(v) for v in p["lerp"]] == lerps, mode
    finally:
        r.close()


def test_upload_refuses_a_malformed_blend_field():
    from swf_renderer_amd import api
    r = hf.host()
    try:
        e, p, s = r.build_frame({"children": [_tri((200, 100, 50, 119), blend_mode="screen")]})
        assert int(p["lerp"][0]) == bm.OPERATORS["screen"] << 8
        for bad in (1 | (2 << 8), 2, 9 << 8, 1 << 16, 0x80000000):
            q = p.copy()
            q["lerp"][0] = bad
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, q, s)
            assert ei.value.code == api.ERR_INVALID, hex(bad)
        with pytest.raises(api.SwfrError) as ei:                     # a well-formed scene: a host-only handle cannot rasterize
            r.upload_edges(e, p, s)
        assert ei.value.code == api.ERR_NO_DEVICE
    finally:
        r.close()
