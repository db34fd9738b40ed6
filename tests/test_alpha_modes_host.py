"""The erase and alpha modes on the host (no GPU): what a handle refuses without SWFR_FLAG_ALPHA_MODES and accepts with it, how the
frame builder lowers the two modes -- operator bytes, the grown rectangles of ALPHA groups, the transparent-source forms, the
clear-surface bookkeeping -- what swfr_upload_edges validates, and that the new numpy renderer is tests/frame_model.py on frames
without the two operators."""
import numpy as np
import pytest

import alpha_modes_model as am
import alpha_modes_scenes as scenes
import blend_model as bm
import composite_scenes as cs
import fade_scenes as fs
import frame_model
import host_frames as hf
import layer_scenes as ls
from alpha_modes_scenes import FOLLOW, _faded, _layer, _masked, _pair, _rect
from blend_scenes import _shape as bs_shape

BEGIN, END, MASK = 2, 3, 4
ERASE, ALPHA = am.OP_ERASE << 8, am.OP_ALPHA << 8
OBJECT_TYPES = (5, 8, 11, 13)


@pytest.fixture(scope="module", autouse=True)
def need_library():
    import swf_renderer_amd as S
    import os
    assert os.path.exists(S.library_path()), "libswfr.so must be built"


def flagged(w=64, h=48, **kw):
    return hf.host(w, h, alpha_modes=True, **kw)


def union(rects):
    return (min(r[0] for r in rects), min(r[1] for r in rects), max(r[2] for r in rects), max(r[3] for r in rects))


def _raw(r, obj_type, mode, opacity=255):
    """(code, message) of swfr_build_frame for a raw display object of `obj_type` with the mode in its id"""
    import scenarios
    sid = r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": scenarios._rgba(9, 9, 9, 100)}))
    s, keep = hf.raw_stage(obj_type, mode | (opacity << 8 if obj_type == 13 else 0), sid)      # (type 11: the one child is the mask)
    rc, msg, _ = hf.build_raw(r, s)
    return rc, msg


# ---------------------------------------------------------------------------------------------------------------- the flag
def test_without_the_flag_every_call_is_refused_as_it_was():
    from swf_renderer_amd import api
    assert api.PATH_OPERATORS == bm.OPERATORS and api.ALPHA_MODE_OPERATORS == am.OPERATORS
    assert api.BLEND_MODES["alpha"] == am.MODES["alpha"] and api.BLEND_MODES["erase"] == am.MODES["erase"]
    r = hf.host()
    try:
        for t in OBJECT_TYPES:
            for mode in (9, 10, 11, 12):
                assert _raw(r, t, mode) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), (t, mode)
        for key, make in (("blend_mode", lambda m: dict(hf.tri((1, 2, 3, 200)), blend_mode=m)), ("layer", lambda m: _layer(m, _pair())),
                          ("mask", lambda m: _masked(m, _pair(), _pair())), ("opacity", lambda m: _faded(m, 128, _pair()))):
            for mode in ("erase", "alpha"):
                with pytest.raises(api.SwfrError) as ei:
                    r.build_frame({"children": [make(mode)]})
                assert ei.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedBlendMode" in str(ei.value), (key, mode)
        # upload: operators 9 and 10 are no operators, on a path and on an END, with the message of every value above 8
        e, p, s = r.build_frame({"children": [hf.tri((1, 2, 3, 255)), _layer("multiply", [hf.tri((9, 9, 9, 100))])]})
        assert hf.kinds(p) == [0, BEGIN, 0, END]
        for at, field, text in ((0, ERASE, "path blend field"), (0, ALPHA, "path blend field"), (3, ERASE, "GROUP_END"), (3, ALPHA, "GROUP_END")):
            q = p.copy()
            q["lerp"][at] = field
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, q, s)
            assert ei.value.code == api.ERR_INVALID and text in str(ei.value) and "at most 8" in str(ei.value), (at, field, str(ei.value))
    finally:
        r.close()


def test_with_the_flag_the_refusals_that_stay():
    from swf_renderer_amd import api
    r = flagged()
    try:
        for t in OBJECT_TYPES:
            for mode in (9, 10):                                     # subtract, invert
                assert _raw(r, t, mode) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"), (t, mode)
            assert _raw(r, t, 15)[0] == api.ERR_INVALID
            assert _raw(r, t, 12)[0] == api.OK, t                    # erase: everywhere
        assert _raw(r, 5, 11) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode")      # alpha per path
        for t in (8, 11, 13):
            assert _raw(r, t, 11)[0] == api.OK, t
        assert _raw(r, 5, 2) == (api.ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode")       # "layer" as a per-path mode, as ever
        # five alpha layers nested: the depth limit is the layers'
        with pytest.raises(api.SwfrError) as ei:
            r.build_frame({"children": [_layer("alpha", [_layer("alpha", [_layer("alpha", [_layer("alpha", [_layer("alpha", _pair())])])])])]})
        assert ei.value.code == api.ERR_CAPACITY and "LayerDepth" in str(ei.value)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- the lowering
def test_the_lowered_paths_of_the_golden_scenes():
    """every golden scene builds on a flagged handle; an ERASE path carries operator 9 and lerp 0; an ALPHA END's rectangle, shared with
    its BEGIN (and MASK), contains every path before it on its surface; and the new renderer draws the arrays as libcairo drew the scene"""
    for fname, (make, aliased) in sorted(scenes.files().items()):
        gold = np.load(scenes.golden_path(fname))
        for name, sc in sorted(make().items()):
            r = flagged(sc["width"], sc["height"], antialias="none" if aliased else "default")
            try:
                for b in sc.get("bitmaps", []):
                    r.add_bitmap(b)
                e, p, s = r.build_frame(sc["stage"])
                with pytest.raises(Exception) as ei:                 # the upload validation accepts what the builder emits
                    r.upload_edges(e, p, s)
                assert "host-only" in str(ei.value), (name, str(ei.value))
            finally:
                r.close()
            for q in p:
                field = int(q["lerp"]) & 0xffffffff
                if int(q["kind"]) < BEGIN and (field >> 8) & 0xff >= am.OP_ERASE:
                    assert field == ERASE, (name, hex(field))
            img = am.render(e, p, s, sc["width"], sc["height"], aliased=aliased, bitmaps=hf.bitmaps_of(sc))      # (raises where the rectangle rule is broken)
            assert (img == gold[name]).all(), (fname, name)


def test_an_alpha_layer_swallows_its_earlier_siblings():
    r = flagged(256, 64)
    try:
        sc = scenes.structure_scenes()["siblings_alpha"]
        _, p, _ = r.build_frame(sc["stage"])
        assert hf.kinds(p) == [0, 0, BEGIN, 0, 1, END] and hf.lerps(p)[-1] == ALPHA
        rc = hf.rects(p)
        assert rc[2] == rc[5] == union(rc[:2] + rc[3:5]) and rc[2][:2] == (2, 2) and rc[3][0] >= 100      # with the corners, not the members' alone
        _, p, _ = r.build_frame(scenes.structure_scenes()["siblings_erase"]["stage"])
        rc = hf.rects(p)
        assert rc[2] == rc[5] == (100, 20, 150, 50) and hf.lerps(p)[-1] == ERASE
        # inside a layer the surface is the layer's: the sibling outside it does not count, the enclosing group's rectangle follows
        _, p, _ = r.build_frame(scenes.structure_scenes()["siblings_alpha_in_layer"]["stage"])
        assert hf.kinds(p) == [0, BEGIN, 0, BEGIN, 0, 1, END, END]
        rc = hf.rects(p)
        assert rc[3] == rc[6] == union(rc[2:3] + rc[4:6]) and rc[3][0] == 100 and rc[1] == rc[7] == rc[3]
        # masked: the three markers share the grown rectangle
        _, p, _ = r.build_frame(scenes.structure_scenes()["siblings_alpha_masked"]["stage"])
        k = hf.kinds(p)
        assert k[2] == BEGIN and MASK in k and k[-1] == END
        rc = hf.rects(p)
        assert rc[2] == rc[k.index(MASK)] == rc[-1] == union(rc[:2] + [q for q, kk in zip(rc, k) if kk < BEGIN])
    finally:
        r.close()


@pytest.mark.parametrize("form", ["empty", "opacity0", "emptymask", "emptycontent"])
def test_alpha_with_a_transparent_source_is_emitted(form):
    ground = hf.tri((1, 2, 3, 200))
    layer = {"empty": _layer("alpha", []), "opacity0": _faded("alpha", 0, _pair()), "emptymask": _masked("alpha", _pair(), []),
             "emptycontent": _masked("alpha", [], _pair())}[form]
    erase = {"empty": _layer("erase", []), "opacity0": _faded("erase", 0, _pair()), "emptymask": _masked("erase", _pair(), []),
             "emptycontent": _masked("erase", [], _pair())}[form]
    r = flagged()
    try:
        _, p, _ = r.build_frame({"children": [ground, layer, FOLLOW[0]]})
        assert hf.kinds(p) == [0, BEGIN, END, 0] and hf.lerps(p) == [1, 0, ALPHA, 0]
        assert hf.rects(p)[1] == hf.rects(p)[2] == hf.rects(p)[0]           # it clears what was drawn
        # on an empty surface there is nothing to clear: nothing is emitted, yet the next path is no first paint
        _, p, _ = r.build_frame({"children": [layer, FOLLOW[0]]})
        assert hf.kinds(p) == [0] and hf.lerps(p) == [0]
        # under ERASE a transparent source changes no pixel: nothing is emitted
        _, p, _ = r.build_frame({"children": [ground, erase, FOLLOW[0]]})
        assert hf.kinds(p) == [0, 0]
        # ... and libcairo's bookkeeping: opacity 0 and an untouched mask return at once (the surface stays clear), the others count as drawn
        _, p, _ = r.build_frame({"children": [erase, FOLLOW[0]]})
        assert hf.lerps(p) == [1 if form in ("opacity0", "emptymask") else 0]
    finally:
        r.close()


def test_the_clear_surface_bookkeeping():
    """after an ERASE path or an ERASE / ALPHA composite the surface is no longer clear: the next translucent path has lerp 0"""
    r = flagged()
    try:
        for name in scenes.PRELUDES:
            sc = scenes.structure_scenes()[name]
            _, p, _ = r.build_frame(sc["stage"])
            plain = [int(q["lerp"]) for q in p if int(q["kind"]) < BEGIN]
            assert plain[-2:] == [0, 0], (name, plain)
        # inside a group: an ERASE path as the group's first paint, then a translucent one
        _, p, _ = r.build_frame({"children": [_layer("normal", [dict(_pair()[0], blend_mode="erase"), _pair()[1]])]})
        assert hf.lerps(p) == [0, ERASE, 0, 0]
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- upload
def test_upload_validates_the_operators_and_the_rectangle_rule():
    from swf_renderer_amd import api
    r = flagged(256, 64)
    try:
        sc = scenes.structure_scenes()["siblings_alpha_in_layer"]
        e, p, s = r.build_frame(sc["stage"])
        assert hf.kinds(p) == [0, BEGIN, 0, BEGIN, 0, 1, END, END]

        def refused(edit, code=api.ERR_INVALID, text=None):
            q = p.copy()
            edit(q)
            with pytest.raises(api.SwfrError) as ei:
                r.upload_edges(e, q, s)
            assert ei.value.code == code and (text is None or text in str(ei.value)), ei.value
        refused(lambda q: None, api.ERR_NO_DEVICE)                   # the well-formed scene: a host-only handle cannot rasterize
        refused(lambda q: q["lerp"].__setitem__(0, ERASE), api.ERR_NO_DEVICE)              # ERASE on an ordinary path, and on an END
        refused(lambda q: q["lerp"].__setitem__(7, ERASE), api.ERR_NO_DEVICE)
        refused(lambda q: q["lerp"].__setitem__(7, ERASE | 77 << 24), api.ERR_NO_DEVICE)   # faded
        refused(lambda q: q["lerp"].__setitem__(4, ALPHA), text="GROUP_END only")          # ALPHA on an ordinary path
        refused(lambda q: q["lerp"].__setitem__(4, ERASE | 1))       # an operator needs lerp bits 0
        refused(lambda q: q["lerp"].__setitem__(6, 11 << 8))         # no such operator
        refused(lambda q: q["lerp"].__setitem__(6, ALPHA | 1))
        refused(lambda q: q["lerp"].__setitem__(3, ALPHA))           # BEGIN carries no operator

        def shrink(q):                                               # the ALPHA group's rectangle no longer holds its earlier sibling (path 2)
            for i in (3, 6):
                q["x_max"][i], q["y_max"][i] = 150, 50
        refused(shrink, text="ALPHA group")
        # the outer group as ALPHA: its rectangle would have to hold path 0 as well
        refused(lambda q: q["lerp"].__setitem__(7, ALPHA), text="ALPHA group")

        def grow_outer(q):
            q["lerp"][7] = ALPHA
            for i in (1, 7):
                q["x_min"][i], q["y_min"][i] = 2, 2
        refused(grow_outer, api.ERR_NO_DEVICE)
    finally:
        r.close()


def test_upload_checks_the_rule_on_the_masks_surface():
    from swf_renderer_amd import api
    r = flagged()
    try:
        sc = scenes.structure_scenes()["alpha_in_mask"]
        e, p, s = r.build_frame(sc["stage"])
        k = hf.kinds(p)
        m = k.index(MASK)
        assert k[m + 2] == BEGIN and hf.lerps(p)[-2] == ALPHA
        rc = hf.rects(p)
        assert rc[m + 2] == union([rc[m + 1]] + rc[m + 3:-2])            # grown by the mask's earlier rectangle, not by the content's
        q = p.copy()
        inner = [i for i in range(m + 2, len(p) - 1) if k[i] >= BEGIN]
        for i in inner:
            q["x_min"][i] = int(q["x_min"][i]) + 8
        for i in range(m + 3, len(p) - 2):                           # (members stay inside)
            q["x_min"][i] = max(int(q["x_min"][i]), int(q["x_min"][inner[0]]))
        with pytest.raises(api.SwfrError) as ei:
            r.upload_edges(e, q, s)
        assert ei.value.code == api.ERR_INVALID and "ALPHA group" in str(ei.value)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- the renderers
def test_the_two_renderers_agree_on_frames_without_the_operators():
    for seed in range(6):
        sc = fs.rand_faded_scene(np.random.default_rng(3300 + seed))
        arrays = hf.build_on_host(sc, bool(seed % 2))
        args = dict(aliased=bool(seed % 2))
        assert (am.render(*arrays, sc["width"], sc["height"], **args) == frame_model.render(*arrays, sc["width"], sc["height"], **args)).all(), seed
    for first, depth in cs.NESTINGS[::3]:
        fr = cs.raw_nesting_frame(first, depth)
        assert (am.render(*fr.arrays(), fr.W, fr.H) == frame_model.render(*fr.arrays(), fr.W, fr.H)).all()
    # and the old one refuses the new operators, as an unflagged handle does
    import alpha_modes_raw as ar
    with pytest.raises(ValueError):
        frame_model.render(*ar.cleared_strips_frame("alpha").arrays(), ar.W, ar.H)


def test_the_model_refuses_what_upload_refuses():
    import alpha_modes_raw as ar
    fr = ar.AlphaRawFrame(ar.W, ar.H)
    fr.rect_tor(2, 2, 100, 30, 0x80402010, 1)
    fr.begin()
    fr.rect_tor(10, 4, 40, 20, 0xff102030, 1)
    fr.end("alpha", grow=False)
    with pytest.raises(ValueError, match="ALPHA group"):
        am.render(*fr.arrays(), fr.W, fr.H)
    from swf_renderer_amd import api
    r = flagged(ar.W, ar.H)
    try:
        with pytest.raises(api.SwfrError) as ei:
            r.upload_edges(*fr.arrays())
        assert ei.value.code == api.ERR_INVALID and "ALPHA group" in str(ei.value)
    finally:
        r.close()


def test_the_fuzz_seeds_build():
    """the seeds of tests/test_alpha_modes_gpu.py's differential fuzz, on a host-only handle: at most 5 % are refused for capacity"""
    for aliased in (False, True):
        skipped = sum(scenes.buildable(scenes.fuzz_scene(seed, aliased), aliased) is None for seed in range(24))
        assert skipped * 20 <= 24, (aliased, skipped)


def test_a_flagged_handle_builds_in_one_walk():
    """enough top-level objects for a threaded build (pieces of 64): an ALPHA layer late in the frame still takes in everything drawn
    before it, and the arrays are those of a single thread"""
    import os
    rng = np.random.default_rng(3)
    kids = []
    for i in range(300):
        x, y = float(rng.uniform(0, 50)), float(rng.uniform(0, 36))
        kids.append(bs_shape([(x, y), (x + 9.3, y + 2.1), (x + 3.2, y + 8.7)], (int(rng.integers(256)), 90, 200, int(rng.integers(1, 255)))))
    kids.insert(250, _layer("alpha", _pair()))
    stage = {"children": [{"type": "container", "children": kids}]}
    out = []
    for threads in ("1", "8"):
        os.environ["SWFR_BUILD_THREADS"] = threads
        try:
            r = flagged()
            out.append(r.build_frame(stage))
            r.close()
        finally:
            del os.environ["SWFR_BUILD_THREADS"]
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    p = out[0][1]
    k = hf.kinds(p)
    b = k.index(BEGIN)
    assert b == 250 and hf.rects(p)[b] == union(hf.rects(p)[:b] + hf.rects(p)[b + 1:k.index(END)])
    assert (am.render(*out[0], 64, 48) == am.render(*out[1], 64, 48)).all()
