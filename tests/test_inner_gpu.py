"""Inner shadows on the device ("Inner shadows").

1. the kernels alone: a frame is rendered, captured as a bitmap, given its inner shadow (swfr_shadow_bitmap), drawn 1:1 with a nearest fill
   and read back -- against tests/inner_model.py (itself held against libcairo + pixman by tests/test_inner_model.py) on the first frame's
   pixels, zero differing bytes; then in place, and twice in place;
2. the chain inside render: the inner entry first (it reads the framebuffer), in the middle and last (it reads texels), against
   inner_model.apply of the plainly rendered group;
3. every cairo_inner_* golden (libcairo + pixman) through render, and again through render_resident, zero differing bytes;
4. ALPHA and ERASE on a flagged handle, against the frame model of the composite;
5. an empty group with an inner shadow is the frame without it;
6. a frame without an inner shadow behind one with it is the frame a fresh handle renders.
Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import itertools

import numpy as np
import pytest

import blur_scenes as bl
import device_routes as dr
import filter_model as fm
import inner_model as im
import inner_scenes as isc
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats
from shadow_model import COLORS, STRENGTHS, offsets

pytestmark = pytest.mark.gpu

FAMILY = dr.FAMILIES["inner"]
SIZES = dr.SIZES_AND_LOOPS_TWICE
FLAGS = {"atop": {"inner": True}, "knockout": {"inner": True, "knockout": True}}
SRC, DST = 7, 9
_content, _whole_frame_bitmap = dr.content, dr.whole_frame_bitmap


def _cases(w, h):
    """the whole product of offsets, strengths, colours and the two flag states on the smallest image; on the others each value at least
    once (the passes are pointwise in strength, colour and flag: the image's size changes nothing there)"""
    offs, boxes = offsets(w, h), ((3, 4, 1), (1, 1, 1), (2, 0, 3), (64, 255, 1))
    if w * h <= 13 * 11:
        for n, ((dx, dy), strength, color, flags) in enumerate(itertools.product(offs, STRENGTHS, sorted(COLORS), sorted(FLAGS))):
            yield (dx, dy), boxes[n % 3], strength, color, flags
        yield (1, -1), boxes[3], 2, "translucent", "atop"
        return
    few = 4 if w * h > 1000000 else 6
    for n in range(few):
        yield offs[n % len(offs)], boxes[n % len(boxes)], STRENGTHS[n % len(STRENGTHS)], sorted(COLORS)[n % 3], sorted(FLAGS)[n % 2]
    if few > 4:
        yield offs[4], boxes[1], 255, "translucent", "knockout"


def _shadow(off, box, strength, color, flags):
    return dict(FLAGS[flags], color=COLORS[color], dx=off[0], dy=off[1], x=box[0], y=box[1], passes=box[2], strength=strength)


# ---- 1. the kernels alone
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_shadow_bitmap_against_the_model(size):
    w, h = size
    r = dr.handle(w, h)
    try:
        r.render({"children": _content(w, h)})
        frame = r.read_image(premultiplied=True)
        assert len(np.unique(frame[..., 3])) > 8 and (frame[..., 3] == 0).any(), "the frame holds many alphas, and clear pixels"
        r.capture_bitmap(SRC)
        draw = {"children": [_whole_frame_bitmap(w, h, DST)]}
        seen = set()
        for case in _cases(w, h):
            sh = _shadow(*case)
            r.shadow_bitmap(DST, SRC, sh)
            r.render(draw)
            n, mx = diff_stats(r.read_image(premultiplied=True), im.inner_shadow(frame, sh))
            if (n, mx) != (0, 0) or w * h > 13 * 11:
                print("inner %dx%d %r: differing pixels %d max %d" % (w, h, sh, n, mx))
            assert (n, mx) == (0, 0), (size, sh)
            seen.add(case[0]), seen.add(case[2]), seen.add(case[3]), seen.add(case[4])
        assert seen >= (set(offsets(w, h)) | set(STRENGTHS) if w * h <= 1000000 else set()) | set(COLORS) | set(FLAGS)
        # the source is untouched; then the inner shadow in place (dst == src), and the inner shadow of that
        r.render({"children": [_whole_frame_bitmap(w, h, SRC)]})
        assert diff_stats(r.read_image(premultiplied=True), frame) == (0, 0), "the source bitmap is still the frame"
        first, second = _shadow((2, 1), (3, 2, 1), 2, "translucent", "atop"), _shadow((-1, 0), (2, 2, 1), 1, "opaque", "knockout")
        r.shadow_bitmap(SRC, SRC, first)
        r.render({"children": [_whole_frame_bitmap(w, h, SRC)]})
        want = im.inner_shadow(frame, first)
        assert (want != frame).any() and (want[..., 3] == frame[..., 3]).all()
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), "in place"
        r.shadow_bitmap(SRC, SRC, second)
        r.render({"children": [_whole_frame_bitmap(w, h, SRC)]})
        assert diff_stats(r.read_image(premultiplied=True), im.inner_shadow(want, second)) == (0, 0), "in place, twice"
    finally:
        r.close()


# ---- 2. the chain inside render
E = isc.E
CHAINS = {"first": [E["inner"], E["blur_odd"], E["drop"]], "first_alone": [E["ikglow"]], "first_then_blur": [E["iglow"], E["blur"]],
          "middle": [E["blur_odd"], E["inner"], E["drop"]], "middle_even": [E["drop"], E["ikglow"], E["blur"]],
          "last": [E["drop"], E["blur_odd"], E["inner"]], "last_of_two": [E["blur"], E["iglow"]], "chain_of_four": isc.LISTS["chain_of_four"]}


@pytest.mark.parametrize("size", ((13, 11), (257, 3)), ids=lambda s: "%dx%d" % s)
def test_the_chain_inside_render_against_the_model(size):
    w, h = size
    r = dr.handle(w, h)
    try:
        kids = _content(w, h)
        r.render({"children": kids})
        G = r.read_image(premultiplied=True)
        assert len(np.unique(G[..., 3])) > 8 and (G[..., 3] == 0).any(), "the group holds many alphas, and clear pixels"
        for name, chain in sorted(CHAINS.items()):
            r.render({"children": [{"type": "container", "children": kids, "filters": chain}]})
            dr.not_refused(r, name)
            assert r.built_filters() == [im.as_dicts(chain)]
            n, mx = diff_stats(r.read_image(premultiplied=True), im.apply(G, chain))
            print("inner chain %dx%d %s: differing pixels %d max %d" % (w, h, name, n, mx))
            assert (n, mx) == (0, 0), (size, name)
        # the lone "shadow" key (a type-19 object) is the list of that one entry
        for sh in (isc.INNER, dict(isc.INNER_GLOW, knockout=True)):
            r.render({"children": [{"type": "container", "children": kids, "shadow": sh}]})
            assert r.built_layers()[0][4] == im.as_dict(sh)
            assert diff_stats(r.read_image(premultiplied=True), im.inner_shadow(G, sh)) == (0, 0), (size, sh)
    finally:
        r.close()


# ---- 3. the goldens of libcairo + pixman
@pytest.mark.parametrize("fname", sorted(isc.files()))
def test_goldens_through_render_and_render_resident(fname):
    dr.goldens_through_render_and_resident(FAMILY, fname)


# ---- 4. ALPHA and ERASE
def test_alpha_and_erase_inner_shadowed_layers():
    dr.alpha_and_erase(FAMILY, "cairo_inner_operators", "shadow_normal_clear", "shadow_normal_opaque")


# ---- 5. an empty group
def test_an_empty_group_with_an_inner_shadow_is_the_frame_without_it():
    """no child, and a child wholly outside the frame: the sub-frame has no path and its texture is cleared, not filtered -- which is what
    the rule gives (tests/test_inner_model.py: G = 0 gives 0 in both forms), so the layer adds nothing"""
    ground = isc.bs._grounds(isc.W, isc.H)["translucent"]
    base = isc._scene(ground)
    want = dr.through_render(base)
    assert want.any()
    far = [bl._rect(isc.W + 40, 5, isc.W + 60, 25, (255, 0, 0, 255))]
    for kids in ([], far):
        for sh in (dict(isc.INNER, strength=255), dict(isc.INNER_GLOW, knockout=True), dict(isc.INNER, dx=-isc.W)):
            for stage in ({"children": ground + [isc._shadowed(kids, sh)]}, {"children": ground + [isc._filtered(kids, [isc.E["blur"], fm.shadow(sh)])]}):
                dr.zero(dr.through_render(dict(base, stage=stage)), want, (len(kids), sh))


# ---- 6. nothing of an inner-shadowed frame stays behind
def test_a_plain_frame_after_an_inner_shadowed_one_is_a_fresh_handles_frame():
    dr.plain_frame_after(FAMILY, ("two_inner_and_an_outer", "list_chain_of_four", "list_and_mask_opacity"), "cairo_inner_structure")
