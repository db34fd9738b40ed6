"""tests/inner_model.py against live libcairo 1.16 + pixman 0.40 (ctypes): the byte rule of an inner shadow's steps 2' to 6' (DESIGN.md,
"Inner shadows") is what the literal call sequence computes -- an opaque paint and a DEST_OUT cairo_mask_surface for the inverse alpha,
pixman's convolution for the blur, ADD paints for the strength, cairo_mask_surface for the tint, an ATOP paint onto the group or a DEST_IN
paint of it.  Zero differing bytes.  No GPU.
"""
import itertools

import numpy as np
import pytest

import blur_model as bm
import filter_model as fm
import inner_model as im
import shadow_model as sm
from oracle import cairo_backend as cb
from shadow_model import COLORS, STRENGTHS, offsets
from shadow_scenes import DROP, GLOW

SIZES = ((13, 11), (70, 5))                   # width x height
BOXES = ((1, 1), (2, 3), (5, 4), (255, 255))
PASSES = (1, 3)
FLAGS = {"atop": {"inner": True}, "knockout": {"inner": True, "knockout": True}}
# the entries of the pairs and the chain: a blur of three box steps, an outer drop shadow, an inner shadow, an inner knockout glow
ENTRIES = {"blur_odd": fm.blur(2, 0, 3), "drop": fm.shadow(DROP), "inner": fm.shadow(DROP, inner=True),
           "inner_kglow": fm.shadow(GLOW, inner=True, knockout=True)}
CHAIN_OF_FOUR = [ENTRIES["inner"], fm.blur(2, 2, 2), ENTRIES["drop"], ENTRIES["inner_kglow"]]


def _images():
    rng = np.random.default_rng(20261021)
    return {(w, h): bm.random_premultiplied(rng, h, w) for w, h in SIZES}


IMAGES = _images()


def test_the_libraries_are_cairo_1_16_and_pixman_0_40():
    assert cb.version().startswith("1.16."), "the yardstick is libcairo 1.16"
    assert bm.pixman().pixman_version_string().decode().startswith("0.40."), "the yardstick is pixman 0.40"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flags", sorted(FLAGS))
@pytest.mark.parametrize("color", sorted(COLORS))
def test_the_model_is_the_call_sequence(size, flags, color):
    w, h = size
    words = IMAGES[size]
    img = bm.words_to_bytes(words)
    assert (img[..., 3] == 255).any() and (img[..., 3] == 0).any()
    done = 0
    for (dx, dy), (bx, by), passes, strength in itertools.product(offsets(w, h), BOXES, PASSES, STRENGTHS):
        sh = dict(FLAGS[flags], color=COLORS[color], dx=dx, dy=dy, x=bx, y=by, passes=passes, strength=strength)
        want = bm.words_to_bytes(im.cairo_inner_shadow(words, sh))
        got = im.inner_shadow(img, sh, order="bgra")
        assert int((got != want).sum()) == 0, (size, sh)
        done += 1
    assert done == 5 * 4 * 2 * 4


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_inverse_alpha_surface_alone(size):
    """step 2' against the opaque paint and the DEST_OUT mask call: 255 - Ga shifted, 255 where the source pixel lies outside, clear
    colour channels"""
    w, h = size
    words = IMAGES[size]
    a = bm.words_to_bytes(words)[..., 3]
    for dx, dy in offsets(w, h):
        out = bm.words_to_bytes(im.cairo_inverse_alpha(words, dx, dy))
        want = im.inverse_alpha(a, dx, dy)
        assert not out[..., :3].any(), (dx, dy)
        assert (out[..., 3] == want).all(), (dx, dy)
        for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 3)):
            inside = 0 <= x - dx < w and 0 <= y - dy < h
            assert want[y, x] == (255 - a[y - dy, x - dx] if inside else 255)
    assert (im.inverse_alpha(a, w, 0) == 255).all(), "everything shifted out: empty everywhere"
    one_left = im.inverse_alpha(np.full_like(a, 200), -(w - 1), h - 1)
    assert np.count_nonzero(one_left != 255) == 1 and one_left[h - 1, 0] == 55, "one pixel left"


def test_alpha_is_the_groups_and_no_colour_is_above_its_alpha():
    for size in SIZES:
        w, h = size
        img = bm.words_to_bytes(IMAGES[size])
        for (dx, dy), (bx, by, passes), strength, color in itertools.product(offsets(w, h), ((1, 1, 1), (5, 4, 3)), STRENGTHS, sorted(COLORS)):
            sh = dict(color=COLORS[color], dx=dx, dy=dy, x=bx, y=by, passes=passes, strength=strength, inner=True)
            out = im.inner_shadow(img, sh, order="bgra")
            assert (out[..., 3] == img[..., 3]).all(), (size, sh)
            assert (out[..., :3] <= out[..., 3:]).all(), (size, sh)
            out = im.inner_shadow(img, dict(sh, knockout=True), order="bgra")
            assert (out[..., :3] <= out[..., 3:]).all() and (out[..., 3] <= img[..., 3]).all(), (size, sh)


def test_everything_shifted_out_tints_the_object_uniformly():
    """the second edge consequence: Sa = 255 everywhere, so Tc is the colour's pixel everywhere (1 x 1 box: the blur reads nothing
    beyond the frame)"""
    w, h = SIZES[0]
    img = bm.words_to_bytes(IMAGES[SIZES[0]]).astype(np.int64)
    r, g, b, a = sm.premultiplied_pixel(COLORS["translucent"])
    cp = np.array((b, g, r, a), np.int64)
    out = im.inner_shadow(img.astype(np.uint8), {"color": COLORS["translucent"], "dx": w, "x": 1, "y": 1, "inner": True}, order="bgra")
    want = np.minimum(255, sm.mul_un8(cp[None, None, :], img[..., 3:]) + sm.mul_un8(img, 255 - a))
    assert (out == want).all()


def test_an_empty_group_stays_empty():
    clear = np.zeros((5, 9, 4), np.uint8)
    for flags in FLAGS.values():
        sh = dict(flags, color=COLORS["opaque"], dx=1, x=3, y=3, strength=255)
        assert not im.inner_shadow(clear, sh).any()
        assert not im.cairo_inner_shadow(np.zeros((5, 9), np.uint32), sh).any()


def _hold(size, chain):
    words = IMAGES[size]
    want = bm.words_to_bytes(im.cairo_apply(words, chain))
    got = im.apply(bm.words_to_bytes(words), chain, order="bgra")
    assert int((got != want).sum()) == 0, (size, chain)
    return got


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_ordered_pair_and_a_chain_of_four(size):
    results = {}
    for a, b in itertools.product(sorted(ENTRIES), repeat=2):
        results[a, b] = _hold(size, [ENTRIES[a], ENTRIES[b]])
    assert len(results) == 16
    for a, b in (("inner", "drop"), ("blur_odd", "inner"), ("inner_kglow", "drop"), ("inner", "inner_kglow")):
        assert int((results[a, b] != results[b, a]).sum()) > 0, (a, b)
    assert sum(im.is_inner(e.get("shadow", {})) for e in CHAIN_OF_FOUR) == 2 and len(CHAIN_OF_FOUR) == 4
    _hold(size, CHAIN_OF_FOUR)


def test_an_inner_shadow_is_not_the_outer_one_and_the_dispatch_keeps_the_old_rules():
    for size in SIZES:
        img = bm.words_to_bytes(IMAGES[size])
        for sh in (DROP, GLOW, dict(GLOW, knockout=True)):
            inner = im.shadow(img, dict(sh, inner=True), "bgra")
            assert (im.shadow(img, sh, "bgra") == sm.shadow(img, sh, "bgra")).all()
            assert int((inner != sm.shadow(img, sh, "bgra")).sum()) > 0, sh
            assert (im.apply(img, [fm.shadow(sh, inner=True)], "bgra") == inner).all()
        chain = [fm.blur(2, 0, 3), fm.shadow(DROP), fm.shadow(GLOW, hide_object=True)]
        assert (im.apply(img, chain, "bgra") == fm.apply(img, chain, "bgra")).all()
        assert (im.cairo_apply(IMAGES[size], chain) == fm.cairo_apply(IMAGES[size], chain)).all()


def test_as_dict_reports_inner_only_where_it_is_set():
    assert im.as_dict(DROP) == sm.as_dict(DROP) and "inner" not in im.as_dict(dict(DROP, inner=False))
    assert im.as_dict(dict(DROP, inner=True)) == dict(sm.as_dict(DROP), inner=True)
    assert im.as_dicts([fm.blur(2, 3), fm.shadow(GLOW, inner=True, knockout=True)]) == \
        [{"blur": {"x": 2, "y": 3, "passes": 1}}, {"shadow": dict(sm.as_dict(dict(GLOW, knockout=True)), inner=True)}]
