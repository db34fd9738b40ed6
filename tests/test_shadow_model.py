"""tests/shadow_model.py against live libcairo 1.16 + pixman 0.40 (ctypes): the byte rule of a shadowed layer's steps 2 to 6 (DESIGN.md,
"Shadowed layers") is what the literal call sequence computes -- cairo_mask_surface for the shifted alpha and for the tint, pixman's
convolution for the blur, ADD paints for the strength, an OVER or DEST_OUT paint of the group.  Zero differing bytes.  No GPU.
"""
import itertools

import numpy as np
import pytest

import blur_model as bm
import shadow_model as sm
from oracle import cairo_backend as cb
from shadow_model import COLORS, FLAGS, STRENGTHS, offsets

SIZES = ((13, 11), (70, 5))                   # width x height
BOXES = ((1, 1), (2, 3), (5, 4), (255, 255))
PASSES = (1, 3)


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
        want = bm.words_to_bytes(sm.cairo_shadow(words, sh))
        got = sm.shadow(img, sh, order="bgra")
        assert int((got != want).sum()) == 0, (size, sh)
        done += 1
    assert done == 5 * 4 * 2 * 4


def test_the_steps_one_by_one():
    """what each step is expected to be, on its own: the shifted alpha with clear colour channels, the saturating strength, the tint's
    0x80 rounding from the colour's premultiplied pixel"""
    words = IMAGES[SIZES[0]]
    img = bm.words_to_bytes(words)
    h, w = words.shape
    a = img[..., 3]
    # steps 2, 4 and 5 alone: a 1 x 1 box, an opaque white colour (cp = 255 everywhere), the object hidden -> alpha in every channel
    for dx, dy in offsets(w, h):
        out = bm.words_to_bytes(sm.cairo_shadow(words, {"color": (255, 255, 255, 255), "dx": dx, "dy": dy, "hide_object": True}))
        want = sm.shifted_alpha(a, dx, dy)
        assert (out == want[..., None]).all(), (dx, dy)
        for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 3)):
            inside = 0 <= x - dx < w and 0 <= y - dy < h
            assert want[y, x] == (a[y - dy, x - dx] if inside else 0)
    assert sm.shifted_alpha(a, w, 0).max() == 0 and np.count_nonzero(sm.shifted_alpha(np.full_like(a, 9), -(w - 1), h - 1)) == 1
    out = bm.words_to_bytes(sm.cairo_shadow(words, {"color": (255, 255, 255, 255), "strength": 3, "hide_object": True}))
    assert (out[..., 3] == np.minimum(255, 3 * a.astype(np.int64))).all()
    color = COLORS["translucent"]
    out = bm.words_to_bytes(sm.cairo_shadow(words, {"color": color, "hide_object": True}))
    r, g, b, al = sm.premultiplied_pixel(color)
    for k, c in enumerate((b, g, r, al)):
        assert (out[..., k] == sm.mul_un8(np.int64(c), a.astype(np.int64))).all(), k


def test_a_transparent_colour_leaves_the_group_and_knocks_out_nothing_visible():
    words = IMAGES[SIZES[1]]
    img = bm.words_to_bytes(words)
    sh = {"color": COLORS["clear"], "x": 5, "y": 4, "strength": 3}
    assert (sm.shadow(img, sh, order="bgra") == img).all()
    assert not sm.shadow(img, dict(sh, knockout=True), order="bgra").any()
    assert not sm.shadow(img, dict(sh, hide_object=True), order="bgra").any()


def test_premultiplied_pixel_is_cairos_for_every_alpha():
    """against cairo_set_source_rgba + cairo_paint(SOURCE would do; OVER onto clear is the source) on a 1 x 1 surface"""
    lib = sm.cairo()
    rng = np.random.default_rng(7)
    for a in list(range(0, 256, 5)) + [1, 254, 255]:
        r, g, b = (int(v) for v in rng.integers(0, 256, 3))
        s = sm._Surface(lib, np.zeros((1, 1), np.uint32))
        try:
            lib.cairo_set_source_rgba(s.cr, r / 255.0, g / 255.0, b / 255.0, a / 255.0)
            lib.cairo_paint(s.cr)
            word = int(s.flush()[0, 0])
        finally:
            s.close()
        pr, pg, pb, pa = sm.premultiplied_pixel((r, g, b, a))
        assert word == (pa << 24 | pr << 16 | pg << 8 | pb), (r, g, b, a)
