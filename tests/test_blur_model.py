"""tests/blur_model.py against pixman 0.40 itself (libpixman-1 through ctypes): the rule a blurred layer's box passes follow
("Blurred layers") is what PIXMAN_FILTER_CONVOLUTION computes for a box kernel, byte for byte.  No GPU.
"""
import itertools

import numpy as np
import pytest

import blur_model as bm

WIDTHS = (1, 2, 3, 4, 5, 8, 16, 255)          # 255 is wider than both images
SIZES = ((13, 11), (70, 5))                   # width x height

def _images():
    rng = np.random.default_rng(20261020)
    return {(w, h): bm.random_premultiplied(rng, h, w) for w, h in SIZES}


IMAGES = _images()


def test_pixman_is_0_40():
    assert bm.pixman().pixman_version_string().decode().startswith("0.40."), "the yardstick is pixman 0.40"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("axis", (1, 0), ids=("horizontal", "vertical"))
def test_one_pass_is_pixman_convolution(size, axis):
    words = IMAGES[size]
    for w in WIDTHS:
        want = bm.pixman_pass(words, w, axis)
        got = bm.bytes_to_words(bm.box_pass(bm.words_to_bytes(words), w, axis))
        assert int((bm.words_to_bytes(got) != bm.words_to_bytes(want)).sum()) == 0, (size, axis, w)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("passes", (1, 2, 3))
def test_blur_is_pixman_pass_by_pass(size, passes):
    words = IMAGES[size]
    for bx, by in itertools.product(WIDTHS, WIDTHS):
        want = bm.pixman_blur(words, bx, by, passes)
        got = bm.bytes_to_words(bm.blur(bm.words_to_bytes(words), bx, by, passes))
        assert int((bm.words_to_bytes(got) != bm.words_to_bytes(want)).sum()) == 0, (size, bx, by, passes)


def test_zero_width_is_width_one():
    img = bm.words_to_bytes(IMAGES[SIZES[0]])
    assert (bm.blur(img, 0, 0, 3) == img).all()
    assert (bm.blur(img, 0, 5, 2) == bm.blur(img, 1, 5, 2)).all()


def test_a_flat_region_keeps_its_value_for_every_width():
    """|f * w - 65536| <= 127, so a window that lies inside a flat region returns the region's value: every byte value, every w"""
    for w in range(1, 256):
        f = (65536 + w // 2) // w
        assert abs(f * w - 65536) <= 127, w
        v = np.arange(256, dtype=np.int64)
        assert (np.minimum(255, (f * v * w + 0x8000) >> 16) == v).all(), w
        if w >= 2:
            assert f * 255 * w + 0x8000 < 2 ** 32, w
    # and through the model on an image wider than the widest box: the pixels whose window lies inside
    img = np.full((3, 600, 4), 255, np.uint8)
    for w in (3, 7, 128, 255):
        out = bm.box_pass(img, w, 1)
        assert (out[:, w // 2:600 - (w - 1 - w // 2)] == 255).all(), w


def test_opaque_white_stays_white_in_pixman():
    words = np.full((3, 600), 0xffffffff, np.uint32)
    for w in (3, 7, 128, 255):
        out = bm.pixman_pass(words, w, 1)
        assert (out[:, w // 2:600 - (w - 1 - w // 2)] == 0xffffffff).all(), w
