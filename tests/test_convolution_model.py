"""tests/convolution_model.py against pixman 0.40 itself (libpixman-1 through ctypes): the rule of a convolution filter (DESIGN.md,
"Convolution filters") is what PIXMAN_FILTER_CONVOLUTION computes for the same taps, byte for byte; a kernel of equal taps is
blur_model's box pass; and the list model against libcairo + pixman applied in turn.  Zero differing bytes.  No GPU.  Skipped on a
machine without libpixman.
"""
import itertools

import numpy as np
import pytest

import blur_model as bm
import convolution_model as cm
import filter_scenes as fsc
from shadow_scenes import DROP, GLOW

pytestmark = pytest.mark.skipif(bm.pixman() is None, reason="no libpixman-1 on this machine: nothing to hold the rule against")

SIZES = ((37, 23), (3, 2))                    # width x height; the second is smaller than most kernels
DIMS = tuple(itertools.product(range(1, cm.MAX_DIM + 1), repeat=2))
KINDS = ("signed", "sparse", "bound", "negative", "zero")


def _images():
    rng = np.random.default_rng(20261022)
    return {(w, h): bm.random_premultiplied(rng, h, w) for w, h in SIZES}


IMAGES = _images()


def _hold(words, value):
    want = bm.words_to_bytes(cm.pixman_convolve(words, value))
    got = cm.convolve(bm.words_to_bytes(words), value)
    assert int((got != want).sum()) == 0, value
    return got


def test_pixman_is_0_40():
    assert bm.pixman().pixman_version_string().decode().startswith("0.40."), "the yardstick is pixman 0.40"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_every_size_of_kernel_is_pixman_convolution(size, kind):
    rng = np.random.default_rng(sum(map(ord, kind)) * 100 + size[0])
    words = IMAGES[size]
    assert len(DIMS) == 49
    above = 0
    for kw, kh in DIMS:
        value = cm.random_kernel(rng, kw, kh, kind)
        rows = cm.taps_of(value)
        assert (len(rows[0]), len(rows)) == (kw, kh) and cm.in_range(rows)
        if kind == "bound":
            assert sum(abs(t) for r in rows for t in r) == cm.MAX_ABS_SUM
        if kind == "negative":
            assert all(t < 0 for r in rows for t in r)
        got = _hold(words, value)
        if kind == "zero":
            assert not got.any(), "nothing but clear pixels"
        if kind == "negative":
            assert set(np.unique(got)) <= {0, 255}, "a negative sum is 255 to pixman's unsigned accumulators, and 0 where 0x8000 outweighs it"
        px = got.astype(np.int64)
        above += int((px[..., :3] > px[..., 3:]).any(-1).sum())
    if kind in ("signed", "bound") and size == SIZES[0]:
        assert above > 0, "signed taps make pixels whose colour exceeds their alpha"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_named_kernels_and_the_identity(size):
    words = IMAGES[size]
    for name, value in sorted(cm.NAMED.items()):
        assert cm.in_range(cm.taps_of(value)), name
        _hold(words, value)
    assert (_hold(words, cm.IDENTITY) == bm.words_to_bytes(words)).all()
    assert sum(t for r in cm.taps_of(cm.EDGE) for t in r) == 0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_equal_taps_are_the_box_pass(size):
    img = bm.words_to_bytes(IMAGES[size])
    for w in range(2, 8):
        f = (65536 + w // 2) // w
        across, down = {"taps": [[f] * w]}, {"taps": [[f]] * w}
        assert int((cm.convolve(img, across) != bm.box_pass(img, w, 1)).sum()) == 0, w
        assert int((cm.convolve(img, down) != bm.box_pass(img, w, 0)).sum()) == 0, w
        _hold(IMAGES[size], across)
        _hold(IMAGES[size], down)


def test_a_matrix_with_a_divisor_is_rounded_taps():
    assert cm.taps_of({"matrix": [[1, 1, 1]], "divisor": 3}) == [[21845, 21845, 21845]]
    assert cm.taps_of({"matrix": [[-1, 0.5]], "divisor": 3}) == [[-21845, 10923]]
    assert cm.taps_of({"matrix": [[2]]}) == [[131072]]
    assert cm.taps_of({"taps": [[7, -7]]}) == [[7, -7]]
    assert cm.as_dict(cm.SHARPEN) == {"taps": [[0, -65536, 0], [-65536, 5 * 65536, -65536], [0, -65536, 0]]}
    assert not cm.in_range([[cm.MAX_ABS_SUM, 1]]) and cm.in_range([[cm.MAX_ABS_SUM]]) and cm.in_range([[-cm.MAX_ABS_SUM]])


# ---- the list model: convolutions among the other kinds, every step by the libraries
C = cm.convolution
CHAINS = {
    "sharpen_alone": [C(cm.SHARPEN)],
    "blur_odd_sharpen": [fsc.BLUR_ODD, C(cm.SHARPEN)],
    "blur_even_emboss": [fsc.BLUR_EVEN, C(cm.EMBOSS)],
    "edge_drop": [C(cm.EDGE), fsc.ENTRIES["drop"]],
    "drop_edge": [fsc.ENTRIES["drop"], C(cm.EDGE)],
    "sharpen_inner_glow": [C(cm.SHARPEN), {"shadow": dict(GLOW, inner=True)}],
    "inner_shadow_emboss": [{"shadow": dict(DROP, inner=True)}, C(cm.EMBOSS)],
    "two_in_a_row": [C(cm.EVEN_2X2), C(cm.EVEN_4X6)],
    "four": [C(cm.EMBOSS), fsc.ENTRIES["kglow"], C(cm.MOTION_7X1), fsc.BLUR_ODD],
}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_the_list_model_is_the_call_sequences_in_turn(size, name):
    from oracle import cairo_backend as cb
    assert cb.version().startswith("1.16."), "the yardstick is libcairo 1.16"
    words = IMAGES[size]
    chain = CHAINS[name]
    want = bm.words_to_bytes(cm.cairo_apply(words, chain))
    got = cm.apply(bm.words_to_bytes(words), chain, order="bgra")
    assert int((got != want).sum()) == 0, (size, name)
    assert len(cm.as_dicts(chain)) == len(chain)


def test_the_order_matters():
    img = bm.words_to_bytes(IMAGES[SIZES[0]])
    a = cm.apply(img, CHAINS["edge_drop"], order="bgra")
    b = cm.apply(img, CHAINS["drop_edge"], order="bgra")
    assert int((a != b).sum()) > 0
