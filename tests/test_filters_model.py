"""tests/filter_model.py against live libcairo 1.16 + pixman 0.40 (ctypes): the fold of the numpy models of a blurred and a shadowed
layer (blur_model.blur, shadow_model.shadow applied in turn) is what the libraries' call sequences applied in turn compute
(blur_model.pixman_blur, shadow_model.cairo_shadow) -- DESIGN.md, "Filter lists".  Zero differing bytes.  No GPU.
"""
import itertools

import numpy as np
import pytest

import blur_model as bm
import filter_model as fm
import filter_scenes as fsc
from oracle import cairo_backend as cb
from shadow_scenes import DROP, GLOW

SIZES = ((13, 11), (70, 5))                   # width x height
ENTRIES = fsc.ENTRIES
# chains of three and four: the issue's chain of four; a 255-wide box, strength 255 and an offset that shifts everything out (of both
# sizes); every kind behind every kind
CHAINS = {
    "chain_of_four": fsc.CHAIN_OF_FOUR,
    "wide_strong_out": [fm.blur(255, 3, 1), fm.shadow(GLOW, strength=255), fm.shadow(DROP, dx=70, dy=0), fm.blur(2, 2, 1)],
    "out_first": [fm.shadow(DROP, dx=-70, dy=11, hide_object=True), fm.blur(3, 3, 2), fm.shadow(GLOW, strength=255, color=(0, 200, 90, 90))],
    "three_shadows": [ENTRIES["drop"], ENTRIES["kglow"], ENTRIES["glow"]],
    "three_blurs_and_a_glow": [fm.blur(2, 0, 1), fm.blur(0, 255, 1), fm.blur(5, 4, 3), ENTRIES["glow"]],
    "noop_in_the_middle": [ENTRIES["glow"], fm.blur(1, 1, 1), ENTRIES["hdrop"]],
}


def _images():
    rng = np.random.default_rng(20261021)
    return {(w, h): bm.random_premultiplied(rng, h, w) for w, h in SIZES}


IMAGES = _images()


def _hold(size, chain):
    words = IMAGES[size]
    want = bm.words_to_bytes(fm.cairo_apply(words, chain))
    got = fm.apply(bm.words_to_bytes(words), chain, order="bgra")
    assert int((got != want).sum()) == 0, (size, chain)
    return got


def test_the_libraries_are_cairo_1_16_and_pixman_0_40():
    assert cb.version().startswith("1.16."), "the yardstick is libcairo 1.16"
    assert bm.pixman().pixman_version_string().decode().startswith("0.40."), "the yardstick is pixman 0.40"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_ordered_pair_is_the_call_sequences_in_turn(size):
    assert len(ENTRIES) == 6
    results = {}
    for a, b in itertools.product(sorted(ENTRIES), repeat=2):
        results[a, b] = _hold(size, [ENTRIES[a], ENTRIES[b]])
    assert len(results) == 36
    # the order matters: the two orders of a pair of unlike entries are not the same picture
    for a, b in (("glow", "drop"), ("blur_even", "drop"), ("kglow", "blur_even"), ("blur_odd", "hdrop")):
        assert int((results[a, b] != results[b, a]).sum()) > 0, (a, b)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chains_of_three_and_four(name, size):
    chain = CHAINS[name]
    assert 3 <= len(chain) <= fm.MAX_FILTERS
    _hold(size, chain)


def test_the_chains_hold_the_extremes():
    flat = [e for chain in CHAINS.values() for e in chain]
    assert sum(len(c) == 3 for c in CHAINS.values()) >= 2 and sum(len(c) == 4 for c in CHAINS.values()) >= 2
    assert any("blur" in e and 255 in (e["blur"]["x"], e["blur"]["y"]) for e in flat), "a 255-wide box"
    assert any("shadow" in e and e["shadow"].get("strength") == 255 for e in flat), "strength 255"
    assert any("shadow" in e and abs(e["shadow"].get("dx", 0)) >= max(w for w, _ in SIZES) for e in flat), "an offset that shifts everything out"


def test_a_list_of_one_is_the_single_rule_and_a_1x1_blur_changes_nothing():
    for size in SIZES:
        img = bm.words_to_bytes(IMAGES[size])
        import shadow_model as sm
        assert (fm.apply(img, [ENTRIES["drop"]], "bgra") == sm.shadow(img, DROP, "bgra")).all()
        assert (fm.apply(img, [ENTRIES["blur_odd"]], "bgra") == bm.blur(img, 2, 0, 3)).all()
        with_noop = fm.apply(img, [ENTRIES["glow"], fm.blur(1, 1, 2), ENTRIES["drop"]], "bgra")
        assert (with_noop == fm.apply(img, [ENTRIES["glow"], ENTRIES["drop"]], "bgra")).all()


def test_no_intermediate_surface_holds_a_colour_above_its_alpha():
    """every R_i stays premultiplied, so the next entry's rule reads what Cairo would read"""
    for size in SIZES:
        img = bm.words_to_bytes(IMAGES[size])
        for chain in list(CHAINS.values()) + [[ENTRIES[a], ENTRIES[b]] for a, b in itertools.product(sorted(ENTRIES), repeat=2)]:
            for n in range(1, len(chain) + 1):
                out = fm.apply(img, chain[:n], "bgra")
                assert (out[..., :3] <= out[..., 3:]).all(), (size, chain[:n])
