"""The masked-layer rule ("Masked layers") in numpy: what compositing a content group through a mask group's alpha leaves in
a pixel of the parent.

    result = combine_<operator>(mul_un8(C, Ma), d)

with C the content group's premultiplied pixel, Ma the mask group's ALPHA (its colour channels play no part), mul_un8 per channel with
pixman's 0x80 rounding, d the parent's pixel and combine the unmasked combiner of tests/layer_model.py -- libcairo's cairo_mask with a
group as the source and a group as the mask.  A transparent mask pixel makes the product transparent, and a transparent source leaves d
as it is under all nine operators: working inside the union of the member rectangles is exact.  tests/test_mask_model.py checks it
against libcairo.
"""
import numpy as np

import blend_model as bm
import layer_model as lm

MODES = lm.MODES
MAX_DEPTH = lm.MAX_DEPTH                     # a masked group takes two of these levels
PATH_GROUP_BEGIN, PATH_GROUP_END, PATH_GROUP_MASK = 2, 3, 4
OBJECT_MASKED_LAYER = 11


def masked(content, mask):
    """(..., 4) uint8: mul_un8(content, mask alpha) per channel"""
    content, mask = np.asarray(content), np.asarray(mask)
    return bm.mul_un8(content.astype(np.int64), mask[..., 3:4].astype(np.int64)).astype(np.uint8)


def composite(mode, content, mask, d):
    """(..., 4) uint8: the parent's pixels `d` after the content group's pixels are composited onto them through the mask group's"""
    return lm.composite(mode, masked(content, mask), d)


def nothing_to_do(mode, content_still_clear, mask_still_clear):
    """libcairo's bookkeeping: cairo_mask with a still-clear mask surface is NOTHING_TO_DO under every operator, with a still-clear
    source surface under OVER and ADD only.  Then a parent that was still clear stays so; otherwise -- both were drawn on, even if every
    pixel of them is zero -- the parent counts as drawn."""
    return mask_still_clear or (content_still_clear and mode in ("normal", "add"))
