"""The layer-opacity rule ("Layer opacity") in numpy: what compositing a group with an opacity leaves in a pixel of its
parent.

    result = combine_<operator>(mul_un8(g, a), d)

with g the group's premultiplied pixel, a the opacity 0..255, mul_un8 per channel -- alpha included -- with pixman's 0x80 rounding, d
the parent's pixel and combine the unmasked combiner of tests/layer_model.py: libcairo's cairo_push_group; the children;
cairo_pop_group_to_source; cairo_set_operator; cairo_paint_with_alpha(a / 255.0).  Opacity 255 is the plain layer byte for byte,
opacity 0 leaves d as it is, and a transparent group pixel still changes nothing under any operator: working inside the union of the
member rectangles stays exact.  tests/test_fade_model.py checks all of it against libcairo, for every opacity.
"""
import numpy as np

import blend_model as bm
import layer_model as lm

MODES = lm.MODES
MAX_DEPTH = lm.MAX_DEPTH                     # a faded layer takes one of these levels
PATH_GROUP_BEGIN, PATH_GROUP_END, PATH_GROUP_MASK = 2, 3, 4
OBJECT_FADED_LAYER = 13


def faded(g, opacity):
    """(..., 4) uint8: mul_un8(g, opacity) per channel (`opacity` a number, or an array that broadcasts against g)"""
    return bm.mul_un8(np.asarray(g).astype(np.int64), np.asarray(opacity).astype(np.int64)).astype(np.uint8)


def composite(mode, g, opacity, d):
    """(..., 4) uint8: the parent's pixels `d` after the group's pixels `g` are composited onto them with `mode` at `opacity`"""
    return lm.composite(mode, faded(g, opacity), d)


def end_lerp(operator, opacity):
    """swfr_path::lerp of a faded group's GROUP_END: the operator in bits 8..15, the fade 255 - opacity in bits 24..31"""
    return (int(operator) << 8) | ((255 - int(opacity)) << 24)


def parent_stays_clear(mode, group_still_clear, opacity):
    """libcairo's bookkeeping behind cairo_paint_with_alpha (tests/test_fade_model.py establishes each case on the live library):
    opacity 0 is a no-op under all nine operators whatever the group holds -- a parent that was still clear stays so; opacity 255 is
    cairo_paint, layer_model.parent_stays_clear; in between it is a cairo_mask with a solid mask that is not clear, NOTHING_TO_DO for a
    still-clear group under OVER and ADD only.  Everything else marks the parent as drawn."""
    return int(opacity) == 0 or lm.parent_stays_clear(mode, group_still_clear)
