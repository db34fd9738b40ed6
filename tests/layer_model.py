"""The isolated-layer rule ("Isolated layers") in numpy: what compositing a group leaves in a pixel of its parent.

    result = combine_<operator>(g, d)

with g the group's premultiplied pixel and d the parent's -- pixman's unified combiners WITHOUT a mask: the source is the group pixel
itself, there is no mul_un8 by a coverage (mul_un8(x, 255) = x, so it is also tests/blend_model.py's rule at coverage 255).  "normal"
(modes 0, 1 and 2) is OVER: g + mul_un8(d, 255 - ga).  A transparent group pixel leaves d as it is under all nine operators, which is
why compositing only inside the union of the group's path rectangles is exact.  Inside the group every rule of the frame holds, seen
from the group's surface, which starts clear.  tests/test_layer_model.py checks it against libcairo.
"""
import numpy as np

import blend_model as bm

MODES = dict(bm.MODES, normal=1)             # the modes a layer can be composited with ("layer", 2, is "normal")
REFUSED = {"subtract": 9, "invert": 10, "alpha": 11, "erase": 12}
MAX_DEPTH = 4
PATH_GROUP_BEGIN, PATH_GROUP_END = 2, 3


def composite(mode, g, d):
    """(..., 4) uint8: the parent's pixels `d` after the group's pixels `g` are composited onto them with `mode`"""
    g = np.asarray(g)
    return bm.blend(mode, g, np.full(g.shape[:-1], 255, np.int64), d)


def parent_stays_clear(mode, group_still_clear):
    """libcairo's bookkeeping: painting a group whose surface is still clear (nothing was drawn on it: it is empty, all its paths
    miss the frame, or it holds only clear sources under OVER / ADD) is NOTHING_TO_DO under OVER and ADD -- a parent that was still
    clear stays so.  Under any other operator, and behind any group that was drawn on, the parent counts as drawn."""
    return group_still_clear and mode in ("normal", "add")
