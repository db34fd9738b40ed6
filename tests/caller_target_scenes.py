"""The golden scenes of tests/test_caller_targets_gpu.py: one scene each of the layer, mask, fade and pad families, taken from the
family's own golden files (tests/device_routes.py golden_scenes) and re-framed to 192 x 24 -- three tile columns, one whole tile row
of strips and a half one -- so that the k2_tiles instance of each family stores interior strips and clipped ones with group and bitmap
content.  The re-framed stage is the scene's own objects twice: as they are, and again 64 pixels to the right and 24 pixels up (whole
pixels: no sample moves against the texel grid), so that the frame's 24 rows show the scene's rows 0..23 and 24..47.

The expected pictures are what libcairo renders for the re-framed stage with the family's own replay class
(tools/make_caller_target_goldens.py writes tests/golden/cairo_caller_targets.npz; committed, so the device tests need no libcairo).
"""
import os

import numpy as np

import fade_scenes
import layer_scenes
import mask_scenes
import pad_scenes
import scenarios

W, H = 192, 24
SHIFT = (64, -24)                                     # the second copy, in pixels
# family -> (scenes module, the k2_tiles instance its scenes pick, golden file, scene)
PICKS = {"layer": (layer_scenes, "4", "cairo_layer_sources_multiply", "multiply_bitmap_repeat_over_solid"),
         "mask": (mask_scenes, "5", "cairo_mask_sources", "bitmap_repeat_over_solid_gradientmask"),
         "fade": (fade_scenes, "6", "cairo_fade_sources", "bitmap_repeat_over_solid_normal_128"),
         "pad": (pad_scenes, "1", "cairo_pad_reach", "beyond_each_in_one_frame")}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cairo_caller_targets.npz")


def reframed(sc):
    kids = sc["stage"]["children"]
    again = {"type": "container", "matrix": scenarios._m(1, 1, SHIFT[0] * 20, SHIFT[1] * 20), "children": kids}
    return dict(sc, width=W, height=H, stage={"children": list(kids) + [again]})


def cairo_goldens(pick):
    """{family: libcairo's picture of its re-framed scene}; pick(family) -> the scene as the family's golden file has it"""
    out = {}
    for family, (module, _, _, _) in sorted(PICKS.items()):
        sc = pick(family)
        assert sc["exact"], family
        img = module.cairo_render(reframed(sc))
        assert (img[..., 3] == 0).any() and len(np.unique(img.reshape(-1, 4), axis=0)) > 16, (family, "clear pixels, and a picture")
        for x0 in range(0, W, 64):
            assert img[:, x0:x0 + 64, 3].any(), (family, "content in every tile column", x0)
        out[family] = img
    return out
