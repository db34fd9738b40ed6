"""Generates the libcairo goldens of one compositing family: what libcairo 1.16 renders for the family's scenes module, with the Cairo
calls of its replay class around every object that carries the family's key.  Needs the system libcairo; the outputs are data and are
committed, so the tests on a GPU machine need no libcairo.

usage: python tools/make_composite_goldens.py {blend,layer,mask,fade} [--check] [--no-s1]
       (--check: regenerate in memory and compare with the committed files; --no-s1: layer only, without the 4K frame)

blend   tests/blend_scenes.py, BlendReplay: cairo_set_operator around every blended object
  cairo_blend_solids.npz              every mode x three alphas x {clear, opaque, translucent} ground (key <mode>_<ground>)
  cairo_blend_sources_<mode>.npz      strokes over their fills, morph shapes, gradients, bitmaps under one mode (key <mode>_<scenario>)
  cairo_blend_structure.npz           blended containers, colour transforms inside / outside, nested modes, culling, clear sources
  cairo_blend_s1_crops.npz            S1 at 4K, every third star blended: sha256 of the premultiplied frame and five 256 x 256 crops

layer   tests/layer_scenes.py, LayerReplay: cairo_push_group / cairo_pop_group_to_source / cairo_set_operator / cairo_paint around
        every object that carries "layer"
  cairo_layer_overlap.npz             every operator x {clear, opaque, translucent} ground: overlapping translucent children (key <mode>_<ground>)
  cairo_layer_sources_<mode>.npz      strokes over their fills, morph shapes, gradients, bitmaps inside a layer (key <mode>_<scenario>)
  cairo_layer_structure_<mode>.npz    blend modes inside / around, nesting 2-4 deep, colour transforms, culling, sparse and off-frame
                                      groups, the clear-surface bookkeeping
  cairo_layer_s1_crops.npz            S1 at 4K, its stars in layers of four: sha256 of the premultiplied frame and five 256 x 256 crops
  No file may be larger than the largest blend golden.

mask    tests/mask_scenes.py, MaskReplay: cairo_push_group / cairo_pop_group twice and cairo_set_source / cairo_set_operator /
        cairo_mask around every object that carries "mask"
  cairo_mask_sources.npz      solid, gradient and bitmap content under solid, translucent and gradient masks; the geometry-only mask;
                              strokes in a mask; "mask" on a shape and a morph shape
  cairo_mask_operators.npz    every operator x {clear, opaque, translucent} ground (key <mode>_<ground>)
  cairo_mask_structure.npz    masks off the frame and beside the content, nesting, plain layers in either half, blend modes, colour
                              transforms, culling, sparse groups, the clear-surface bookkeeping (key <kind>_<mode>)

fade    tests/fade_scenes.py, FadeReplay: cairo_push_group / cairo_pop_group_to_source / cairo_set_operator / cairo_paint_with_alpha
        around every object that carries "opacity"
  cairo_fade_sources.npz      gradient, bitmap and stroked members; "opacity" on a shape and a morph shape; opacity 255 and 0; the
                              overlapping children faded as a whole, and per definition by a colour transform
  cairo_fade_operators.npz    every operator x opacity {1, 128, 254} x {opaque, translucent} ground, 128 over a clear one
                              (key <mode>_<opacity>_<ground>)
  cairo_fade_structure.npz    nesting, plain layers around and inside, faded around masked and inside either half, blend modes, colour
                              transforms, culling, sparse and off-frame groups, the clear-surface bookkeeping (key <kind>_<opacity>_<mode>)

Every family also writes cairo_<family>_aliased_*.npz: the same under CAIRO_ANTIALIAS_NONE.

The wrong-rule gate (layer, mask, fade): before anything is written, and under --check, every scene of the module's
wrong_rule_scenes() is rendered under the rule it must not be confused with; a scene that does not differ from it in at least one
pixel, antialiased, is reported and fails the run.  So is one that differs from the rule DESIGN.md states for it, and, for fade, the
"as a whole" scene if it equals its "per definition" twin.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import blend_scenes  # noqa: E402
import fade_scenes  # noqa: E402
import layer_scenes  # noqa: E402
import mask_scenes  # noqa: E402

FAMILIES = {"blend": blend_scenes, "layer": layer_scenes, "mask": mask_scenes, "fade": fade_scenes}


def discriminates(ms):
    """every bookkeeping scene against its right- and wrong-rule renderings: the number of scenes that fail"""
    scenes = ms.structure_scenes()
    bad = 0
    for name, (right, wrong) in sorted(ms.wrong_rule_scenes().items()):
        want = ms.cairo_render(scenes[name])

        def differing(other):
            img = ms.cairo_render(other)
            if other.get("speck"):
                img[47, 63] = want[47, 63]                             # (the speck itself is not part of the scene)
            return int((img != want).any(-1).sum())
        same = differing(right) if right is not None else 0
        diff = differing(wrong)
        ok = same == 0 and diff > 0
        print("discriminates" if ok else "DOES NOT DISCRIMINATE", name, "pixels differing from the right rule", same, "from the wrong rule", diff)
        bad += not ok
    if ms is fade_scenes:
        src = ms.source_scenes()
        n = int((ms.cairo_render(src["whole_not_per_definition"]) != ms.cairo_render(src["per_definition"])).any(-1).sum())
        print("as a whole differs from per definition in", n, "pixels")
        bad += n == 0
    return bad


def main():
    family = next((a for a in sys.argv[1:] if a in FAMILIES), None)
    if family is None:
        sys.exit(__doc__[__doc__.index("usage:"):].split("\n\n")[0])
    ms = FAMILIES[family]
    check = "--check" in sys.argv
    bad = discriminates(ms) if hasattr(ms, "wrong_rule_scenes") else 0
    if bad:
        print("%d bookkeeping scenes do not discriminate" % bad)
        sys.exit(1)
    limit = 1 << 20
    if family == "layer":
        limit = max(os.path.getsize(os.path.join(blend_scenes.GOLD, f)) for f in os.listdir(blend_scenes.GOLD) if f.startswith("cairo_blend_"))
    arrays_of = ms.goldens(with_s1="--no-s1" not in sys.argv) if family == "layer" else ms.goldens()
    for fname, arrays in arrays_of.items():
        path = ms.golden_path(fname)
        if check:
            old = np.load(path)
            for k, v in arrays.items():
                if not (k in old.files and (old[k] == v).all()):
                    print("differs:", fname, k)
                    bad += 1
        else:
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            print("wrote", path, size, "bytes")
            assert size <= limit, "larger than %d bytes" % limit
    if check:
        print("all goldens match" if not bad else "%d differ" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
