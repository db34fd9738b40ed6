"""Generates tests/golden/cairo_layer_*.npz: what libcairo 1.16 renders for the isolated-layer scenes of tests/layer_scenes.py, with
cairo_push_group / cairo_pop_group_to_source / cairo_set_operator / cairo_paint around every object that carries "layer"
(LayerReplay there).  Needs the system libcairo; the outputs are data and are committed, so the tests on a GPU machine need no
libcairo.

  cairo_layer_overlap.npz             every operator x {clear, opaque, translucent} ground: overlapping translucent children (key <mode>_<ground>)
  cairo_layer_sources_<mode>.npz      strokes over their fills, morph shapes, gradients, bitmaps inside a layer (key <mode>_<scenario>)
  cairo_layer_structure_<mode>.npz    blend modes inside / around, nesting 2-4 deep, colour transforms, culling, sparse and off-frame
                                      groups, the clear-surface bookkeeping
  cairo_layer_aliased_*.npz           the same under CAIRO_ANTIALIAS_NONE
  cairo_layer_s1_crops.npz            S1 at 4K, its stars in layers of four: sha256 of the premultiplied frame and five 256 x 256 crops

Before anything is written (and under --check) every scene of layer_scenes.wrong_rule_scenes() is rendered under the rule it must not
be confused with; a scene that does not differ from it in at least one pixel, antialiased, is reported and fails the run.  So is one
that differs from the rule DESIGN.md states for it.

usage: python tools/make_layer_goldens.py [--check] [--no-s1]   (--check: regenerate in memory and compare with the committed files)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import layer_scenes as ls  # noqa: E402


def discriminates():
    """every bookkeeping scene against its right- and wrong-rule renderings: the number of scenes that fail"""
    scenes = ls.structure_scenes()
    bad = 0
    for name, (right, wrong) in sorted(ls.wrong_rule_scenes().items()):
        want = ls.cairo_render(scenes[name])

        def differing(other):
            img = ls.cairo_render(other)
            if other.get("speck"):
                img[47, 63] = want[47, 63]                             # (the speck itself is not part of the scene)
            return int((img != want).any(-1).sum())
        same = differing(right) if right is not None else 0
        diff = differing(wrong)
        ok = same == 0 and diff > 0
        print("discriminates" if ok else "DOES NOT DISCRIMINATE", name, "pixels differing from the right rule", same, "from the wrong rule", diff)
        bad += not ok
    return bad


def main():
    check = "--check" in sys.argv
    bad = discriminates()
    if bad:
        print("%d bookkeeping scenes do not discriminate" % bad)
        sys.exit(1)
    biggest = max(os.path.getsize(os.path.join(ls.bs.GOLD, f)) for f in os.listdir(ls.bs.GOLD) if f.startswith("cairo_blend_"))
    for fname, arrays in ls.goldens(with_s1="--no-s1" not in sys.argv).items():
        path = ls.golden_path(fname)
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
            assert size <= biggest, "larger than the largest blend golden (%d bytes)" % biggest
    if check:
        print("all goldens match" if not bad else "%d differ" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
