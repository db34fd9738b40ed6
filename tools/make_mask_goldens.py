"""Generates tests/golden/cairo_mask_*.npz: what libcairo 1.16 renders for the masked-layer scenes of tests/mask_scenes.py, with
cairo_push_group / cairo_pop_group twice and cairo_set_source / cairo_set_operator / cairo_mask around every object that carries "mask"
(MaskReplay there).  Needs the system libcairo; the outputs are data and are committed, so the tests on a GPU machine need no libcairo.

  cairo_mask_sources.npz      solid, gradient and bitmap content under solid, translucent and gradient masks; the geometry-only mask;
                              strokes in a mask; "mask" on a shape and a morph shape
  cairo_mask_operators.npz    every operator x {clear, opaque, translucent} ground (key <mode>_<ground>)
  cairo_mask_structure.npz    masks off the frame and beside the content, nesting, plain layers in either half, blend modes, colour
                              transforms, culling, sparse groups, the clear-surface bookkeeping (key <kind>_<mode>)
  cairo_mask_aliased_*.npz    the same under CAIRO_ANTIALIAS_NONE

Before anything is written (and under --check) every scene of mask_scenes.wrong_rule_scenes() is rendered under the rule it must not be
confused with; a scene that does not differ from it in at least one pixel, antialiased, is reported and fails the run.  So is one that
differs from the rule DESIGN.md states for it.

usage: python tools/make_mask_goldens.py [--check]   (--check: regenerate in memory and compare with the committed files)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mask_scenes as ms  # noqa: E402


def discriminates():
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
        same, diff = differing(right), differing(wrong)
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
    for fname, arrays in ms.goldens().items():
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
            assert size <= 1 << 20
    if check:
        print("all goldens match" if not bad else "%d differ" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
