"""Generates tests/golden/cairo_fade_*.npz: what libcairo 1.16 renders for the layer-opacity scenes of tests/fade_scenes.py, with
cairo_push_group / cairo_pop_group_to_source / cairo_set_operator / cairo_paint_with_alpha around every object that carries "opacity"
(FadeReplay there).  Needs the system libcairo; the outputs are data and are committed, so the tests on a GPU machine need no libcairo.

  cairo_fade_sources.npz      gradient, bitmap and stroked members; "opacity" on a shape and a morph shape; opacity 255 and 0; the
                              overlapping children faded as a whole, and per definition by a colour transform
  cairo_fade_operators.npz    every operator x opacity {1, 128, 254} x {opaque, translucent} ground, 128 over a clear one
                              (key <mode>_<opacity>_<ground>)
  cairo_fade_structure.npz    nesting, plain layers around and inside, faded around masked and inside either half, blend modes, colour
                              transforms, culling, sparse and off-frame groups, the clear-surface bookkeeping (key <kind>_<opacity>_<mode>)
  cairo_fade_aliased_*.npz    the same under CAIRO_ANTIALIAS_NONE

Before anything is written (and under --check) every scene of fade_scenes.wrong_rule_scenes() is rendered under the rule it must not be
confused with; a scene that does not differ from it in at least one pixel, antialiased, is reported and fails the run.  So is one that
differs from the rule DESIGN.md states for it, and so is the "as a whole" scene if it equals its "per definition" twin.

usage: python tools/make_fade_goldens.py [--check]   (--check: regenerate in memory and compare with the committed files)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import fade_scenes as ms  # noqa: E402


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
    src = ms.source_scenes()
    n = int((ms.cairo_render(src["whole_not_per_definition"]) != ms.cairo_render(src["per_definition"])).any(-1).sum())
    print("as a whole differs from per definition in", n, "pixels")
    return bad + (n == 0)


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
