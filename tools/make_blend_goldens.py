"""Generates tests/golden/cairo_blend_*.npz: what libcairo 1.16 renders for the blend-mode scenes of tests/blend_scenes.py, with
cairo_set_operator around every blended object (BlendReplay there).  Needs the system libcairo; the outputs are data and are
committed, so the tests on a GPU machine need no libcairo.

  cairo_blend_solids.npz              every mode x three alphas x {clear, opaque, translucent} ground (key <mode>_<ground>)
  cairo_blend_sources_<mode>.npz      strokes over their fills, morph shapes, gradients, bitmaps under one mode (key <mode>_<scenario>)
  cairo_blend_structure.npz           blended containers, colour transforms inside / outside, nested modes, culling, clear sources
  cairo_blend_aliased_*.npz           the same under CAIRO_ANTIALIAS_NONE
  cairo_blend_s1_crops.npz            S1 at 4K, every third star blended: sha256 of the premultiplied frame and five 256 x 256 crops
  cairo_blend_aliased_s1_crops.npz    the same under CAIRO_ANTIALIAS_NONE

usage: python tools/make_blend_goldens.py [--check]    (--check: regenerate in memory and compare with the committed files)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import blend_scenes as bs  # noqa: E402


def main():
    check = "--check" in sys.argv
    bad = 0
    for fname, arrays in bs.goldens().items():
        path = bs.golden_path(fname)
        if check:
            old = np.load(path)
            for k, v in arrays.items():
                if not (k in old.files and (old[k] == v).all()):
                    print("differs:", fname, k)
                    bad += 1
        else:
            np.savez_compressed(path, **arrays)
            print("wrote", path, os.path.getsize(path), "bytes")
    if check:
        print("all goldens match" if not bad else "%d differ" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
