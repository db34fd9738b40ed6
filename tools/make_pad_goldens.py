"""Generates the libcairo goldens of the padded bitmap fills: what libcairo 1.16 renders for tests/pad_scenes.py, with
cairo_pattern_set_extend(CAIRO_EXTEND_PAD) on the surface pattern of every fill that carries "pad".  Needs the system libcairo; the
outputs are data and are committed, so the tests on a GPU machine need no libcairo.

usage: python tools/make_pad_goldens.py [--check]
       (--check: regenerate in memory and compare with the committed files)

  cairo_pad_fit.npz        every bitmap (1 x 1, 2 x 2, 3 x 5, 8 x 8) as a shape of exactly its own rectangle, 1 x, 2.5 x and 7.75 x magnified,
                           at integer and fractional offsets
  cairo_pad_reach.npz      shapes that reach past the bitmap on all sides, past each side and each corner; rows that straddle the
                           bitmap's edge and rows wholly outside; coverage 255; the three edge rules of one bitmap in one frame
  cairo_pad_matrices.npz   rotated, skewed and mirrored matrices, an object matrix; minified below 0.75 on one axis and on both
  cairo_pad_structure.npz  under "blend_mode", "layer", "mask", "opacity"; a 300 x 40 frame
  cairo_pad_cxform.npz     under colour transforms (variant textures), one of which makes every texel translucent
  cairo_pad_aliased_*.npz  the same under CAIRO_ANTIALIAS_NONE
  No file may be larger than the largest blend golden.

The gate, before anything is written and under --check; a scene that fails it is reported and fails the run:
  wrong rule   every padded scene, in both antialias modes, must differ in at least one pixel from the same scene rendered with
               EXTEND_NONE on every bitmap fill and from the same scene rendered with EXTEND_REPEAT.  The counts are printed.
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pad_scenes as ps  # noqa: E402


def gate(rendered):
    bad = 0
    for fname, (make, aliased) in sorted(dict(ps.files(), **ps.cxform_files()).items()):
        for name, sc in sorted(make().items()):
            counts = {}
            for extend in ("none", "repeat"):
                other = ps.cairo_render(dict(sc, stage=ps.with_extend(sc["stage"], extend)), aliased)
                counts[extend] = int((rendered[fname][name] != other).any(-1).sum())
            ok = all(counts.values())
            print("discriminates" if ok else "DOES NOT DISCRIMINATE", fname, name, "pixels differing from none", counts["none"], "from repeat", counts["repeat"])
            bad += not ok
    return bad


def main():
    check = "--check" in sys.argv
    rendered = ps.goldens()
    bad = gate(rendered)
    if bad:
        print("%d scenes fail the gate" % bad)
        return 1
    limit = max(os.path.getsize(f) for f in glob.glob(os.path.join(ps.bs.GOLD, "cairo_blend_*.npz")))
    mismatch = 0
    for fname, scenes in sorted(rendered.items()):
        path = ps.golden_path(fname)
        if check:
            gold = np.load(path)
            same = sorted(gold.files) == sorted(scenes) and all((gold[k] == v).all() for k, v in scenes.items())
            print("matches" if same else "DIFFERS", fname)
            mismatch += not same
        else:
            np.savez_compressed(path, **scenes)
            size = os.path.getsize(path)
            print("wrote", fname, len(scenes), "scenes", size, "bytes")
            if size > limit:
                print("TOO LARGE", fname, size, ">", limit)
                mismatch += 1
    if check:
        print("all goldens match" if not mismatch else "%d golden files differ" % mismatch)
    return 1 if mismatch else 0


if __name__ == "__main__":
    sys.exit(main())
