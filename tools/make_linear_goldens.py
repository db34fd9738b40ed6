"""Generates the libcairo goldens of the pixman-exact linear gradients: what libcairo 1.16 renders for tests/linear_scenes.py, with
cairo_pattern_set_extend(PAD | REFLECT | REPEAT) on every gradient as its fill says.  Needs the system libcairo; the outputs are data and
are committed, so the tests on a GPU machine need no libcairo.

usage: python tools/make_linear_goldens.py [--check]
       (--check: regenerate in memory and compare with the committed files)

  cairo_linear_<spread>_plain.npz      horizontal, vertical, rotated and sheared matrices under a polygon and under one box; a shape cut by
                                       the frame's left edge; coincident and translucent stops; a notched shape; a box off the pixel
                                       grid; the gradient_linear_ext fill
  cairo_linear_<spread>_structure.npz  a colour transform, "blend_mode", "layer", "mask", "opacity"
  No file may be larger than the largest spread golden.

The gate, before anything is written and under --check: every reflect and repeat scene must differ from its padded rendering and from
the other spread's in at least one pixel (bar config_fill, whose shape lies inside the gradient's first period).
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import linear_scenes as ls  # noqa: E402


def gates():
    bad = 0
    rendered = {(spread, name): ls.cairo_render(sc) for spread in ls.SPREADS for name, sc in sorted(ls.all_scenes(spread).items())}
    for spread in ("reflect", "repeat"):
        other = "repeat" if spread == "reflect" else "reflect"
        for name in sorted(ls.all_scenes(spread)):
            if name == "config_fill":                                # (the shape lies inside the gradient's first period)
                continue
            n_pad = int((rendered[spread, name] != rendered["pad", name]).any(-1).sum())
            n_other = int((rendered[spread, name] != rendered[other, name]).any(-1).sum())
            ok = n_pad > 0 and n_other > 0
            bad += not ok
            print("discriminates" if ok else "DOES NOT DISCRIMINATE", spread, name, "pixels differing from pad", n_pad, "from", other, n_other)
    return bad


def main():
    check = "--check" in sys.argv[1:]
    bad = gates()
    limit = max(os.path.getsize(f) for f in glob.glob(os.path.join(ROOT, "tests", "golden", "cairo_spread_*.npz")))
    for fname, scenes in sorted(ls.goldens().items()):
        path = ls.golden_path(fname)
        if check:
            old = np.load(path)
            same = sorted(old.files) == sorted(scenes) and all((old[k] == v).all() for k, v in scenes.items())
            print("same" if same else "DIFFERS", fname)
            bad += not same
        else:
            np.savez_compressed(path, **scenes)
            size = os.path.getsize(path)
            print("wrote", fname, len(scenes), "scenes,", size, "bytes")
            if size > limit:
                print("TOO LARGE", fname, size, ">", limit)
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
