"""Generates the libcairo goldens of the unsmoothed bitmap fills: what libcairo 1.16 renders for tests/nearest_scenes.py, with
cairo_pattern_set_filter(CAIRO_FILTER_NEAREST) on the surface pattern of every fill that carries "filter": "nearest".  Needs the
system libcairo; the outputs are data and are committed, so the tests on a GPU machine need no libcairo.

usage: python tools/make_nearest_goldens.py [--check]
       (--check: regenerate in memory and compare with the committed files)

  cairo_nearest_none.npz / _repeat / _pad   one edge rule each: 3 x and 7.3 x magnified, 1:1 at a fractional offset, 0.45 x and 0.3 x minified,
                                            rotated, mirrored; the 1 x 1, 2 x 2, 1 x 7 and 7 x 1 bitmaps; the 80 x 24 one at 1:1 and 3 x
  cairo_nearest_edges.npz                   the texel-edge fills: every sample exactly on a texel edge, per edge rule
  cairo_nearest_shapes.npz                  a triangle, a stroked shape, a nearest beside a good fill, a morph shape over a nearest fill
  cairo_nearest_structure.npz               under "blend_mode", "layer", "mask", "opacity"; a 300 x 40 frame
  cairo_nearest_cxform.npz                  under colour transforms (variant textures)
  cairo_nearest_aliased_*.npz               the same under CAIRO_ANTIALIAS_NONE
  No file may be larger than the largest pad golden.

The gate, before anything is written and under --check; a scene that fails it is reported and fails the run:
  wrong rule   every texel-edge scene, in both antialias modes, must differ in at least one pixel from what tests/nearest_model.py's
               floor(f) rule gives for its box (and equal what its own rule gives); every minified scene must differ from the same
               scene rendered with CAIRO_FILTER_GOOD.  The counts are printed.
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import host_frames as hf  # noqa: E402
import nearest_model as nm  # noqa: E402
import nearest_scenes as ns  # noqa: E402

EXTEND = {"none": nm.NONE, "repeat": nm.REPEAT, "pad": nm.PAD}


def gate(rendered):
    bad = 0
    texels = hf.bitmaps_of(dict(bitmaps=ns.BITMAPS))[ns.EDGE_BITMAP]
    for aliased in (False, True):
        fname = "cairo_nearest_%sedges" % ("aliased_" if aliased else "")
        for name, b in sorted(ns.edge_boxes().items()):
            frames = {rule: nm.frame([b["matrix"]], texels, b["rect"], EXTEND[b["extend"]], ns.W, ns.H, fetch)[0]
                      for rule, fetch in (("nearest", nm.nearest_many), ("floor", nm.floor_many))}
            n_own = int((rendered[fname][name] != frames["nearest"]).any(-1).sum())
            n_floor = int((rendered[fname][name] != frames["floor"]).any(-1).sum())
            ok = n_own == 0 and n_floor > 0
            print("discriminates" if ok else "DOES NOT DISCRIMINATE", fname, name, "pixels differing from the model", n_own, "from floor(f)", n_floor)
            bad += not ok
        for extend in ns.EXTENDS:
            fname = "cairo_nearest_%s%s" % ("aliased_" if aliased else "", extend)
            scenes = ns.extend_scenes(extend)
            for name in ns.MINIFIED:
                good = ns.cairo_render(dict(scenes[name], stage=ns.with_filter(scenes[name]["stage"], "good")), aliased)
                n = int((rendered[fname][name] != good).any(-1).sum())
                print("discriminates" if n else "DOES NOT DISCRIMINATE", fname, name, "pixels differing from CAIRO_FILTER_GOOD", n)
                bad += not n
    return bad


def main():
    check = "--check" in sys.argv
    rendered = ns.goldens()
    bad = gate(rendered)
    if bad:
        print("%d scenes fail the gate" % bad)
        return 1
    limit = max(os.path.getsize(f) for f in glob.glob(os.path.join(ns.bs.GOLD, "cairo_pad_*.npz")))
    mismatch = 0
    for fname, scenes in sorted(rendered.items()):
        path = ns.golden_path(fname)
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
