"""Generates the libcairo goldens of the erase and alpha modes ("Erase and alpha modes"): what libcairo 1.16 renders for
tests/alpha_modes_scenes.py, with CAIRO_OPERATOR_DEST_OUT for "erase" and CAIRO_OPERATOR_DEST_IN for "alpha" in the replays of the
blend, layer, mask and fade families.  Needs the system libcairo; the outputs are data and are committed, so the tests on a GPU
machine need no libcairo.

usage: python tools/make_alpha_mode_goldens.py [--check]
       (--check: regenerate in memory and compare with the committed files)

  cairo_alphamode_layers.npz       erase and alpha layers, plain, faded and masked, over an opaque and a translucent ground
  cairo_alphamode_transparent.npz  layers with a transparent source (empty, opacity 0, empty mask, empty content, a clear fill), over
                                   a ground and on a clear frame, translucent triangles behind them
  cairo_alphamode_paths.npz        erase per path: solid, radial, focal and bitmap sources, a stroke over its fill, inside a layer
  cairo_alphamode_structure.npz    nesting to four levels, earlier siblings in far corners, groups in a masked layer's halves, opaque
                                   covers, off-frame groups, the clear-surface bookkeeping
and cairo_alphamode_aliased_*.npz: the same under CAIRO_ANTIALIAS_NONE.

The clear-state gate: before anything is written, and under --check, every scene of alpha_modes_scenes.PRELUDES must differ, in at
least one pixel, from the same scene with its prelude taken out (the rule "the surface is still clear") wherever the prelude changes
no pixel -- so a golden of these cannot be met by the wrong bookkeeping.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import alpha_modes_scenes as scenes  # noqa: E402


def gate():
    sc = scenes.structure_scenes()
    bad = 0
    for name in scenes.PRELUDES:
        s = sc[name]
        kids = s["stage"]["children"]
        n_follow = len(scenes.FOLLOW)
        with_prelude = scenes.cairo_render(s)
        still_clear = scenes.cairo_render(dict(s, stage={"children": kids[-n_follow:]}))
        n = int((with_prelude != still_clear).any(-1).sum())
        print("%-28s differs from the still-clear rule in %d pixels" % (name, n))
        bad += n == 0
    return bad


def main():
    check = "--check" in sys.argv
    if gate():
        sys.exit("a clear-state scene does not tell the two rules apart")
    bad = 0
    for fname, images in sorted(scenes.goldens().items()):
        path = scenes.golden_path(fname)
        if check:
            old = np.load(path)
            same = sorted(old.files) == sorted(images) and all((old[k] == v).all() for k, v in images.items())
            print("%-40s %s" % (fname, "same" if same else "DIFFERS"))
            bad += not same
        else:
            np.savez_compressed(path, **images)
            print("%-40s %d scenes, %d bytes" % (fname, len(images), os.path.getsize(path)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
