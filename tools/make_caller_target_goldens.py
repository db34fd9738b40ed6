"""Generates tests/golden/cairo_caller_targets.npz: what libcairo 1.16 renders for the four re-framed golden scenes of
tests/caller_target_scenes.py (one each of the layer, mask, fade and pad families at 192 x 24), each with its family's own replay
class.  Needs the system libcairo; the output is data and is committed, so the tests on a GPU machine need no libcairo.

usage: python tools/make_caller_target_goldens.py [--check]
       (--check: regenerate in memory and compare with the committed file)

Before anything is written, and under --check, every picked scene is rendered at its own size too and must equal its family's
committed golden: the replay classes here are the ones those files came from.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import caller_target_scenes as cts  # noqa: E402


def pick(family):
    module, _, fname, name = cts.PICKS[family]
    make, aliased = module.files()[fname]
    assert not aliased
    sc = make()[name]
    own = np.load(module.golden_path(fname))[name]
    assert (module.cairo_render(sc) == own).all(), (family, "libcairo here does not reproduce the family's committed golden")
    return sc


def main():
    arrays = cts.cairo_goldens(pick)
    if "--check" in sys.argv:
        old = np.load(cts.GOLDEN)
        bad = [k for k, v in arrays.items() if not (k in old.files and old[k].shape == v.shape and (old[k] == v).all())]
        print("all goldens match" if not bad and sorted(old.files) == sorted(arrays) else "differ: %s" % bad)
        return 1 if bad or sorted(old.files) != sorted(arrays) else 0
    np.savez_compressed(cts.GOLDEN, **arrays)
    print("wrote", cts.GOLDEN, os.path.getsize(cts.GOLDEN), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
