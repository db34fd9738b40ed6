"""Generates the libcairo goldens of the gradient spread modes: what libcairo 1.16 renders for tests/spread_scenes.py, with
cairo_pattern_set_extend(REFLECT | REPEAT) on every gradient whose fill says so.  Needs the system libcairo; the outputs are data and
are committed, so the tests on a GPU machine need no libcairo.

usage: python tools/make_spread_goldens.py [--check]
       (--check: regenerate in memory and compare with the committed files)

  cairo_spread_<spread>_radial.npz, _focal_pos.npz, _focal_neg.npz   every stop list (stops at 0 / 255, inner stops only, coincident stops,
                                      a single stop, translucent stops) under the kind, and the kind over a translucent ground
  cairo_spread_<spread>_exact.npz     pixel-aligned boxes whose samples fall exactly on stops and on period seams
  cairo_spread_<spread>_structure.npz rotated and skewed matrices, an object matrix, a colour transform, "blend_mode", "layer", "mask",
                                      "opacity", a padded gradient beside a spread one, the padded linear extension, a 300 x 40 frame
  cairo_spread_<spread>_runstart.npz  the exact boxes cut back to stepped polygons whose covered runs begin on a pixel where the walker's
                                      state decides the colour (tests/spread_scenes.py, runstart_cases)
  cairo_spread_aliased_*.npz          the same under CAIRO_ANTIALIAS_NONE
  No file may be larger than the largest blend golden.

The gates, before anything is written and under --check; a scene that fails one is reported and fails the run:
  wrong rule      every scene (bar the padded linear one and the single-stop ones, which are one colour under any rule) must differ
                  from its padded rendering, and its reflect rendering from its repeat rendering, in at least one pixel
  exact samples   tests/spread_model.py must paint every box of the exact file as libcairo does, byte for byte, and report at least one
                  sample exactly on an interval end per gradient kind and spread
  run starts      tests/spread_model.py's frame() must compose every run-start scene as libcairo paints it, in both antialias modes, from
                  a coverage made without libcairo; its caveat pixels -- where a walker that sees every sample of the rectangle paints
                  otherwise -- are printed: some under REFLECT in either mode, none under REPEAT
  pixman's range  the padded rendering of every scene of the kind and exact files must equal the oracle's (a gradient whose shape leaves
                  pixman's 16.16 range is not what libcairo says it is: tests/spread_scenes.py)
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import spread_model as sm  # noqa: E402
import spread_scenes as ss  # noqa: E402

EXTEND = {"reflect": sm.REFLECT, "repeat": sm.REPEAT}


def gates():
    bad = 0
    rendered = {}
    for spread in ss.SPREADS:
        for name, sc in sorted(ss.all_scenes(spread).items()):
            rendered[spread, name] = ss.cairo_render(sc)
    for spread in ss.SPREADS:
        other = [s for s in ss.SPREADS if s != spread][0]
        for name, sc in sorted(ss.all_scenes(spread).items()):
            if name == "linear_pad" or name.endswith("_single"):
                continue
            padded = ss.cairo_render(ss.with_spread(sc, "pad"))
            n_pad = int((rendered[spread, name] != padded).any(-1).sum())
            n_other = int((rendered[spread, name] != rendered[other, name]).any(-1).sum())
            ok = n_pad > 0 and n_other > 0
            print("discriminates" if ok else "DOES NOT DISCRIMINATE", spread, name, "pixels differing from pad", n_pad, "from", other, n_other)
            bad += not ok
    # pixman's range: padded, the plain scenes are what the oracle draws
    from helpers import oracle_render
    for group in ("radial", "focal_pos", "focal_neg", "exact"):
        for name, sc in sorted(ss.GROUPS[group]("pad").items()):
            n = int((ss.cairo_render(sc) != oracle_render(sc)).any(-1).sum())
            print("in range" if n == 0 else "OUT OF PIXMAN'S RANGE", name, "padded pixels differing from the oracle", n)
            bad += n != 0
    # exact samples
    for spread in ss.SPREADS:
        hits = {}
        for name, (sc, md) in sorted(ss.exact_cases(spread).items()):
            x0, y0, x1, y1 = md["rect"]
            out = sm.source(sm.pattern_matrix(md["matrices"]), md["circles"], md["stops"], EXTEND[spread], md["rect"])
            n = int((sm.rgba_bytes(out["stateful"]) != rendered[spread, name][y0:y1, x0:x1]).any(-1).sum())
            kind = name.rsplit("_r", 1)[0]
            hits[kind] = hits.get(kind, 0) + out["exact_hits"]
            print("model" if n == 0 else "MODEL DIFFERS", spread, name, "differing pixels", n, "samples on an interval end", out["exact_hits"],
                  "of them on the left end of the walker's interval", out["on_left_end"], "pixels a fresh reset paints otherwise", out["state_pixels"])
            bad += n != 0
        for kind, n in sorted(hits.items()):
            if n == 0:
                print("NO SAMPLE ON AN INTERVAL END", spread, kind)
                bad += 1
    # run starts
    import spread_fuzz as sf
    for spread in ss.SPREADS:
        for aliased in (False, True):
            total = 0
            for name, case in sorted(ss.runstart_cases(spread, aliased).items()):
                e = sf.expected(case)
                n = int((e["truth"] != ss.cairo_render(case["scene"], aliased)).any(-1).sum())
                where = [(int(y), int(x)) for y, x in np.argwhere(e["caveat"])]
                print("model" if n == 0 else "MODEL DIFFERS", spread, "aliased" if aliased else "antialiased", name, "differing pixels", n, "caveat pixels", where)
                bad += n != 0
                total += len(where)
            if (total == 0) != (spread == "repeat"):
                print("CAVEAT PIXELS", spread, aliased, total)
                bad += 1
    return bad


def main():
    check = "--check" in sys.argv
    bad = gates()
    if bad:
        print("%d scenes fail a gate" % bad)
        return 1
    limit = max(os.path.getsize(f) for f in glob.glob(os.path.join(ss.bs.GOLD, "cairo_blend_*.npz")))
    mismatch = 0
    for fname, scenes in sorted(ss.goldens().items()):
        path = ss.golden_path(fname)
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
