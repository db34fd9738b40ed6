"""Records tests/golden/cairo_filters_*.npz: the scenes of tests/filter_scenes.py through libcairo 1.16 and pixman 0.40 (FilterReplay: the
popped group's surface is replaced by what the list's call sequences make of it, entry after entry, between cairo_pop_group and the
paint), premultiplied RGBA, key = scene name.  Before anything is written, every scene is also rendered
  - with its filter lists replaced by plain layers: a golden that does not differ from that would prove nothing;
  - without the last entry of its lists: a golden other than noop_* that does not differ from that would not show the whole chain ran;
  - noop_* scenes without their 1 x 1 blur entries: those must be the same picture;
and every order_a_b is held against its order_b_a, which must differ.  The tool stops where one of these fails.

usage: python tools/make_filter_goldens.py [--check]      --check: compare with the recorded files instead of writing them
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blur_model  # noqa: E402
import filter_scenes as fsc  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402


def _changed(sc, change, aliased):
    return fsc.cairo_render(dict(sc, stage={"children": change(sc["stage"]["children"])}), aliased)


def main():
    check = "--check" in sys.argv
    assert cb.version().startswith("1.16."), "the goldens are libcairo 1.16's"
    assert blur_model.pixman().pixman_version_string().decode().startswith("0.40."), "the goldens are pixman 0.40's"
    files = {}
    for fname, (make, aliased) in sorted(fsc.files().items()):
        out = {}
        for name, sc in sorted(make().items()):
            assert sc["width"] <= 96 and sc["height"] <= 64, name
            img = fsc.cairo_render(sc, aliased)
            plain = int((img != _changed(sc, fsc.without_filters, aliased)).any(-1).sum())
            assert plain > 0, "%s/%s: the filters change no pixel" % (fname, name)
            shorter = int((img != _changed(sc, fsc.without_last, aliased)).any(-1).sum())
            if name.startswith("noop_"):
                same = int((img != _changed(sc, fsc.without_noops, aliased)).any(-1).sum())
                assert same == 0, "%s/%s: the 1 x 1 blur entry changes %d pixels" % (fname, name, same)
            else:
                assert shorter > 0, "%s/%s: the last entry changes no pixel" % (fname, name)
            out[name] = img
            print("%-34s %-30s %dx%d  %5d pixels differ from the plain layer, %5d from the list without its last entry"
                  % (fname, name, sc["width"], sc["height"], plain, shorter))
        orders = [name for name in out if name.startswith("order_")]
        assert orders or "structure" not in fname, fname
        for name in orders:
            _, a, b = name.split("_")
            twin = "order_%s_%s" % (b, a)
            assert twin in out, "%s/%s has no twin of the other order" % (fname, name)
            differing = int((out[name] != out[twin]).any(-1).sum())
            assert differing > 0, "%s/%s: the other order is the same picture" % (fname, name)
            print("%-34s %-30s %5d pixels differ from %s" % (fname, name, differing, twin))
        if "structure" in fname:
            assert any(name.startswith("noop_") for name in out), fname
        files[fname] = out
    bad = 0
    for fname, out in files.items():                    # (every condition held: only now is anything written)
        path = fsc.golden_path(fname)
        if check:
            old = np.load(path)
            same = sorted(old.files) == sorted(out) and all((old[k] == out[k]).all() for k in out)
            print("%s: %s" % (fname, "unchanged" if same else "DIFFERS"))
            bad += 0 if same else 1
        else:
            np.savez_compressed(path, **out)
            print("wrote %s (%d scenes, %d bytes)" % (path, len(out), os.path.getsize(path)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
