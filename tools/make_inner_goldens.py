"""Records tests/golden/cairo_inner_*.npz: the scenes of tests/inner_scenes.py through libcairo 1.16 and pixman 0.40 (InnerReplay: the
popped group's surface is replaced by what the inner shadow's call sequence, or the list's sequences entry after entry, make of it,
between cairo_pop_group and the paint), premultiplied RGBA, key = scene name.  Before anything is written, every scene is also rendered
  - with its inner-shadowed objects as plain layers: a golden that does not differ from that would prove nothing;
  - with the "inner" flag cleared: a golden that does not differ from the outer shadow of the same values would not show the inner rule;
and every knockout_X is held against its plain_X, which must differ.  The tool stops where one of these fails.

usage: python tools/make_inner_goldens.py [--check]      --check: compare with the recorded files instead of writing them
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blur_model  # noqa: E402
import inner_scenes as isc  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402


def _changed(sc, change, aliased):
    return isc.cairo_render(dict(sc, stage={"children": change(sc["stage"]["children"])}), aliased)


def main():
    check = "--check" in sys.argv
    assert cb.version().startswith("1.16."), "the goldens are libcairo 1.16's"
    assert blur_model.pixman().pixman_version_string().decode().startswith("0.40."), "the goldens are pixman 0.40's"
    files = {}
    for fname, (make, aliased) in sorted(isc.files().items()):
        out = {}
        for name, sc in sorted(make().items()):
            assert sc["width"] <= 96 and sc["height"] <= 64, name
            img = isc.cairo_render(sc, aliased)
            plain = int((img != _changed(sc, isc.without_filters, aliased)).any(-1).sum())
            assert plain > 0, "%s/%s: the inner shadow changes no pixel" % (fname, name)
            outer = int((img != _changed(sc, isc.flag_cleared, aliased)).any(-1).sum())
            assert outer > 0, "%s/%s: the flag changes no pixel" % (fname, name)
            out[name] = img
            print("%-32s %-30s %dx%d  %5d pixels differ from the plain layer, %5d from the flag cleared" % (fname, name, sc["width"], sc["height"], plain, outer))
        knockouts = [name for name in out if name.startswith("knockout_")]
        assert knockouts or "structure" not in fname, fname
        for name in knockouts:
            twin = "plain_" + name[len("knockout_"):]
            assert twin in out, "%s/%s has no twin without the knockout" % (fname, name)
            differing = int((out[name] != out[twin]).any(-1).sum())
            assert differing > 0, "%s/%s: the knockout is the same picture" % (fname, name)
            print("%-32s %-30s %5d pixels differ from %s" % (fname, name, differing, twin))
        files[fname] = out
    bad = 0
    for fname, out in files.items():                    # (every condition held: only now is anything written)
        path = isc.golden_path(fname)
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
