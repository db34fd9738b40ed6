"""Records tests/golden/cairo_blur_*.npz: the scenes of tests/blur_scenes.py through libcairo 1.16 and pixman 0.40 (BlurReplay: the
popped group's surface is convolved by pixman between cairo_pop_group and the paint), premultiplied RGBA, key = scene name.  Before
anything is written every scene is also rendered with its blurs replaced by plain layers: a golden that does not differ from that in
at least one byte would prove nothing, and the tool stops.

usage: python tools/make_blur_goldens.py [--check]      --check: compare with the recorded files instead of writing them
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blur_model  # noqa: E402
import blur_scenes as bl  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402


def main():
    check = "--check" in sys.argv
    assert cb.version().startswith("1.16."), "the goldens are libcairo 1.16's"
    assert blur_model.pixman().pixman_version_string().decode().startswith("0.40."), "the goldens are pixman 0.40's"
    bad = 0
    for fname, (make, aliased) in sorted(bl.files().items()):
        scenes = make()
        out = {}
        for name, sc in sorted(scenes.items()):
            assert sc["width"] <= 96 and sc["height"] <= 64, name
            img = bl.cairo_render(sc, aliased)
            plain = bl.cairo_render(dict(sc, stage={"children": bl.without_blur(sc["stage"]["children"])}), aliased)
            differing = int((img != plain).any(-1).sum())
            assert differing > 0, "%s/%s: the blur changes no pixel" % (fname, name)
            out[name] = img
            print("%-28s %-26s %dx%d  %5d pixels differ from the unblurred layer" % (fname, name, sc["width"], sc["height"], differing))
        path = bl.golden_path(fname)
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
