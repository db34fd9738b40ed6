"""Records tests/golden/cairo_shadow_*.npz: the scenes of tests/shadow_scenes.py through libcairo 1.16 and pixman 0.40 (ShadowReplay: the
popped group's surface is replaced by the final surface the rule's call sequence makes of it, between cairo_pop_group and the paint),
premultiplied RGBA, key = scene name.  Before anything is written every scene is also rendered with its shadows replaced by plain layers:
a golden that does not differ from that in at least one byte would prove nothing, and the tool stops.  So it does when a knockout scene
(knockout_*) does not differ from its hide-object twin (hide_*).

usage: python tools/make_shadow_goldens.py [--check]      --check: compare with the recorded files instead of writing them
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blur_model  # noqa: E402
import shadow_scenes as ss  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402


def main():
    check = "--check" in sys.argv
    assert cb.version().startswith("1.16."), "the goldens are libcairo 1.16's"
    assert blur_model.pixman().pixman_version_string().decode().startswith("0.40."), "the goldens are pixman 0.40's"
    files = {}
    for fname, (make, aliased) in sorted(ss.files().items()):
        out = {}
        for name, sc in sorted(make().items()):
            assert sc["width"] <= 96 and sc["height"] <= 64, name
            img = ss.cairo_render(sc, aliased)
            plain = ss.cairo_render(dict(sc, stage={"children": ss.without_shadow(sc["stage"]["children"])}), aliased)
            differing = int((img != plain).any(-1).sum())
            assert differing > 0, "%s/%s: the shadow changes no pixel" % (fname, name)
            out[name] = img
            print("%-32s %-28s %dx%d  %5d pixels differ from the plain layer" % (fname, name, sc["width"], sc["height"], differing))
        knockouts = [name for name in out if name.startswith("knockout_")]
        assert knockouts or "structure" not in fname, fname
        for name in knockouts:
            twin = "hide_" + name[len("knockout_"):]
            assert twin in out, "%s/%s has no hide-object twin" % (fname, name)
            differing = int((out[name] != out[twin]).any(-1).sum())
            assert differing > 0, "%s/%s: the knockout is its hide-object twin" % (fname, name)
            print("%-32s %-28s %5d pixels differ from %s" % (fname, name, differing, twin))
        files[fname] = out
    bad = 0
    for fname, out in files.items():                    # (every condition held: only now is anything written)
        path = ss.golden_path(fname)
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
