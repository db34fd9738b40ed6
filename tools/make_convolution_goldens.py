"""Records tests/golden/cairo_convolution_*.npz: the scenes of tests/convolution_scenes.py through libcairo 1.16 and pixman 0.40
(ConvolutionReplay: the popped group's surface is replaced by what the list's call sequences make of it, entry after entry -- a
convolution entry is one pixman_image_composite32(SRC) from an image carrying PIXMAN_FILTER_CONVOLUTION -- between cairo_pop_group and the
paint), premultiplied RGBA, key = scene name.  Before anything is written, every scene is also rendered
  - with its filter lists replaced by plain layers: a golden that does not differ from that would prove nothing;
  - without the last entry of its lists, where a list has more than one: a golden that does not differ from that would not show the
    whole chain ran;
and the filtered surface of every scene named after a sharpen, emboss or edge kernel is made of the scene's group alone (libcairo for the
group, pixman for the list): it must hold pixels whose colour exceeds their alpha -- the invalid premultiplied pixels the tile pass and
the later entries have to treat as libcairo treats them.  The tool stops where one of these fails.

usage: python tools/make_convolution_goldens.py [--check]      --check: compare with the recorded files instead of writing them
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blur_model  # noqa: E402
import convolution_model as cm  # noqa: E402
import convolution_scenes as csc  # noqa: E402
from oracle import cairo_backend as cb  # noqa: E402


def _changed(sc, change, aliased):
    return csc.cairo_render(dict(sc, stage={"children": change(sc["stage"]["children"])}), aliased)


def _above_alpha(sc, aliased):
    """pixels of the scene's filtered surface with a colour channel above alpha: the group alone through libcairo, the list through pixman"""
    kids, filters = sc["group"]
    rgba = csc.cairo_render(dict(sc, stage={"children": kids}), aliased)
    words = blur_model.bytes_to_words(np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]))
    out = blur_model.words_to_bytes(cm.cairo_apply(words, filters)).astype(np.int64)
    return int((out[..., :3] > out[..., 3:]).any(-1).sum())


def main():
    check = "--check" in sys.argv
    assert cb.version().startswith("1.16."), "the goldens are libcairo 1.16's"
    assert blur_model.pixman().pixman_version_string().decode().startswith("0.40."), "the goldens are pixman 0.40's"
    files = {}
    for fname, (make, aliased) in sorted(csc.files().items()):
        out = {}
        for name, sc in sorted(make().items()):
            assert sc["width"] <= 96 and sc["height"] <= 64, name
            img = csc.cairo_render(sc, aliased)
            plain = int((img != _changed(sc, csc.without_filters, aliased)).any(-1).sum())
            assert plain > 0, "%s/%s: the filters change no pixel" % (fname, name)
            shorter = -1
            if len(sc["group"][1]) > 1:
                shorter = int((img != _changed(sc, csc.without_last, aliased)).any(-1).sum())
                assert shorter > 0, "%s/%s: the last entry changes no pixel" % (fname, name)
            above = _above_alpha(sc, aliased)
            if any(k in name for k in csc.ABOVE_ALPHA):
                assert above > 0, "%s/%s: no pixel of the filtered surface has a colour above its alpha" % (fname, name)
            out[name] = img
            print("%-30s %-34s %dx%d  %5d pixels differ from the plain layer, %5d from the list without its last entry, %5d with colour above alpha"
                  % (fname, name, sc["width"], sc["height"], plain, shorter, above))
        files[fname] = out
    bad = 0
    for fname, out in files.items():                    # (every condition held: only now is anything written)
        path = csc.golden_path(fname)
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
