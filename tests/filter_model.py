"""The filter list of a filtered layer ("Filter lists") in numpy and through libcairo 1.16 + pixman 0.40: the fold of the two
existing rules.  A list is a sequence of entries, each a dict with exactly one key:

    {"blur": {"x", "y", "passes"}}      R_i = blur_model.blur(R_(i-1), x, y, passes), on all four channels
    {"shadow": a shadow_model shadow}   R_i = shadow_model.shadow(R_(i-1), shadow): the final surface with G := R_(i-1)

apply() folds the numpy models, cairo_apply() the libraries' call sequences (blur_model.pixman_blur, shadow_model.cairo_shadow);
tests/test_filters_model.py holds the two against each other byte for byte.
"""
import numpy as np

import blur_model
import shadow_model

MAX_FILTERS = 4


def kind_of(entry):
    """("blur" | "shadow", its value) of one entry"""
    assert isinstance(entry, dict) and len(entry) == 1, entry
    (kind, value), = entry.items()
    assert kind in ("blur", "shadow"), entry
    return kind, value


def blur_of(value):
    return int(value.get("x", 0)), int(value.get("y", 0)), int(value.get("passes", 1))


def as_dicts(filters):
    """the list with every key of every entry filled in: what Renderer.built_filters() reports"""
    out = []
    for entry in filters:
        kind, value = kind_of(entry)
        if kind == "blur":
            out.append({"blur": dict(zip(("x", "y", "passes"), blur_of(value)))})
        else:
            out.append({"shadow": shadow_model.as_dict(value)})
    return out


def apply(img, filters, order="rgba"):
    """R_n of an HxWx4 uint8 premultiplied group image whose bytes are in `order` (shadow_model.shadow: "rgba" a frame as read back,
    "bgra" the bytes of ARGB words)"""
    assert 1 <= len(filters) <= MAX_FILTERS
    out = np.ascontiguousarray(img, dtype=np.uint8)
    for entry in filters:
        kind, value = kind_of(entry)
        out = blur_model.blur(out, *blur_of(value)) if kind == "blur" else shadow_model.shadow(out, value, order)
    return out


def cairo_apply(words, filters):
    """R_n of an HxW uint32 image of premultiplied ARGB words, every step by libcairo and pixman"""
    assert 1 <= len(filters) <= MAX_FILTERS
    out = np.ascontiguousarray(words, dtype=np.uint32).copy()
    for entry in filters:
        kind, value = kind_of(entry)
        out = blur_model.pixman_blur(out, *blur_of(value)) if kind == "blur" else shadow_model.cairo_shadow(out, value)
    return out


def blur(x, y, passes=1):
    return {"blur": {"x": x, "y": y, "passes": passes}}


def shadow(value, **changes):
    return {"shadow": dict(value, **changes)}
