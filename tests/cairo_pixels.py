"""What the per-pixel model tests (tests/test_{blend,layer,mask,fade}_model.py) share when they hold a rule against live libcairo:
the pixels of a CairoBackend's surface as an array, and random premultiplied pixels of one kind."""
import numpy as np


def surface_bytes(be):
    be.lib.cairo_surface_flush(be.surf)
    stride = be.lib.cairo_image_surface_get_stride(be.surf)
    ptr = be.lib.cairo_image_surface_get_data(be.surf)
    return np.ctypeslib.as_array(ptr, shape=(be.h, stride))[:, : be.w * 4].reshape(be.h, be.w, 4)


def random_premultiplied(rng, n, kind):
    if kind == "clear":
        return np.zeros((n, 4), np.uint8)
    a = np.full(n, 255) if kind == "opaque" else rng.integers(0, 256, n)
    a[: n // 16] = rng.choice([0, 1, 254, 255], n // 16) if kind != "opaque" else 255
    rgb = (rng.integers(0, 256, (n, 3)) * a[:, None] + 127) // 255
    return np.concatenate([rgb, a[:, None]], 1).astype(np.uint8)
