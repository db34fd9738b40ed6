"""Colour transforms (swf-tree ColorTransformWithAlpha on containers, shapes and morph shapes): the lowering that defines them,
and tests/golden/cairo_cxform_<transform>.npz, what libcairo 1.16 renders for every tests/scenarios.py scenario under each of the
transforms below (key = scenario name, premultiplied RGBA).

The rule ("Colour transforms"): a channel maps as c' = clamp(((c * mult) >> 8) + add, 0, 255), nested transforms apply
innermost first and each one clamps, and what is transformed is the straight colour a definition holds -- solid and line colours,
gradient stops, both colours of a morph shape, every straight texel of a bitmap.  So a transformed stage renders exactly as its
LOWERED stage: the transforms removed, recoloured deep copies of the definitions in their place, and every bitmap a fill samples under
a transform recoloured and registered under a fresh id.  The oracle (oracle/canvas_replay.py with libcairo or the C restatement) renders
the lowered stage unchanged; tests/test_color_transform.py imports this module for the lowering and the transforms.

usage: python tools/make_cxform_goldens.py [--check]    (--check: regenerate in memory and compare with the committed files)
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import canvas_replay as cr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRESH_BITMAP_ID = 60000               # lowered bitmaps are registered from here up (ids stay below 65536)
CHANNELS = ("red", "green", "blue", "alpha")


def cxform(mult=(256, 256, 256, 256), add=(0, 0, 0, 0)):
    """a ColorTransformWithAlpha dict in swf-tree's snake_case; mult in Sfixed8P8 epsilons"""
    d = {}
    for c, m, a in zip(CHANNELS, mult, add):
        d[c + "_mult"] = {"epsilons": int(m)}
        d[c + "_add"] = int(a)
    return d


# the transforms every scenario is checked under (nested: applied as an outer container and an inner one on every top-level object)
TRANSFORMS = {
    "fade": [cxform(mult=(256, 256, 256, 96))],
    "tint": [cxform(mult=(128, 200, 90, 256), add=(90, -20, 40, 0))],
    "invert": [cxform(mult=(-256, -256, -256, 256), add=(255, 255, 255, 0))],
    "saturate": [cxform(add=(160, 120, -40, 60))],
    "nested": [cxform(mult=(128, 128, 128, 128)), cxform(mult=(512, 512, 512, 384), add=(10, 0, -5, 0))],
    "identity": [cxform()],
}


def values(ct):
    """the eight integers of a transform dict (mult as {"epsilons": n}, or a number read as its value)"""
    def mult(v):
        return int(v["epsilons"]) if isinstance(v, dict) else int(round(float(v) * 256))
    return (tuple(mult(ct[c + "_mult"]) if c + "_mult" in ct else 256 for c in CHANNELS) +
            tuple(int(ct.get(c + "_add", 0)) for c in CHANNELS))


def table(ct):
    """4 x 256 uint8: the transform's value of every channel value, clamped"""
    v = values(ct)
    c = np.arange(256, dtype=np.int64)
    return np.stack([np.clip(((c * v[k]) >> 8) + v[4 + k], 0, 255) for k in range(4)]).astype(np.uint8)


def compose(outer, inner_ct):
    """the chain `outer` (a table or None) after the transform `inner_ct`: innermost first, each clamps; None when identity"""
    t = table(inner_ct)
    if outer is not None:
        t = np.stack([outer[k][t[k]] for k in range(4)])
    return None if (t == np.arange(256, dtype=np.uint8)[None, :]).all() else t


def _rgba(lut, c):
    return {"r": int(lut[0][c["r"]]), "g": int(lut[1][c["g"]]), "b": int(lut[2][c["b"]]), "a": int(lut[3][c["a"]])}


class Lowering:
    """Removes the colour transforms of stages that share one set of bitmaps: lower(stage) -> the lowered stage; `extra` collects
    the recoloured bitmaps (id -> (width, height, straight RGBA bytes)) the lowered stages use."""

    def __init__(self, bitmaps=()):
        self.straight = {}                 # original bitmap id -> (w, h, straight RGBA ndarray)
        for tag in bitmaps:
            data = tag["data"]
            if isinstance(data, str):
                data = bytes.fromhex(data)
            w, h, px = cr.decode_x_swf_bmp(bytes(data))
            self.straight[tag["id"]] = (w, h, np.frombuffer(px, np.uint8).reshape(h, w, 4))
        self.extra = {}
        self._fresh = {}                   # (bitmap id, table bytes) -> fresh id
        self._defs = {}                    # (id(definition), table bytes) -> recoloured copy

    def bitmap(self, bid, lut):
        key = (bid, lut.tobytes())
        if key not in self._fresh:
            w, h, px = self.straight[bid]
            out = np.stack([lut[k][px[..., k]] for k in range(4)], -1).astype(np.uint8)
            nid = FRESH_BITMAP_ID + len(self._fresh)
            assert nid < 65536
            self._fresh[key] = nid
            self.extra[nid] = (w, h, out.tobytes())
        return self._fresh[key]

    def _fill(self, f, lut):
        if "color" in f:
            f["color"] = _rgba(lut, f["color"])
        if "morph_color" in f:
            f["morph_color"] = _rgba(lut, f["morph_color"])
        for s in (f.get("gradient") or {}).get("colors", []):
            s["color"] = _rgba(lut, s["color"])
            if "morph_color" in s:
                s["morph_color"] = _rgba(lut, s["morph_color"])
        if f.get("type") == "bitmap" and f.get("bitmap_id") in self.straight:
            f["bitmap_id"] = self.bitmap(f["bitmap_id"], lut)

    def definition(self, tag, lut):
        key = (id(tag), lut.tobytes())
        if key not in self._defs:
            d = copy.deepcopy(tag)
            styles = [d["shape"]["initial_styles"]] + [r["new_styles"] for r in d["shape"]["records"] if r.get("new_styles")]
            for st in styles:
                for f in st["fill"]:
                    self._fill(f, lut)
                for ln in st["line"]:
                    self._fill(ln["fill"], lut)
            self._defs[key] = (d, tag)      # (the original is kept alive: its id() must not be reused)
        return self._defs[key][0]

    def _object(self, obj, lut):
        ct = obj.get("color_transform")
        if ct is not None:
            lut = compose(lut, ct)
        out = {k: v for k, v in obj.items() if k != "color_transform"}
        if obj["type"] == "container":
            out["children"] = [self._object(c, lut) for c in obj["children"]]
        elif lut is not None:
            out["definition"] = self.definition(obj["definition"], lut)
        return out

    def lower(self, stage):
        out = {k: v for k, v in stage.items() if k != "children"}
        out["children"] = [self._object(c, None) for c in stage["children"]]
        return out


def apply_transform(stage, name):
    """the stage with TRANSFORMS[name]: one transform on every top-level object, or the nested pair as an outer container and an
    inner transform on every top-level object"""
    chain = TRANSFORMS[name]
    kids = [dict(c, color_transform=chain[-1]) for c in stage["children"]]
    if len(chain) > 1:
        kids = [{"type": "container", "color_transform": chain[0], "children": kids}]
    return dict(stage, children=kids)


def apply_transform_value(stage, ct):
    """the stage's objects inside one container with the transform `ct`"""
    return dict(stage, children=[{"type": "container", "color_transform": ct, "children": stage["children"]}])


def render_lowered(backend, sc, stage):
    """premultiplied RGBA of a (transformed) stage of scenario `sc` through CanvasReplay on `backend` (CairoBackend / OracleBackend
    instance of the scenario's size), by way of its lowered stage"""
    low = Lowering(sc.get("bitmaps", []))
    lowered = low.lower(stage)
    if sc.get("even_odd"):
        backend.set_fill_rule(True)
    rp = cr.CanvasReplay(backend, linear_extension=True)
    for b in sc.get("bitmaps", []):
        rp.add_bitmap(b)
    for bid, (w, h, px) in low.extra.items():
        rp.bitmaps[bid] = backend.create_bitmap(w, h, px)
    rp.render(lowered)
    return backend.premultiplied_rgba()


def cairo_cxform(sc, stage):
    from oracle import cairo_backend as cb
    be = cb.CairoBackend(sc["width"], sc["height"])
    try:
        return render_lowered(be, sc, stage)
    finally:
        be.close()


def oracle_cxform(sc, stage):
    from oracle import oracle_backend as ob
    be = ob.OracleBackend(sc["width"], sc["height"])
    try:
        return render_lowered(be, sc, stage)
    finally:
        be.close()


def goldens():
    import scenarios
    SC = scenarios.scenarios()
    out = {}
    for t in TRANSFORMS:
        if t == "identity":
            continue                        # (identity: the scenarios' own goldens, tests/golden/cairo_<scenario>.npz)
        out["cairo_cxform_" + t] = {name: cairo_cxform(sc, apply_transform(sc["stage"], t)) for name, sc in sorted(SC.items())}
    return out


def main():
    check = "--check" in sys.argv
    bad = 0
    for fname, arrays in goldens().items():
        path = os.path.join(OUT, fname + ".npz")
        if check:
            old = np.load(path)
            for k, v in arrays.items():
                if not (k in old.files and (old[k] == v).all()):
                    print("differs:", fname, k)
                    bad += 1
        else:
            np.savez_compressed(path, **arrays)
            print("wrote", path, os.path.getsize(path), "bytes")
    if check:
        print("all goldens match" if not bad else "%d differ" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
