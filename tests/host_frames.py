"""Host-only handles for the tests of the frame builder (no GPU): a handle, swfr_build_frame's arrays for a scene, raw swfr_stage
structs handed to swfr_build_frame directly, and what the blend, layer, mask and fade host tests read from the built paths."""
import ctypes as C

import blend_scenes as bs


def host(w=64, h=48, **kw):
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    return S.Renderer(w, h, device=api.DEVICE_HOST_ONLY, **kw)


def build_on_host(sc, aliased=False):
    """swfr_build_frame's arrays (edges, paths, styles) for the scene, from a host-only handle that holds the scene's bitmaps"""
    r = host(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")), antialias="none" if aliased else "default")
    try:
        for b in sc.get("bitmaps", []):
            r.add_bitmap(b)
        for bid, (w, h, px) in sc.get("raw_bitmaps", {}).items():
            r.register_bitmap(bid, w, h, px)
        return r.build_frame(sc["stage"])
    finally:
        r.close()


def bitmaps_of(sc):
    """{id: (h, w) uint32 premultiplied 0xAARRGGBB}: the texels of the scene's bitmaps as tests/frame_model.py takes them -- the
    DefineBitmap tags of sc["bitmaps"] through the oracle's decoder, sc["raw_bitmaps"] ({id: (w, h, straight RGBA bytes)}) as they are"""
    import numpy as np

    import pad_model as pm
    from oracle import canvas_replay as cr
    out = {}
    for tag in sc.get("bitmaps", []):
        data = tag["data"]
        w, h, rgba = cr.decode_x_swf_bmp(bytes.fromhex(data) if isinstance(data, str) else bytes(data))
        out[tag["id"]] = pm.premultiply(np.frombuffer(rgba, np.uint8).reshape(h, w, 4))
    for bid, (w, h, rgba) in sc.get("raw_bitmaps", {}).items():
        out[bid] = pm.premultiply(np.frombuffer(rgba, np.uint8).reshape(h, w, 4))
    return out


def raw_stage(obj_type, obj_id, child_shape_id):
    from swf_renderer_amd import api
    kid = api.DisplayObject()
    kid.type, kid.id = api.OBJECT_SHAPE, child_shape_id
    kids = (api.DisplayObject * 1)(kid)
    d = api.DisplayObject()
    d.type, d.id = obj_type, obj_id
    d.n_children, d.children = 1, C.cast(kids, C.POINTER(api.DisplayObject))
    objs = (api.DisplayObject * 1)(d)
    s = api.Stage()
    s.width = s.height = 16
    s.n_children, s.children = 1, C.cast(objs, C.POINTER(api.DisplayObject))
    return s, (kids, objs)


def build_raw(r, s):
    n = C.c_size_t()
    args = (C.byref(C.c_void_p()), C.byref(C.c_size_t()), C.byref(C.c_void_p()), C.byref(n), C.byref(C.c_void_p()), C.byref(C.c_size_t()))
    rc = r.L.swfr_build_frame(r.h, C.byref(s), *args)
    return rc, r.L.swfr_last_error(r.h).decode(), n.value


def tri(colour, dx=0.0, **kw):
    return bs._shape([(2 + dx, 2), (40 + dx, 5), (20 + dx, 44)], colour, **kw)


def masked(mode, kids, mask, **kw):
    obj = {"type": "container", "children": list(kids), "mask": list(mask), **kw}
    if mode is not None:
        obj["layer"] = mode
    return obj


def lerps(p):
    return [int(v) for v in p["lerp"]]


def kinds(p):
    return [int(v) for v in p["kind"]]


def rects(p):
    return [tuple(int(p[k][i]) for k in ("x_min", "y_min", "x_max", "y_max")) for i in range(len(p))]
