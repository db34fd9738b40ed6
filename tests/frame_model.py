"""The compositing rule of a whole frame in numpy: what a frame in swfr_upload_edges form (include/swfr.h) leaves in every pixel.

    render(edges, paths, styles, W, H, even_odd_from_paths=True, aliased=False, bitmaps=None) -> H x W x 4 premultiplied RGBA

`edges` / `paths` are EDGE_DTYPE / PATH_DTYPE arrays and `styles` Style structs: what Renderer.build_frame returns and what
Renderer.render_edges takes, in the PUBLIC form of swfr_path -- `lerp` is lerp | operator << 8 | fade << 24, groups are
SWFR_PATH_GROUP_BEGIN / _MASK / _END marker paths.  Paths are painted in order onto a clear frame.

- Coverage of a path, 0..255 per pixel of its rectangle (nothing is painted outside it):
  antialiased tor paths -- the oracle's scan converter (OracleBackend.fill_edges) over the path's rectangle, opaque white on a clear
  scratch surface of the rectangle's size, alpha channel (the edges are moved by the rectangle's corner, whole pixels: the sample
  grid moves with them); box paths -- Cairo's exact area of the disjoint boxes in 16.16, alpha = (c >> 8) - (c >> 16); aliased --
  the spans and boxes of tests/mono_model.py, every covered pixel at 255.
- The source of a path, per pixel of its rectangle: a solid style's colour; a SWFR_STYLE_BITMAP style's bitmap fetch -- filter_of,
  to_pixman and the bilinear / convolution fetch of tests/pad_model.py under the style's `extend` (0 none, 1 repeat, 2 pad), the
  texels from `bitmaps` ({id: (h, w) uint32 premultiplied 0xAARRGGBB}; tests/host_frames.py, bitmaps_of); a SWFR_STYLE_RADIAL
  style's (focal included) gradient by tests/spread_model.py's walker that sees EVERY sample of a row of the rectangle from its left
  edge on, the device's documented rule ("Gradient spread modes"; libcairo's sees the covered samples only and may differ
  in spread_model.frame's caveat pixels).  `inv` is Cairo's pattern matrix; pixman's 16.16 transform is anchored in the path's own
  rectangle, x_min .. y_max.  Padded radial gradients (extend 0), which the device draws with another routine than the spread
  ones, are in: tests/test_shaded_frame_model.py holds the model's padded source against the oracle on 60 random scenes, zero
  differing bytes.
- A solid path whose lerp bit is set is a SOURCE lerp (blend_model.lerp_source); otherwise a path is its operator's combiner on
  mul_un8(source, coverage) (blend_model.blend; operator 0 is OVER).
- The lerp bit with a bitmap or radial style is mul_un8(source, coverage) with the destination ignored (pixman's IN, 0x80 rounding:
  not the 0x7f span lerp of a solid).  It is defined only where the destination under the path's rectangle is clear -- the frame
  builder sets the bit for such a style only while the surface, the frame's or inside a group the group's, is clear -- and is a
  ValueError otherwise.
- A group is BEGIN; paths; END(operator), or, masked, BEGIN; content paths; MASK; mask paths; END(operator).  BEGIN sets the pixels
  of its rectangle aside and starts them clear.  MASK sets what was drawn since -- the content -- aside in turn and starts clear
  again; the END of a masked group multiplies the content by the alpha of what was drawn since MASK (mask_model.masked).  An END
  whose `lerp` carries a fade, 255 - opacity, in bits 24..31 multiplies the group's pixels by the opacity (fade_model.faded: every
  channel, alpha included).  Then END composites the group onto what BEGIN set aside with layer_model.composite(operator).
  Members lie inside the group's rectangle and a transparent group pixel leaves its destination as it is under all nine operators
  (tests/layer_model.py), so working inside the rectangle is the rule on a surface of the frame's size.
- Groups nest to SWFR_MAX_LAYER_DEPTH levels; a masked group counts two from its BEGIN on.
- Refused with ValueError, as swfr_upload_edges refuses them: an unknown operator or lerp value, lerp bits beside an operator,
  bits 16..23 of `lerp`; a fade on anything but the END of an unmasked group; markers that do not pair up, carry another rectangle
  than their BEGIN, or nest too deep; a MASK with edges or a lerp field, outside a group or second in its group; a path outside its
  group's rectangle.
- NotImplementedError: a SWFR_STYLE_LINEAR style (a float ramp within 1 LSB of libcairo by design: no exact model) and a bitmap
  style that names a colour-transformed (variant) texture, bitmap >= 65536 (its texels belong to the handle that walked the stage).

The model states the rule; it shares no code with the kernels (swf_renderer_amd/csrc) and knows nothing of strips, staging rounds,
class bytes or culling.  All work is cropped to a path's rectangle: a 4K frame of thousands of small paths stays affordable.
tests/test_frame_model.py, tests/test_shaded_frame_model.py, tests/test_mask_frame_model.py and tests/test_fade_frame_model.py pin it
against the committed libcairo goldens, live libcairo and the oracle.
"""
import numpy as np

import blend_model as bm
import fade_model as fd
import layer_model as lm
import mask_model as mk
import mono_model as mm
import pad_model as pm
import spread_model as sm
from oracle import oracle_backend as ob

PATH_TOR, PATH_BOXES, PATH_GROUP_BEGIN, PATH_GROUP_END, PATH_GROUP_MASK = 0, 1, 2, 3, 4
STYLE_SOLID, STYLE_RADIAL, STYLE_LINEAR, STYLE_BITMAP = 0, 1, 2, 3
VARIANT_BASE = 65536
PAD_RADIAL = True                                     # (tests/test_shaded_frame_model.py: the padded source equals the oracle's)
OPERATOR_NAMES = {v: ("normal" if k == "over" else k) for k, v in bm.OPERATORS.items()}      # SWFR_OP_* -> blend_model's mode names


def _rect(p, W, H):
    x0, y0, x1, y1 = (int(p[k]) for k in ("x_min", "y_min", "x_max", "y_max"))
    return max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)


def tor_coverage(e, rect, even_odd):
    """(y1 - y0) x (x1 - x0) uint8: Cairo's antialiased coverage of the edges `e` over the pixel rectangle rect = (x0, y0, x1, y1)"""
    x0, y0, x1, y1 = rect
    w, h = x1 - x0, y1 - y0
    if len(e) == 0:
        return np.zeros((h, w), np.uint8)
    m = np.array(e, copy=True)
    for k in ("x1", "x2"):
        m[k] -= x0 * 256
    for k in ("y1", "y2", "top", "bottom"):
        m[k] -= y0 * 256
    be = ob.OracleBackend(w, h)
    try:
        be.fill_edges(m, (0, 0, w, h), even_odd, 0xffffffff)
        return be.premultiplied_rgba()[..., 3].copy()
    finally:
        be.close()


def box_coverage(e, rect):
    """Cairo's exact-area rule for disjoint boxes (x1, y1)-(x2, y2) in 24.8: the covered area of a pixel in 16.16, c, gives alpha
    (c >> 8) - (c >> 16)"""
    x0, y0, x1, y1 = rect
    area = np.zeros((y1 - y0, x1 - x0), np.int64)
    px = np.arange(x0, x1, dtype=np.int64) * 256
    py = np.arange(y0, y1, dtype=np.int64) * 256
    for b in e:
        wx = np.minimum(int(b["x2"]), px + 256) - np.maximum(int(b["x1"]), px)
        wy = np.minimum(int(b["y2"]), py + 256) - np.maximum(int(b["y1"]), py)
        area += np.maximum(wy, 0)[:, None] * np.maximum(wx, 0)[None, :]
    assert int(area.max(initial=0)) <= 65536, "boxes of one path overlap"
    return (((area >> 8) - (area >> 16)) & 255).astype(np.uint8)


def aliased_coverage(e, p, rect, even_odd, W, H):
    """tests/mono_model.py's spans (tor) and rounded boxes, as 0 / 255 over the rectangle"""
    x0, y0, x1, y1 = rect
    cov = np.zeros((y1 - y0, x1 - x0), bool)
    if int(p["kind"]) == PATH_TOR:
        rows, xs, xe = mm.tor_spans(e, y0, y1, x0, x1, even_odd, H, W)
        diff = np.zeros((y1 - y0, x1 - x0 + 1), np.int64)
        np.add.at(diff, (rows - y0, xs - x0), 1)
        np.add.at(diff, (rows - y0, xe - x0), -1)
        cov = np.cumsum(diff[:, :-1], 1) > 0
    else:
        for b in e:
            a0, a1 = max(mm._round(int(b["x1"])), x0), min(mm._round(int(b["x2"])), x1)
            c0, c1 = max(mm._round(int(b["y1"])), y0), min(mm._round(int(b["y2"])), y1)
            if a0 < a1 and c0 < c1:
                cov[c0 - y0:c1 - y0, a0 - x0:a1 - x0] = True
    return np.where(cov, 255, 0).astype(np.uint8)


def path_coverage(edges, p, W, H, even_odd_from_paths=True, aliased=False):
    """(rectangle, coverage over it) of one tor or box path"""
    rect = _rect(p, W, H)
    e = edges[int(p["first_edge"]):int(p["first_edge"]) + int(p["n_edges"])]
    even_odd = bool(p["fill_rule"]) and even_odd_from_paths
    kind = int(p["kind"])
    assert kind in (PATH_TOR, PATH_BOXES), "unknown path kind"
    if aliased:
        return rect, aliased_coverage(e, p, rect, even_odd, W, H)
    return rect, (tor_coverage(e, rect, even_odd) if kind == PATH_TOR else box_coverage(e, rect))


def masked_begins(paths):
    """the indices of the GROUP_BEGINs whose group holds a MASK (a MASK belongs to the innermost group open where it stands)"""
    out, opened = set(), []
    for i, p in enumerate(paths):
        kind = int(p["kind"])
        if kind == PATH_GROUP_BEGIN:
            opened.append(i)
        elif kind == PATH_GROUP_END and opened:
            opened.pop()
        elif kind == PATH_GROUP_MASK:
            if not opened or opened[-1] in out:
                raise ValueError("GROUP_MASK outside a group, or a second one in its group")
            out.add(opened[-1])
    return out


def source_pixels(st, p, rect, bitmaps):
    """(y1 - y0) x (x1 - x0) x 4 premultiplied RGBA: the source of a bitmap or radial style over rect, the path's rectangle cut to the
    frame.  pixman's transform is anchored in the path's own rectangle, x_min .. y_max as they stand in the path."""
    anchor = tuple(int(p[k]) for k in ("x_min", "y_min", "x_max", "y_max"))
    inv = tuple(float(v) for v in st.inv)
    x0, y0, x1, y1 = rect
    if int(st.kind) == STYLE_BITMAP:
        if int(st.bitmap) >= VARIANT_BASE:
            raise NotImplementedError("a colour-transformed (variant) texture: its texels belong to the handle that walked the stage")
        if bitmaps is None or int(st.bitmap) not in bitmaps:
            raise ValueError("bitmap %d is not among `bitmaps`" % int(st.bitmap))
        if int(st.extend) not in (pm.NONE, pm.REPEAT, pm.PAD):
            raise ValueError("swfr_style::extend %d of a bitmap style" % int(st.extend))
        if x0 >= x1 or y0 >= y1:
            return np.zeros((0, 0, 4), np.uint8)
        return pm.rgba_bytes(pm.source_pixels(inv, np.asarray(bitmaps[int(st.bitmap)], np.uint32), rect, int(st.extend), anchor))
    if int(st.extend) not in (sm.PAD, sm.REPEAT, sm.REFLECT):
        raise ValueError("swfr_style::extend %d of a gradient style" % int(st.extend))
    if int(st.extend) == sm.PAD and not PAD_RADIAL:
        raise NotImplementedError("a padded radial gradient")
    if x0 >= x1 or y0 >= y1 or anchor[0] >= anchor[2] or anchor[1] >= anchor[3]:
        return np.zeros((max(y1 - y0, 0), max(x1 - x0, 0), 4), np.uint8)
    circles = tuple(float(getattr(st, k)) for k in ("c0x", "c0y", "r0", "c1x", "c1y", "r1"))
    stops = [(float(st.stop_offset[i]),) + tuple(float(v) for v in st.stop_rgba[i]) for i in range(int(st.n_stops))]
    if not stops:
        return np.zeros((y1 - y0, x1 - x0, 4), np.uint8)
    src = sm.source(inv, circles, stops, int(st.extend), anchor)["stateful"]      # the every-sample walker, from the rectangle's left edge
    return sm.rgba_bytes(src[y0 - anchor[1]:y1 - anchor[1], x0 - anchor[0]:x1 - anchor[0]])


def render(edges, paths, styles, W, H, even_odd_from_paths=True, aliased=False, bitmaps=None):
    """premultiplied RGBA (H x W x 4 uint8) of a frame in swfr_upload_edges form, masked and faded groups included.  bitmaps: the
    texels of the bitmap styles, {id: (h, w) uint32 premultiplied 0xAARRGGBB} (tests/host_frames.py, bitmaps_of)"""
    edges, paths = np.asarray(edges), np.asarray(paths)
    two = masked_begins(paths)
    img = np.zeros((H, W, 4), np.uint8)
    stack = []                                                   # open groups: [rectangle, the parent's pixels, the content's or None, levels]
    levels = 0
    for i, p in enumerate(paths):
        kind, field = int(p["kind"]), int(p["lerp"]) & 0xffffffff
        lerp, op, fade = field & 0xff, (field >> 8) & 0xffff, field >> 24
        if fade and kind != PATH_GROUP_END:
            raise ValueError("swfr_path::lerp %#x: a fade on a path that is no GROUP_END" % field)
        if op not in OPERATOR_NAMES or lerp > 1:
            raise ValueError("swfr_path::lerp %#x: no such operator or lerp value" % field)
        x0, y0, x1, y1 = rect = _rect(p, W, H)
        if kind == PATH_GROUP_BEGIN:
            need = 2 if i in two else 1
            if field or levels + need > lm.MAX_DEPTH:
                raise ValueError("GROUP_BEGIN with a lerp field, or deeper than SWFR_MAX_LAYER_DEPTH")
            levels += need
            stack.append([rect, img[y0:y1, x0:x1].copy(), None, need])
            img[y0:y1, x0:x1] = 0
            continue
        if kind == PATH_GROUP_MASK:
            if not stack or stack[-1][0] != rect or field or int(p["n_edges"]) or stack[-1][2] is not None:
                raise ValueError("GROUP_MASK outside a group, with another rectangle than its group's, with edges or a lerp field, or a second one")
            stack[-1][2] = img[y0:y1, x0:x1].copy()
            img[y0:y1, x0:x1] = 0
            continue
        if kind == PATH_GROUP_END:
            if not stack or stack[-1][0] != rect or lerp:
                raise ValueError("GROUP_END without its GROUP_BEGIN, or with lerp bits")
            _, below, content, need = stack.pop()
            levels -= need
            if fade and content is not None:
                raise ValueError("GROUP_END: a fade on a group with a GROUP_MASK")
            g = img[y0:y1, x0:x1] if content is None else mk.masked(content, img[y0:y1, x0:x1])
            if fade:
                g = fd.faded(g, 255 - fade)
            img[y0:y1, x0:x1] = lm.composite(OPERATOR_NAMES[op], g, below)
            continue
        if stack:
            g = stack[-1][0]
            if x0 < g[0] or y0 < g[1] or x1 > g[2] or y1 > g[3]:
                raise ValueError("a path lies outside the rectangle of its group")
        if lerp and op:
            raise ValueError("an operator needs lerp bits 0")
        st = styles[int(p["style"])]
        shaded = int(st.kind) != STYLE_SOLID
        if shaded and int(st.kind) not in (STYLE_RADIAL, STYLE_BITMAP):
            raise NotImplementedError("a linear gradient: a float ramp within 1 LSB by design, no exact model")
        if x0 >= x1 or y0 >= y1:
            if shaded:
                source_pixels(st, p, rect, bitmaps)                  # (what the model cannot draw it refuses wherever it stands)
            continue
        _, cov = path_coverage(edges, p, W, H, even_odd_from_paths, aliased)
        d = img[y0:y1, x0:x1]
        if shaded:
            cc = source_pixels(st, p, rect, bitmaps)
            if lerp:
                if d.any():
                    raise ValueError("the lerp bit with a bitmap or gradient style on a surface that is not clear under the path's rectangle")
                img[y0:y1, x0:x1] = sm.mul_un8(cc, cov)
                continue
        else:
            pix = int(st.pixel) & 0xffffffff
            cc = np.broadcast_to(np.array([(pix >> 16) & 255, (pix >> 8) & 255, pix & 255, pix >> 24], np.uint8), d.shape)
        img[y0:y1, x0:x1] = bm.lerp_source(cc, cov, d) if lerp else bm.blend(OPERATOR_NAMES[op], cc, cov, d)
    if stack:
        raise ValueError("GROUP_BEGIN without a GROUP_END")
    return img
