"""tests/mask_frame_model.py's compositing loop restated with faded groups ("Layer opacity"):

    render(edges, paths, styles, W, H, even_odd_from_paths=True, aliased=False) -> H x W x 4 premultiplied RGBA

for a frame in swfr_upload_edges form whose groups may hold a SWFR_PATH_GROUP_MASK marker and whose GROUP_ENDs may carry a fade,
255 - opacity, in bits 24..31 of `lerp`: the END of a faded group multiplies the group's pixels by the opacity (fade_model.faded: every
channel, alpha included) and composites the product (layer_model.composite); a fade on any other path, on a masked group's END, or
bits 16..23 set are refused.  Masked groups are mask_frame_model's: BEGIN; content paths; MASK; mask paths; END(operator).  BEGIN sets the pixels of its rectangle aside and starts them clear; MASK sets what was drawn since -- the content --
aside in turn and starts clear again; the END of a masked group multiplies the content by the alpha of what was drawn since MASK
(mask_model.masked) and composites the product onto what BEGIN set aside (layer_model.composite).  A masked group counts two levels of
SWFR_MAX_LAYER_DEPTH from its BEGIN on.  Coverage, the lerp rule and the operators are frame_model's (its functions are used as they
are; frame_model.py itself knows nothing of masks or fades).  The model shares no code with the kernels.
tests/test_fade_frame_model.py pins it against the committed libcairo goldens and live libcairo.
"""
import numpy as np

import blend_model as bm
import fade_model as fd
import frame_model as fm
import layer_model as lm
import mask_model as mk

PATH_GROUP_BEGIN, PATH_GROUP_END, PATH_GROUP_MASK = mk.PATH_GROUP_BEGIN, mk.PATH_GROUP_END, mk.PATH_GROUP_MASK
OPERATOR_NAMES = fm.OPERATOR_NAMES


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


def render(edges, paths, styles, W, H, even_odd_from_paths=True, aliased=False):
    """premultiplied RGBA (H x W x 4 uint8) of a frame in swfr_upload_edges form, masked and faded groups included"""
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
        x0, y0, x1, y1 = rect = fm._rect(p, W, H)
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
        if int(st.kind) != fm.STYLE_SOLID:
            raise NotImplementedError("the model draws solid styles only")
        if x0 >= x1 or y0 >= y1:
            continue
        pix = int(st.pixel) & 0xffffffff
        c = np.array([(pix >> 16) & 255, (pix >> 8) & 255, pix & 255, pix >> 24], np.uint8)
        _, cov = fm.path_coverage(edges, p, W, H, even_odd_from_paths, aliased)
        d = img[y0:y1, x0:x1]
        cc = np.broadcast_to(c, d.shape)
        img[y0:y1, x0:x1] = bm.lerp_source(cc, cov, d) if lerp else bm.blend(OPERATOR_NAMES[op], cc, cov, d)
    if stack:
        raise ValueError("GROUP_BEGIN without a GROUP_END")
    return img
