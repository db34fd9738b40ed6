"""An exact model of the aliased mode (Renderer(antialias="none"), SWFR_FLAG_ANTIALIAS_NONE): Cairo 1.16's CAIRO_ANTIALIAS_NONE rule as
csrc/mono.hip states it, restated in exact integer arithmetic over a frame in swfr_upload_edges form.

    render(edges, paths, styles, W, H) -> H x W x 4 premultiplied RGBA

`edges` / `paths` are EDGE_DTYPE / PATH_DTYPE arrays and `styles` Style structs: what Renderer.build_frame returns and what
Renderer.render_edges takes.  Paths are painted in order onto a clear frame.

- Tor paths.  With I(v) = (v + 127) >> 8 an edge is active in pixel row y when I(top) <= y < I(bottom), inside the path's rows; its
  crossing there is the pixel I(x1 + floor((256 y + 127 - y1) (x2 - x1) / (y2 - y1))).  Crossings at one pixel form a group; a group
  opens a span when the winding before it is zero (by the fill rule) and it is the row's first or lies more than one pixel right of the
  group before it, and closes the span when the winding after it is zero and it is the row's last or the next group lies more than one
  pixel further -- so a one-pixel gap between two spans is filled.  Spans are clipped to the path's columns and the frame.
- Box paths.  A box covers the pixels [I(x1), I(x2)) x [I(y1), I(y2)) inside the path's rectangle (the frame builder hands over boxes
  already rounded by (v + 127) & ~255, where I(v) = v >> 8; a caller's boxes are rounded the same way on upload).
- Compositing.  Solid styles only, every covered pixel at full coverage: the colour itself when the path blends with the lerp rule or
  the colour is opaque, else pixman's OVER (MUL_UN8 of the destination by 255 - alpha, saturating add).

All arithmetic is in int64 with every product checked to stay below 2^62; the work is vectorised over all (edge, row) pairs of a path."""
import numpy as np

PATH_TOR, PATH_BOXES = 0, 1
STYLE_SOLID = 0
_LIMIT = 1 << 62


def _round(v):
    return (v + 127) >> 8


def _checked_mul(a, b):
    """a * b in int64, refusing any product that could reach 2^62 (checked with a float bound well above the rounding error)"""
    bound = np.abs(a).astype(np.float64) * np.abs(b).astype(np.float64)
    assert not len(bound) or float(bound.max()) < _LIMIT / 2, "product out of the exact int64 range"
    return a * b


def tor_spans(e, y_min, y_max, x_min, x_max, even_odd, H, W):
    """The spans of one tor path: arrays (row, x_start, x_end), clipped to the path's rectangle and the frame, x_start < x_end."""
    empty = (np.zeros(0, np.int64),) * 3
    if len(e) == 0:
        return empty
    x1, y1, x2, y2 = (e[k].astype(np.int64) for k in ("x1", "y1", "x2", "y2"))
    top, bottom = e["top"].astype(np.int64), e["bottom"].astype(np.int64)
    up = np.where(e["dir"] > 0, 1, -1).astype(np.int64)
    r0, r1 = max(int(y_min), 0), min(int(y_max), H)
    ra = np.maximum(_round(top), r0)
    rb = np.where(top < bottom, np.minimum(_round(bottom), r1), ra)
    n = np.maximum(rb - ra, 0)
    if int(n.sum()) == 0:
        return empty
    # every (edge, row) pair with the edge active in the row
    k = np.repeat(np.arange(len(e)), n)
    start = np.repeat(np.cumsum(n) - n, n)
    row = ra[k] + (np.arange(len(k)) - start)
    dx, dy = x2[k] - x1[k], y2[k] - y1[k]
    assert (dy > 0).all(), "an active edge with y2 <= y1"
    px = _round(x1[k] + np.floor_divide(_checked_mul(256 * row + 127 - y1[k], dx), dy))
    d = up[k]
    # groups: the pairs of one row at one pixel, in x order
    o = np.lexsort((px, row))
    row, px, d = row[o], px[o], d[o]
    new = np.ones(len(row), bool)
    new[1:] = (row[1:] != row[:-1]) | (px[1:] != px[:-1])
    gi = np.flatnonzero(new)
    grow, gpx, gd = row[gi], px[gi], np.add.reduceat(d, gi)
    first = np.ones(len(gi), bool)
    first[1:] = grow[1:] != grow[:-1]
    last = np.ones(len(gi), bool)
    last[:-1] = first[1:]
    cs = np.cumsum(gd)
    row_base = np.maximum.accumulate(np.where(first, np.arange(len(gi)), 0))
    w_after = cs - (cs[row_base] - gd[row_base])
    w_before = w_after - gd
    zero = (lambda w: (w & 1) == 0) if even_odd else (lambda w: w == 0)
    far_prev = np.ones(len(gi), bool)
    far_prev[1:] = gpx[1:] > gpx[:-1] + 1
    far_next = np.ones(len(gi), bool)
    far_next[:-1] = gpx[1:] > gpx[:-1] + 1
    opens = zero(w_before) & (first | far_prev)
    closes = zero(w_after) & (last | far_next)
    # the events alternate open, close, open, ... within each row (a close is followed by an open of the next group, an open by a close
    # before the next open); a row whose directions do not balance leaves a span open -- not a closed polygon, refused
    ev = np.stack([opens, closes], 1).ravel()
    ev_row, ev_px = np.repeat(grow, 2)[ev], np.repeat(gpx, 2)[ev]
    kind = np.tile([0, 1], len(gi))[ev]
    if len(kind) % 2 or (kind[0::2] != 0).any() or (kind[1::2] != 1).any() or (ev_row[0::2] != ev_row[1::2]).any():
        raise ValueError("edge directions do not balance along a pixel row (no closed polygon)")
    srow, xs, xe = ev_row[0::2], ev_px[0::2], ev_px[1::2]
    xs = np.maximum(xs, max(int(x_min), 0))
    xe = np.minimum(xe, min(int(x_max), W))
    keep = xs < xe
    return srow[keep], xs[keep], xe[keep]


def _coverage(H, W, rows, xs, xe):
    diff = np.zeros((H, W + 1), np.int64)
    np.add.at(diff, (rows, xs), 1)
    np.add.at(diff, (rows, xe), -1)
    return np.cumsum(diff[:, :W], 1) > 0


def path_coverage(edges, p, W, H):
    """H x W bool: the pixels one path covers (at full coverage: the mode has no other)"""
    e = edges[int(p["first_edge"]):int(p["first_edge"]) + int(p["n_edges"])]
    x_min, y_min, x_max, y_max = (int(p[k]) for k in ("x_min", "y_min", "x_max", "y_max"))
    if int(p["kind"]) == PATH_TOR:
        return _coverage(H, W, *tor_spans(e, y_min, y_max, x_min, x_max, bool(p["fill_rule"]), H, W))
    assert int(p["kind"]) == PATH_BOXES, "unknown path kind"
    cov = np.zeros((H, W), bool)
    bx0, bx1 = max(x_min, 0), min(x_max, W)
    by0, by1 = max(y_min, 0), min(y_max, H)
    for b in e:
        a0, a1 = max(_round(int(b["x1"])), bx0), min(_round(int(b["x2"])), bx1)
        c0, c1 = max(_round(int(b["y1"])), by0), min(_round(int(b["y2"])), by1)
        if a0 < a1 and c0 < c1:
            cov[c0:c1, a0:a1] = True
    return cov


def _mul_un8(x, a):
    """pixman UN8x4_MUL_UN8 on uint32 ARGB words (int64 arrays), a in 0..255"""
    rb = (x & 0xff00ff) * a + 0x800080
    rb = ((rb + ((rb >> 8) & 0xff00ff)) >> 8) & 0xff00ff
    ag = ((x >> 8) & 0xff00ff) * a + 0x800080
    ag = ((ag + ((ag >> 8) & 0xff00ff)) >> 8) & 0xff00ff
    return rb | (ag << 8)


def _add_sat(x, y):
    rb = (x & 0xff00ff) + (y & 0xff00ff)
    rb = (rb | (0x1000100 - ((rb >> 8) & 0xff00ff))) & 0xff00ff
    ag = ((x >> 8) & 0xff00ff) + ((y >> 8) & 0xff00ff)
    ag = (ag | (0x1000100 - ((ag >> 8) & 0xff00ff))) & 0xff00ff
    return rb | (ag << 8)


def over(src, dst):
    """pixman OVER of a premultiplied ARGB word onto premultiplied ARGB words"""
    return _add_sat(_mul_un8(dst, 255 - (src >> 24)), src)


def render(edges, paths, styles, W, H):
    """premultiplied RGBA (H x W x 4 uint8) of a frame in swfr_upload_edges form under the aliased rule"""
    edges = np.asarray(edges)
    img = np.zeros((H, W), np.int64)
    for p in np.asarray(paths):
        st = styles[int(p["style"])]
        if int(st.kind) != STYLE_SOLID:
            raise NotImplementedError("the model draws solid styles only")
        pix = int(st.pixel) & 0xffffffff
        cov = path_coverage(edges, p, W, H)
        if int(p["lerp"]) or (pix >> 24) == 0xff:
            img[cov] = pix
        else:
            img[cov] = over(np.int64(pix), img[cov])
    out = np.empty((H, W, 4), np.uint8)
    out[..., 0] = (img >> 16) & 255
    out[..., 1] = (img >> 8) & 255
    out[..., 2] = img & 255
    out[..., 3] = (img >> 24) & 255
    return out
