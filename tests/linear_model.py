"""A model of a linear gradient as cairo 1.16 hands it to pixman 0.40 and as pixman paints it, in Python integers and floats over
tests/spread_model.py's transform, walker and ramp -- DESIGN.md, "Pixman-exact linear gradients".  It shares no code with csrc.

    to pixman     _cairo_gradient_pattern_fit_to_range (the line's end points into +-16383, the matrix takes the factor), then
                  spread_model.to_pixman: the 16.16 transform anchored at the centre of the operation's rectangle
    position      pixman-linear-gradient.c linear_get_scanline, the affine branch.  Per scanline of a PIECE (what libcairo hands to
                  pixman_image_composite32 as one rectangle), with v the 16.16 sample position of the pixel centre at the piece's left
                  edge, dx, dy = p2 - p1 and l = dx^2 + dy^2 as 64-bit integers:
                      invden = 65536.0 / (double) l
                      t      = ((double) (dx v.x + dy v.y) - (double) (dx p1.x + dy p1.y)) * invden
                      inc    = (double) (dx m00 + dy m10) * invden
                  the i-th pixel from the left edge asks the walker for  trunc(t) + trunc(inc * i)  -- two truncations to a 64-bit
                  integer -- unless trunc(inc * width) == 0: then the whole scanline is the walker's pixel at trunc(t).
    rows          _pixman_linear_gradient_iter_init: when the position moves by less than one 16.16 unit over the piece's HEIGHT
                  (linear_gradient_is_horizontal: -1 < height * 65536 * (dx m01 + dy m11) / l < 1) pixman computes the piece's FIRST
                  scanline once, without looking at the mask, and repeats it for every row.
    colour        spread_model.Walker / ramp_pixels (pixman-gradient-walker.c), one walker per scanline of a piece; it is asked only
                  for pixels whose mask is not zero -- except in the two shortcuts above, which never see the mask.

A piece: a rectilinear outline on whole pixels is composited box by box, every box a piece of its own -- inside the one transform
anchored at the whole operation's rectangle.  Every other antialiased shape goes through libcairo's span renderer
(cairo-image-compositor.c, _inplace_spans, with run_length 256 for a gradient source), which hands pixman every ROW of spans on its
own: one composite from the row's first span to its last, cut where a span of 256 or more pixels has coverage 255 (composited alone,
without the mask) and where an empty span follows more than 256 gathered pixels: span_pieces().  The spans are the scan converter's --
one wherever the raw area changes; this model sees the 8-bit coverage only and takes a span for every run of equal coverage, which
differs where a first pixel's area rounds to coverage 0 (its piece then starts one pixel late here) and where a pixel beside a
255-pixel-long full run has coverage 255 without being full: the tests count those frames.
source() returns both: `one_piece` (the rectangle as a single piece) and `pieces` (piece by piece, where pieces are given).
"""
import numpy as np

import spread_model as sm

PAD, REPEAT, REFLECT = sm.PAD, sm.REPEAT, sm.REFLECT
INT64 = 2 ** 63
INT32 = 2 ** 31


def to_pixman(m, line, rect):
    """(base, rows, p1, (dx, dy)): the 16.16 transform and line pixman gets for pattern matrix m, the line (x1, y1, x2, y2) in pattern
    units and the operation's rectangle"""
    x1, y1, x2, y2 = (float(v) for v in line)
    dim = max(abs(x1), abs(y1), abs(x2), abs(y2), abs(x1 - x2), abs(y1 - y2))
    if dim > 16383.0:
        dim = 16383.0 / dim
        x1, y1, x2, y2 = x1 * dim, y1 * dim, x2 * dim, y2 * dim
        m = sm.multiply(m, (dim, 0.0, 0.0, dim, 0.0, 0.0))
    base, rows = sm.to_pixman(m, rect)
    p1 = (sm.fixed(x1), sm.fixed(y1))
    return base, rows, p1, (sm.fixed(x2) - p1[0], sm.fixed(y2) - p1[1])


def in_range(m, line, rect):
    """whether libcairo is defined for this gradient over this rectangle ("Pixman-exact linear gradients", the range):
    pixman composites a piece only if its rectangle GROWN BY ONE PIXEL maps into 16.16 with eight units to spare (pixman.c,
    analyze_extent: the pixel centres of the grown box, IS_16BIT) -- else the piece is silently left out, so libcairo paints some
    rows of the shape and not others.  Tested on the operation's rectangle, which holds every piece.  It also keeps
    dx v.x + dy v.y inside 64 bits."""
    (bx, by), ((m00, m01), (m10, m11)), _, _ = to_pixman(m, line, rect)
    lim = INT32 - 8
    for px in (rect[0] - 1, rect[2]):
        for py in (rect[1] - 1, rect[3]):
            vx, vy = bx + px * m00 + py * m01, by + px * m10 + py * m11
            if not (-lim <= vx < lim and -lim <= vy < lim):
                return False
    return True


RUN_LENGTH = 256


def row_step(m, line, rect):
    """by how many 16.16 units the position moves from one pixel row to the next"""
    _, ((m00, m01), (m10, m11)), _, (dx, dy) = to_pixman(m, line, rect)
    l = dx * dx + dy * dy
    return float(dx * m01 + dy * m11) * (65536.0 * 65536.0 / (float(l) * 65536.0)) if l else 0.0


def accepted(m, line, rect):
    """what the product draws: inside the range, and the position stands still from row to row or moves by a 16.16 unit
    or more -- in between pixman evaluates a piece's first scanline for all its rows, and which rows make a piece is libcairo's
    business (NotImplementedLinearRowStep)"""
    if not in_range(m, line, rect):
        return False
    rs = row_step(m, line, rect)
    return rs == 0 or abs(rs) >= 1


def span_pieces(alpha, rect):
    """the pieces of a shape composited through the span renderer: [(x0, y, x1, y + 1)] per row, from the 8-bit coverage"""
    x0r, y0, x1r, y1 = rect
    out = []
    for y in range(y0, y1):
        row = alpha[y, x0r:x1r]
        runs, s = [], 0
        for x in range(1, len(row) + 1):
            if x == len(row) or row[x] != row[s]:
                runs.append((s + x0r, x + x0r, int(row[s])))
                s = x
        if runs and runs[0][2] == 0:
            runs = runs[1:]
        if runs and runs[-1][2] == 0:
            runs = runs[:-1]
        if not runs:
            continue
        x0 = x1 = runs[0][0]
        for a, b, c in runs:
            if b - a > 1:
                if b - a >= RUN_LENGTH and c == 255:
                    if x1 != x0:
                        out.append((x0, y, x1, y + 1))
                    out.append((a, y, b, y + 1))
                    x0 = b
                elif c == 0 and x1 - x0 > RUN_LENGTH:
                    out.append((x0, y, x1, y + 1))
                    x0 = b
            x1 = b
        if x1 != x0:
            out.append((x0, y, x1, y + 1))
    return out


def piece_positions(tr, piece):
    """(pos, constant_rows, constant_row): the walker positions of a piece (x0, y0, x1, y1), int64 H x W; constant_rows: the piece's
    first scanline serves every row (and ignores the mask); constant_row[y]: that scanline is one pixel, filled without the mask"""
    (bx, by), ((m00, m01), (m10, m11)), (p1x, p1y), (dx, dy) = tr
    x0, y0, x1, y1 = piece
    w, h = x1 - x0, y1 - y0
    pos = np.zeros((h, w), np.int64)
    flat = np.zeros(h, bool)
    l = dx * dx + dy * dy
    if l == 0:
        return pos, False, np.ones(h, bool)
    inc_rows = h * 65536.0 * 65536.0 * float(dx * m01 + dy * m11) / (65536.0 * float(l))
    constant_rows = -1 < inc_rows < 1
    invden = 65536.0 * 65536.0 / (float(l) * 65536.0)
    inc = float(dx * m00 + dy * m10) * invden
    steps = np.array([int(inc * i) for i in range(w)], np.int64)
    for r in range(h):
        y = y0 if constant_rows else y0 + r
        vx, vy = bx + x0 * m00 + y * m01, by + x0 * m10 + y * m11
        a, b = dx * vx + dy * vy, dx * p1x + dy * p1y
        assert -INT64 <= a < INT64 and -INT64 <= b < INT64, "outside pixman's 64-bit arithmetic: not in the documented range"
        t = int((float(a) - float(b) * 1.0) * invden)
        if int(inc * w) == 0:
            pos[r, :] = t
            flat[r] = True
        else:
            pos[r, :] = t + steps
    return pos, constant_rows, flat


def _paint(pos, constant_rows, flat, S, extend, covered):
    """the stateful walker over a piece: uint32 premultiplied ARGB, zero where pixman does not ask (mask zero)"""
    h, w = pos.shape
    img = np.zeros((h, w), np.uint32)
    iv, where = [], []
    for r in range(h):
        if constant_rows and r:
            img[r] = img[0]
            continue
        walker = sm.Walker(S, extend)
        unmasked = constant_rows or flat[r]
        for x in range(1 if flat[r] else w):
            if not unmasked and not covered[r, x]:
                continue
            iv.append(walker.at(int(pos[r, x])))
            where.append((r, x))
    if iv:
        ys, xs = np.array([q[0] for q in where]), np.array([q[1] for q in where])
        img[ys, xs] = sm.ramp_pixels(pos[ys, xs], [q[0] for q in iv], [q[1] for q in iv], [q[2] for q in iv], [q[3] for q in iv])
    for r in range(h):
        if constant_rows and r:
            img[r] = img[0]
        elif flat[r]:
            img[r, :] = img[r, 0]
    return img


def source(m, line, stops, extend, rect, covered=None, pieces=None):
    """The source pixels of a linear gradient over the operation's rectangle: dict(one_piece=, pieces=) of uint32 premultiplied ARGB
    (H x W of the rectangle).  `covered` (bool per pixel of the rectangle; default all): the pixels whose mask is not zero.  `pieces`:
    the boxes [(x0, y0, x1, y1)] libcairo composites one by one (default: the rectangle); outside them `pieces` is zero."""
    tr = to_pixman(m, line, rect)
    S = sm.pixman_stops(stops)
    x0, y0, x1, y1 = rect
    if covered is None:
        covered = np.ones((y1 - y0, x1 - x0), bool)
    out = {"one_piece": _paint(*piece_positions(tr, rect), S, extend, covered)}
    img = np.zeros((y1 - y0, x1 - x0), np.uint32)
    for (a, b, c, d) in (pieces or [rect]):
        img[b - y0:d - y0, a - x0:c - x0] = _paint(*piece_positions(tr, (a, b, c, d)), S, extend, covered[b - y0:d - y0, a - x0:c - x0])
    out["pieces"] = img
    return out


def state_pixels(m, line, stops, extend, rect, rows=2):
    """bool, rows x W: where, in the first rows of the rectangle taken as one piece, the walker's state along the scanline decides the
    pixel -- a walker reset at every pixel paints otherwise (a sample exactly on a stop in an odd reflected period)"""
    pos, constant_rows, flat = piece_positions(to_pixman(m, line, rect), (rect[0], rect[1], rect[2], rect[1] + rows))
    S = sm.pixman_stops(stops)
    stateful = _paint(pos, constant_rows, flat, S, extend, np.ones(pos.shape, bool))
    w = sm.Walker(S, extend)
    iv = [w.reset(int(p)) for p in pos.ravel()]
    fresh = sm.ramp_pixels(pos.ravel(), [q[0] for q in iv], [q[1] for q in iv], [q[2] for q in iv], [q[3] for q in iv]).reshape(pos.shape)
    return stateful != fresh


def frame(m, line, stops, extend, rect, alpha, boxes=None, hidden_rows=()):
    """One shape filled with the gradient over a clear frame, as spread_model.frame: dict(truth=, every_sample=, caveat=, one_piece=).
    `boxes`: the whole-pixel boxes of a rectilinear outline (composited box by box); None: the span renderer's pieces of `alpha`.
    every_sample is the device's rule: the same pieces, the walker of each seeing every sample from the piece's first column on.
    `hidden_rows`: frame rows whose first piece begins one pixel further left than the 8-bit coverage shows (a first pixel whose area
    rounds to coverage 0: the module's docstring) -- how a test shows that a frame differs from libcairo for that reason alone."""
    x0, y0, x1, y1 = rect
    a = alpha[y0:y1, x0:x1]
    out = {}
    pieces = list(boxes) if boxes is not None else span_pieces(alpha, rect)
    for y in hidden_rows:
        k = min(i for i, q in enumerate(pieces) if q[1] == y)
        pieces[k] = (max(pieces[k][0] - 1, x0),) + tuple(pieces[k][1:])
    src = source(m, line, stops, extend, rect, covered=a > 0, pieces=pieces)
    out["one_piece"] = np.zeros(alpha.shape + (4,), np.uint8)
    out["one_piece"][y0:y1, x0:x1] = sm.mul_un8(sm.rgba_bytes(src["one_piece"]), a)
    for key, s in (("truth", src["pieces"]), ("every_sample", source(m, line, stops, extend, rect, pieces=pieces)["pieces"])):
        img = np.zeros(alpha.shape + (4,), np.uint8)
        img[y0:y1, x0:x1] = sm.mul_un8(sm.rgba_bytes(s), a)
        out[key] = img
    out["caveat"] = (out["truth"] != out["every_sample"]).any(-1)
    return out
