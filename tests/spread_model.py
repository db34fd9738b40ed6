"""A model of a radial (or focal) gradient with a spread mode as cairo 1.16 hands it to pixman 0.40 and as pixman paints it, in
Python integers and numpy.float32 -- DESIGN.md, "Gradient spread modes".  It shares no code with csrc.

    matrices      cairo_matrix_multiply / cairo_matrix_invert, the gstate's incrementally kept inverse CTM (pattern_matrix)
    to pixman     _cairo_gradient_pattern_fit_to_range (circles into +-16383), _cairo_matrix_to_pixman_matrix_offset and the
                  re-anchoring of _pixman_image_set_properties at the centre of the operation's rectangle (to_pixman)
    position      pixman-radial-gradient.c radial_get_scanline / radial_compute_color: b and c as 64-bit integers, the root in doubles
    colour        pixman-gradient-walker.c: the sentinel stops of the repeat kind, gradient_walker_reset in single precision from
                  the interval ends shifted into the position's own period, the pixel by + .5 and truncation

The walker keeps state along a scanline (it resets only when the position leaves [left_x, right_x)).  source() evaluates a
rectangle both ways: `stateful` -- one walker per scanline, started at the rectangle's left edge, what libcairo does -- and `fresh`,
a reset at every pixel.  Where the two can differ at all is counted (`on_left_end`: positions that sit exactly on the left end of
the interval the walker is in while a fresh reset picks another interval) and so is where they do (`state_pixels`).

pixman asks the walker only for pixels whose coverage is not zero, and libcairo composites a shape span by span under
CAIRO_ANTIALIAS_NONE and box by box where its outline is rectilinear on whole pixels: source(covered=, per_run=).  frame() composes a whole frame of one shape from that and a coverage, and beside it what a walker
gives that sees every sample of the rectangle -- the device's rule -- and where the two differ (`caveat`).
"""
import math

import numpy as np

PAD, REPEAT, REFLECT = 0, 1, 2               # swfr_style::extend of a gradient (cairo_extend_t: PAD 3, REPEAT 1, REFLECT 2)
CAIRO_EXTEND = {PAD: 3, REPEAT: 1, REFLECT: 2}
F = np.float32
FLT_MIN = 1.17549435e-38
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------------------- matrices
def multiply(a, b):
    """cairo_matrix_multiply: a first, then b; matrices are (xx, yx, xy, yy, x0, y0)"""
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3],
            a[4] * b[0] + a[5] * b[2] + b[4], a[4] * b[1] + a[5] * b[3] + b[5])


def invert(m):
    """cairo_matrix_invert; None for a singular matrix"""
    xx, yx, xy, yy, x0, y0 = m
    if xy == 0.0 and yx == 0.0:
        x0, y0 = -x0, -y0
        if xx != 1.0:
            if xx == 0.0:
                return None
            xx = 1.0 / xx
            x0 *= xx
        if yy != 1.0:
            if yy == 0.0:
                return None
            yy = 1.0 / yy
            y0 *= yy
        return (xx, yx, xy, yy, x0, y0)
    det = xx * yy - yx * xy
    if det == 0.0 or det != det or math.isinf(det):
        return None
    s = 1.0 / det
    return tuple(v * s for v in (yy, -yx, -xy, xx, xy * y0 - yy * x0, yx * x0 - xx * y0))


def swf_matrix(m):
    return (m["scale_x"] / 65536.0, m["rotate_skew0"] / 65536.0, m["rotate_skew1"] / 65536.0, m["scale_y"] / 65536.0,
            float(m["translate_x"]), float(m["translate_y"]))


def pattern_matrix(matrices):
    """the inverse CTM the gstate holds after cairo_scale(1/20, 1/20) and cairo_transform of every matrix of the list (swf-tree
    matrices, outermost first, the fill's own last): what a pattern created there gets as its matrix"""
    inv = multiply((1.0, 0.0, 0.0, 1.0, 0.0, 0.0), (1.0 / (1.0 / 20.0), 0.0, 0.0, 1.0 / (1.0 / 20.0), 0.0, 0.0))
    for m in matrices:
        mi = invert(swf_matrix(m))
        if mi is None:
            return None
        inv = multiply(inv, mi)
    return inv


def fixed(d):
    """_cairo_fixed_16_16_from_double: round to nearest, ties to even"""
    return int(round(d * 65536.0))


def apply(m, x, y):
    return m[0] * x + m[2] * y + m[4], m[1] * x + m[3] * y + m[5]


def to_pixman(m, rect):
    """the 16.16 transform pixman gets for pattern matrix m and the operation rectangle (x0, y0, x1, y1): ((base_x, base_y), rows) with
    the 16.16 position of pixel (px, py)'s centre = base + px * (m00, m10) + py * (m01, m11)"""
    xc, yc = rect[0] + (rect[2] - rect[0]) / 2.0, rect[1] + (rect[3] - rect[1]) / 2.0
    xx, yx, xy, yy, x0, y0 = m
    ox = oy = 0
    if x0 != 0.0 or y0 != 0.0:
        tx, ty = x0, y0
        norm = max(abs(tx), abs(ty))
        for i in (-1, 1):
            for j in (-1, 1):
                den = (xx + i) * (yy + j) - xy * yx
                if abs(den) < 2.220446049250313e-16:
                    continue
                x, y = y0 * xy - x0 * (yy + j), x0 * yx - y0 * (xx + i)
                den = 1 / den
                x *= den
                y *= den
                if norm > max(abs(x), abs(y)):
                    norm, tx, ty = max(abs(x), abs(y)), x, y
        tx, ty = math.floor(tx), math.floor(ty)
        ox, oy = int(-tx), int(-ty)
        xx, yx, xy, yy, x0, y0 = multiply((1.0, 0.0, 0.0, 1.0, tx, ty), (xx, yx, xy, yy, x0, y0))
    p = [[fixed(xx), fixed(xy), fixed(x0)], [fixed(yx), fixed(yy), fixed(y0)]]
    eps, det = 1.0 / 256.0, xx * yy - yx * xy
    unity = abs(det * det - 1.0) < eps and ((abs(xy) < eps and abs(yx) < eps) or (abs(xx) < eps and abs(yy) < eps))
    inv = invert((xx, yx, xy, yy, x0, y0))
    if not unity and inv is not None:
        for _ in range(5):
            vx, vy = fixed(xc), fixed(yc)
            tx = (p[0][0] * vx + p[0][1] * vy + p[0][2] * 65536 + 0x8000) >> 16
            ty = (p[1][0] * vx + p[1][1] * vy + p[1][2] * 65536 + 0x8000) >> 16
            if not (-2 ** 31 <= tx < 2 ** 31 and -2 ** 31 <= ty < 2 ** 31):
                break
            x, y = apply(inv, tx / 65536.0, ty / 65536.0)
            x -= xc
            y -= yc
            x, y = xx * x + xy * y, yx * x + yy * y
            dx, dy = fixed(x), fixed(y)
            p[0][2] -= dx
            p[1][2] -= dy
            if dx == 0 and dy == 0:
                break
    X0, Y0 = ox * 65536 + 0x8000, oy * 65536 + 0x8000
    base = ((p[0][0] * X0 + p[0][1] * Y0 + p[0][2] * 65536 + 0x8000) >> 16, (p[1][0] * X0 + p[1][1] * Y0 + p[1][2] * 65536 + 0x8000) >> 16)
    return base, ((p[0][0], p[0][1]), (p[1][0], p[1][1]))


# ---------------------------------------------------------------------------------------------------------------- the walker
def short(v):
    """_cairo_color_double_to_short"""
    return int(v * 65535.0 + 0.5) & 0xffff


class Walker:
    """pixman_gradient_walker_t: stops is [(x 16.16, (a, r, g, b) 16 bit)], sorted"""

    def __init__(self, stops, extend):
        assert extend in (PAD, REPEAT, REFLECT) and stops
        first, last = stops[0], stops[-1]
        if extend == PAD:
            self.stops = [(INT32_MIN, first[1])] + list(stops) + [(INT32_MAX, last[1])]
        elif extend == REPEAT:
            self.stops = [(last[0] - 0x10000, last[1])] + list(stops) + [(first[0] + 0x10000, first[1])]
        else:
            self.stops = [(-first[0], first[1])] + list(stops) + [(0x20000 - last[0], last[1])]
        self.extend = extend
        self.left_x = self.right_x = None

    def reset(self, pos):
        """gradient_walker_reset: (left_x, right_x, left colour, right colour)"""
        if self.extend == PAD:                                       # (the position as it is, between the sentinels at the ends of int32)
            S = self.stops
            n = 1
            while n < len(S) - 1 and not pos < S[n][0]:
                n += 1
            (self.left_x, self.left_c), (self.right_x, self.right_c) = S[n - 1], S[n]
            return self.left_x, self.right_x, self.left_c, self.right_c
        low = pos & 0xffff                                           # ((int32_t) pos & 0xffff: the low bits of a two's complement number)
        odd = self.extend == REFLECT and bool(pos & 0x10000)
        x = 0x10000 - low if odd else low
        S = self.stops
        n = 1
        while n < len(S) - 1 and not x < S[n][0]:
            n += 1
        (lx, lc), (rx, rc) = S[n - 1], S[n]
        if odd:
            lx, rx, lc, rc = 0x10000 - rx, 0x10000 - lx, rc, lc
            x = 0x10000 - x
        lx += pos - x
        rx += pos - x
        self.left_x, self.right_x, self.left_c, self.right_c = lx, rx, lc, rc
        return lx, rx, lc, rc

    def at(self, pos):
        """the interval the walker is in once it has been asked for pos"""
        if self.left_x is None or pos < self.left_x or pos >= self.right_x:
            self.reset(pos)
        return self.left_x, self.right_x, self.left_c, self.right_c


def ramp_pixels(pos, lx, rx, lc, rc):
    """the walker's pixel for arrays of positions and of the interval each is evaluated in: premultiplied ARGB, uint32"""
    pos, lx, rx = np.asarray(pos, np.int64), np.asarray(lx, np.int64), np.asarray(rx, np.int64)
    lc, rc = np.asarray(lc, np.int64).reshape(-1, 4), np.asarray(rc, np.int64).reshape(-1, 4)
    k = F(1.0) / F(65536.0)
    flx, frx = lx.astype(F) * k, rx.astype(F) * k
    w = frx - flx
    flat = (np.abs(w) < F(FLT_MIN)) | (lx == INT32_MIN) | (rx == INT32_MAX)      # (PAD's sentinels: the end stop's colour)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_rec = F(1.0) / w
    y = pos.astype(F) * k
    ch = []
    for c in range(4):
        l, r = lc[:, c].astype(F) * (F(1.0) / F(257.0)), rc[:, c].astype(F) * (F(1.0) / F(257.0))
        with np.errstate(invalid="ignore", over="ignore"):
            b = np.where(flat, (l + r) / F(510.0), (l * frx - r * flx) * w_rec * (F(1.0) / F(255.0)))
            s = np.where(flat, F(0.0), (r - l) * w_rec * (F(1.0) / F(255.0)))
        ch.append((s * y + b).astype(F))
    fa = F(255.0) * ch[0]
    out = ((fa + F(0.5)).astype(np.int64) & 255) << 24
    for c, sh in ((1, 16), (2, 8), (3, 0)):
        out |= ((fa * ch[c] + F(0.5)).astype(np.int64) & 255) << sh
    return out.astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- a radial gradient
def radial_positions(m, circles, rect):
    """(valid, pos): per pixel of the rectangle whether the gradient is defined there and the 48.16 position the walker is asked for"""
    c = list(circles)
    dim = max(abs(v) for v in c + [c[0] - c[3], c[1] - c[4], c[2] - c[5]])
    if dim > 16383.0:
        dim = 16383.0 / dim
        c = [v * dim for v in c]
        m = multiply(m, (dim, 0.0, 0.0, dim, 0.0, 0.0))
    (bx, by), ((m00, m01), (m10, m11)) = to_pixman(m, rect)
    c1x, c1y, c1r = fixed(c[0]), fixed(c[1]), fixed(c[2])
    dx, dy, dr = fixed(c[3]) - c1x, fixed(c[4]) - c1y, fixed(c[5]) - c1r
    a = float(dx * dx + dy * dy - dr * dr)
    inva = 65536.0 / a if a != 0 else 0.0
    mindr = -65536.0 * float(c1r)
    px, py = np.meshgrid(np.arange(rect[0], rect[2], dtype=np.int64), np.arange(rect[1], rect[3], dtype=np.int64))
    vx, vy = bx + px * m00 + py * m01 - c1x, by + px * m10 + py * m11 - c1y
    b = (vx * dx + vy * dy + c1r * dr).astype(np.float64)
    cc = (vx * vx + vy * vy - c1r * c1r).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if a == 0:
            t = 32768.0 * cc / b
            valid = (b != 0) & (t * float(dr) >= mindr)
        else:
            discr = b * b + a * -cc
            sq = np.sqrt(np.where(discr >= 0, discr, 0.0))
            t0, t1 = (b + sq) * inva, (b - sq) * inva
            ok0, ok1 = t0 * float(dr) >= mindr, t1 * float(dr) >= mindr
            t = np.where(ok0, t0, t1)
            valid = (discr >= 0) & (ok0 | ok1)
    pos = np.where(valid, t, 0.0).astype(np.int64)
    return valid, pos


def pixman_stops(stops):
    """[(offset, r, g, b, a)] in doubles (0..1), sorted by offset -> [(x 16.16, (a, r, g, b) 16 bit)]"""
    return [(fixed(o), (short(a), short(r), short(g), short(b))) for o, r, g, b, a in stops]


def source(m, circles, stops, extend, rect, covered=None, per_run=False):
    """The source pixels of a radial gradient over the rectangle: dict(stateful=, fresh= (uint32 ARGB, premultiplied), on_left_end=,
    state_pixels=).  `covered` (bool per pixel; default all): the pixels pixman evaluates -- those with a non-zero mask; the walker
    of a row skips the others.  `per_run` (with `covered`): the stateful walker starts anew at the first pixel of every covered run of
    a row -- libcairo where it composites a shape span by span or box by box, each a scanline of its own (frame())."""
    valid, pos = radial_positions(m, circles, rect)
    starts = np.zeros(valid.shape, bool)
    if covered is not None:
        valid = valid & covered
        if per_run:
            starts[:, 1:] = covered[:, 1:] & ~covered[:, :-1]
    h, w = pos.shape
    S = pixman_stops(stops)
    out = {}
    on_left_end = 0
    iv = {"stateful": [], "fresh": []}
    where = []
    for yy in range(h):
        walker, fresh = Walker(S, extend), Walker(S, extend)
        for xx in range(w):
            if starts[yy, xx]:
                walker = Walker(S, extend)
            if not valid[yy, xx]:
                continue
            p = int(pos[yy, xx])
            st, fr = walker.at(p), fresh.reset(p)
            if st[0] == p and st != fr:
                on_left_end += 1
            iv["stateful"].append(st)
            iv["fresh"].append(fr)
            where.append((yy, xx))
    ys, xs = np.array([q[0] for q in where], np.int64), np.array([q[1] for q in where], np.int64)
    for kind, L in iv.items():
        img = np.zeros((h, w), np.uint32)
        if L:
            img[ys, xs] = ramp_pixels(pos[ys, xs], [q[0] for q in L], [q[1] for q in L], [q[2] for q in L], [q[3] for q in L])
        out[kind] = img
    out["on_left_end"] = on_left_end
    out["state_pixels"] = int((out["stateful"] != out["fresh"]).sum())
    out["exact_hits"] = sum(1 for (yy, xx), fr in zip(where, iv["fresh"]) if int(pos[yy, xx]) in (fr[0], fr[1]))
    return out


def mul_un8(rgba, a):
    """pixman's MUL_UN8 of every channel of HxWx4 bytes by the HxW bytes a: (t + (t >> 8)) >> 8 with t = c * a + 0x80"""
    t = rgba.astype(np.int64) * a.astype(np.int64)[..., None] + 0x80
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def frame(m, circles, stops, extend, rect, alpha, per_run):
    """One shape filled with the gradient over a clear frame.  `alpha` is the shape's coverage over the whole frame (H x W bytes, zero
    outside `rect`, the operation's rectangle).  On a clear surface OVER leaves source IN coverage, mul_un8(source, alpha).
    `per_run`: libcairo composites the shape piece by piece -- under CAIRO_ANTIALIAS_NONE span by span, and in either mode a
    rectilinear outline on whole pixels box by box -- and not once through a mask.  dict of
        truth         libcairo: pixman asks the walker for the pixels with coverage only -- through a mask, one walker per row of the
                      rectangle that skips the others; piece by piece, a walker per covered run of a row (source's per_run)
        every_sample  the device's documented rule ("Gradient spread modes"): a walker that sees every sample of the row
                      from the rectangle's left edge on, covered or not
        caveat        H x W bool, where the two differ: a covered run that begins exactly on a stop in an odd reflected period
    all premultiplied R, G, B, A bytes of the frame's size."""
    x0, y0, x1, y1 = rect
    inside = np.zeros(alpha.shape, bool)
    inside[y0:y1, x0:x1] = True
    assert not alpha[~inside].any(), "coverage outside the operation's rectangle"
    a = alpha[y0:y1, x0:x1]
    out = {}
    for key, kw in (("truth", dict(covered=a > 0, per_run=per_run)), ("every_sample", {})):
        img = np.zeros(alpha.shape + (4,), np.uint8)
        img[y0:y1, x0:x1] = mul_un8(rgba_bytes(source(m, circles, stops, extend, rect, **kw)["stateful"]), a)
        out[key] = img
    out["caveat"] = (out["truth"] != out["every_sample"]).any(-1)
    return out


def rgba_bytes(argb):
    """uint32 premultiplied ARGB -> HxWx4 uint8 in R, G, B, A order"""
    return np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255, argb >> 24], axis=-1).astype(np.uint8)
