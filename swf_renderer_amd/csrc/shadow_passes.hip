// shadow_passes.hip -- the bodies of the two streaming passes of a shadow, outer and inner, and the launch shapes they share (included
// inside namespace swfr, behind pixman_ops.hip, by shadow.hip -- and so by raster2.hip -- and by shadow_inner.hip; not a translation
// unit of its own).  shadow.hip's header has the rule; the kernels are instances of the templates here.

#define SHADOW_THREADS 256
#define SHADOW_MAX_BLOCKS 2048

// the alpha word of output pixel i of a width x height image: the source's alpha at (x - dx, y - dy); INV: 255 less that alpha, a
// pixel outside the image counting as clear
template <bool INV>
__device__ __forceinline__ uint32_t shadow_alpha_at(const uint32_t* __restrict__ src, int width, int height, int x, int y, int dx, int dy) {
    const int sx = x - dx, sy = y - dy;
    const uint32_t a = (sx >= 0 && sx < width && sy >= 0 && sy < height) ? (src[(size_t)sy * width + sx] & 0xff000000u) : 0u;
    return INV ? a ^ 0xff000000u : a;
}

template <bool INV>
__device__ __forceinline__ void shadow_alpha(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int dx, int dy, uint32_t quads) {
    const uint32_t n = (uint32_t)width * (uint32_t)height;           // (at most 32768 x 32768 words)
    const uint32_t stride = gridDim.x * SHADOW_THREADS, first = blockIdx.x * SHADOW_THREADS + threadIdx.x;
    for (uint32_t q = first; q < quads; q += stride) {
        const uint32_t i = q << 2;
        int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = shadow_alpha_at<INV>(src, width, height, x, y, dx, dy);
            if (++x == width) { x = 0; ++y; }
        }
        *reinterpret_cast<uint4*>(dst + i) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    for (uint32_t i = (quads << 2) + first; i < n; i += stride) {     // the words behind the last quad
        const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
        dst[i] = shadow_alpha_at<INV>(src, width, height, x, y, dx, dy);
    }
}
// one pixel of the final surface: `s` the blurred alpha word, `g` the group's premultiplied ARGB pixel
__device__ __forceinline__ uint32_t shadow_pixel(uint32_t s, uint32_t g, uint32_t cp, uint32_t strength, uint32_t flags) {
    uint32_t a = (s >> 24) * strength;
    a = a > 255u ? 255u : a;
    const uint32_t tc = mul_un8(cp, a);
    if (flags & SWFR_SHADOW_HIDE_OBJECT) return tc;
    if (flags & SWFR_SHADOW_KNOCKOUT) return mul_un8(tc, 255u - (g >> 24));
    return over_pixel(g, tc);
}
// the same of an inner shadow: `s` the blurred inverse alpha word
__device__ __forceinline__ uint32_t shadow_inner_pixel(uint32_t s, uint32_t g, uint32_t cp, uint32_t strength, uint32_t flags) {
    uint32_t a = (s >> 24) * strength;
    a = a > 255u ? 255u : a;
    const uint32_t tc = mul_un8(cp, a);
    const uint32_t in = mul_un8(tc, g >> 24);
    if (flags & SWFR_SHADOW_KNOCKOUT) return in;
    const uint32_t m = mul_un8(g, 255u - (tc >> 24));
    return add8x2_sat(in & 0xff00ffu, m & 0xff00ffu) | (add8x2_sat((in >> 8) & 0xff00ffu, (m >> 8) & 0xff00ffu) << 8);
}
template <bool INNER>
__device__ __forceinline__ uint32_t shadow_final(uint32_t s, uint32_t g, uint32_t cp, uint32_t strength, uint32_t flags) {
    return INNER ? shadow_inner_pixel(s, g, cp, strength, flags) : shadow_pixel(s, g, cp, strength, flags);
}
__device__ __forceinline__ uint32_t shadow_group_word(uint32_t p, bool rgba) {
    return rgba ? ((p & 0xff00ff00u) | ((p & 0xffu) << 16) | ((p >> 16) & 0xffu)) : p;
}

template <bool RGBA, bool INNER>
__device__ __forceinline__ void shadow_finish(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads, uint32_t cp,
                                              uint32_t strength, uint32_t flags) {
    // (no __restrict__: `out` may be `alpha` or `group`; a lane reads its words before it writes them and no other lane touches them)
    const size_t stride = (size_t)gridDim.x * SHADOW_THREADS, first = (size_t)blockIdx.x * SHADOW_THREADS + threadIdx.x;
    for (size_t q = first; q < quads; q += stride) {
        const uint4 s = reinterpret_cast<const uint4*>(alpha)[q], g = reinterpret_cast<const uint4*>(group)[q];
        uint4 o;
        o.x = shadow_final<INNER>(s.x, shadow_group_word(g.x, RGBA), cp, strength, flags);
        o.y = shadow_final<INNER>(s.y, shadow_group_word(g.y, RGBA), cp, strength, flags);
        o.z = shadow_final<INNER>(s.z, shadow_group_word(g.z, RGBA), cp, strength, flags);
        o.w = shadow_final<INNER>(s.w, shadow_group_word(g.w, RGBA), cp, strength, flags);
        reinterpret_cast<uint4*>(out)[q] = o;
    }
    for (size_t i = (quads << 2) + first; i < n; i += stride)          // the words behind the last quad
        out[i] = shadow_final<INNER>(alpha[i], shadow_group_word(group[i], RGBA), cp, strength, flags);
}

// quads: how many groups of four words go 16 bytes wide -- all whole ones of n words, or none when a buffer is not 16-byte aligned (a
// caller's render target, swfr_set_targets, may be; the handle's own allocations never are): the word loop then takes the whole image
static inline size_t shadow_quads(size_t n, const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) ? 0 : n >> 2;
}
static inline unsigned shadow_blocks(size_t n, size_t quads) {
    const size_t items = quads > n - (quads << 2) ? quads : n - (quads << 2);
    const size_t want = (items + SHADOW_THREADS - 1) / SHADOW_THREADS;
    return (unsigned)(want > SHADOW_MAX_BLOCKS ? SHADOW_MAX_BLOCKS : want ? want : 1);
}
