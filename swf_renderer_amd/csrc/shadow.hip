// shadow.hip -- drop shadow and glow of a group's texture (included by raster2.hip, not a translation unit of its own).  DESIGN.md,
// "Shadowed layers".
//
// A shadow is made of the group G in four steps, two of them here; the box passes between them are blur.hip's:
//
//   k_shadow_alpha   S(x, y) = Ga(x - dx, y - dy) << 24, 0 where that pixel lies outside the image -- cairo_mask_surface(G, dx, dy) under
//                    an opaque black source onto a clear surface.  The source words carry alpha in the top byte, as premultiplied
//                    RGBA8 framebuffer words and as ARGB texels alike.
//   k_shadow_finish  a = min(255, n * Sa) (n saturating ADD paints), Tc = mul_un8(cp, a) (the colour's premultiplied pixel under the mask),
//                    then by flag: HIDE_OBJECT Tc; KNOCKOUT mul_un8(Tc, 255 - Ga) (DEST_OUT); neither G OVER Tc.  G comes as framebuffer
//                    words (RGBA, turned into ARGB as k_blur_capture does) or as ARGB texels.  Pointwise: it may run in place, over
//                    the blurred alpha or over G.
//
// Both are streaming passes: a lane takes four consecutive words, a wavefront 256 of them; at most SHADOW_MAX_BLOCKS workgroups stride over
// the image.  The words a lane writes start at a multiple of four words in an allocation of the device's, so stores are 16 bytes wide,
// and so are the loads of the finish pass; the shifted loads of the alpha pass are aligned to four bytes only and go word by word.  The
// last one to three words of an image whose size is no multiple of four go word by word, too -- as does a whole image in a buffer that
// is not 16-byte aligned (shadow_quads).  No LDS.

#define SHADOW_THREADS 256
#define SHADOW_MAX_BLOCKS 2048

// the alpha word of output pixel i of a width x height image: the source's alpha at (x - dx, y - dy)
__device__ __forceinline__ uint32_t shadow_alpha_at(const uint32_t* __restrict__ src, int width, int height, int x, int y, int dx, int dy) {
    const int sx = x - dx, sy = y - dy;
    return (sx >= 0 && sx < width && sy >= 0 && sy < height) ? (src[(size_t)sy * width + sx] & 0xff000000u) : 0u;
}

__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_alpha(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int dx, int dy, uint32_t quads) {
    const uint32_t n = (uint32_t)width * (uint32_t)height;           // (at most 32768 x 32768 words)
    const uint32_t stride = gridDim.x * SHADOW_THREADS, first = blockIdx.x * SHADOW_THREADS + threadIdx.x;
    for (uint32_t q = first; q < quads; q += stride) {
        const uint32_t i = q << 2;
        int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = shadow_alpha_at(src, width, height, x, y, dx, dy);
            if (++x == width) { x = 0; ++y; }
        }
        *reinterpret_cast<uint4*>(dst + i) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    for (uint32_t i = (quads << 2) + first; i < n; i += stride) {     // the words behind the last quad
        const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
        dst[i] = shadow_alpha_at(src, width, height, x, y, dx, dy);
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
__device__ __forceinline__ uint32_t shadow_group_word(uint32_t p, bool rgba) {
    return rgba ? ((p & 0xff00ff00u) | ((p & 0xffu) << 16) | ((p >> 16) & 0xffu)) : p;
}

template <bool RGBA>
__device__ __forceinline__ void shadow_finish(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads, uint32_t cp,
                                              uint32_t strength, uint32_t flags) {
    // (no __restrict__: `out` may be `alpha` or `group`; a lane reads its words before it writes them and no other lane touches them)
    const size_t stride = (size_t)gridDim.x * SHADOW_THREADS, first = (size_t)blockIdx.x * SHADOW_THREADS + threadIdx.x;
    for (size_t q = first; q < quads; q += stride) {
        const uint4 s = reinterpret_cast<const uint4*>(alpha)[q], g = reinterpret_cast<const uint4*>(group)[q];
        uint4 o;
        o.x = shadow_pixel(s.x, shadow_group_word(g.x, RGBA), cp, strength, flags);
        o.y = shadow_pixel(s.y, shadow_group_word(g.y, RGBA), cp, strength, flags);
        o.z = shadow_pixel(s.z, shadow_group_word(g.z, RGBA), cp, strength, flags);
        o.w = shadow_pixel(s.w, shadow_group_word(g.w, RGBA), cp, strength, flags);
        reinterpret_cast<uint4*>(out)[q] = o;
    }
    for (size_t i = (quads << 2) + first; i < n; i += stride)          // the words behind the last quad
        out[i] = shadow_pixel(alpha[i], shadow_group_word(group[i], RGBA), cp, strength, flags);
}

// k_shadow_finish with the group as framebuffer words (swfr_render) and as ARGB texels (swfr_shadow_bitmap)
__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_finish_fb(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads,
                                                                     uint32_t cp, uint32_t strength, uint32_t flags) {
    shadow_finish<true>(alpha, group, out, n, quads, cp, strength, flags);
}
__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_finish_tex(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads,
                                                                      uint32_t cp, uint32_t strength, uint32_t flags) {
    shadow_finish<false>(alpha, group, out, n, quads, cp, strength, flags);
}

// quads: how many groups of four words go 16 bytes wide -- all whole ones of n words, or none when a buffer is not 16-byte aligned (a
// caller's render target, swfr_set_targets, may be; the handle's own allocations never are): the word loop then takes the whole image
static size_t shadow_quads(size_t n, const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) ? 0 : n >> 2;
}
static unsigned shadow_blocks(size_t n, size_t quads) {
    const size_t items = quads > n - (quads << 2) ? quads : n - (quads << 2);
    const size_t want = (items + SHADOW_THREADS - 1) / SHADOW_THREADS;
    return (unsigned)(want > SHADOW_MAX_BLOCKS ? SHADOW_MAX_BLOCKS : want ? want : 1);
}
// the alpha of the width x height image `src`, shifted by (dx, dy), into `dst` (another buffer)
void launch_shadow_alpha(hipStream_t st, const uint32_t* src, uint32_t* dst, uint32_t width, uint32_t height, int32_t dx, int32_t dy) {
    if (!width || !height) return;
    const size_t n = (size_t)width * height, quads = shadow_quads(n, dst, nullptr, nullptr);
    hipLaunchKernelGGL(k_shadow_alpha, dim3(shadow_blocks(n, quads)), dim3(SHADOW_THREADS), 0, st, src, dst, (int)width, (int)height, (int)dx, (int)dy, (uint32_t)quads);
}
// n words of blurred alpha and of the group (`rgba`: framebuffer words; else ARGB texels) -> n ARGB words of the final surface;
// `out` another buffer or one of the two inputs
void launch_shadow_finish(hipStream_t st, const uint32_t* alpha, const uint32_t* group, bool rgba, uint32_t* out, size_t n, uint32_t cp, uint32_t strength, uint32_t flags) {
    if (!n) return;
    const size_t quads = shadow_quads(n, alpha, group, out);
    const dim3 grid(shadow_blocks(n, quads));
    if (rgba) hipLaunchKernelGGL(k_shadow_finish_fb, grid, dim3(SHADOW_THREADS), 0, st, alpha, group, out, n, quads, cp, strength, flags);
    else hipLaunchKernelGGL(k_shadow_finish_tex, grid, dim3(SHADOW_THREADS), 0, st, alpha, group, out, n, quads, cp, strength, flags);
}
