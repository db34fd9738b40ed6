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
// An inner shadow (SWFR_SHADOW_INNER; DESIGN.md, "Inner shadows") runs the same two steps with other arithmetic, as instances of the
// same two bodies (shadow_passes.hip).  Its kernels live in a translation unit of their own, shadow_inner.hip: raster2.hip's set of
// kernels is held as it is, field for field, by the resource-budget tests, and the launch helpers below hand an inner shadow over:
//
//   k_shadow_alpha_inv  S(x, y) = (255 - Ga(x - dx, y - dy)) << 24, 0xff000000 where that pixel lies outside the image -- an opaque black
//                       paint, then cairo_mask_surface(G, dx, dy) under DEST_OUT.
//   k_shadow_inner      a and Tc as above, then In = mul_un8(Tc, Ga); KNOCKOUT: In (DEST_IN of G); else In + mul_un8(G, 255 - Tca),
//                       saturating (Tc ATOP G: pixman's UN8x4_MUL_UN8_ADD_UN8x4_MUL_UN8).  The group as for k_shadow_finish.
//
// Both are streaming passes: a lane takes four consecutive words, a wavefront 256 of them; at most SHADOW_MAX_BLOCKS workgroups stride over
// the image.  The words a lane writes start at a multiple of four words in an allocation of the device's, so stores are 16 bytes wide,
// and so are the loads of the finish pass; the shifted loads of the alpha pass are aligned to four bytes only and go word by word.  The
// last one to three words of an image whose size is no multiple of four go word by word, too -- as does a whole image in a buffer that
// is not 16-byte aligned (shadow_quads).  No LDS.

#include "shadow_passes.hip"

__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_alpha(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int dx, int dy, uint32_t quads) {
    shadow_alpha<false>(src, dst, width, height, dx, dy, quads);
}

// k_shadow_finish with the group as framebuffer words (swfr_render) and as ARGB texels (swfr_shadow_bitmap)
__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_finish_fb(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads,
                                                                     uint32_t cp, uint32_t strength, uint32_t flags) {
    shadow_finish<true, false>(alpha, group, out, n, quads, cp, strength, flags);
}
__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_finish_tex(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads,
                                                                      uint32_t cp, uint32_t strength, uint32_t flags) {
    shadow_finish<false, false>(alpha, group, out, n, quads, cp, strength, flags);
}

// the inner shadow's two launches (shadow_inner.hip)
void launch_shadow_alpha_inv(hipStream_t st, const uint32_t* src, uint32_t* dst, uint32_t width, uint32_t height, int32_t dx, int32_t dy);
void launch_shadow_inner(hipStream_t st, const uint32_t* alpha, const uint32_t* group, bool rgba, uint32_t* out, size_t n, uint32_t cp, uint32_t strength, uint32_t flags);

// the alpha of the width x height image `src`, shifted by (dx, dy), into `dst` (another buffer); `inner`: the inverse alpha
void launch_shadow_alpha(hipStream_t st, const uint32_t* src, uint32_t* dst, uint32_t width, uint32_t height, int32_t dx, int32_t dy, bool inner) {
    if (!width || !height) return;
    if (inner) return launch_shadow_alpha_inv(st, src, dst, width, height, dx, dy);
    const size_t n = (size_t)width * height, quads = shadow_quads(n, dst, nullptr, nullptr);
    hipLaunchKernelGGL(k_shadow_alpha, dim3(shadow_blocks(n, quads)), dim3(SHADOW_THREADS), 0, st, src, dst, (int)width, (int)height, (int)dx, (int)dy, (uint32_t)quads);
}
// n words of blurred alpha and of the group (`rgba`: framebuffer words; else ARGB texels) -> n ARGB words of the final surface;
// `out` another buffer or one of the two inputs.  SWFR_SHADOW_INNER in `flags` picks the inner instances
void launch_shadow_finish(hipStream_t st, const uint32_t* alpha, const uint32_t* group, bool rgba, uint32_t* out, size_t n, uint32_t cp, uint32_t strength, uint32_t flags) {
    if (!n) return;
    if (flags & SWFR_SHADOW_INNER) return launch_shadow_inner(st, alpha, group, rgba, out, n, cp, strength, flags);
    const size_t quads = shadow_quads(n, alpha, group, out);
    const dim3 grid(shadow_blocks(n, quads));
    if (rgba) hipLaunchKernelGGL(k_shadow_finish_fb, grid, dim3(SHADOW_THREADS), 0, st, alpha, group, out, n, quads, cp, strength, flags);
    else hipLaunchKernelGGL(k_shadow_finish_tex, grid, dim3(SHADOW_THREADS), 0, st, alpha, group, out, n, quads, cp, strength, flags);
}
