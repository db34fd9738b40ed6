// shadow_inner.hip -- the two passes of an inner shadow or inner glow (SWFR_SHADOW_INNER; DESIGN.md, "Inner shadows"), CDNA4 / gfx950.
// A device translation unit of its own beside raster2.hip: the kernels are the other instances of the two templated bodies of
// shadow_passes.hip, which shadow.hip's header describes, and are reached through shadow.hip's launch helpers alone.
//
//   k_shadow_alpha_inv  S(x, y) = (255 - Ga(x - dx, y - dy)) << 24, 0xff000000 where that pixel lies outside the image
//   k_shadow_inner_fb, k_shadow_inner_tex
//                       a = min(255, n * Sa), Tc = mul_un8(cp, a), In = mul_un8(Tc, Ga); KNOCKOUT: In; else In + mul_un8(G, 255 - Tca),
//                       saturating.  The group as framebuffer words or as ARGB texels; pointwise, so it may run in place
//
// The launch shapes are the outer passes': 256 threads, four words a lane stored as 16 bytes, a grid capped at SHADOW_MAX_BLOCKS that
// strides, a word loop for the tail and for buffers that are not 16-byte aligned.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.hpp"

namespace swfr {

#include "pixman_ops.hip"
#include "shadow_passes.hip"

__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_alpha_inv(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int dx, int dy, uint32_t quads) {
    shadow_alpha<true>(src, dst, width, height, dx, dy, quads);
}

// the inner shadow's finish pass, with the group in the same two forms
__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_inner_fb(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads,
                                                                    uint32_t cp, uint32_t strength, uint32_t flags) {
    shadow_finish<true, true>(alpha, group, out, n, quads, cp, strength, flags);
}
__global__ __launch_bounds__(SHADOW_THREADS) void k_shadow_inner_tex(const uint32_t* alpha, const uint32_t* group, uint32_t* out, size_t n, size_t quads,
                                                                     uint32_t cp, uint32_t strength, uint32_t flags) {
    shadow_finish<false, true>(alpha, group, out, n, quads, cp, strength, flags);
}

void launch_shadow_alpha_inv(hipStream_t st, const uint32_t* src, uint32_t* dst, uint32_t width, uint32_t height, int32_t dx, int32_t dy) {
    if (!width || !height) return;
    const size_t n = (size_t)width * height, quads = shadow_quads(n, dst, nullptr, nullptr);
    hipLaunchKernelGGL(k_shadow_alpha_inv, dim3(shadow_blocks(n, quads)), dim3(SHADOW_THREADS), 0, st, src, dst, (int)width, (int)height, (int)dx, (int)dy, (uint32_t)quads);
}
void launch_shadow_inner(hipStream_t st, const uint32_t* alpha, const uint32_t* group, bool rgba, uint32_t* out, size_t n, uint32_t cp, uint32_t strength, uint32_t flags) {
    if (!n) return;
    const size_t quads = shadow_quads(n, alpha, group, out);
    const dim3 grid(shadow_blocks(n, quads));
    if (rgba) hipLaunchKernelGGL(k_shadow_inner_fb, grid, dim3(SHADOW_THREADS), 0, st, alpha, group, out, n, quads, cp, strength, flags);
    else hipLaunchKernelGGL(k_shadow_inner_tex, grid, dim3(SHADOW_THREADS), 0, st, alpha, group, out, n, quads, cp, strength, flags);
}

}  // namespace swfr
