// convolve.hip -- the general convolution of a group's surface (SWFR_FILTER_CONVOLUTION, swfr_convolve_bitmap; DESIGN.md, "Convolution
// filters"), CDNA4 / gfx950.  A device translation unit of its own beside raster2.hip, reached through launch_convolve alone.
//
// A kernel of kw x kh signed 16.16 taps (1..7 each way, row-major) over a premultiplied image, EXTEND_NONE: per channel, alpha included,
//     S = sum_j sum_i tap[j][i] * c(x - kw / 2 + i, y - kh / 2 + j) + 0x8000,   out = S < 0 ? 255 : min(255, S >> 16),
// a tap outside the image reading 0 -- pixman 0.40's PIXMAN_FILTER_CONVOLUTION under PIXMAN_OP_SRC, whose accumulators are unsigned: a
// negative sum is a huge one and clips to 255, not to 0.  sum |tap| <= 8 388 607: every tap fits a signed 24-bit multiply and
// 255 * sum |tap| + 0x8000 < 2^31, so the 32-bit sums below are exact and a set top bit means a negative sum.
//
//   k_convolve_fb    the input is premultiplied RGBA8 framebuffer words (r in the low byte), the output ARGB texels
//   k_convolve_tex   the input is ARGB texels, and so is the output
// The rule is blind to the channels' order: the two are one body that differs in the store.
//
// A workgroup of 256 threads owns a CONV_TILE_W x CONV_TILE_H output tile.  The tile, four columns to its left (a whole quad: the
// staged rows begin 16-byte aligned wherever the image's rows do), four to its right and kh - 1 rows around it are staged into LDS --
// 16 bytes a lane where the input's base is 16-byte aligned and the width a multiple of four, word by word otherwise (a caller's
// render target may be word aligned only; swfr_set_targets) --, pixels outside the image as 0.  A lane then computes CONV_RUN adjacent
// pixels of one row: per kernel row it loads the row's taps (wave-uniform: a kernel argument, one scalar load into SGPRs), reads the
// CONV_RUN + kw - 1 staged words its outputs share (in pairs behind uniform branches), unpacks each into its four channels once, and
// runs the row's taps over them: a zero tap is skipped with a uniform branch as pixman skips it, and a tap that counts is
// CONV_RUN x 4 signed 24-bit multiply-accumulates.  The dimensions are runtime
// values: the loop over kernel rows is a loop, the taps of a row and the staged words are unrolled to CONV_MAX_DIM with uniform
// guards, so that every register index is static.  The staged row pitch is 73 words: a wavefront's 64 lanes (16 runs of four rows)
// read 64 different banks.  No scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.hpp"

namespace swfr {

#define CONV_THREADS 256
#define CONV_TILE_W 64
#define CONV_TILE_H 16
#define CONV_RUN 4
#define CONV_MAX_DIM SWFR_MAX_KERNEL_DIM
#define CONV_LEFT 4
#define CONV_COLS (CONV_LEFT + CONV_TILE_W + 4)
#define CONV_ROWS (CONV_TILE_H + CONV_MAX_DIM - 1)
#define CONV_PITCH 73
#define CONV_TAP_PITCH 8
#define CONV_WIDE_IN 1
#define CONV_WIDE_OUT 2
static_assert(CONV_TILE_W / CONV_RUN * CONV_TILE_H == CONV_THREADS, "a lane per run");
static_assert(CONV_MAX_DIM / 2 < CONV_LEFT && CONV_MAX_DIM - 1 - CONV_MAX_DIM / 2 <= 4, "the apron fits the staged columns");
static_assert(CONV_PITCH >= CONV_COLS && CONV_PITCH % 4 == 1, "rows r, r + 1, r + 2, r + 3 start on banks 0, 1, 2, 3 modulo 4");
static_assert(CONV_COLS % 4 == 0 && CONV_RUN == 4, "quads");

// the taps as the kernels take them: row j at t[j * CONV_TAP_PITCH ..], whatever the kernel's width
struct ConvTaps { int32_t t[CONV_MAX_DIM * CONV_TAP_PITCH]; };

// pixman's reduce_32: the sum as an unsigned number, divided by 65536, clipped to 255 -- a negative sum gives 255
__device__ __forceinline__ uint32_t conv_byte(int32_t acc) {
    const uint32_t v = (uint32_t)acc >> 16;
    return v > 255u ? 255u : v;
}

template <bool RGBA>
__device__ __forceinline__ void convolve_tile(uint32_t* tile, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int kw,
                                              int kh, int wide, const ConvTaps& taps) {
    const int x0 = (int)blockIdx.x * CONV_TILE_W, y0 = (int)blockIdx.y * CONV_TILE_H;
    const int rows = CONV_TILE_H + kh - 1, top = y0 - (kh >> 1), left = x0 - CONV_LEFT;
    if (wide & CONV_WIDE_IN) {
        for (int q = (int)threadIdx.x; q < rows * (CONV_COLS / 4); q += CONV_THREADS) {
            const int r = q / (CONV_COLS / 4), s = (q - r * (CONV_COLS / 4)) * 4;
            const int y = top + r, x = left + s;                          // (x and the width are multiples of four: a quad is inside or outside)
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (y >= 0 && y < height && x >= 0 && x < width) v = *reinterpret_cast<const uint4*>(src + (size_t)y * width + x);
            uint32_t* p = tile + r * CONV_PITCH + s;
            p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        }
    } else {
        for (int i = (int)threadIdx.x; i < rows * CONV_COLS; i += CONV_THREADS) {
            const int r = i / CONV_COLS, s = i - r * CONV_COLS;
            const int y = top + r, x = left + s;
            tile[r * CONV_PITCH + s] = (y >= 0 && y < height && x >= 0 && x < width) ? src[(size_t)y * width + x] : 0u;
        }
    }
    __syncthreads();
    const int l = (int)threadIdx.x & (CONV_TILE_W / CONV_RUN - 1), ry = (int)threadIdx.x / (CONV_TILE_W / CONV_RUN);
    int32_t acc[CONV_RUN][4];
#pragma unroll
    for (int o = 0; o < CONV_RUN; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[o][c] = 0x8000;
    // staged word i of the lane's row is the pixel x0 + CONV_RUN * l - kw / 2 + i: output o under tap t reads word o + t
    const uint32_t* in = tile + ry * CONV_PITCH + CONV_RUN * l + (CONV_LEFT - (kw >> 1));
    int32_t ch[CONV_RUN + CONV_MAX_DIM - 1][4];
#pragma unroll
    for (int i = 0; i < CONV_RUN + CONV_MAX_DIM - 1; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) ch[i][c] = 0;
    for (int j = 0; j < kh; ++j, in += CONV_PITCH) {
        // the row's taps, all CONV_TAP_PITCH of the table's row in one scalar load, before the staged words are waited for
        int32_t f[CONV_MAX_DIM];
#pragma unroll
        for (int t = 0; t < CONV_MAX_DIM; ++t) f[t] = taps.t[j * CONV_TAP_PITCH + t];
        // words 0..3 serve every width; two more per two more taps (kw = 2 reads one word it does not use)
#pragma unroll
        for (int i = 0; i < CONV_RUN + CONV_MAX_DIM - 1; i += 2) {
            if (i >= CONV_RUN && kw <= i - (CONV_RUN - 1)) break;
#pragma unroll
            for (int k = i; k < i + 2; ++k) {
                const uint32_t w = in[k];
                ch[k][0] = (int32_t)(w & 0xffu); ch[k][1] = (int32_t)((w >> 8) & 0xffu); ch[k][2] = (int32_t)((w >> 16) & 0xffu); ch[k][3] = (int32_t)(w >> 24);
            }
        }
#pragma unroll
        for (int t = 0; t < CONV_MAX_DIM; ++t) {
            if (t >= kw) break;
            if (f[t] == 0) continue;
#pragma unroll
            for (int o = 0; o < CONV_RUN; ++o)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[o][c] += __mul24(f[t], ch[o + t][c]);
        }
    }
    const int y = y0 + ry, x = x0 + CONV_RUN * l;
    if (y >= height || x >= width) return;
    uint32_t out[CONV_RUN];
#pragma unroll
    for (int o = 0; o < CONV_RUN; ++o) {
        const uint32_t b0 = conv_byte(acc[o][0]), b1 = conv_byte(acc[o][1]), b2 = conv_byte(acc[o][2]), b3 = conv_byte(acc[o][3]);
        out[o] = RGBA ? (b2 | (b1 << 8) | (b0 << 16) | (b3 << 24)) : (b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
    }
    uint32_t* p = dst + (size_t)y * width + x;
    if (wide & CONV_WIDE_OUT) {
        *reinterpret_cast<uint4*>(p) = make_uint4(out[0], out[1], out[2], out[3]);     // (the width is a multiple of four: the run is inside)
    } else {
#pragma unroll
        for (int o = 0; o < CONV_RUN; ++o)
            if (x + o < width) p[o] = out[o];
    }
}

__global__ __launch_bounds__(CONV_THREADS) void k_convolve_fb(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int kw, int kh,
                                                              int wide, ConvTaps taps) {
    __shared__ uint32_t tile[CONV_ROWS * CONV_PITCH + 8];       // (+ 8: a lane of the last row may read a word or two past it that it does not use)
    convolve_tile<true>(tile, src, dst, width, height, kw, kh, wide, taps);
}
__global__ __launch_bounds__(CONV_THREADS) void k_convolve_tex(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int kw, int kh,
                                                               int wide, ConvTaps taps) {
    __shared__ uint32_t tile[CONV_ROWS * CONV_PITCH + 8];       // (+ 8: a lane of the last row may read a word or two past it that it does not use)
    convolve_tile<false>(tile, src, dst, width, height, kw, kh, wide, taps);
}

// one pass of the kernel `k` (checked by the caller: kernel_valid) over the width x height image `src` into `dst`, another buffer; rgba:
// `src` holds framebuffer words.  `dst` holds ARGB texels either way
void launch_convolve(hipStream_t st, const uint32_t* src, uint32_t* dst, uint32_t width, uint32_t height, const swfr_kernel& k, bool rgba) {
    if (!width || !height || k.width < 1u || k.width > CONV_MAX_DIM || k.height < 1u || k.height > CONV_MAX_DIM) return;
    ConvTaps taps{};
    for (uint32_t j = 0; j < k.height; ++j)
        for (uint32_t i = 0; i < k.width; ++i) taps.t[j * CONV_TAP_PITCH + i] = k.taps[j * k.width + i];
    const bool quads = (width & 3u) == 0u;
    const int wide = (quads && (reinterpret_cast<uintptr_t>(src) & 15u) == 0u ? CONV_WIDE_IN : 0) | (quads && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u ? CONV_WIDE_OUT : 0);
    const dim3 grid((width + CONV_TILE_W - 1) / CONV_TILE_W, (height + CONV_TILE_H - 1) / CONV_TILE_H);
    if (rgba) hipLaunchKernelGGL(k_convolve_fb, grid, dim3(CONV_THREADS), 0, st, src, dst, (int)width, (int)height, (int)k.width, (int)k.height, wide, taps);
    else hipLaunchKernelGGL(k_convolve_tex, grid, dim3(CONV_THREADS), 0, st, src, dst, (int)width, (int)height, (int)k.width, (int)k.height, wide, taps);
}

}  // namespace swfr
