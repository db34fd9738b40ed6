// blur.hip -- box blur of a group's texture (included by raster2.hip, not a translation unit of its own).  DESIGN.md, "Blurred layers".
//
// One 1-D pass of box width w (2..255) is what pixman 0.40 computes for PIXMAN_FILTER_CONVOLUTION with w equal taps of
// f = (65536 + w / 2) / w over a premultiplied ARGB image, EXTEND_NONE: per channel, alpha included,
//     out = min(255, (f * S + 0x8000) >> 16),   S = the sum of the channel over the window [x - w / 2, x - w / 2 + w - 1],
// a tap outside the image reading 0.  All taps are equal, so pixman's sum of products is f * S and a running sum is exact.  S is at most
// 255 * 255 = 65 025: the sums of two channels travel in the halves of one 32-bit word (b | r << 16 and g | a << 16; a window is
// added before the pixel that leaves it is subtracted, so no half ever borrows), and f * S + 0x8000 < 2^32 for every w >= 2.
//
//   k_blur_capture   premultiplied RGBA8 framebuffer words (r in the low byte) -> the premultiplied ARGB words textures hold: a streaming pass.
//   k_blur_h         a workgroup blurs BLUR_H_SEG pixels of BLUR_H_ROWS rows: the segment and its apron of w - 1 pixels (up to 254, more
//                    than a lane's run) are staged through LDS by coalesced loads; a wavefront then owns one row, a lane a run of BLUR_H_RUN
//                    pixels -- it sums one whole window, then slides it --, the results go back through LDS to coalesced stores.  A pixel
//                    j of the staged row lives at word j + j / 16: the lanes' runs start 17 words apart, on 64 different banks.
//   k_blur_v         lanes run along x; a lane owns BLUR_V_SEG rows of its column: one whole window summed from global memory, then one
//                    row added and one subtracted per pixel, every access a row segment of consecutive words.
// The work per pixel does not grow with w: only the first pixel of a run sums a window.

#define BLUR_THREADS 256
#define BLUR_H_SEG 1024
#define BLUR_H_ROWS 4
#define BLUR_H_RUN 16
#define BLUR_MAX_W 255
#define BLUR_H_STAGED (BLUR_H_SEG + BLUR_MAX_W - 1)
#define BLUR_H_PITCH (BLUR_H_STAGED + BLUR_H_STAGED / 16 + 1)
#define BLUR_V_SEG 64
static_assert(BLUR_H_ROWS * (BLUR_H_SEG / BLUR_H_RUN) == BLUR_THREADS, "a lane per run");

__device__ __forceinline__ uint32_t blur_slot(uint32_t j) { return j + (j >> 4); }
__device__ __forceinline__ uint32_t blur_lo(uint32_t p) { return p & 0x00ff00ffu; }            // b | r << 16
__device__ __forceinline__ uint32_t blur_hi(uint32_t p) { return (p >> 8) & 0x00ff00ffu; }     // g | a << 16
__device__ __forceinline__ uint32_t blur_channel(uint32_t s, uint32_t f) {
    const uint32_t v = (f * s + 0x8000u) >> 16;
    return v > 255u ? 255u : v;
}
// the pixel of the window sums lo = Sb | Sr << 16, hi = Sg | Sa << 16
__device__ __forceinline__ uint32_t blur_pixel(uint32_t lo, uint32_t hi, uint32_t f) {
    return blur_channel(lo & 0xffffu, f) | (blur_channel(hi & 0xffffu, f) << 8) | (blur_channel(lo >> 16, f) << 16) | (blur_channel(hi >> 16, f) << 24);
}

__global__ __launch_bounds__(BLUR_THREADS) void k_blur_capture(const uint32_t* __restrict__ fb, uint32_t* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * BLUR_THREADS;
    for (size_t i = (size_t)blockIdx.x * BLUR_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t p = fb[i];
        out[i] = (p & 0xff00ff00u) | ((p & 0xffu) << 16) | ((p >> 16) & 0xffu);
    }
}

__global__ __launch_bounds__(BLUR_THREADS) void k_blur_h(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int w, uint32_t f) {
    __shared__ uint32_t row[BLUR_H_ROWS][BLUR_H_PITCH];
    const int x0 = (int)blockIdx.x * BLUR_H_SEG, y0 = (int)blockIdx.y * BLUR_H_ROWS;
    const int staged = BLUR_H_SEG + w - 1, left = x0 - w / 2;
    for (int r = 0; r < BLUR_H_ROWS; ++r) {
        const int y = y0 + r;
        for (int j = (int)threadIdx.x; j < staged; j += BLUR_THREADS) {
            const int x = left + j;
            row[r][blur_slot((uint32_t)j)] = (y < height && x >= 0 && x < width) ? src[(size_t)y * width + x] : 0u;
        }
    }
    __syncthreads();
    const int r = (int)threadIdx.x / (BLUR_H_SEG / BLUR_H_RUN), j0 = ((int)threadIdx.x % (BLUR_H_SEG / BLUR_H_RUN)) * BLUR_H_RUN;
    const uint32_t* in = row[r];
    uint32_t lo = 0u, hi = 0u;
    for (int k = 0; k < w; ++k) { const uint32_t p = in[blur_slot((uint32_t)(j0 + k))]; lo += blur_lo(p); hi += blur_hi(p); }
    uint32_t o[BLUR_H_RUN];
    o[0] = blur_pixel(lo, hi, f);
#pragma unroll
    for (int i = 1; i < BLUR_H_RUN; ++i) {
        const uint32_t a = in[blur_slot((uint32_t)(j0 + i + w - 1))], b = in[blur_slot((uint32_t)(j0 + i - 1))];
        lo += blur_lo(a); hi += blur_hi(a);
        lo -= blur_lo(b); hi -= blur_hi(b);
        o[i] = blur_pixel(lo, hi, f);
    }
    __syncthreads();                                   // every lane has read its windows: the staged pixels make way for the results
#pragma unroll
    for (int i = 0; i < BLUR_H_RUN; ++i) row[r][blur_slot((uint32_t)(j0 + i))] = o[i];
    __syncthreads();
    for (int q = 0; q < BLUR_H_ROWS; ++q) {
        const int y = y0 + q;
        if (y >= height) break;
        for (int j = (int)threadIdx.x; j < BLUR_H_SEG; j += BLUR_THREADS) {
            const int x = x0 + j;
            if (x < width) dst[(size_t)y * width + x] = row[q][blur_slot((uint32_t)j)];
        }
    }
}

__global__ __launch_bounds__(BLUR_THREADS) void k_blur_v(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int width, int height, int w, uint32_t f) {
    const int x = (int)blockIdx.x * BLUR_THREADS + (int)threadIdx.x;
    if (x >= width) return;
    const int y0 = (int)blockIdx.y * BLUR_V_SEG, y1 = y0 + BLUR_V_SEG < height ? y0 + BLUR_V_SEG : height;
    const int up = w / 2;
    uint32_t lo = 0u, hi = 0u;
    {
        const int a = y0 - up < 0 ? 0 : y0 - up, b = y0 - up + w < height ? y0 - up + w : height;      // the first window's rows inside the image
        for (int y = a; y < b; ++y) { const uint32_t p = src[(size_t)y * width + x]; lo += blur_lo(p); hi += blur_hi(p); }
    }
    for (int y = y0; y < y1; ++y) {
        dst[(size_t)y * width + x] = blur_pixel(lo, hi, f);
        const int in = y - up + w, out = y - up;                                                       // the row that enters the next window, the row that leaves
        if (in < height) { const uint32_t p = src[(size_t)in * width + x]; lo += blur_lo(p); hi += blur_hi(p); }
        if (out >= 0) { const uint32_t p = src[(size_t)out * width + x]; lo -= blur_lo(p); hi -= blur_hi(p); }
    }
}

// n framebuffer words -> n texture words
void launch_blur_capture(hipStream_t st, const uint32_t* fb, uint32_t* out, size_t n) {
    if (!n) return;
    const size_t want = (n + BLUR_THREADS - 1) / BLUR_THREADS;
    hipLaunchKernelGGL(k_blur_capture, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(BLUR_THREADS), 0, st, fb, out, n);
}
// one pass of box width w (2..255) over the width x height image `src` into `dst` (another buffer), along x (vertical == false) or y
void launch_blur_pass(hipStream_t st, const uint32_t* src, uint32_t* dst, uint32_t width, uint32_t height, uint32_t w, bool vertical) {
    if (!width || !height || w < 2u || w > BLUR_MAX_W) return;
    const uint32_t f = (65536u + w / 2u) / w;
    if (vertical)
        hipLaunchKernelGGL(k_blur_v, dim3((width + BLUR_THREADS - 1) / BLUR_THREADS, (height + BLUR_V_SEG - 1) / BLUR_V_SEG), dim3(BLUR_THREADS), 0, st,
                           src, dst, (int)width, (int)height, (int)w, f);
    else
        hipLaunchKernelGGL(k_blur_h, dim3((width + BLUR_H_SEG - 1) / BLUR_H_SEG, (height + BLUR_H_ROWS - 1) / BLUR_H_ROWS), dim3(BLUR_THREADS), 0, st,
                           src, dst, (int)width, (int)height, (int)w, f);
}
