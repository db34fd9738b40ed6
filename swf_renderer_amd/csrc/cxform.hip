// cxform.hip -- the texel pass of colour-transformed bitmaps (included by raster2.hip, not a translation unit of its own).
//
// A bitmap fill under a non-identity colour-transform chain samples a texture of its own: the bitmap's straight RGBA8 texels as
// registered, every channel mapped through the chain's table, then premultiplied exactly as putImageData does it (c * a / 255,
// truncating) into the premultiplied ARGB words the tile kernel's bitmap shader reads.  The host points the style's DevFilter::pixels
// at that texture (renderer.cpp, resolve_variants), so k2_tiles does not know the difference.
//
//   k_cxform_texels   a streaming pass over the texels as one flat tight array: the chain (4 x 256 bytes, packed as 256 words
//                     r | g << 8 | b << 16 | a << 24, in device memory behind the texture) is staged in LDS as four tables of words; each lane moves 16-byte loads
//                     and stores (four texels) in a grid-stride loop, four vectors in flight per lane; the last n % 4 texels go word by
//                     word.  Reads 4 and writes 4 bytes per texel.

#define CX_THREADS 256
#define CX_UNROLL 4

// c * a / 255 for c, a in 0..255, truncating, as (x + 1 + (x >> 8)) >> 8 of x = c * a: exact on that domain (tests/test_color_transform.py
// checks all 65 536 pairs)
__device__ __forceinline__ uint32_t cx_mul_div255(uint32_t c, uint32_t a) {
    const uint32_t x = c * a;
    return (x + 1u + (x >> 8)) >> 8;
}

// one straight RGBA8 texel (r in the low byte) -> premultiplied ARGB of its transformed colour.  The four tables are whole words in LDS
// on purpose: with bytes the compiler knows to be bytes (a packed table, masked), the compiler for gfx950 (ROCm 7) fuses the channels'
// products into v_dot4_u32_u8 and gets them wrong -- twice the value, measured on an MI355X; words loaded from LDS keep the products
// plain 32-bit multiplies.
__device__ __forceinline__ uint32_t cx_texel(const uint32_t (*lut)[256], uint32_t w) {
    const uint32_t r = lut[0][w & 255u], g = lut[1][(w >> 8) & 255u], b = lut[2][(w >> 16) & 255u], a = lut[3][w >> 24];
    return (a << 24) | (cx_mul_div255(r, a) << 16) | (cx_mul_div255(g, a) << 8) | cx_mul_div255(b, a);
}

__device__ __forceinline__ uint4 cx_vec(const uint32_t (*lut)[256], uint4 v) {
    return make_uint4(cx_texel(lut, v.x), cx_texel(lut, v.y), cx_texel(lut, v.z), cx_texel(lut, v.w));
}

__global__ __launch_bounds__(CX_THREADS) void k_cxform_texels(const uint4* __restrict__ in, uint4* __restrict__ out, size_t n_vec,
                                                              const uint32_t* __restrict__ tail_in, uint32_t* __restrict__ tail_out,
                                                              uint32_t n_tail, const uint32_t* __restrict__ chain) {
    __shared__ uint32_t lut[4][256];
    const uint32_t t = chain[threadIdx.x];
    lut[0][threadIdx.x] = t & 255u;
    lut[1][threadIdx.x] = (t >> 8) & 255u;
    lut[2][threadIdx.x] = (t >> 16) & 255u;
    lut[3][threadIdx.x] = t >> 24;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * CX_THREADS;
    size_t i = (size_t)blockIdx.x * CX_THREADS + threadIdx.x;
    for (; i + (CX_UNROLL - 1) * stride < n_vec; i += CX_UNROLL * stride) {
        uint4 v[CX_UNROLL];
#pragma unroll
        for (int k = 0; k < CX_UNROLL; ++k) v[k] = in[i + k * stride];
#pragma unroll
        for (int k = 0; k < CX_UNROLL; ++k) out[i + k * stride] = cx_vec(lut, v[k]);
    }
    for (; i < n_vec; i += stride) out[i] = cx_vec(lut, in[i]);
    if (blockIdx.x == 0 && threadIdx.x < n_tail) tail_out[threadIdx.x] = cx_texel(lut, tail_in[threadIdx.x]);
}

// n texels of straight RGBA8 at `straight` (16-byte aligned) -> n premultiplied ARGB words at `out` (16-byte aligned); `chain`: the 256
// packed table words in device memory (entry c: the chain's value of c in channel r (bits 0-7), g, b, a (bits 24-31))
void launch_cxform_texels(hipStream_t st, const uint8_t* straight, uint32_t* out, size_t n, const uint32_t* chain) {
    if (!n) return;
    const size_t n_vec = n / 4;
    const uint32_t n_tail = (uint32_t)(n % 4);
    // enough workgroups to fill every CU several times over, each lane then loops (the table is staged once per workgroup)
    const size_t want = (n_vec + CX_THREADS - 1) / CX_THREADS;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    hipLaunchKernelGGL(k_cxform_texels, dim3(blocks), dim3(CX_THREADS), 0, st, reinterpret_cast<const uint4*>(straight),
                       reinterpret_cast<uint4*>(out), n_vec, reinterpret_cast<const uint32_t*>(straight) + n_vec * 4, out + n_vec * 4,
                       n_tail, chain);
}
