// pixman_ops.hip -- pixman's packed 8-bit operators on a premultiplied 32-bit pixel (included inside namespace swfr by
// raster_common.hip and by shadow_inner.hip; not a translation unit of its own).
__device__ __forceinline__ uint32_t add8x2_sat(uint32_t a, uint32_t b) {
    uint32_t t = a + b;
    t |= 0x1000100u - ((t >> 8) & 0xff00ffu);
    return t & 0xff00ffu;
}
// pixman UN8x4_MUL_UN8 (0x80 rounding) and OVER
__device__ __forceinline__ uint32_t mul_un8(uint32_t x, uint32_t a) {
    uint32_t rb = (x & 0xff00ffu) * a + 0x800080u;
    rb = ((rb + ((rb >> 8) & 0xff00ffu)) >> 8) & 0xff00ffu;
    uint32_t ag = ((x >> 8) & 0xff00ffu) * a + 0x800080u;
    ag = ((ag + ((ag >> 8) & 0xff00ffu)) >> 8) & 0xff00ffu;
    return rb | (ag << 8);
}
__device__ __forceinline__ uint32_t over_pixel(uint32_t src, uint32_t dst) {
    const uint32_t m = mul_un8(dst, 255u - (src >> 24));
    const uint32_t rb = add8x2_sat(m & 0xff00ffu, src & 0xff00ffu);
    const uint32_t ag = add8x2_sat((m >> 8) & 0xff00ffu, (src >> 8) & 0xff00ffu);
    return rb | (ag << 8);
}
