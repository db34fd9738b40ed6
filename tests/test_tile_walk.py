"""The packed 16-bit form of k2_tiles' rounded products (csrc/raster2.hip mul8x2_7f_24, mul_un8_24; csrc/raster_common.hip pk_*)
against the masked 32-bit form it replaced, for all 65 536 (channel, factor) pairs and both roundings: the same integers, and no
intermediate of a half leaves sixteen bits -- which is all the packed instructions need, since neither half sees the other."""
import numpy as np
import pytest


def _masked32(lo, hi, f, rnd):
    """two channels in the 0x00ff00ff layout times an 8-bit factor, as one 32-bit product with masks between the steps"""
    x = (lo | (hi << 16)).astype(np.uint64)
    t = (x * f + (rnd | (rnd << 16))) & 0xffffffff
    return (((t + ((t >> 8) & 0xff00ff)) & 0xffffffff) >> 8) & 0xff00ff


def _packed16(lo, hi, f, rnd):
    """the same through v_pk_mad_u16, v_pk_lshrrev_b16, v_pk_add_u16, v_pk_lshrrev_b16: each half modulo 2^16 on its own"""
    out = []
    for c in (lo, hi):
        t = (c.astype(np.uint64) * f + rnd) & 0xffff
        out.append((((t + (t >> 8)) & 0xffff) >> 8))
    return out[0] | (out[1] << 16)


@pytest.mark.parametrize("rnd", [0x7f, 0x80], ids=["lerp_0x7f", "over_0x80"])
def test_packed_products_equal_the_masked_ones(rnd):
    c, f = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(256, dtype=np.uint64), indexing="ij")
    c, f = c.ravel(), f.ravel()
    # the channel under test in either half, the extreme neighbours in the other: nothing crosses between the halves
    for other in (np.zeros_like(c), np.full_like(c, 255), 255 - c):
        for lo, hi in ((c, other), (other, c)):
            assert (_packed16(lo, hi, f, rnd) == _masked32(lo, hi, f, rnd)).all()
    # the claimed bounds: every intermediate fits sixteen bits, so the modulo above never acts
    t = c * f + rnd
    assert int(t.max()) == 255 * 255 + rnd < 1 << 16
    assert int((t + (t >> 8)).max()) == 255 * 255 + rnd + 254 < 1 << 16
    # and the result is the rounded quotient the blends are specified by: (x + rnd + ((x + rnd) >> 8)) >> 8 of x = channel * factor
    assert ((_packed16(c, c, f, rnd) & 0xffff) == ((t + (t >> 8)) >> 8)).all() and int(((t + (t >> 8)) >> 8).max()) == 255
