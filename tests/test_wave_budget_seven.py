"""The register budget of k2_tiles' solid instance at seven wavefronts per SIMD, from the compiler's own resource remarks
(tools/kernel_resources.py: one device-only compile for gfx950, no GPU).

The bounds are allocation arithmetic, not measurements.  Vector registers are handed out in blocks of 8 from 512 per SIMD: 7 x 72 =
504 fits, 7 x 80 does not.  Scalar registers are handed out in blocks of 16 plus 16: 96 is the most that seven wavefronts get.  A CU's
four SIMDs then hold 28 wavefronts, each a workgroup of its own with its own LDS: 28 x the kernel's LDS size must fit the CU's
160 KB.  The kernel may not pay with scratch or spilled registers -- a spilled scalar register is a lane of one more vector register.
Everything else stays what it was: the tile instances 1 to 7 and every row and bin kernel have exactly the lines of the parent of
this change (profiles/w7_kernel_resources_parent.txt)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "profiles", "w7_kernel_resources_parent.txt")
LDS_PER_CU = 160 * 1024
TILE_INSTANCES = ("k2_tiles_bitmap_b", "k2_tiles_shaded_b", "k2_tiles_blend_b", "k2_tiles_layer_b", "k2_tiles_mask_b", "k2_tiles_fade_b", "k2_tiles_alpha_b")


def _parse(lines):
    out = {}
    for l in lines:
        if l.strip() and not l.startswith("#"):
            f = l.split()
            out[f[0]] = {k: int(v) for k, v in (x.split("=") for x in f[1:])}
    return out


@pytest.fixture(scope="module")
def now():
    from swf_renderer_amd import build as b
    try:
        hipcc = b.hipcc()
    except Exception:
        hipcc = None
    if not hipcc or not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is missing")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return _parse(kernel_resources.listing())


@pytest.fixture(scope="module")
def parent():
    with open(PARENT) as f:
        return _parse(f)


def test_the_solid_tile_kernel_fits_seven_wavefronts_per_simd(now):
    k = now["k2_tiles_solid_b"]
    print("k2_tiles_solid_b", k)
    assert k["VGPRs"] <= 72, k
    assert k["TotalSGPRs"] <= 96, k
    assert k["ScratchSize"] == 0 and k["VGPRsSpill"] == 0 and k["SGPRsSpill"] == 0, k
    assert k["Occupancy"] >= 7, k


def test_twenty_eight_wavefronts_fit_a_cus_lds(now):
    k = now["k2_tiles_solid_b"]
    assert 28 * k["LDSSize"] <= LDS_PER_CU, k


def test_the_other_tile_instances_are_the_parents(now, parent):
    assert len(TILE_INSTANCES) == 7 and set(TILE_INSTANCES) <= set(parent)
    for name in TILE_INSTANCES:
        assert now[name] == parent[name], (name, now[name], parent[name])


def test_every_row_and_bin_kernel_is_the_parents(now, parent):
    names = sorted(n for n in parent if n.startswith("k2_rows") or n.startswith("k2_bin"))
    assert "k2_rows_b" in names and "k2_rows_wide_b" in names and "k2_bin_b" in names and "k2_bin_small_b" in names, names
    for name in names:
        assert now[name] == parent[name], (name, now[name], parent[name])
