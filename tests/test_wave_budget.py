"""The register budget of the two hot kernels, from the compiler's own resource remarks (tools/kernel_resources.py: one device-only
compile for gfx950, no GPU).

Vector registers are handed out in blocks of 8 from 512 per SIMD.  A wavefront of k2_tiles_solid_b with at most 80 of them fits six
times (6 x 80 = 480), with 81 it is charged 88 and fits five times: the bound 80 is that arithmetic, not a measurement.  The kernel
may not pay for it with scratch or spilled registers -- a spilled scalar register is a lane of one more vector register.  k2_rows_b
stays the parent's (89 registers, charged 96: beside 80-register tile wavefronts a SIMD holds the mixes (6,0), (5,1) and (4,2)), and
no other kernel may get worse than the parent of this change (profiles/w6_kernel_resources_parent.txt) in scratch, spilled vector
registers or wavefronts per SIMD."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "profiles", "w6_kernel_resources_parent.txt")
HOT = ("k2_tiles_solid_b", "k2_rows_b")


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


def test_the_solid_tile_kernel_fits_six_wavefronts_per_simd(now):
    k = now["k2_tiles_solid_b"]
    print("k2_tiles_solid_b", k)
    assert k["VGPRs"] <= 80, k
    assert k["ScratchSize"] == 0 and k["VGPRsSpill"] == 0 and k["SGPRsSpill"] == 0, k
    assert k["Occupancy"] >= 6, k


def test_the_row_kernel_is_the_parents(now, parent):
    """The 88-register variant of k2_rows_b (the header stores reading `rows` where they are used) measured no gain beside the six
    tile wavefronts and was not shipped (profiles/w6_tables.md): the kernel's line is the parent's."""
    print("k2_rows_b", now["k2_rows_b"])
    assert now["k2_rows_b"] == parent["k2_rows_b"], (now["k2_rows_b"], parent["k2_rows_b"])


def test_no_other_kernel_got_worse(now, parent):
    assert set(parent) <= set(now), sorted(set(parent) - set(now))
    worse = []
    for name, p in sorted(parent.items()):
        if name in HOT:
            continue
        k = now[name]
        if k["ScratchSize"] > p["ScratchSize"] or k["VGPRsSpill"] > p["VGPRsSpill"] or k["Occupancy"] < p["Occupancy"]:
            worse.append((name, p, k))
    assert not worse, worse


def test_the_wide_row_kernel_is_the_parents(now, parent):
    """163 vector registers, three wavefronts per SIMD, no scratch"""
    k, p = now["k2_rows_wide_b"], parent["k2_rows_wide_b"]
    assert k["VGPRs"] <= p["VGPRs"] and k["ScratchSize"] == 0 and k["Occupancy"] >= p["Occupancy"], (k, p)
