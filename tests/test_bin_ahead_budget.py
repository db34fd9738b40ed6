"""The compiler's resource lines for k2_rows_ahead_b, the row launch that also bins the next frame ("k2_bin of the next
frame in the row launch"), and for every kernel beside it.  No GPU: tools/kernel_resources.py compiles raster2.hip for gfx950 and reads
the remarks.

* the fused kernel: no more VGPRs than k2_rows_b, five wavefronts per SIMD, no scratch, no spilled register, at most 8 192 bytes of LDS
  (twenty row wavefronts of a CU then still fit its 160 KB beside the tile wavefronts);
* every other kernel: its line equals profiles/ahead_kernel_resources_parent.txt, the listing of the commit before, field for field."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARENT = os.path.join(ROOT, "profiles", "ahead_kernel_resources_parent.txt")
FUSED = "k2_rows_ahead_b"


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


@pytest.fixture(scope="module")
def lines():
    import shutil
    from swf_renderer_amd import build as b
    try:
        hipcc = b.hipcc()
    except Exception:
        hipcc = None
    if not hipcc or not (os.path.exists(hipcc) or shutil.which(hipcc)):     # (as the other budget tests: no compiler, nothing to read)
        pytest.skip("hipcc is missing")
    import kernel_resources
    return {l.split()[0]: l for l in kernel_resources.listing()}


def test_the_fused_kernel_keeps_the_row_kernels_budget(lines):
    assert FUSED in lines, sorted(lines)
    fused, rows = _fields(lines[FUSED]), _fields(lines["k2_rows_b"])
    print(lines[FUSED])
    print(lines["k2_rows_b"])
    assert int(fused["VGPRs"]) <= int(rows["VGPRs"]), (fused, rows)
    assert int(fused["Occupancy"]) == 5, fused
    assert int(fused["ScratchSize"]) == 0 and int(fused["VGPRsSpill"]) == 0, fused      # (k2_rows_b itself parks two SGPRs in VGPR lanes; no memory is involved)
    assert int(fused["LDSSize"]) <= 8192, fused
    assert int(fused["AGPRs"]) == 0, fused


def test_every_other_kernel_keeps_its_line(lines):
    parent = {l.split()[0]: l.split()[1:] for l in open(PARENT) if l.strip() and not l.startswith("#")}
    assert "k2_rows_b" in parent and "k2_bin_small_b" in parent and "k2_tiles_solid_b" in parent
    assert FUSED not in parent
    for name, want in parent.items():
        assert name in lines, "kernel %s is gone" % name
        assert lines[name].split()[1:] == want, (name, want, lines[name])
    assert sorted(set(lines) - set(parent)) == [FUSED]
