"""The compiler's resource remarks of every kernel in csrc/raster2.hip (gfx950; needs hipcc, no GPU): SGPRs, VGPRs, scratch,
spills, LDS, occupancy -- one line per kernel.  A pull request that must leave existing kernels alone compares this listing before
and after (profiles/blend_kernel_resources.txt).  listing() is raster2.hip's, the unit the budget tests hold; listing(unit) is that
of another device translation unit of the build (shadow_inner.hip), and the command line lists them all, raster2.hip first.

usage: python tools/kernel_resources.py [-o listing.txt] [--diff older_listing.txt]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


_LISTING = {}                                                          # (one compile per unit and process, however many callers)


def device_units():
    from swf_renderer_amd import build as b
    return [s for s in b.SOURCES if s.endswith(".hip")]


def listing(unit="raster2.hip"):
    if unit not in _LISTING:
        _LISTING[unit] = _compile_listing(unit)
    return list(_LISTING[unit])


def _compile_listing(unit):
    from swf_renderer_amd import build as b
    src = os.path.join(b.CSRC, unit)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [b.hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DSWFR_BUILD",
               "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "dev.o"), "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, stderr=subprocess.PIPE, check=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip() or m.group(1)
            cur = out.setdefault(name.split("(")[0].replace("swfr::", ""), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return ["%-22s %s" % (k, "  ".join("%s=%s" % (f.split(" [")[0].replace(" ", ""), v.get(f, "?")) for f in FIELDS)) for k, v in sorted(out.items())]


def main():
    lines = [l for unit in device_units() for l in listing(unit)]
    text = "\n".join(lines) + "\n"
    if "-o" in sys.argv:
        open(sys.argv[sys.argv.index("-o") + 1], "w").write(text)
    sys.stdout.write(text)
    if "--diff" in sys.argv:
        old = {l.split()[0]: l.split()[1:] for l in open(sys.argv[sys.argv.index("--diff") + 1]) if l.strip() and not l.startswith("#")}
        bad = 0
        for l in lines:
            k, v = l.split()[0], l.split()[1:]
            if k not in old:
                print("new kernel:", k)
            elif old[k] != v:
                print("CHANGED:", k, old[k], "->", v)
                bad += 1
        print("existing kernels unchanged" if not bad else "%d existing kernels changed" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
