"""Static instruction counts of the compiled row pass (k2_rows_b, k2_rows_wide_b; gfx950; needs hipcc, no GPU).

The library's own flags plus --cuda-device-only -S give the compiler's listing.  Two compilations:
  * the plain one: whole-kernel counts, code size and registers -- what ships;
  * one with -DR3_MARKS: the listing cut at the region markers of csrc/rows3.hip (R3MARK(1) .. (11)).  A marker is a position in the
    LISTING: the compiler may move an instruction across one, and a region's count says nothing of how often it runs.
Counts are of static instructions.  `vector` = v_*, `scalar` = s_* without s_waitcnt / s_nop / branches, `mem` = ds_* / global_* / flat_* /
buffer_* / scratch_*, `mask` = 64-bit scalar logic, selects and moves (lane masks) including *_saveexec, `mov k` = v_mov_b32 of a constant.

usage: python tools/rows_regions.py [--csrc DIR] [-o table.md] [--against older_table.md]
  --csrc DIR      compile DIR/raster2.hip instead of this tree's (a checkout of the parent commit)
  --against FILE  compare the whole-kernel lines with those of FILE (written by -o) and fail where a count the change must not raise rose
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k2_rows_b", "k2_rows_wide_b")
COLS = ("vector", "scalar", "mem", "s_load", "s_waitcnt", "lgkmcnt(0)", "v_cndmask", "v_mov", "mov k", "v_cmp", "mask", "saveexec", "branch")
REGIONS = {0: "prologue: chunk, path, band records", 1: "stage the edges", 2: "edges' row masks", 3: "rows' edge masks, nmax", 4: "evaluate slots",
           5: "sort, ties, roles", 6: "room", 7: "FULL cells", 8: "FULL masks, clear staging", 9: "sample passes", 10: "headers, slow queue", 11: "classification"}
MASK_OPS = re.compile(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor|not|mov|cselect)_b64\b|s_\w+_saveexec_b64\b")


def compile_listing(csrc, marks):
    from swf_renderer_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        cmd = [b.hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "-fno-fast-math",
               "-Wno-unused-function", "-DSWFR_BUILD", "--cuda-device-only", "-S", os.path.join(csrc, "raster2.hip"), "-o", out]
        if marks:
            cmd.append("-DR3_MARKS")
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        return open(out).read().splitlines()


def kernel_lines(lines, name):
    """the listing of one kernel: from its label to its .Lfunc_end, and its resource comments"""
    body, info, on = [], {}, False
    for l in lines:
        if not on:
            if re.match(r"_ZN4swfr%d%sE\w*:" % (len(name), name), l):
                on = True
            continue
        if l.startswith(".Lfunc_end"):
            on = "tail"
            continue
        if on == "tail":
            m = re.match(r";\s*(codeLenInByte|NumVgprs|TotalNumSgprs|Occupancy)\s*[:=]\s*(\d+)", l)
            if m:
                info[m.group(1)] = int(m.group(2))
            if l.startswith("; Occupancy") or l.startswith("\t.globl"):
                break
            continue
        body.append(l)
    return body, info


def count(body):
    """{region: {column: count}}; the region is the last marker seen"""
    out, reg = {}, 0
    for l in body:
        m = re.search(r"; R3MARK (\d+)", l)
        if m:
            reg = int(m.group(1))
            continue
        t = l.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        c = out.setdefault(reg, dict.fromkeys(COLS, 0))
        if op.startswith("v_"):
            c["vector"] += 1
            if op.startswith("v_cndmask"):
                c["v_cndmask"] += 1
            elif op.startswith("v_mov_b32"):
                c["v_mov"] += 1
                src = t.split(",")[-1].split(";")[0].strip()
                if not re.match(r"[vs]\d|[vs]\[|vcc|exec|ttmp|m0", src):
                    c["mov k"] += 1
            elif op.startswith("v_cmp"):
                c["v_cmp"] += 1
        elif op.startswith(("ds_", "global_", "flat_", "buffer_", "scratch_")):
            c["mem"] += 1
        elif op.startswith("s_"):
            if op == "s_waitcnt":
                c["s_waitcnt"] += 1
                if "lgkmcnt(0)" in t:
                    c["lgkmcnt(0)"] += 1
            elif op.startswith(("s_cbranch", "s_branch")):
                c["branch"] += 1
            elif op in ("s_nop", "s_endpgm", "s_barrier"):
                pass
            else:
                c["scalar"] += 1
                if op.startswith("s_load"):
                    c["s_load"] += 1
                if MASK_OPS.match(op):
                    c["mask"] += 1
                if "saveexec" in op:
                    c["saveexec"] += 1
    return out


def total(regs, first=0):
    t = dict.fromkeys(COLS, 0)
    for r, c in regs.items():
        if r >= first:
            for k in COLS:
                t[k] += c[k]
    return t


def table(csrc):
    plain, marked = compile_listing(csrc, False), compile_listing(csrc, True)
    L = []
    for k in KERNELS:
        body, info = kernel_lines(plain, k)
        t = total(count(body))
        L.append("`%s`, whole kernel as shipped: %d B of code, %d VGPRs, %d SGPRs, %d waves/SIMD (scratch: tools/kernel_resources.py); vector + scalar = %d" % (
            k, info.get("codeLenInByte", 0), info.get("NumVgprs", 0), info.get("TotalNumSgprs", 0), info.get("Occupancy", 0), t["vector"] + t["scalar"]))
        L.append("")
        L.append("| `%s` | %s |" % (k, " | ".join(COLS)))
        L.append("|---|%s" % ("---|" * len(COLS)))
        L.append("| whole kernel | %s |" % " | ".join("%d" % t[c] for c in COLS))
        mbody, minfo = kernel_lines(marked, k)
        regs = count(mbody)
        for r in sorted(regs):
            L.append("| %d %s | %s |" % (r, REGIONS.get(r, ""), " | ".join("%d" % regs[r][c] for c in COLS)))
        tm, tp = total(regs), total(regs, 1)
        L.append("| with markers: all regions (%d B) | %s |" % (minfo.get("codeLenInByte", 0), " | ".join("%d" % tm[c] for c in COLS)))
        L.append("| with markers: after the prologue (1 ..) | %s |" % " | ".join("%d" % tp[c] for c in COLS))
        L.append("")
    return L


def whole(path):
    """{kernel: {column: count}} of the `whole kernel` and `after the prologue` lines of a table written by -o"""
    out, cur = {}, None
    for l in open(path):
        m = re.match(r"\| `(\w+)` \|", l)
        if m:
            cur = m.group(1)
        for key, tagname in (("| whole kernel |", "whole"), ("| with markers: after the prologue (1 ..) |", "post")):
            if l.startswith(key) and cur:
                v = [int(x) for x in l[len(key):].strip().strip("|").split("|")]
                out[(cur, tagname)] = dict(zip(COLS, v))
    return out


def main():
    csrc = sys.argv[sys.argv.index("--csrc") + 1] if "--csrc" in sys.argv else os.path.join(ROOT, "swf_renderer_amd", "csrc")
    L = table(os.path.abspath(csrc))
    text = "\n".join(L) + "\n"
    sys.stdout.write(text)
    if "-o" in sys.argv:
        open(sys.argv[sys.argv.index("-o") + 1], "w").write(text)
    if "--against" in sys.argv:
        old = whole(sys.argv[sys.argv.index("--against") + 1])
        tmp = tempfile.NamedTemporaryFile("w", suffix=".md", delete=False)
        tmp.write(text)
        tmp.close()
        new = whole(tmp.name)
        os.unlink(tmp.name)
        bad = 0
        for k in KERNELS:
            o, n, op, np_ = old[(k, "whole")], new[(k, "whole")], old[(k, "post")], new[(k, "post")]
            checks = (("vector + scalar must fall", o["vector"] + o["scalar"], n["vector"] + n["scalar"], lambda a, b: b < a),
                      ("s_load after the prologue must fall", op["s_load"], np_["s_load"], lambda a, b: b < a),
                      ("v_mov of a constant must not rise", o["mov k"], n["mov k"], lambda a, b: b <= a),
                      ("mask ops must not rise", o["mask"], n["mask"], lambda a, b: b <= a))
            for what, a, b, ok in checks:
                good = ok(a, b)
                bad += not good
                print("%-16s %-38s %6d -> %6d  %s" % (k, what, a, b, "ok" if good else "NOT MET"))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
