"""Tables of the k2_bin instance work (profiles/b1_tables.md) from the raw files of one run directory:

  trace_<lib>/**/*kernel_trace.csv      rocprofv3 --kernel-trace of tools/bench_with_lib.py (the bench's own, pipelined mode)
  trace1_<lib>/**/*kernel_trace.csv     the same with SWFR_FRAMES_IN_FLIGHT=1 (one frame in flight)
  bench.txt, order_sweep.txt            "bench <lib> <workload> <steps> <json line>" per run, the libraries alternating
  one_frame.txt, config_bench.txt       "<probe> <lib> <text>" lines: full_bench, short_run_probe, config_bench
  suite.txt, soak.txt                   the last lines of the GPU suite and of tools/soak.py gpu

  python tools/summarize_bin.py reduce <run dir> <out dir> <tag>    the traces cut down to kernel, frames per launch, workgroup, start, end
  python tools/summarize_bin.py tables <dir with the reduced files> <tag>    -> the markdown, to stdout

A launch's frames: Grid_Size_Y / Workgroup_Size_Y (blockIdx.y = frame)."""
import csv
import glob
import json
import os
import statistics
import sys

KERNELS = ("k2_bin_b", "k2_bin_small_b", "k2_rows_b", "k2_tiles_solid_b")


def kernel_of(name):
    name = name.split("(")[0].strip().split("::")[-1]
    return name if name in KERNELS else None


def reduce_trace(src_dir, dst):
    files = sorted(glob.glob(os.path.join(src_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        return False
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                k = kernel_of(r["Kernel_Name"])
                if k:
                    rows.append((int(r["Start_Timestamp"]), k, int(r["Grid_Size_Y"]) // max(int(r["Workgroup_Size_Y"]), 1), int(r["Workgroup_Size_X"]),
                                 int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1), int(r["Queue_Id"]), int(r["End_Timestamp"])))
    rows.sort()
    t0 = rows[0][0] if rows else 0
    with open(dst, "w") as out:
        out.write("kernel,frames,workgroup,blocks_x,queue,start_ns,end_ns\n")
        for s, k, fy, wg, gx, q, e in rows:
            out.write("%s,%d,%d,%d,%d,%d,%d\n" % (k, fy, wg, gx, q, s - t0, e - t0))
    return True


def read_reduced(path):
    with open(path, newline="") as fh:
        return [dict(r, frames=int(r["frames"]), start=int(r["start_ns"]), end=int(r["end_ns"]), queue=int(r["queue"])) for r in csv.DictReader(fh)]


def durations(rows):
    """{(kernel, frames per launch): [us, ...]}"""
    d = {}
    for r in rows:
        d.setdefault((r["kernel"], r["frames"]), []).append((r["end"] - r["start"]) * 1e-3)
    return d


def trace_table(path):
    rows = read_reduced(path)
    out = ["| kernel | frames per launch | launches | median us | p10 | p90 |", "|---|---|---|---|---|---|"]
    for (k, fy), v in sorted(durations(rows).items()):
        v.sort()
        out.append("| %s | %d | %d | %.2f | %.2f | %.2f |" % (k, fy, len(v), statistics.median(v), v[len(v) // 10], v[(len(v) * 9) // 10 - (1 if len(v) >= 10 else 0)]))
    # how much of k2_bin's span another stream's kernel overlaps (the two chains of the pipelined region)
    two = [r for r in rows if r["frames"] == 2]
    if two:
        bins = [r for r in two if r["kernel"].startswith("k2_bin")]
        others = [r for r in two if not r["kernel"].startswith("k2_bin")]
        cov = []
        for b in bins:
            o = sum(max(0, min(b["end"], x["end"]) - max(b["start"], x["start"])) for x in others if x["queue"] != b["queue"])
            cov.append(o / max(b["end"] - b["start"], 1))
        out.append("")
        out.append("Two-frame k2_bin launches: median share of their span during which the other stream's k2_rows or k2_tiles runs: %.0f %%." % (100 * statistics.median(cov)))
    return "\n".join(out)


def bench_table(path):
    runs = {}
    for line in open(path):
        p = line.split(None, 4)
        if len(p) < 5 or p[0] != "bench":
            continue
        try:
            d = json.loads(p[4])
        except ValueError:
            continue
        assert d.get("verified") is True, line[:120]
        runs.setdefault((p[2], int(p[3])), {}).setdefault(p[1], []).append(float(d["ms_per_step"]) * 1e3)
    out = ["| workload, steps | library | runs | us per step: min | median | max | every frame verified |", "|---|---|---|---|---|---|---|"]
    notes = []
    for key in sorted(runs):
        for lib in sorted(runs[key], key=lambda n: (n != "parent", n)):
            v = sorted(runs[key][lib])
            out.append("| %s, %d | %s | %d | %.2f | %.2f | %.2f | yes |" % (key[0], key[1], lib, len(v), v[0], statistics.median(v), v[-1]))
        if "parent" in runs[key]:
            pv = runs[key]["parent"]
            for lib, v in runs[key].items():
                if lib == "parent":
                    continue
                gain = 100 * (1 - statistics.median(v) / statistics.median(pv))
                rel = "below the parent's range" if max(v) < min(pv) else "above the parent's range" if min(v) > max(pv) else "overlaps the parent's range"
                notes.append("- %s, %d steps, %s: median %+.1f %% time per step against the parent (%.2f -> %.2f us); its range [%.2f, %.2f] %s [%.2f, %.2f]." %
                             (key[0], key[1], lib, -gain, statistics.median(pv), statistics.median(v), min(v), max(v), rel, min(pv), max(pv)))
    return "\n".join(out + [""] + notes)


def probes_table(path):
    """full_path and ms_per_step of the whole bench, the fit of tools/short_run_probe.py, tools/config_bench.py: every run's figure, per library"""
    rows = {}
    for line in open(path):
        p = line.split(None, 2)
        if len(p) < 3:
            continue
        probe, lib, rest = p
        if probe == "full_bench":
            w = rest.split()
            rows.setdefault("bench.py, whole line: S1 us per step", {}).setdefault(lib, []).append("%.1f" % (float(w[1]) * 1e3))
            rows.setdefault("bench.py: `full_path.frames_per_sec`", {}).setdefault(lib, []).append(w[3])
            k = json.loads(rest.split("kernel_ms_per_frame", 1)[1])
            rows.setdefault("bench.py: k2_bin us, one frame in flight (HIP events)", {}).setdefault(lib, []).append("%.1f" % (k["k2_bin"] * 1e3))
        elif probe == "short_run_probe" and rest.startswith("{"):
            fit = json.loads(rest)["fit_over_K_20_to_300"]
            rows.setdefault("short_run_probe: us per frame (fit over 20..300 frames)", {}).setdefault(lib, []).append("%.2f" % fit["per_frame_us"])
            rows.setdefault("short_run_probe: fixed us per call", {}).setdefault(lib, []).append("%.1f" % fit["fixed_us"])
        elif probe == "short_run_probe" and rest.split()[0] in ("1", "4"):
            us = rest.split("'us_p50': ")[1].split(",")[0]
            rows.setdefault("short_run_probe: render_resident(%s), us p50" % rest.split()[0], {}).setdefault(lib, []).append(us)
        elif probe == "config_bench":
            d = json.loads(rest)
            if "device_frames_per_s" in d:
                rows.setdefault("config_bench %s: device frames / s" % d["config"], {}).setdefault(lib, []).append("%.0f" % d["device_frames_per_s"])
                rows.setdefault("config_bench %s: full path frames / s" % d["config"], {}).setdefault(lib, []).append("%.0f" % d["full_path_frames_per_s"])
                rows.setdefault("config_bench %s: batch frames / s" % d["config"], {}).setdefault(lib, []).append("%.0f" % d["batch_frames_per_s"])
    out = ["| figure (every run) | parent | change |", "|---|---|---|"]
    for k, v in rows.items():
        out.append("| %s | %s | %s |" % (k, ", ".join(v.get("parent", [])), ", ".join(v.get("change", []))))
    return "\n".join(out)


def text_block(path):
    return "```\n" + open(path).read().rstrip() + "\n```"


def main():
    if sys.argv[1] == "reduce":
        run, dst, tag = sys.argv[2:5]
        for d in sorted(glob.glob(os.path.join(run, "trace*_*"))):
            if os.path.isdir(d) and reduce_trace(d, os.path.join(dst, "%s_%s_dispatches.csv" % (tag, os.path.basename(d)))):
                print("reduced", d)
        return
    d, tag = sys.argv[2:4]
    print("# k2_bin sized to the scene: measurements (%s)\n" % tag)
    print("Generated by `python tools/summarize_bin.py tables profiles %s` from the files named in each section.\n" % tag)
    for f in sorted(glob.glob(os.path.join(d, tag + "_trace*_dispatches.csv"))):
        name = os.path.basename(f)[len(tag) + 1:-len("_dispatches.csv")]
        mode = "one frame in flight (SWFR_FRAMES_IN_FLIGHT=1)" if name.startswith("trace1_") else "the bench's own mode (four frame sets, two frames per launch in the timed region)"
        print("## Kernel durations, %s: %s\n\n`%s` (rocprofv3 --kernel-trace, S1, 100 steps)\n" % (name.split("_", 1)[1], mode, os.path.basename(f)))
        print(trace_table(f) + "\n")
    for name, title, fn in (("bench.txt", "Bench, parent and change alternating", bench_table),
                            ("order_sweep.txt", "Where the ordering workgroups stand in the grid (vA: first in the small instance, last in the large one = the change; vB: last in both; vC: first in both)", bench_table),
                            ("one_frame.txt", "One frame in flight and the other probes", probes_table),
                            ("config_bench.txt", "tools/config_bench.py, change and parent alternating", probes_table),
                            ("suite.txt", "GPU suite", text_block), ("soak.txt", "Soak", text_block)):
        f = os.path.join(d, "%s_%s" % (tag, name))
        if os.path.exists(f):
            print("## %s\n\n`%s`\n" % (title, os.path.basename(f)))
            print(fn(f) + "\n")


if __name__ == "__main__":
    main()
