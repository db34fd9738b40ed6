"""What the nearest filter costs on one MI355X: the existing bitmap configurations, which must not move, and nearest frames beside
the same frames with filter 0.  Recorded only: there is no threshold (profiles/nearest_bench.txt).

Frames, resident on the device and rendered with several frames in flight (swfr_render_resident), taken in turn `--rounds` times;
ms per frame, medians:
  config4_magnified      BASELINE config 4: the textured fixture magnified to 3840 x 2160 (bilinear; tools/config_bench.py)
  config4_large_texture  a 4096 x 4096 texture sampled about 1:1 at 3840 x 2160 (bilinear, HBM-bound; tests/helpers.py)
  box_magnified_repeat   a 1024 x 1024 box, the fixture's 139 x 208 bitmap 3 x magnified, repeating (bilinear)
  box_minified_repeat    the same 0.45 x minified (pixman's separable convolution)
  *_nearest              the last two and config4_magnified with "filter": "nearest" on every bitmap fill (one texel per pixel)
The *_nearest frames need this library; --no-nearest leaves them out, which is how another build (--lib, the parent's say) is timed.

One run:      python tools/nearest_bench.py [--frames 200] [--rounds 5] [--lib path] [--no-nearest]          -> one JSON line
A session:    python tools/nearest_bench.py --against parent/libswfr.so [--alternations 3] [--headline-steps 300] [--out table.txt]
              the parent's library and this one taken in turn, each run a fresh process; with --headline-steps also bench.py's
              headline (tools/bench_with_lib.py for the parent).  Prints the table of profiles/nearest_bench.txt."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _with_filter(obj, value):
    if isinstance(obj, list):
        return [_with_filter(o, value) for o in obj]
    if isinstance(obj, dict):
        out = {k: _with_filter(v, value) for k, v in obj.items()}
        if out.get("type") == "bitmap":
            out["filter"] = value
        return out
    return obj


def frames(nearest):
    """name -> (width, height, stage, bitmaps)"""
    import scenarios
    from helpers import fixture, large_texture_scene
    m = scenarios._m
    bmp = fixture("homestuck-beta-3.bitmap")
    out = {}
    tag4 = fixture("homestuck-beta-4")
    b = tag4["bounds"]
    sx, sy = 3840 * 20 / (b["x_max"] - b["x_min"]), 2160 * 20 / (b["y_max"] - b["y_min"])
    out["config4_magnified"] = (3840, 2160, {"children": [{"type": "shape", "definition": tag4, "matrix": m(sx, sy, -b["x_min"] * sx, -b["y_min"] * sy)}]}, [bmp])
    big = large_texture_scene()
    out["config4_large_texture"] = (3840, 2160, big["stage"], big["bitmaps"])
    box = [(0, 0), (1024 * 20, 0), (1024 * 20, 1024 * 20), (0, 1024 * 20)]

    def boxed(k, x, y):
        fill = {"type": "bitmap", "bitmap_id": bmp["id"], "repeating": True, "smoothed": True, "matrix": m(20 * k, 20 * k, round(20 * x), round(20 * y))}
        return (1024, 1024, {"children": [{"type": "shape", "definition": scenarios._poly_shape(box, fill)}]}, [bmp])
    out["box_magnified_repeat"] = boxed(3, 303.4, 200.2)
    out["box_minified_repeat"] = boxed(0.45, 480.3, 465.1)
    if nearest:
        for name in ("config4_magnified", "box_magnified_repeat", "box_minified_repeat"):
            w, h, stage, bitmaps = out[name]
            out[name + "_nearest"] = (w, h, _with_filter(stage, "nearest"), bitmaps)
    return out


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(n_frames, rounds, nearest):
    import swf_renderer_amd as S
    handles = {}
    for name, (w, h, stage, bitmaps) in frames(nearest).items():
        r = S.Renderer(w, h)
        for b in bitmaps:
            r.add_bitmap(b)
        r.upload_edges(*r.build_frame(stage))
        r.render_resident(20)                                     # warm-up
        handles[name] = r
    series = {n: [] for n in handles}
    for _ in range(rounds):
        for n, r in handles.items():                              # the frames in turn: drift hits them alike
            r.render_resident(n_frames)
            t = r.timing()
            series[n].append(t["total_ms"] / max(t["frames"], 1))
    refused = 0
    for r in handles.values():
        st = r.stats()
        refused += sum(st[k] for k in ("pairtest_limit", "start_group_limit", "history_limit"))
        r.close()
    out = {"library": S.library_path(), "frames": n_frames, "rounds": rounds, "capacity_refusals": refused}
    for n, v in series.items():
        out[n] = {"ms_per_frame_median": round(_median(v), 4), "ms_per_frame_all": [round(x, 4) for x in v]}
    if nearest:
        for n in [n for n in series if n.endswith("_nearest")]:
            out[n + "_over_good"] = round(out[n]["ms_per_frame_median"] / out[n[:-len("_nearest")]]["ms_per_frame_median"], 3)
    return out


def _last_json(text):
    for line in reversed(text.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError("no JSON line in:\n" + text[-2000:])


def session(a):
    """the two libraries in turn, every run a fresh process (none of them replaces its program); the table"""
    me = os.path.abspath(__file__)
    runs = {"parent": [], "this": []}
    heads = {"parent": [], "this": []}
    for _ in range(a.alternations):
        for who in ("parent", "this"):
            cmd = [sys.executable, me, "--frames", str(a.frames), "--rounds", str(a.rounds)] + (["--lib", a.against, "--no-nearest"] if who == "parent" else [])
            runs[who].append(_last_json(subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600).stdout))
            if a.headline_steps:
                args = ["--gpus", "1", "--steps", str(a.headline_steps), "--warmup", "30", "--no-cpu-baseline", "--no-full-path", "--no-batched"]
                cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_with_lib.py"), os.path.relpath(os.path.abspath(a.against), ROOT)] + args if who == "parent" \
                    else [sys.executable, os.path.join(ROOT, "bench.py")] + args
                heads[who].append(_last_json(subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600, cwd=ROOT).stdout))
    lines = ["# tools/nearest_bench.py --against <the parent commit's libswfr.so> --alternations %d --frames %d --rounds %d: ms per frame, the two" % (a.alternations, a.frames, a.rounds),
             "# libraries taken in turn in one session.  Per library: the medians of its runs and (min..max) over all rounds.",
             "%-28s %-44s %-44s %s" % ("frame", "parent medians (min..max)", "this medians (min..max)", "this / parent (medians of medians)")]
    names = [n for n in runs["this"][0] if isinstance(runs["this"][0][n], dict)]

    def cell(rs, n):
        if n not in rs[0]:
            return "-", None
        meds = [r[n]["ms_per_frame_median"] for r in rs]
        every = [x for r in rs for x in r[n]["ms_per_frame_all"]]
        return "%s (%.4f..%.4f)" % (" ".join("%.4f" % x for x in meds), min(every), max(every)), _median(meds)
    for n in names:
        (pc, pm), (tc, tm) = cell(runs["parent"], n), cell(runs["this"], n)
        lines.append("%-28s %-44s %-44s %s" % (n, pc, tc, "%.3f" % (tm / pm) if pm else ""))
    for n in [n for n in runs["this"][0] if n.endswith("_over_good")]:
        lines.append("%-28s %s" % (n, " ".join("%.3f" % r[n] for r in runs["this"])))
    lines.append("capacity refusals: %d" % sum(r["capacity_refusals"] for rs in runs.values() for r in rs))
    if a.headline_steps:
        key = "value" if "value" in heads["this"][0] else sorted(k for k, v in heads["this"][0].items() if isinstance(v, (int, float)))[0]
        for who in ("parent", "this"):
            lines.append("bench.py headline (%s, --steps %d) %-7s %s" % (key, a.headline_steps, who, " ".join("%.1f" % h[key] for h in heads[who])))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    sys.stdout.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib")
    ap.add_argument("--no-nearest", action="store_true")
    ap.add_argument("--against", help="another build's libswfr.so: run a session of alternating runs and print the table")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--headline-steps", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.against:
        return session(a)
    if a.lib:
        from swf_renderer_amd import api
        lib = os.path.abspath(a.lib)
        api.library_path = lambda: lib
        import swf_renderer_amd as S
        S.library_path = api.library_path
    import torch
    assert torch.cuda.is_available()                 # torch initialises HIP first
    print(json.dumps(measure(a.frames, a.rounds, not a.no_nearest)))


if __name__ == "__main__":
    main()
