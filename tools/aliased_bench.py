"""S1 (4K, 1 000 stars) from the resident edge list in the default (antialiased) and the aliased mode (Renderer(antialias="none")),
alternating within one run: resident frames/s per round and per-kernel times (HIP events, one frame in flight).  One JSON line.
With --rocprof DIR the same is repeated once under `rocprofv3 --kernel-trace --stats` (a child process; its output under DIR).

usage (GPU box): python tools/aliased_bench.py [--rounds 5] [--frames 2000] [--rocprof DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rocprof", default="")
    args = ap.parse_args()
    import torch
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    W, H = synth.S1["width"], synth.S1["height"]
    pts, cols = synth.scene(**synth.S1)
    stage = api.stars_to_stage(pts, cols)
    modes = ("default", "none")
    scenes, handles, timed = {}, {}, {}
    for m in modes:
        host = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY, antialias=m)
        scenes[m] = host.build_frame(stage)
        host.close()
        handles[m] = S.Renderer(W, H, antialias=m)
        handles[m].upload_edges(*scenes[m])
        handles[m].render_resident(64)
        # per-kernel times: a handle with one frame in flight and events on every 4th frame (outside the timed rounds)
        os.environ["SWFR_FRAMES_IN_FLIGHT"], os.environ["SWFR_EVENT_STRIDE"] = "1", "4"
        t = S.Renderer(W, H, antialias=m)
        t.upload_edges(*scenes[m])
        t.render_resident(16)
        t.render_resident(64)
        timed[m] = t.timing()
        t.close()
        del os.environ["SWFR_FRAMES_IN_FLIGHT"], os.environ["SWFR_EVENT_STRIDE"]
    fps = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:                                   # alternating: both modes see the same machine state
            r = handles[m]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.render_resident(args.frames)
            torch.cuda.synchronize()
            fps[m].append(args.frames / (time.perf_counter() - t0))
    out = {"scene": "S1", "width": W, "height": H, "frames_per_round": args.frames, "rounds": args.rounds}
    for m in modes:
        v = sorted(fps[m])
        tm = timed[m]
        n = max(tm["timed_frames"], 1)
        out[m] = {"resident_fps": [round(x) for x in fps[m]], "resident_fps_median": round(v[len(v) // 2]),
                  "bin_us": round(1e3 * tm["setup_ms"] / n, 2), "rows_us": round(1e3 * tm["rows_ms"] / n, 2),
                  "tiles_us": round(1e3 * tm["tiles_ms"] / n, 2), "n_edges": len(scenes[m][0]), "n_paths": len(scenes[m][1])}
        handles[m].close()
    out["aliased_over_default"] = round(out["none"]["resident_fps_median"] / out["default"]["resident_fps_median"], 4)
    print(json.dumps(out), flush=True)
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.rocprof, "-o", "aliased", "--",
               sys.executable, os.path.abspath(__file__), "--rounds", "1", "--frames", "200"]
        rc = subprocess.call(cmd, timeout=600)
        print(json.dumps({"rocprof": args.rocprof, "exit": rc}), flush=True)
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    main()
