"""What colour transforms cost on one MI355X.  One JSON line.

  s1            S1 (4K, 1 000 stars) through swfr_render (render_sequence: every frame built, uploaded, rasterized and waited for),
                plain and inside one alpha-fade container whose alpha changes every frame -- solid colours need no device work, so
                the difference is the host walk's
  texel_pass    config 4's 4096 x 4096 texture (helpers.large_texture_scene): the texel pass alone (swfr_debug_time_cxform, HIP events)
                in us and GB/s (4 bytes read + 4 written per texel), beside a device-to-device copy of the same bytes in the same process
  config4       the same scene through swfr_render: no transform, a steady transform (its texture comes from the cache: no pass) and a
                transform that changes every frame (one pass per frame)
With --rocprof DIR the config-4 part is repeated once under `rocprofv3 --kernel-trace --stats` (a child process; output under DIR):
k_cxform_texels must appear once per changing frame and never for the steady ones.

usage (GPU box): python tools/cxform_bench.py [--frames 200] [--rocprof DIR]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def fade(a, add_r=0):
    import make_cxform_goldens as G
    return G.cxform(mult=(256, 256, 256, a), add=(add_r, 0, 0, 0))


def config4(frames, only_config4=False):
    import swf_renderer_amd as S
    import make_cxform_goldens as G
    from helpers import large_texture_scene
    big = large_texture_scene()
    W, H = 3840, 2160
    r = S.Renderer(W, H)
    out = {}
    try:
        for b in big["bitmaps"]:
            r.add_bitmap(b)
        plain = big["stage"]
        steady = G.apply_transform_value(plain, fade(160))
        changing = [G.apply_transform_value(plain, fade(40 + (i % 200), i % 7)) for i in range(frames)]
        for name, stages in (("none", [plain] * frames), ("steady", [steady] * frames), ("changing", changing)):
            r.render(stages[0])
            secs, _ = r.render_sequence(stages, 1)
            out[name + "_ms_per_frame"] = round(1e3 * secs / frames, 3)
        if not only_config4:
            from swf_renderer_amd import api
            bid = big["bitmaps"][0]["id"]
            v = api.color_transform_values(fade(160))
            ct = api.ColorTransform((C.c_int32 * 4)(*v[:4]), (C.c_int32 * 4)(*v[4:]))
            passes, copies = [], []
            for _ in range(5):
                p, c = C.c_float(), C.c_float()
                r._check(r.L.swfr_debug_time_cxform(r.h, bid, C.byref(ct), 50, C.byref(p), C.byref(c)))
                passes.append(p.value * 1e3)
                copies.append(c.value * 1e3)
            texels = 4096 * 4096
            moved = texels * 8
            pm, cm = _median(passes), _median(copies)
            out["texel_pass"] = {"texels": texels, "bytes_moved": moved, "pass_us": [round(x, 2) for x in passes], "pass_us_median": round(pm, 2),
                                 "pass_gbps": round(moved / pm / 1e3, 1), "copy_us": [round(x, 2) for x in copies], "copy_us_median": round(cm, 2),
                                 "copy_gbps": round(moved / cm / 1e3, 1), "pass_over_copy": round(pm / cm, 3)}
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rocprof", default="")
    ap.add_argument("--config4-only", action="store_true")       # (the rocprofv3 child)
    args = ap.parse_args()
    import torch
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth
    import make_cxform_goldens as G
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    if args.config4_only:
        print(json.dumps({"config4": config4(20, only_config4=True)}), flush=True)
        return
    W, H = synth.S1["width"], synth.S1["height"]
    pts, cols = synth.scene(**synth.S1)
    stage = api.stars_to_stage(pts, cols)
    n = 64
    plain = [stage] * n
    faded = [G.apply_transform_value(stage, fade(32 + 3 * i)) for i in range(n)]
    r = S.Renderer(W, H)
    res = {"plain": [], "fade": []}
    try:
        r.render_sequence(plain[:4], 1)
        r.render_sequence(faded[:4], 1)
        for _ in range(5):                                    # alternating: both see the same machine state
            for name, st in (("plain", plain), ("fade", faded)):
                secs, _ = r.render_sequence(st, 1)
                res[name].append(1e3 * secs / n)
    finally:
        r.close()
    out = {"s1": {"frames_per_round": n, "plain_ms_per_frame": [round(x, 4) for x in res["plain"]], "fade_ms_per_frame": [round(x, 4) for x in res["fade"]],
                  "plain_median": round(_median(res["plain"]), 4), "fade_median": round(_median(res["fade"]), 4)}}
    out["config4"] = config4(args.frames)
    print(json.dumps(out), flush=True)
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.rocprof, "-o", "cxform", "--",
               sys.executable, os.path.abspath(__file__), "--config4-only"]
        rc = subprocess.call(cmd, timeout=600)
        print(json.dumps({"rocprof": args.rocprof, "exit": rc}), flush=True)
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    main()
