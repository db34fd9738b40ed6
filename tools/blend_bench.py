"""What a blend mode costs on one MI355X.  One JSON line.

S1 (4K, 1 000 stars) resident on the device, rendered with several frames in flight (swfr_render_resident) and with one frame in
flight (per-kernel times from the handle's HIP events), in four variants taken in turn, `--rounds` times:
  plain       no blended star: the solid instance of the tile kernel (what bench.py measures)
  multiply    every star under MULTIPLY
  overlay     every star under OVERLAY
and `plain` forced through the tile kernel's instances 2 and 3 (SWFR_TILES_SHADERS, read when a handle is created): what the wider
instance costs a frame that uses none of it.  Medians; multiply / overlay as ratios to plain, instance 3 as a ratio to instance 2.
With --rocprof DIR the blended variants run once more under `rocprofv3 --kernel-trace --stats` in a child process (output under DIR).

usage (GPU box): python tools/blend_bench.py [--frames 200] [--rounds 5] [--rocprof DIR]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if os.environ.get("SWFR_LIB"):                          # another build of the library
    from swf_renderer_amd import api as _api
    _lib = os.path.abspath(os.environ["SWFR_LIB"])
    _api.library_path = lambda: _lib


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def scenes():
    """S1 as (edges, paths, styles) per variant: the plain scene, and every path under an operator"""
    import helpers
    from swf_renderer_amd import api, synth
    W, H, _, _, (edges, paths, styles) = helpers.synth_scene(synth.S1)
    out = {"plain": (edges, paths, styles)}
    for mode in ("multiply", "overlay"):
        p = paths.copy()
        p["lerp"] = api.PATH_OPERATORS[mode] << 8
        out[mode] = (edges, p, styles)
    return W, H, out


def measure(frames, rounds):
    import swf_renderer_amd as S
    W, H, sc = scenes()
    variants = [("plain", "plain", None), ("multiply", "multiply", None), ("overlay", "overlay", None),
                ("plain_instance2", "plain", "2"), ("plain_instance3", "plain", "3")]
    handles = {}
    for name, scene, knob in variants:
        if knob is None:
            os.environ.pop("SWFR_TILES_SHADERS", None)
        else:
            os.environ["SWFR_TILES_SHADERS"] = knob
        r = S.Renderer(W, H)
        r.upload_edges(*sc[scene])
        r.render_resident(20)                                     # warm-up
        handles[name] = r
    os.environ.pop("SWFR_TILES_SHADERS", None)
    series = {name: {"ms_per_frame": [], "one_in_flight": []} for name, _, _ in variants}
    for _ in range(rounds):
        for name, _, _ in variants:                               # the variants in turn: drift hits them alike
            r = handles[name]
            r.render_resident(frames)
            t = r.timing()
            series[name]["ms_per_frame"].append(t["total_ms"] / max(t["frames"], 1))
            r.render_resident(1)
            t1 = r.timing()
            series[name]["one_in_flight"].append({k: t1[k] for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")})
    for r in handles.values():
        r.close()
    out = {"frames": frames, "rounds": rounds, "width": W, "height": H}
    for name, s in series.items():
        out[name] = {"ms_per_frame_median": round(_median(s["ms_per_frame"]), 4),
                     "ms_per_frame_all": [round(v, 4) for v in s["ms_per_frame"]],
                     "mpx_per_s": round(W * H / 1e3 / _median(s["ms_per_frame"]), 1),
                     "one_frame_in_flight_ms": {k: round(_median([o[k] for o in s["one_in_flight"]]), 4)
                                                for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")}}
    base = out["plain"]["ms_per_frame_median"]
    out["multiply_over_plain"] = round(out["multiply"]["ms_per_frame_median"] / base, 3)
    out["overlay_over_plain"] = round(out["overlay"]["ms_per_frame_median"] / base, 3)
    out["instance3_over_instance2"] = round(out["plain_instance3"]["ms_per_frame_median"] / out["plain_instance2"]["ms_per_frame_median"], 3)
    return out


def child(frames):
    import swf_renderer_amd as S
    W, H, sc = scenes()
    for name in ("plain", "multiply", "overlay"):
        r = S.Renderer(W, H)
        r.upload_edges(*sc[name])
        r.render_resident(frames)
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rocprof", metavar="DIR", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.frames)
        return
    out = measure(a.frames, a.rounds)
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        rc = subprocess.call(["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blend", "--output-format", "csv", "--",
                              sys.executable, os.path.abspath(__file__), "--child", "--frames", "30"], timeout=600)
        out["rocprof_exit"] = rc
    print(json.dumps(out))


if __name__ == "__main__":
    main()
