"""What the pixman-exact linear gradient costs on one MI355X, beside the float64 model, and whether the existing frames moved.  One JSON
line.  Recorded only: there is no threshold.

Frames, each resident on the device and rendered with several frames in flight (swfr_render_resident), taken in turn `--rounds` times:
    linear_float64                      BASELINE config 2's linear gradient (1024 x 1024, config2_gradient_linear_ext), the float64 model
    linear_pixman_{pad,repeat,reflect}  the same fill on a linear="pixman" handle under each extend (k2_linear_pieces + shade_linear)
    radial                              config2_gradient_radial
    s1                                  the S1 synthetic scene at its own size
Medians; the pixman variants as a ratio to linear_float64.

With --lib the library is another build (the parent's, say): python tools/linear_bench.py --lib build/parent/libswfr.so --existing-only
times linear_float64, radial and s1 alone, which is what tells whether the existing paths moved.  Alternate the two builds run by run.

usage (GPU box): python tools/linear_bench.py [--frames 200] [--rounds 5] [--lib path] [--existing-only]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def with_spread(obj, spread):
    if isinstance(obj, list):
        return [with_spread(o, spread) for o in obj]
    if isinstance(obj, dict):
        out = {k: with_spread(v, spread) for k, v in obj.items()}
        if "colors" in out and "spread" in out:
            out["spread"] = spread
        return out
    return obj


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def frames_of(existing_only):
    """name -> (width, height, swfr_build_frame's arrays)"""
    import swf_renderer_amd as S
    from scenarios import scenarios
    from swf_renderer_amd import api, synth
    import helpers
    SC = scenarios()
    out = {}

    def built(sc, **kw):
        host = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY, **kw)
        try:
            return sc["width"], sc["height"], host.build_frame(sc["stage"])
        finally:
            host.close()
    lin = SC["config2_gradient_linear_ext"]
    out["linear_float64"] = built(lin)
    if not existing_only:
        for spread in ("pad", "repeat", "reflect"):
            out["linear_pixman_" + spread] = built(dict(lin, stage=with_spread(lin["stage"], spread)), linear="pixman")
    out["radial"] = built(SC["config2_gradient_radial"])
    W, H, _, _, scene = helpers.synth_scene(synth.S1)
    out["s1"] = (W, H, scene)
    return out


def measure(frames, rounds, existing_only):
    import swf_renderer_amd as S
    fr = frames_of(existing_only)
    handles = {}
    for name, (w, h, arrays) in fr.items():
        r = S.Renderer(w, h)
        r.upload_edges(*arrays)
        r.render_resident(20)                                     # warm-up
        handles[name] = r
    series = {n: [] for n in fr}
    kernels = {n: [] for n in fr}                                 # (rows_ms, tiles_ms) of the frames timed kernel by kernel: k2_linear_pieces runs
    for _ in range(rounds):                                       # between the row pass and the tile pass and is booked to rows_ms
        for n, r in handles.items():                              # the frames in turn: drift hits them alike
            r.render_resident(frames)
            t = r.timing()
            series[n].append(t["total_ms"] / max(t["frames"], 1))
            kernels[n].append((t["rows_ms"] / max(t["timed_frames"], 1), t["tiles_ms"] / max(t["timed_frames"], 1)))
    for r in handles.values():
        r.close()
    out = {"library": os.path.relpath(S.library_path(), ROOT), "frames": frames, "rounds": rounds}
    for n in fr:
        out[n] = {"ms_per_frame_median": round(_median(series[n]), 4), "ms_per_frame_all": [round(v, 4) for v in series[n]],
                  "rows_ms_median": round(_median([k[0] for k in kernels[n]]), 4), "tiles_ms_median": round(_median([k[1] for k in kernels[n]]), 4)}
    for n in fr:
        if n.startswith("linear_pixman_"):
            out[n + "_over_float64"] = round(out[n]["ms_per_frame_median"] / out["linear_float64"]["ms_per_frame_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib")
    ap.add_argument("--existing-only", action="store_true")
    a = ap.parse_args()
    if a.lib:
        from swf_renderer_amd import api
        lib = os.path.abspath(a.lib)
        api.library_path = lambda: lib
        import swf_renderer_amd as S
        S.library_path = api.library_path
    print(json.dumps(measure(a.frames, a.rounds, a.existing_only)))


if __name__ == "__main__":
    main()
