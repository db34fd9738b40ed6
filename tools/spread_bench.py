"""What a gradient's spread mode costs on one MI355X, beside the same frame padded.  One JSON line.  Recorded only: there is no threshold.

A 1024 x 1024 frame filled by one radial gradient (BASELINE config 2's gradient half, the radius nearly halved so that two
periods show), resident on the device and rendered with several frames in flight (swfr_render_resident), in three variants taken in
turn, `--rounds` times: the gradient padded, reflected and repeated.  Medians; the two spread variants as a ratio to the padded one.

With --lib the library is another build (the parent's, say): python tools/spread_bench.py --lib build/parent/libswfr.so --pad-only
times the padded frame alone, which is what tells whether the padded path moved.  Alternate the two builds run by run.

usage (GPU box): python tools/spread_bench.py [--frames 200] [--rounds 5] [--lib path] [--pad-only]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W = H = 1024


def stage(spread):
    from scenarios import _circleish, _m, _poly_shape, _rgba
    g = {"spread": spread, "color_space": "s-rgb",
         "colors": [{"ratio": t, "color": _rgba(*c)} for t, c in ((0, (255, 0, 0)), (128, (0, 255, 0)), (255, (0, 0, 255)))]}
    fill = {"type": "radial-gradient", "matrix": _m(530 / 16384, 530 / 16384, 1300, 1100), "gradient": g}
    return {"children": [{"type": "shape", "definition": _poly_shape(_circleish(1300, 1100, 1000), fill), "matrix": _m(1024 / 130, 1024 / 115, 0, 0)}]}


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(frames, rounds, spreads):
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    host = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY)
    handles = {}
    for spread in spreads:
        arrays = host.build_frame(stage(spread))
        r = S.Renderer(W, H)
        r.upload_edges(*arrays)
        r.render_resident(20)                                     # warm-up
        handles[spread] = r
    host.close()
    series = {s: [] for s in spreads}
    for _ in range(rounds):
        for s in spreads:                                         # the variants in turn: drift hits them alike
            r = handles[s]
            r.render_resident(frames)
            t = r.timing()
            series[s].append(t["total_ms"] / max(t["frames"], 1))
    for r in handles.values():
        r.close()
    out = {"library": S.library_path(), "frames": frames, "rounds": rounds, "width": W, "height": H}
    for s in spreads:
        out[s] = {"ms_per_frame_median": round(_median(series[s]), 4), "ms_per_frame_all": [round(v, 4) for v in series[s]]}
    for s in spreads:
        if s != "pad":
            out["%s_over_pad" % s] = round(out[s]["ms_per_frame_median"] / out["pad"]["ms_per_frame_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib")
    ap.add_argument("--pad-only", action="store_true")
    a = ap.parse_args()
    if a.lib:
        from swf_renderer_amd import api
        lib = os.path.abspath(a.lib)
        api.library_path = lambda: lib
        import swf_renderer_amd as S
        S.library_path = api.library_path
    print(json.dumps(measure(a.frames, a.rounds, ("pad",) if a.pad_only else ("pad", "reflect", "repeat"))))


if __name__ == "__main__":
    main()
