"""What a convolution pass costs on one MI355X, beside the streaming roof and the box passes in the same run.  One JSON line.

  passes   one pass of convolve.hip over a 3840 x 2160 texture for a 3 x 3 kernel of nine taps, a 3 x 3 cross (five taps: the zero taps
           are skipped), a 5 x 5 and a 7 x 7 kernel, by the framebuffer instance and by the texel instance (k_convolve_fb,
           k_convolve_tex), beside k_blur_capture over the same words -- one read and one write of the same bytes, the streaming roof --
           and beside one k_blur_h + k_blur_v pair of box width 3, by HIP events (swfr_debug_time_convolve, swfr_debug_time_blur),
           `--reps` passes back to back, the median of `--rounds`, the kernels in turn within a round; each pass as a ratio to the
           capture pass.  The two textures (66 MB) stay in the device's caches between the repetitions: these are cache-resident
           figures, like tools/blur_bench.py's
  render   a whole blocking render() of S1 (4K, 1 000 stars) with its stars in one sharpened layer beside the same frame with one
           one-pass 3 x 3 blurred layer: wall clock of the call (swfr_last_path_timing), the median of `--rounds`, the two in turn
           within a round

usage (GPU box): python tools/convolve_bench.py [--reps 20] [--rounds 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W4K, H4K = 3840, 2160
KERNELS = {
    "3x3_dense": {"matrix": [[-2, -1, 0], [-1, 1, 1], [1, 1, 2]]},
    "3x3_cross": {"matrix": [[0, -1, 0], [-1, 5, -1], [0, -1, 0]]},
    "5x5": {"matrix": [[1, 4, 6, 4, 1], [4, 16, 24, 16, 4], [6, 24, 36, 24, 6], [4, 16, 24, 16, 4], [1, 4, 6, 4, 1]], "divisor": 256},
    "7x7": {"matrix": [[(i * 7 + j) % 5 - 2 or 1 for i in range(7)] for j in range(7)], "divisor": 49},
}


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def passes(reps, rounds):
    import swf_renderer_amd as S
    r = S.Renderer(64, 64)
    try:
        series = {k: {"fb": [], "tex": [], "capture": []} for k in KERNELS}
        box = {"h": [], "v": []}
        for _ in range(rounds):
            for k, value in KERNELS.items():                          # the kernels in turn: drift hits them alike
                fb, tex, cap = r.debug_time_convolve(W4K, H4K, value, reps)
                series[k]["fb"].append(fb)
                series[k]["tex"].append(tex)
                series[k]["capture"].append(cap)
            h, v, _ = r.debug_time_blur(W4K, H4K, 3, reps)
            box["h"].append(h)
            box["v"].append(v)
    finally:
        r.close()
    out = {"width": W4K, "height": H4K, "bytes": W4K * H4K * 4, "reps": reps, "rounds": rounds}
    cap = _median([c for s in series.values() for c in s["capture"]])
    out["capture_ms"] = round(cap, 4)
    out["capture_all"] = [round(c, 4) for s in series.values() for c in s["capture"]]
    for k, s in series.items():
        fb, tex = _median(s["fb"]), _median(s["tex"])
        out[k] = {"fb_ms": round(fb, 4), "tex_ms": round(tex, 4), "fb_over_capture": round(fb / cap, 3), "tex_over_capture": round(tex / cap, 3),
                  "fb_all": [round(x, 4) for x in s["fb"]], "tex_all": [round(x, 4) for x in s["tex"]]}
    h, v = _median(box["h"]), _median(box["v"])
    out["box_3"] = {"h_ms": round(h, 4), "v_ms": round(v, 4), "pair_ms": round(h + v, 4), "pair_over_capture": round((h + v) / cap, 3),
                    "h_all": [round(x, 4) for x in box["h"]], "v_all": [round(x, 4) for x in box["v"]]}
    return out


def render(rounds):
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    kids = api.stars_to_stage(pts, cols)["children"]
    stages = {"sharpened": {"children": [{"type": "container", "children": kids, "filters": [{"convolution": KERNELS["3x3_cross"]}]}]},
              "blurred": {"children": [{"type": "container", "children": kids, "filters": [{"blur": {"x": 3, "y": 3, "passes": 1}}]}]}}
    r = S.Renderer(synth.S1["width"], synth.S1["height"])
    try:
        series = {name: [] for name in stages}
        for name, st in stages.items():
            r.render(st)                                              # warm-up: shapes registered, buffers and textures allocated
        for _ in range(rounds):
            for name, st in stages.items():
                r.render(st)
                series[name].append(r.path_timing()["total_ms"])
    finally:
        r.close()
    out = {"layers": 1, "rounds": rounds}
    for name, v in series.items():
        out[name + "_render_ms"] = round(_median(v), 3)
        out[name + "_all"] = [round(x, 3) for x in v]
    out["sharpened_minus_blurred_ms"] = round(out["sharpened_render_ms"] - out["blurred_render_ms"], 3)
    out["sharpened_over_blurred"] = round(out["sharpened_render_ms"] / out["blurred_render_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps({"passes": passes(a.reps, a.rounds), "render": render(a.rounds)}))


if __name__ == "__main__":
    main()
