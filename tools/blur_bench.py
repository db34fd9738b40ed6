"""What blurred layers cost on one MI355X.  One JSON line.

  passes   one horizontal and one vertical box pass (blur.hip) over a 3840 x 2160 texture for w = 3, 15 and 255, and a device-to-device
           copy of the same bytes -- the yardstick: a pass reads and writes the image once -- by HIP events (swfr_debug_time_blur),
           `--reps` passes back to back, the median of `--rounds`; each pass as a ratio to the copy, and w = 255 as a ratio to w = 3,
           which the running sums should hold near 1
  render   a whole blocking render() of S1 (4K, 1 000 stars) with its stars in 8 blurred layers (5 x 5 box, one pass) beside the same
           frame with the 8 groups as plain layers: wall clock of the call (swfr_last_path_timing), the median of `--rounds`

usage (GPU box): python tools/blur_bench.py [--reps 20] [--rounds 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTHS = (3, 15, 255)
W4K, H4K = 3840, 2160


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def passes(reps, rounds):
    import swf_renderer_amd as S
    r = S.Renderer(64, 64)
    try:
        series = {w: {"h": [], "v": [], "copy": []} for w in WIDTHS}
        for _ in range(rounds):
            for w in WIDTHS:                                          # the widths in turn: drift hits them alike
                h, v, c = r.debug_time_blur(W4K, H4K, w, reps)
                series[w]["h"].append(h)
                series[w]["v"].append(v)
                series[w]["copy"].append(c)
    finally:
        r.close()
    out = {"width": W4K, "height": H4K, "bytes": W4K * H4K * 4, "reps": reps, "rounds": rounds}
    copy = _median([c for w in WIDTHS for c in series[w]["copy"]])
    out["copy_ms"] = round(copy, 4)
    for w in WIDTHS:
        h, v = _median(series[w]["h"]), _median(series[w]["v"])
        out["w%d" % w] = {"h_ms": round(h, 4), "v_ms": round(v, 4), "h_over_copy": round(h / copy, 3), "v_over_copy": round(v / copy, 3),
                          "h_all": [round(x, 4) for x in series[w]["h"]], "v_all": [round(x, 4) for x in series[w]["v"]]}
    out["h_w255_over_w3"] = round(out["w255"]["h_ms"] / out["w3"]["h_ms"], 3)
    out["v_w255_over_w3"] = round(out["w255"]["v_ms"] / out["w3"]["v_ms"], 3)
    return out


def render(rounds, layers=8):
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    kids = api.stars_to_stage(pts, cols)["children"]
    n = (len(kids) + layers - 1) // layers
    groups = [kids[i:i + n] for i in range(0, len(kids), n)]
    stages = {"blurred": {"children": [{"type": "container", "children": g, "blur": {"x": 5, "y": 5}} for g in groups]},
              "plain_layers": {"children": [{"type": "container", "children": g, "layer": True} for g in groups]},
              "no_layers": {"children": kids}}
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
    out = {"layers": len(groups), "rounds": rounds, "box": [5, 5, 1]}
    for name, v in series.items():
        out[name + "_render_ms"] = round(_median(v), 3)
        out[name + "_all"] = [round(x, 3) for x in v]
    out["blurred_over_plain_layers"] = round(out["blurred_render_ms"] / out["plain_layers_render_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps({"passes": passes(a.reps, a.rounds), "render": render(a.rounds)}))


if __name__ == "__main__":
    main()
