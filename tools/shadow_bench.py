"""What shadowed layers cost on one MI355X.  One JSON line.

  passes   the alpha pass and the finish pass (shadow.hip) over a 3840 x 2160 texture, with no offset and with offset (4, 4), and a
           device-to-device copy of the same bytes -- the yardstick: a streaming pass reads and writes the image once (the finish pass
           reads two images) -- by HIP events (swfr_debug_time_shadow), `--reps` passes back to back, the median of `--rounds`; each pass
           as a ratio to the copy
  render   a whole blocking render() of S1 (4K, 1 000 stars) with its stars in 8 shadowed layers (5 x 5 box, one pass, offset (4, 4)) beside
           the same frame with 8 blurred layers of that box and with the 8 groups as plain layers: wall clock of the call
           (swfr_last_path_timing), the median of `--rounds`, the three in turn within a round

usage (GPU box): python tools/shadow_bench.py [--reps 20] [--rounds 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OFFSETS = ((0, 0), (4, 4))
W4K, H4K = 3840, 2160


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def passes(reps, rounds):
    import swf_renderer_amd as S
    r = S.Renderer(64, 64)
    try:
        series = {o: {"alpha": [], "finish": [], "copy": []} for o in OFFSETS}
        for _ in range(rounds):
            for o in OFFSETS:                                         # the offsets in turn: drift hits them alike
                a, f, c = r.debug_time_shadow(W4K, H4K, o[0], o[1], reps)
                series[o]["alpha"].append(a)
                series[o]["finish"].append(f)
                series[o]["copy"].append(c)
    finally:
        r.close()
    out = {"width": W4K, "height": H4K, "bytes": W4K * H4K * 4, "reps": reps, "rounds": rounds}
    copy = _median([c for o in OFFSETS for c in series[o]["copy"]])
    out["copy_ms"] = round(copy, 4)
    out["copy_all"] = [round(c, 4) for o in OFFSETS for c in series[o]["copy"]]
    for o in OFFSETS:
        a, f = _median(series[o]["alpha"]), _median(series[o]["finish"])
        out["offset_%d_%d" % o] = {"alpha_ms": round(a, 4), "finish_ms": round(f, 4), "alpha_over_copy": round(a / copy, 3),
                                   "finish_over_copy": round(f / copy, 3), "alpha_all": [round(x, 4) for x in series[o]["alpha"]],
                                   "finish_all": [round(x, 4) for x in series[o]["finish"]]}
    return out


def render(rounds, layers=8):
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    kids = api.stars_to_stage(pts, cols)["children"]
    n = (len(kids) + layers - 1) // layers
    groups = [kids[i:i + n] for i in range(0, len(kids), n)]
    shadow = {"color": (0, 0, 0, 160), "dx": 4, "dy": 4, "x": 5, "y": 5}
    stages = {"shadowed": {"children": [{"type": "container", "children": g, "shadow": shadow} for g in groups]},
              "blurred": {"children": [{"type": "container", "children": g, "blur": {"x": 5, "y": 5}} for g in groups]},
              "plain_layers": {"children": [{"type": "container", "children": g, "layer": True} for g in groups]}}
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
    out = {"layers": len(groups), "rounds": rounds, "box": [5, 5, 1], "offset": [4, 4]}
    for name, v in series.items():
        out[name + "_render_ms"] = round(_median(v), 3)
        out[name + "_all"] = [round(x, 3) for x in v]
    out["shadowed_minus_blurred_ms"] = round(out["shadowed_render_ms"] - out["blurred_render_ms"], 3)
    out["shadowed_over_blurred"] = round(out["shadowed_render_ms"] / out["blurred_render_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps({"passes": passes(a.reps, a.rounds), "render": render(a.rounds)}))


if __name__ == "__main__":
    main()
