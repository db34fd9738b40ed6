"""What inner shadows cost on one MI355X, beside the outer shadow's passes in the same run.  One JSON line.

  passes   the inverted alpha pass and the inner finish pass (shadow.hip: k_shadow_alpha_inv, k_shadow_inner_fb) and the outer pair
           (k_shadow_alpha, k_shadow_finish_fb) over a 3840 x 2160 texture, with no offset and with offset (4, 4), and a device-to-device
           copy of the same bytes -- the yardstick -- by HIP events (swfr_debug_time_inner_shadow, swfr_debug_time_shadow), `--reps`
           passes back to back, the median of `--rounds`, the two pairs in turn within a round; each pass as a ratio to the copy, and
           each inner pass as a ratio to its outer one.  The three textures (100 MB) stay in the device's caches between the
           repetitions: these are cache-resident figures, like tools/shadow_bench.py's
  render   a whole blocking render() of S1 (4K, 1 000 stars) with its stars in 8 inner-shadowed layers (5 x 5 box, one pass, offset (4, 4))
           beside the same frame with 8 outer shadowed layers of the same values: wall clock of the call (swfr_last_path_timing), the
           median of `--rounds`, the two in turn within a round

usage (GPU box): python tools/inner_bench.py [--reps 20] [--rounds 5]"""
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
        probes = {"outer": r.debug_time_shadow, "inner": r.debug_time_inner_shadow}
        series = {(k, o): {"alpha": [], "finish": [], "copy": []} for k in probes for o in OFFSETS}
        for _ in range(rounds):
            for o in OFFSETS:                                         # the offsets and the two pairs in turn: drift hits them alike
                for k, probe in probes.items():
                    a, f, c = probe(W4K, H4K, o[0], o[1], reps)
                    series[k, o]["alpha"].append(a)
                    series[k, o]["finish"].append(f)
                    series[k, o]["copy"].append(c)
    finally:
        r.close()
    out = {"width": W4K, "height": H4K, "bytes": W4K * H4K * 4, "reps": reps, "rounds": rounds}
    copy = _median([c for s in series.values() for c in s["copy"]])
    out["copy_ms"] = round(copy, 4)
    out["copy_all"] = [round(c, 4) for s in series.values() for c in s["copy"]]
    for o in OFFSETS:
        at = {}
        for k in probes:
            a, f = _median(series[k, o]["alpha"]), _median(series[k, o]["finish"])
            at[k] = {"alpha_ms": round(a, 4), "finish_ms": round(f, 4), "alpha_over_copy": round(a / copy, 3), "finish_over_copy": round(f / copy, 3),
                     "alpha_all": [round(x, 4) for x in series[k, o]["alpha"]], "finish_all": [round(x, 4) for x in series[k, o]["finish"]]}
        at["inner_over_outer"] = {"alpha": round(at["inner"]["alpha_ms"] / at["outer"]["alpha_ms"], 3),
                                  "finish": round(at["inner"]["finish_ms"] / at["outer"]["finish_ms"], 3)}
        out["offset_%d_%d" % o] = at
    return out


def render(rounds, layers=8):
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    kids = api.stars_to_stage(pts, cols)["children"]
    n = (len(kids) + layers - 1) // layers
    groups = [kids[i:i + n] for i in range(0, len(kids), n)]
    shadow = {"color": (0, 0, 0, 160), "dx": 4, "dy": 4, "x": 5, "y": 5}
    stages = {"inner": {"children": [{"type": "container", "children": g, "shadow": dict(shadow, inner=True)} for g in groups]},
              "outer": {"children": [{"type": "container", "children": g, "shadow": shadow} for g in groups]}}
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
    out["inner_minus_outer_ms"] = round(out["inner_render_ms"] - out["outer_render_ms"], 3)
    out["inner_over_outer"] = round(out["inner_render_ms"] / out["outer_render_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps({"passes": passes(a.reps, a.rounds), "render": render(a.rounds)}))


if __name__ == "__main__":
    main()
