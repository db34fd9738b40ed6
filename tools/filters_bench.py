"""What a second filter on a layer costs on one MI355X.  One JSON line.

  render   a whole blocking render() of S1 (4K, 1 000 stars) with its stars in 8 filtered layers, each with the list [glow, drop]
           ("Filter lists"), beside the same frame with 8 single shadowed layers (the drop alone) and with the 8 groups as plain
           layers: wall clock of the call (swfr_last_path_timing), the median of `--rounds`, the three in turn within a round.  The
           expectation the figures confirm or correct: the second entry adds its own passes -- an alpha pass, two box passes and a
           finish pass a layer -- and no second sub-frame render
  --once   renders one filtered frame (after a warm-up frame) and nothing else: the run a kernel trace is taken of, in a process of its
           own, to see a chain's dispatches and that no copy sits between them

usage (GPU box): python tools/filters_bench.py [--rounds 5] | python tools/filters_bench.py --once"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GLOW = {"color": (255, 220, 40, 255), "x": 5, "y": 5, "strength": 2}
DROP = {"color": (0, 0, 0, 160), "dx": 4, "dy": 4, "x": 5, "y": 5}


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def stages(layers=8):
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    kids = api.stars_to_stage(pts, cols)["children"]
    n = (len(kids) + layers - 1) // layers
    groups = [kids[i:i + n] for i in range(0, len(kids), n)]
    return {"filtered": {"children": [{"type": "container", "children": g, "filters": [{"shadow": GLOW}, {"shadow": DROP}]} for g in groups]},
            "shadowed": {"children": [{"type": "container", "children": g, "shadow": DROP} for g in groups]},
            "plain_layers": {"children": [{"type": "container", "children": g, "layer": True} for g in groups]}}, len(groups)


def render(rounds):
    import swf_renderer_amd as S
    from swf_renderer_amd import synth
    st, n_layers = stages()
    r = S.Renderer(synth.S1["width"], synth.S1["height"])
    try:
        series = {name: [] for name in st}
        for name in st:
            r.render(st[name])                                        # warm-up: shapes registered, buffers and textures allocated
        for _ in range(rounds):
            for name in st:
                r.render(st[name])
                series[name].append(r.path_timing()["total_ms"])
    finally:
        r.close()
    out = {"layers": n_layers, "rounds": rounds, "lists": ["glow 5x5 strength 2", "drop 5x5 offset (4, 4)"]}
    for name, v in series.items():
        out[name + "_render_ms"] = round(_median(v), 3)
        out[name + "_all"] = [round(x, 3) for x in v]
    out["filtered_minus_shadowed_ms"] = round(out["filtered_render_ms"] - out["shadowed_render_ms"], 3)
    out["second_entry_per_layer_ms"] = round(out["filtered_minus_shadowed_ms"] / n_layers, 4)
    out["filtered_over_shadowed"] = round(out["filtered_render_ms"] / out["shadowed_render_ms"], 3)
    return out


def once():
    import swf_renderer_amd as S
    from swf_renderer_amd import synth
    st, _ = stages()
    r = S.Renderer(synth.S1["width"], synth.S1["height"])
    try:
        r.render(st["filtered"])
        r.render(st["filtered"])
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.once:
        once()
        return
    print(json.dumps({"render": render(a.rounds)}))


if __name__ == "__main__":
    main()
