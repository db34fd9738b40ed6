"""What a layer's opacity costs on one MI355X, beside the same layer without one.  One JSON line.  Recorded only: there is no threshold.

S1 (4K, 1 000 stars) resident on the device, rendered with several frames in flight (swfr_render_resident) and with one frame in
flight (per-kernel times from the handle's HIP events), in these variants taken in turn, `--rounds` times:
  layers_k4_over / _multiply    the stars in plain groups of four index neighbours: tools/layer_bench.py's variant (instance 4)
  layers6_k4_over / _multiply   the same frames forced through the instance that fades (SWFR_TILES_SHADERS=6): what the instance costs
                                a frame that fades nothing
  faded_k4_over / _multiply     the same groups with opacity 128: a fade in every GROUP_END, the same paths, the same rectangles
  near_*                        the same with the stars first put into the order of the 256-pixel block their rectangle starts in
                                (a group's members lie near each other, as a clip's children do)
Medians; every faded variant as a ratio to its plain-layer twin and to the twin forced through the same instance.

usage (GPU box): python tools/fade_bench.py [--frames 200] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import layer_bench as lb  # noqa: E402

K = 4
OPACITY = 128
FADE_INSTANCE = "6"


def faded(paths, k, op, opacity):
    """layer_bench.grouped with the fade 255 - opacity in bits 24..31 of every GROUP_END's lerp"""
    from swf_renderer_amd import api
    out = lb.grouped(paths, k, op)
    ends = out["kind"] == api.PATH_GROUP_END
    out["lerp"][ends] = (out["lerp"][ends].astype(np.int64) | ((255 - opacity) << 24)).astype(out["lerp"].dtype)
    return out


def scenes():
    import helpers
    from swf_renderer_amd import api, synth
    W, H, _, _, (edges, paths, styles) = helpers.synth_scene(synth.S1)
    near = paths[np.lexsort((paths["x_min"] // 256, paths["y_min"] // 256))]
    out = {}
    for prefix, order in (("", paths), ("near_", near)):
        for mode in ("over", "multiply"):
            op = api.PATH_OPERATORS[mode]
            out["%slayers_k%d_%s" % (prefix, K, mode)] = ((edges, lb.grouped(order, K, op), styles), None)
            out["%slayers6_k%d_%s" % (prefix, K, mode)] = ((edges, lb.grouped(order, K, op), styles), FADE_INSTANCE)
            out["%sfaded_k%d_%s" % (prefix, K, mode)] = ((edges, faded(order, K, op, OPACITY), styles), None)
    return W, H, out


def measure(frames, rounds):
    import swf_renderer_amd as S
    W, H, sc = scenes()
    handles = {}
    for name, (arrays, knob) in sc.items():
        if knob is None:
            os.environ.pop("SWFR_TILES_SHADERS", None)
        else:
            os.environ["SWFR_TILES_SHADERS"] = knob
        r = S.Renderer(W, H)
        r.upload_edges(*arrays)
        r.render_resident(20)                                     # warm-up
        handles[name] = r
    os.environ.pop("SWFR_TILES_SHADERS", None)
    series = {name: {"ms_per_frame": [], "one_in_flight": []} for name in sc}
    for _ in range(rounds):
        for name in sc:                                           # the variants in turn: drift hits them alike
            r = handles[name]
            r.render_resident(frames)
            t = r.timing()
            series[name]["ms_per_frame"].append(t["total_ms"] / max(t["frames"], 1))
            r.render_resident(1)
            t1 = r.timing()
            series[name]["one_in_flight"].append({k: t1[k] for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")})
    refused = 0
    for r in handles.values():
        st = r.stats()
        refused += sum(st[k] for k in ("pairtest_limit", "start_group_limit", "history_limit"))
        r.close()
    out = {"frames": frames, "rounds": rounds, "width": W, "height": H, "group": K, "opacity": OPACITY, "capacity_refusals": refused}
    for name, s in series.items():
        out[name] = {"ms_per_frame_median": round(lb._median(s["ms_per_frame"]), 4),
                     "ms_per_frame_all": [round(v, 4) for v in s["ms_per_frame"]],
                     "one_frame_in_flight_ms": {k: round(lb._median([o[k] for o in s["one_in_flight"]]), 4)
                                                for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")}}
    for name in sc:
        if "faded_" in name:
            for twin in ("layers_", "layers6_"):
                out["%s_over_%s" % (name, twin.rstrip("_"))] = round(out[name]["ms_per_frame_median"] / out[name.replace("faded_", twin)]["ms_per_frame_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(measure(a.frames, a.rounds)))


if __name__ == "__main__":
    main()
