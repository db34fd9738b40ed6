"""What the erase and alpha modes cost on one MI355X, beside their neighbours.  One JSON line.  Recorded only: there is no threshold.

S1 (4K, 1 000 stars) resident on the device, rendered with several frames in flight (swfr_render_resident) and with one frame in
flight (per-kernel times from the handle's HIP events), in these variants taken in turn, `--rounds` times:
  plain                    the frame as it is: no layer
  half_multiply            the first half of the stars as they are, the second half in ONE layer composited with multiply; the layer's
                           markers carry the union of all rectangles (what an ALPHA layer must carry), in every half_* variant
  half7_multiply           the same frame forced through instance 7 (SWFR_TILES_SHADERS=7): what the instance costs a frame without
                           the two operators
  half_erase / half_alpha  the same layer composited with ERASE and with ALPHA (on a handle with SWFR_FLAG_ALPHA_MODES)
  k4_multiply / k4_erase   the stars in groups of four index neighbours (tools/layer_bench.py's variant), multiply and ERASE
  path_multiply / path_erase   every star composited per path with multiply and with ERASE
Medians; every erase / alpha variant as a ratio to its multiply twin.

usage (GPU box): python tools/alpha_modes_bench.py [--frames 200] [--rounds 5]"""
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
INSTANCE = "7"


def half_layer(paths, op):
    """the first half of the paths as they are, the second half in one group whose markers carry the union of all rectangles"""
    half = len(paths) // 2
    g = lb.grouped(paths[half:], len(paths) - half, op)
    for k, f in (("x_min", np.min), ("y_min", np.min), ("x_max", np.max), ("y_max", np.max)):
        g[k][0] = g[k][-1] = f(paths[k])
    return np.concatenate([paths[:half], g])


def scenes():
    import helpers
    from swf_renderer_amd import api, synth
    W, H, _, _, (edges, paths, styles) = helpers.synth_scene(synth.S1)
    ops = dict(api.PATH_OPERATORS, **api.ALPHA_MODE_OPERATORS)
    out = {"plain": ((edges, paths, styles), None)}
    for mode in ("multiply", "erase", "alpha"):
        out["half_%s" % mode] = ((edges, half_layer(paths, ops[mode]), styles), None)
    out["half7_multiply"] = ((edges, half_layer(paths, ops["multiply"]), styles), INSTANCE)
    for mode in ("multiply", "erase"):
        out["k%d_%s" % (K, mode)] = ((edges, lb.grouped(paths, K, ops[mode]), styles), None)
        p = paths.copy()
        p["lerp"] = ops[mode] << 8
        out["path_%s" % mode] = ((edges, p, styles), None)
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
        r = S.Renderer(W, H, alpha_modes=True)
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
    out = {"frames": frames, "rounds": rounds, "width": W, "height": H, "group": K, "capacity_refusals": refused}
    for name, s in series.items():
        out[name] = {"ms_per_frame_median": round(lb._median(s["ms_per_frame"]), 4),
                     "ms_per_frame_all": [round(v, 4) for v in s["ms_per_frame"]],
                     "one_frame_in_flight_ms": {k: round(lb._median([o[k] for o in s["one_in_flight"]]), 4)
                                                for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")}}
    for name in sc:
        kind, _, mode = name.partition("_")
        if mode in ("erase", "alpha"):
            out["%s_over_%s_multiply" % (name, kind)] = round(out[name]["ms_per_frame_median"] / out["%s_multiply" % kind]["ms_per_frame_median"], 3)
    out["half7_multiply_over_half_multiply"] = round(out["half7_multiply"]["ms_per_frame_median"] / out["half_multiply"]["ms_per_frame_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(measure(a.frames, a.rounds)))


if __name__ == "__main__":
    main()
