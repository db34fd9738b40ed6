"""What masked layers cost on one MI355X, beside plain isolated layers.  One JSON line.  Recorded only: there is no threshold.

S1 (4K, 1 000 stars) resident on the device, rendered with several frames in flight (swfr_render_resident) and with one frame in
flight (per-kernel times from the handle's HIP events), in these variants taken in turn, `--rounds` times:
  layers_k<K>_over / _multiply   the stars in plain groups of K neighbours (K = 4, 16): tools/layer_bench.py's variant, the reference point
  masks_k<K>_over / _multiply    the same stars in the same groups, the first half of a group its content and the second half its
                                 mask: one marker more per group, the same paths, the same rectangles
  near_layers_* / near_masks_*   the same with the stars first put into the order of the 256-pixel block their rectangle starts in
                                 (a group's members lie near each other, as a clip's children do)
Medians; every masked variant as a ratio to its plain-layer twin.

usage (GPU box): python tools/mask_bench.py [--frames 200] [--rounds 5]"""
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


def masked(paths, k, op):
    """the paths in groups of k neighbours: BEGIN, the first half, MASK, the second half, END -- the three markers on the union of the
    members' rectangles; the first member of each half is its surface's first paint"""
    from swf_renderer_amd import api
    out = []
    for i in range(0, len(paths), k):
        members = paths[i:i + k].copy()
        if len(members) < 2:
            out.append(members)
            continue
        half = len(members) // 2
        members["lerp"][0] = members["lerp"][half] = 1
        marker = members[:1].copy()
        marker["n_edges"], marker["fill_rule"], marker["style"], marker["lerp"] = 0, 0, 0, 0
        marker["x_min"], marker["y_min"] = members["x_min"].min(), members["y_min"].min()
        marker["x_max"], marker["y_max"] = members["x_max"].max(), members["y_max"].max()
        begin, mask, end = marker.copy(), marker.copy(), marker.copy()
        begin["kind"], mask["kind"], end["kind"] = api.PATH_GROUP_BEGIN, api.PATH_GROUP_MASK, api.PATH_GROUP_END
        end["lerp"] = op << 8
        out += [begin, members[:half], mask, members[half:], end]
    return np.concatenate(out)


def scenes():
    import helpers
    from swf_renderer_amd import api, synth
    W, H, _, _, (edges, paths, styles) = helpers.synth_scene(synth.S1)
    near = paths[np.lexsort((paths["x_min"] // 256, paths["y_min"] // 256))]
    out = {}
    for k in lb.GROUPS:
        for mode in ("over", "multiply"):
            op = api.PATH_OPERATORS[mode]
            out["layers_k%d_%s" % (k, mode)] = (edges, lb.grouped(paths, k, op), styles)
            out["masks_k%d_%s" % (k, mode)] = (edges, masked(paths, k, op), styles)
            out["near_layers_k%d_%s" % (k, mode)] = (edges, lb.grouped(near, k, op), styles)
            out["near_masks_k%d_%s" % (k, mode)] = (edges, masked(near, k, op), styles)
    return W, H, out


def measure(frames, rounds):
    import swf_renderer_amd as S
    W, H, sc = scenes()
    handles = {}
    for name in sc:
        r = S.Renderer(W, H)
        r.upload_edges(*sc[name])
        r.render_resident(20)                                     # warm-up
        handles[name] = r
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
    refused = {}
    for name, r in handles.items():
        st = r.stats()
        refused[name] = sum(st[k] for k in ("pairtest_limit", "start_group_limit", "history_limit"))
        r.close()
    out = {"frames": frames, "rounds": rounds, "width": W, "height": H, "capacity_refusals": sum(refused.values())}
    for name, s in series.items():
        out[name] = {"ms_per_frame_median": round(lb._median(s["ms_per_frame"]), 4),
                     "ms_per_frame_all": [round(v, 4) for v in s["ms_per_frame"]],
                     "one_frame_in_flight_ms": {k: round(lb._median([o[k] for o in s["one_in_flight"]]), 4)
                                                for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")}}
    for name in sc:
        if "masks_" in name:
            out[name + "_over_layers"] = round(out[name]["ms_per_frame_median"] / out[name.replace("masks_", "layers_")]["ms_per_frame_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(measure(a.frames, a.rounds)))


if __name__ == "__main__":
    main()
