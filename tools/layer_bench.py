"""What isolated layers cost on one MI355X.  One JSON line.

S1 (4K, 1 000 stars) resident on the device, rendered with several frames in flight (swfr_render_resident) and with one frame in
flight (per-kernel times from the handle's HIP events), in these variants taken in turn, `--rounds` times:
  plain                 no group: the solid instance of the tile kernel (what bench.py measures)
  layers_k<K>_over      the stars in groups of K neighbours (K = 4, 16), every group composited with OVER: instance 4
  layers_k<K>_multiply  the same groups composited with MULTIPLY
  near_k<K>_over / _multiply   the same with the stars first put into the order of the 256-pixel block their rectangle starts in, so
                        that a group's members lie near each other as a clip's children do (another picture: the painter's order
                        changes; `near_plain` is that order without groups) -- a group's markers reach every strip of the union of
                        its members' rectangles, so S1's index neighbours, which lie all over the frame, are the worst case
  per_path_multiply     no group, every star under MULTIPLY on its own: instance 3 (tools/blend_bench.py's `multiply`)
  plain_instance3 / 4   `plain` forced through the tile kernel's instances 3 and 4 (SWFR_TILES_SHADERS, read when a handle is
                        created): what the stack's 8 KB of LDS and the wider walk cost a frame that uses none of it
Medians; the layered variants as ratios to plain and to per_path_multiply, instance 4 as a ratio to instance 3.

usage (GPU box): python tools/layer_bench.py [--frames 200] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if os.environ.get("SWFR_LIB"):                          # another build of the library
    from swf_renderer_amd import api as _api
    _lib = os.path.abspath(os.environ["SWFR_LIB"])
    _api.library_path = lambda: _lib
GROUPS = (4, 16)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def grouped(paths, k, op):
    """the paths in groups of k neighbours between GROUP_BEGIN / GROUP_END markers (rectangle: the union of the members'); a group's
    first member is its surface's first paint"""
    from swf_renderer_amd import api
    out = []
    for i in range(0, len(paths), k):
        members = paths[i:i + k].copy()
        members["lerp"][0] = 1
        marker = members[:1].copy()
        marker["n_edges"], marker["fill_rule"], marker["style"], marker["lerp"] = 0, 0, 0, 0
        marker["x_min"], marker["y_min"] = members["x_min"].min(), members["y_min"].min()
        marker["x_max"], marker["y_max"] = members["x_max"].max(), members["y_max"].max()
        begin, end = marker.copy(), marker.copy()
        begin["kind"], end["kind"] = api.PATH_GROUP_BEGIN, api.PATH_GROUP_END
        end["lerp"] = op << 8
        out += [begin, members, end]
    return np.concatenate(out)


def scenes():
    """S1 as (edges, paths, styles) per variant"""
    import helpers
    from swf_renderer_amd import api, synth
    W, H, _, _, (edges, paths, styles) = helpers.synth_scene(synth.S1)
    out = {"plain": (edges, paths, styles)}
    p = paths.copy()
    p["lerp"] = api.PATH_OPERATORS["multiply"] << 8
    out["per_path_multiply"] = (edges, p, styles)
    near = paths[np.lexsort((paths["x_min"] // 256, paths["y_min"] // 256))]
    out["near_plain"] = (edges, near, styles)
    for k in GROUPS:
        for mode in ("over", "multiply"):
            out["layers_k%d_%s" % (k, mode)] = (edges, grouped(paths, k, api.PATH_OPERATORS[mode]), styles)
            out["near_k%d_%s" % (k, mode)] = (edges, grouped(near, k, api.PATH_OPERATORS[mode]), styles)
    return W, H, out


def measure(frames, rounds):
    import swf_renderer_amd as S
    W, H, sc = scenes()
    variants = [(name, name, None) for name in sc] + [("plain_instance3", "plain", "3"), ("plain_instance4", "plain", "4")]
    handles = {}
    for name, scene, knob in variants:
        if knob is None:
            os.environ.pop("SWFR_TILES_SHADERS", None)
        else:
            os.environ["SWFR_TILES_SHADERS"] = knob
        r = S.Renderer(W, H)
        r.upload_edges(*sc[scene])
        r.render_resident(20)                                     # warm-up
        handles[name] = r
    os.environ.pop("SWFR_TILES_SHADERS", None)
    series = {name: {"ms_per_frame": [], "one_in_flight": []} for name, _, _ in variants}
    for _ in range(rounds):
        for name, _, _ in variants:                               # the variants in turn: drift hits them alike
            r = handles[name]
            r.render_resident(frames)
            t = r.timing()
            series[name]["ms_per_frame"].append(t["total_ms"] / max(t["frames"], 1))
            r.render_resident(1)
            t1 = r.timing()
            series[name]["one_in_flight"].append({k: t1[k] for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")})
    for r in handles.values():
        r.close()
    out = {"frames": frames, "rounds": rounds, "width": W, "height": H}
    for name, s in series.items():
        out[name] = {"ms_per_frame_median": round(_median(s["ms_per_frame"]), 4),
                     "ms_per_frame_all": [round(v, 4) for v in s["ms_per_frame"]],
                     "mpx_per_s": round(W * H / 1e3 / _median(s["ms_per_frame"]), 1),
                     "one_frame_in_flight_ms": {k: round(_median([o[k] for o in s["one_in_flight"]]), 4)
                                                for k in ("total_ms", "setup_ms", "rows_ms", "tiles_ms")}}
    base, per_path = out["plain"]["ms_per_frame_median"], out["per_path_multiply"]["ms_per_frame_median"]
    for name in sc:
        if name.startswith("near_k"):
            out[name + "_over_near_plain"] = round(out[name]["ms_per_frame_median"] / out["near_plain"]["ms_per_frame_median"], 3)
        if name.startswith("layers_"):
            out[name + "_over_plain"] = round(out[name]["ms_per_frame_median"] / base, 3)
            out[name + "_over_per_path_multiply"] = round(out[name]["ms_per_frame_median"] / per_path, 3)
    out["instance4_over_instance3"] = round(out["plain_instance4"]["ms_per_frame_median"] / out["plain_instance3"]["ms_per_frame_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(measure(a.frames, a.rounds)))


if __name__ == "__main__":
    main()
