"""What the third bitmap edge rule costs on one MI355X: the existing bitmap configurations, which must not move, and padded frames
beside the same frames unpadded.  One JSON line.  Recorded only: there is no threshold (profiles/pad_bench.txt).

Frames, resident on the device and rendered with several frames in flight (swfr_render_resident), taken in turn `--rounds` times;
ms per frame, medians:
  config4_magnified      BASELINE config 4: the textured fixture magnified to 3840 x 2160 (bilinear; tools/config_bench.py)
  config4_large_texture  a 4096 x 4096 texture sampled about 1:1 at 3840 x 2160 (bilinear, HBM-bound; tests/helpers.py)
  minified_repeat        a 1024 x 1024 box, the fixture's 139 x 208 bitmap 0.5 x, repeating (pixman's separable convolution)
  box_magnified_<rule>   a 1024 x 1024 box, the bitmap 3 x magnified in its middle (417 x 624 pixels): none, repeat, pad
  box_minified_<rule>    the same 0.45 x minified (63 x 94 pixels): none, repeat, pad
The *_pad frames need this library; --no-pad leaves them out, which is how another build (--lib, the parent's say) is timed.
Alternate the two builds run by run.

usage (GPU box): python tools/pad_bench.py [--frames 200] [--rounds 5] [--lib path] [--no-pad] [--only box_magnified]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frames(pad):
    """name -> (width, height, stage, bitmaps)"""
    import scenarios
    from helpers import fixture, large_texture_scene
    m = scenarios._m
    bmp = fixture("homestuck-beta-3.bitmap")
    out = {}
    tag4 = fixture("homestuck-beta-4")
    b = tag4["bounds"]
    sx, sy = 3840 * 20 / (b["x_max"] - b["x_min"]), 2160 * 20 / (b["y_max"] - b["y_min"])
    out["config4_magnified"] = (3840, 2160, {"children": [{"type": "shape", "definition": tag4, "matrix": m(sx, sy, -b["x_min"] * sx, -b["y_min"] * sy)}]}, [bmp])
    big = large_texture_scene()
    out["config4_large_texture"] = (3840, 2160, big["stage"], big["bitmaps"])
    box = [(0, 0), (1024 * 20, 0), (1024 * 20, 1024 * 20), (0, 1024 * 20)]

    def boxed(k, x, y, rule):
        fill = {"type": "bitmap", "bitmap_id": bmp["id"], "repeating": rule == "repeat", "smoothed": True, "matrix": m(20 * k, 20 * k, round(20 * x), round(20 * y))}
        if rule == "pad":
            fill["pad"] = True
        return (1024, 1024, {"children": [{"type": "shape", "definition": scenarios._poly_shape(box, fill)}]}, [bmp])
    out["minified_repeat"] = boxed(0.5, 0.3, 0.7, "repeat")
    for rule in ("none", "repeat") + (("pad",) if pad else ()):
        out["box_magnified_" + rule] = boxed(3, 303.4, 200.2, rule)
        out["box_minified_" + rule] = boxed(0.45, 480.3, 465.1, rule)
    return out


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(n_frames, rounds, pad, only=""):
    import swf_renderer_amd as S
    handles = {}
    for name, (w, h, stage, bitmaps) in frames(pad).items():
        if only not in name:
            continue
        r = S.Renderer(w, h)
        for b in bitmaps:
            r.add_bitmap(b)
        r.upload_edges(*r.build_frame(stage))
        r.render_resident(20)                                     # warm-up
        handles[name] = r
    series = {n: [] for n in handles}
    for _ in range(rounds):
        for n, r in handles.items():                              # the frames in turn: drift hits them alike
            r.render_resident(n_frames)
            t = r.timing()
            series[n].append(t["total_ms"] / max(t["frames"], 1))
    refused = 0
    for r in handles.values():
        st = r.stats()
        refused += sum(st[k] for k in ("pairtest_limit", "start_group_limit", "history_limit"))
        r.close()
    out = {"library": S.library_path(), "frames": n_frames, "rounds": rounds, "capacity_refusals": refused}
    for n, v in series.items():
        out[n] = {"ms_per_frame_median": round(_median(v), 4), "ms_per_frame_all": [round(x, 4) for x in v]}
    if pad and not only:
        for kind in ("box_magnified", "box_minified"):
            for rule in ("none", "repeat"):
                out["%s_pad_over_%s" % (kind, rule)] = round(out[kind + "_pad"]["ms_per_frame_median"] / out[kind + "_" + rule]["ms_per_frame_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib")
    ap.add_argument("--no-pad", action="store_true")
    ap.add_argument("--only", default="", help="only the frames whose name contains this")
    a = ap.parse_args()
    if a.lib:
        from swf_renderer_amd import api
        lib = os.path.abspath(a.lib)
        api.library_path = lambda: lib
        import swf_renderer_amd as S
        S.library_path = api.library_path
    import torch
    assert torch.cuda.is_available()                 # torch initialises HIP first
    print(json.dumps(measure(a.frames, a.rounds, not a.no_pad, a.only)))


if __name__ == "__main__":
    main()
