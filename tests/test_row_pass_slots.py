"""The row pass (k2_rows, csrc/rows3.hip) at the places where its slot loops, FULL-cell routine and sample passes change path:
small frames, a handful of paths each, byte for byte against the oracle, through every route a frame can take to the device.

  * slot counts: a zigzag of T teeth has rows with exactly 2 T active edges; a kink in its left side gives one row 2 T + 1.  Rows of
    2 .. 8 edges in the eight-slot instance, 2 .. 16 in the sixteen-slot one, 9 in the eight-slot one (the queue), SWFR_FAST_LIMIT
    0 / 2 / 8, and a chunk whose rows have different counts (teeth of different lengths);
  * FULL rows: slivers whose sides cross 1, 2, 16, 17, 18 and 40 pixel columns per row (the short and the long form of full_cells3),
    leaning both ways, in both fill rules, wholly inside the frame and cut by it at x = 0 and at x = width;
  * sample passes: chunks with 1, 4, 5 and 9 rows that hold a vertex (one, one, two and three passes; a last pass of one row), and a
    chunk whose sampled rows have fewer active edges than its analytic ones (the pass's slot bound below the chunk's);
  * chunk shapes: SWFR_CHUNK_ROWS 8, 16, 32 and 64 over a path that starts in the middle of a tile-row.

The geometry is checked too: the frame builder's edges must give the rows the active-edge counts a case is named after.
Exact comparisons: (0 pixels, 0 LSB).  Runs on the GPU (-m gpu) and under tools/emu/run.py, every case through every route."""
import functools
import os

import numpy as np
import pytest

import helpers
import scenarios
from helpers import diff_stats
from host_frames import build_on_host

pytestmark = pytest.mark.gpu
EMU = bool(os.environ.get("SWFR_EMULATOR"))
REFUSALS = ("pairtest_limit", "start_group_limit", "history_limit")
KNOBS = ("SWFR_ROWS_WIDE", "SWFR_FAST_LIMIT", "SWFR_CHUNK_ROWS", "SWFR_FRAMES_IN_FLIGHT", "SWFR_TILES_SHADERS", "SWFR_BATCH_FRAMES")
ROUTES = ("render", "resident_1", "resident_4", "batch")


@pytest.fixture(scope="module", autouse=True)
def need_library(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


# ---------------------------------------------------------------------------------------------------------------- scenes
def shape(pts, rgba):
    """One polygon through `pts` (pixels; snapped to twips, 1 / 20 pixel) as a display-list child -- or, `pts` a list of polygons, all of
    them as ONE shape with one fill: one path, so where they overlap the fill rule decides."""
    polys = [pts] if isinstance(pts[0][0], (int, float)) else list(pts)
    twips = [np.rint(np.asarray(q, float) * 20).astype(int) for q in polys]
    tag = scenarios._poly_shape(twips[0], {"type": "solid", "color": scenarios._rgba(*rgba)})
    for p in twips[1:]:                                              # a further contour: move there, keep the styles
        tag["shape"]["records"].append({"type": "style-change", "move_to": {"x": int(p[0][0]), "y": int(p[0][1])}})
        for k in range(1, len(p) + 1):
            a, b = p[k - 1], p[k % len(p)]
            tag["shape"]["records"].append({"type": "edge", "delta": {"x": int(b[0] - a[0]), "y": int(b[1] - a[1])}})
    every = np.concatenate(twips)
    tag["bounds"] = {"x_min": int(every[:, 0].min()), "x_max": int(every[:, 0].max()), "y_min": int(every[:, 1].min()), "y_max": int(every[:, 1].max())}
    return {"type": "shape", "definition": tag}


def scene(w, h, polys, even_odd=False):
    cols = [(200, 30, 90, 255), (30, 160, 220, 150), (250, 200, 40, 90), (20, 220, 120, 255)]   # (`polys`: polygons, each a path of its own, or lists of polygons, each list one path)
    return dict(width=w, height=h, even_odd=even_odd, stage={"children": [shape(p, cols[i % len(cols)]) for i, p in enumerate(polys)]})


def comb(x0, y_top, y_bottom, teeth, step=12.0, kink=None, lengths=None):
    """A zigzag of `teeth` teeth between y_top and y_bottom (tooth k's tip at y_top + lengths[k] instead; the last one the longest),
    closed by a side that goes down on its left and back under the tips: a row between a tooth's ends crosses two edges per tooth
    that reaches it.  kink: y of an extra vertex in the left side -- its row has one active edge more."""
    zig = []
    for k in range(teeth):
        zig += [(x0 + step * k, y_top), (x0 + step * k + step / 2, y_bottom if lengths is None else y_top + lengths[k])]
    left = [(x0 - 6.0, y_top - 3.0)] + ([(x0 - 7.5, kink)] if kink is not None else []) + [(x0 - 6.0, y_bottom + 4.0), (x0 - 3.0, y_bottom + 4.0)]
    return left + zig[::-1]


def comb_rows(k, x0=10.0, y_top=4.0, y_bottom=28.0):
    """a comb whose rows between the teeth's ends have exactly k active edges (k odd: one row of k, the others k - 1)"""
    return comb(x0, y_top, y_bottom, k // 2, kink=(y_top + 9.5) if k % 2 else None)


def sliver(x0, y0, cols, rows=3, width=5.0, lean=1):
    """both sides advance cols - 0.5 pixels per row: they cross `cols` and `cols` + 1 pixel columns in a row; ends on row boundaries"""
    d = (cols - 0.5) * rows * lean
    return [(x0 + 0.25, y0), (x0 + 0.25 + width, y0), (x0 + 0.25 + width + d, y0 + rows), (x0 + 0.25 + d, y0 + rows)]


def kinked_box(x0, y0, rows_with_vertex, height, width=30.0):
    """a box whose ends lie on row boundaries and whose left side has a vertex in each of `rows_with_vertex` consecutive rows"""
    left = [(x0 + (1.7 if k % 2 else -2.6), y0 + 2 + k + 0.5) for k in range(rows_with_vertex)]
    return [(x0, y0), (x0 + width, y0), (x0 + width, y0 + height), (x0, y0 + height)] + left[::-1]


def active_counts(sc):
    """{path: [active edges per pixel row]} from the frame builder's arrays: an edge counts in every pixel row it overlaps"""
    e, p, _ = build_on_host(sc)
    out = []
    for q in p:
        ed = e[int(q["first_edge"]):int(q["first_edge"]) + int(q["n_edges"])]
        top, bot = np.minimum(ed["y1"], ed["y2"]).astype(np.int64), np.maximum(ed["y1"], ed["y2"]).astype(np.int64)
        ok = bot > top
        out.append([int((ok & (top < (r + 1) * 256) & (bot > r * 256)).sum()) for r in range(sc["height"])])
    return out


def cases():
    """name -> (scene, knobs, what its rows must hold: a set of active-edge counts that must occur in some path)"""
    out = {}
    for k in (2, 3, 4, 5, 6, 7, 8):
        out["slots_%d" % k] = (scene(128, 40, [comb_rows(k)]), {"SWFR_ROWS_WIDE": "0"}, {k})
    for k in (2, 3, 4, 5, 6, 7, 8, 9, 12, 16):
        out["wide_slots_%d" % k] = (scene(128, 40, [comb_rows(k)]), {"SWFR_ROWS_WIDE": "1"}, {k})
    out["slots_9_queued"] = (scene(128, 40, [comb_rows(9)]), {"SWFR_ROWS_WIDE": "0"}, {9})
    mixed = comb(10.0, 4.0, 30.0, 4, lengths=[6.0, 11.0, 17.0, 24.0])                       # rows of 8, 6, 4 and 2 edges in one chunk
    for fl in ("0", "2", "8"):
        out["fast_limit_%s" % fl] = (scene(128, 40, [mixed, comb_rows(6, x0=70.0)]), {"SWFR_FAST_LIMIT": fl}, {2, 4, 6, 8})
    out["mixed_counts"] = (scene(128, 40, [mixed, comb_rows(3, x0=70.0, y_top=9.0, y_bottom=33.0)]), {}, {2, 3, 4, 6, 8})
    for cols in (1, 2, 16, 17, 18, 40):
        w = 256 if cols > 18 else 128
        for eo in (False, True):
            # two slivers of ONE path, wound the same way, leaning right and left: where they cross the winding is 2 -- filled under the
            # nonzero rule, a hole under even-odd -- and the rows have four active edges; inside the frame ...
            inside = [[sliver(8.0, 3.0, cols), sliver(8.0 + (cols - 0.5) * 3, 3.0, cols, lean=-1)]]
            # ... and cut by the frame at x = 0 and at x = width
            cut = [sliver(-cols * 1.5 - 3.0, 12.0, cols), sliver(w - 2.0 + cols * 1.5, 12.0, cols, lean=-1), sliver(w - cols * 1.5 - 4.0, 17.0, cols), sliver(cols * 1.5, 17.0, cols, lean=-1)]
            out["full_%d_%s" % (cols, "evenodd" if eo else "nonzero")] = (scene(w, 24, inside + cut, eo), {}, {4})
    for v in (1, 4, 5, 9):
        out["vertex_rows_%d" % v] = (scene(64, 32, [kinked_box(6.3, 16.0, v, 14)]), {}, {3})
    # analytic rows of eight edges above, sampled rows of three below: the passes' slot bound is under the chunk's
    tall = comb(14.0, 3.0, 12.0, 4)
    tall = tall[:1] + [(14.0 - 7.5, 20.5), (14.0 - 4.5, 21.5), (14.0 - 7.5, 22.5), (14.0 - 4.5, 23.5), (14.0 - 7.5, 24.5), (14.0 - 6.0, 30.0), (14.0 - 3.0, 30.0)] + tall[3:]
    out["pass_bound_below_chunk_bound"] = (scene(96, 32, [tall]), {"SWFR_CHUNK_ROWS": "32"}, {3, 8})
    long_path = kinked_box(9.3, 21.0, 9, 100, width=40.0)
    for cr in ("8", "16", "32", "64"):
        out["chunk_rows_%s" % cr] = (scene(64, 128, [long_path, comb(12.0, 40.0, 110.0, 3)]), {"SWFR_CHUNK_ROWS": cr}, {3, 6})
    return out


CASES = cases()


@functools.lru_cache(maxsize=None)
def oracle(name):
    return helpers.oracle_render(CASES[name][0])


# ---------------------------------------------------------------------------------------------------------------- routes
def not_refused(r, msg):
    st = r.stats()
    assert st["frames"] >= 1 and all(st[k] == 0 for k in REFUSALS), (msg, st)


def through(route, sc):
    import swf_renderer_amd as S
    r = S.Renderer(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")))
    try:
        if route == "render":
            r.render(sc["stage"])
        elif route == "batch":                                       # (the per-frame route: the last frame is what stays in the handle)
            plain = {"children": [shape([(2, 2), (40, 5), (20, 20)], (90, 90, 200, 255))]}
            r.render_batch([plain, sc["stage"], plain, sc["stage"]])
        else:
            r.upload_edges(*build_on_host(sc))
            r.render_resident(int(route[-1]) + 1)                    # (one frame more than fit in flight: a frame set is used again)
        not_refused(r, route)
        return r.read_image(premultiplied=True)
    finally:
        r.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_row_pass_case_vs_oracle(gpu, monkeypatch, name, route):
    sc, knobs, _ = CASES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    if route.startswith("resident"):
        monkeypatch.setenv("SWFR_FRAMES_IN_FLIGHT", route[-1])
    want = oracle(name)
    assert ((want[..., 3] > 0) & (want[..., 3] < 255)).any()        # (edge pixels)
    got = through(route, sc)
    n, mx = diff_stats(got, want)
    print(name, route, "differing pixels", n, "max", mx)
    assert (n, mx) == (0, 0), (name, route)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_case_has_the_rows_it_is_named_after(name):
    sc, _, need = CASES[name]
    seen = set()
    for counts in active_counts(sc):
        seen |= set(counts)
    assert need <= seen, (name, sorted(seen))


def test_the_fill_rules_differ_where_the_slivers_cross():
    for cols in (1, 2, 16, 17, 18, 40):
        assert (oracle("full_%d_nonzero" % cols) != oracle("full_%d_evenodd" % cols)).any(), cols


def test_render_batch_into_a_device_tensor(gpu, monkeypatch):
    """every case of one frame size as ONE batch, one launch per kernel: unlike slot bounds side by side in a launch"""
    if EMU:
        pytest.skip("device tensors need the GPU")
    import torch
    import swf_renderer_amd as S
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    names = [n for n in sorted(CASES) if (CASES[n][0]["width"], CASES[n][0]["height"]) == (128, 40) and not CASES[n][0]["even_odd"]]
    assert len(names) > 12
    r = S.Renderer(128, 40)
    try:
        out = torch.zeros((len(names), 40, 128, 4), dtype=torch.uint8, device="cuda")
        r.render_batch([CASES[n][0]["stage"] for n in names], out.data_ptr(), 40 * 128 * 4)
        got = out.cpu().numpy()
        not_refused(r, "batch")
    finally:
        r.close()
    bad = [(n, diff_stats(got[k], oracle(n))) for k, n in enumerate(names) if diff_stats(got[k], oracle(n)) != (0, 0)]
    assert not bad, bad
