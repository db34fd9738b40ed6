"""Parity tests proper: the HIP path (through the C-ABI of libswfr.so) against the oracle on the same
inputs, against the committed goldens, and at BASELINE.json's full sizes."""
import hashlib
import json
import os

import numpy as np
import pytest

import scenarios
import helpers
from helpers import GOLD, diff_stats, fixture, golden, oracle_render, product_render
from oracle import canvas_replay as cr

pytestmark = pytest.mark.gpu
SC = scenarios.scenarios()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu):
    import swf_renderer_amd as S
    assert os.path.exists(S.library_path()), "libswfr.so must be built: the product has no fallback"


_oracle_polys = helpers.oracle_polys


# ---- every scenario: HIP vs oracle and vs the committed libcairo golden
@pytest.mark.parametrize("name", sorted(SC))
def test_scenario_vs_oracle_and_golden(name):
    sc = SC[name]
    got = product_render(sc)
    n, mx = diff_stats(got, oracle_render(sc))
    if sc["exact"]:
        assert (n, mx) == (0, 0), "HIP vs oracle"          # integer path: bit-exact
    else:
        assert mx <= 1, (n, mx)                            # float shading: +-1 LSB per channel (north star)
    n, mx = diff_stats(got, golden("cairo_" + name, "rgba_premul"))
    if sc["exact"]:
        assert (n, mx) == (0, 0), "HIP vs libcairo golden"
    else:
        assert mx <= sc.get("tolerance", 1), (n, mx)


# ---- the reference's own golden PNGs (straight RGBA through the un-premultiply kernel)
@pytest.mark.parametrize("name", ["squares", "triangle", "homestuck-beta-1"])
def test_reference_golden_png(name):
    import swf_renderer_amd as S
    sc = SC["fixture_" + name]
    r = S.Renderer(sc["width"], sc["height"])
    r.render(sc["stage"])
    assert diff_stats(r.read_image(premultiplied=False), golden("ref_" + name, "rgba_straight")) == (0, 0)
    r.close()


def test_reference_textured_golden_png():
    """The 7th golden of the reference: bitmap fill minified 2.58x (CAIRO_FILTER_GOOD = pixman separable convolution)."""
    import swf_renderer_amd as S
    sc = SC["fixture_homestuck-beta-4"]
    r = S.Renderer(sc["width"], sc["height"])
    for bm in sc["bitmaps"]:
        r.add_bitmap(bm)
    r.render(sc["stage"])
    out = r.read_image(premultiplied=False)
    r.close()
    ref = golden("ref_homestuck-beta-4", "rgba_straight")
    assert diff_stats(out, ref) == (0, 0)      # pixman's own 16.16 sample positions, integer weights and sums: byte for byte


@pytest.mark.parametrize("ratio,fname,allowed", [(0, "0", 0), (0.5, "32768", 4), (1, "65536", 0)])
def test_reference_morph_golden_png(ratio, fname, allowed):
    import swf_renderer_amd as S
    w, h, stage = cr.stage_for_morph_shape(fixture("homestuck-beta-29"), ratio)
    r = S.Renderer(w, h)
    r.render(stage)
    n, mx = diff_stats(r.read_image(premultiplied=False), golden("ref_homestuck-beta-29_" + fname, "rgba_straight"))
    r.close()
    assert n <= allowed and mx <= (1 if allowed else 0)    # 4 px / 1 LSB at ratio 0.5


def test_render_batch_morph_ratios_vs_sequential_and_oracle():
    """swfr_render_batch: different frames pipelined over the streams, each written straight into its slot of a device tensor."""
    import torch
    import swf_renderer_amd as S
    tag = fixture("homestuck-beta-29")
    ratios = [k / 40 for k in range(41)]
    stages = [cr.stage_for_morph_shape(tag, q)[2] for q in ratios]
    w, h, _ = cr.stage_for_morph_shape(tag, 0.0)
    r = S.Renderer(w, h)
    out = torch.zeros((len(stages), h, w, 4), dtype=torch.uint8, device="cuda")
    r.render_batch(stages, out.data_ptr(), h * w * 4)
    got = out.cpu().numpy()
    last = r.read_image(premultiplied=True)
    assert (last == got[-1]).all()
    for i, st in enumerate(stages):
        r.render(st)
        assert (r.read_image(premultiplied=True) == got[i]).all(), i
    r.close()
    for i in (0, 13, 40):
        assert diff_stats(got[i], oracle_render(dict(width=w, height=h, stage=stages[i]))) == (0, 0), i
    # textured + stroked frames in one batch, no destination: the last frame is readable
    sc_a, sc_b = SC["fixture_homestuck-beta-4"], SC["stroke_curves"]
    r = S.Renderer(sc_a["width"], sc_a["height"])
    for bm in sc_a["bitmaps"]:
        r.add_bitmap(bm)
    r.render_batch([sc_a["stage"], sc_a["stage"], sc_a["stage"]])
    got = r.read_image(premultiplied=True)
    r.close()
    assert diff_stats(got, oracle_render(sc_a)) == (0, 0)


def test_render_batch_on_a_handle_that_rendered_a_simpler_scene_before():
    """The per-frame route of swfr_render_batch (no device destination) must launch the queued-row kernels for every frame, whatever
    the handle's previous scene needed: a handle that rendered a scene without queued rows and then batches one with queued rows
    (round-2 advisor finding: 1780 wrong pixels, SWFR_OK)."""
    import swf_renderer_amd as S
    simple, queued = SC["translucent_stack"], SC["morph_round_stroke_090"]
    w, h = max(simple["width"], queued["width"]), max(simple["height"], queued["height"])
    r = S.Renderer(w, h)
    try:
        r.render(simple["stage"])
        assert r.stats()["queued_rows"] == 0
        for n in (1, 4):                                        # (n - 1) % frames-in-flight == 0 and != 0: the kept frame lands on set 0 / another
            r.render_batch([queued["stage"]] * n)
            assert diff_stats(r.read_image(premultiplied=True), oracle_render(dict(queued, width=w, height=h))) == (0, 0), n
        assert r.stats()["queued_rows"] > 0
    finally:
        r.close()


def test_edges_outside_every_path_and_overlapping_edge_ranges_are_refused():
    """swfr_upload_edges: every edge belongs to exactly one path (the kernels index the path table with the edge's owner)."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    sc = SC["fixture_triangle"]
    host = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
    edges, paths, styles = host.build_frame(sc["stage"])
    host.close()
    r = S.Renderer(sc["width"], sc["height"])
    try:
        r.upload_edges(edges, paths, styles)                    # the builder's own output is fine
        orphan = np.concatenate([edges, edges[:1]])             # one more edge than the paths cover, with a wild owner
        orphan[-1]["reserved"] = 50000000
        with pytest.raises(S.SwfrError) as e:
            r.upload_edges(orphan, paths, styles)
        assert e.value.code == api.ERR_INVALID
        twice = np.concatenate([paths, paths[:1]])              # two paths over the same edges
        with pytest.raises(S.SwfrError) as e:
            r.upload_edges(edges, twice, styles)
        assert e.value.code == api.ERR_INVALID
        with pytest.raises(S.SwfrError) as e:
            r.upload_edges(edges, paths[:0], styles)            # edges but no path at all
        assert e.value.code == api.ERR_INVALID
        r.upload_edges(edges, paths, styles)
        r.render_resident(1)
        assert diff_stats(r.read_image(premultiplied=True), oracle_render(sc)) == (0, 0)
    finally:
        r.close()


def test_resident_scene_as_frames_per_launch_and_mapped_read_back():
    """swfr_render_resident_batched (the saturated-GPU measurement of bench.py): every frame of every launch is a full recomputation
    into its own buffers -- the last one equals the oracle, for a scene with queued rows too; swfr_read_image_async/_wait hand out the
    same pixels as swfr_read_image, and the render + read-back loop timed below the ABI leaves the last frame readable."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    for name in ("translucent_stack", "morph_round_stroke_090", "fixture_homestuck-beta-1"):
        sc = SC[name]
        r = S.Renderer(sc["width"], sc["height"])
        try:
            host = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
            scene = host.build_frame(sc["stage"])
            host.close()
            r.upload_edges(*scene)
            ms = r.render_resident_batched(5, 3)
            assert ms > 0
            want = oracle_render(sc)
            got = r.read_image(premultiplied=True)
            assert diff_stats(got, want) == (0, 0), name
            r.read_image_async(premultiplied=True)
            assert (np.asarray(r.read_image_wait()) == got).all()
            r.read_image_async(premultiplied=False)
            assert (np.asarray(r.read_image_wait()) == r.read_image(premultiplied=False)).all()
            for overlap in (True, False):
                assert r.render_sequence_readback([sc["stage"], sc["stage"]], 2, premultiplied=True, overlap=overlap) > 0
                assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), (name, overlap)
        finally:
            r.close()


def test_mapped_read_back_is_not_torn_by_frames_queued_before_the_wait():
    """swfr_read_image_async queues the copy of the last frame and returns; a multi-frame render of ANOTHER scene issued before
    swfr_read_image_wait runs on the other frame sets' streams -- which wait for the copy on the device -- so the image that comes
    back is the first scene's, bit for bit (the advisor's round-3 finding: frame sets 1..3 were not ordered behind the handle's stream)."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api, synth
    cfg = dict(synth.S1)
    W, H = cfg["width"], cfg["height"]                      # a 33 MB frame: the copy takes long enough for seven frames to overtake it
    pts, cols = synth.scene(**cfg)
    host = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY)
    a = host.build_frame(api.stars_to_stage(pts, cols))
    b = host.build_frame(api.stars_to_stage(pts[::-1] + 40, cols[::-1]))       # other painter's order, shifted: different pixels
    host.close()
    r = S.Renderer(W, H)
    try:
        r.upload_edges(*a)
        r.render_resident(7)                                 # the last frame lies in a frame set other than 0
        first = np.array(r.read_image(premultiplied=True))
        for _ in range(3):
            r.upload_edges(*a)
            r.render_resident(7)
            r.read_image_async(premultiplied=True)
            r.upload_edges(*b)
            r.render_resident(7)                             # rasterizes into every frame set, the one being read included
            got = np.asarray(r.read_image_wait())
            assert (got == first).all()
        second = np.array(r.read_image(premultiplied=True))
        assert (second != first).any()
    finally:
        r.close()


# ---- BASELINE config 3: 256 morph ratios through one handle (reduced frame; oracle finishes in seconds)
def test_morph_256_ratios_vs_oracle():
    import swf_renderer_amd as S
    tag = fixture("homestuck-beta-29")
    w, h, _ = cr.stage_for_morph_shape(tag, 0)
    r = S.Renderer(w, h)
    for k in range(256):
        _, _, stage = cr.stage_for_morph_shape(tag, k / 255)
        r.render(stage)
        got = r.read_image(premultiplied=True)
        assert diff_stats(got, oracle_render(dict(width=w, height=h, stage=stage))) == (0, 0), k
    r.close()


# ---- fuzz: random polygons through the whole host+device path
def test_fuzz_polygons_vs_oracle():
    rng = np.random.default_rng(5)
    for it in range(160):
        sc, (mode, eo, pts) = helpers.rand_polygon_scene(rng, it)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), (it, mode, eo, pts)


def test_fuzz_layered_translucent_vs_oracle():
    rng = np.random.default_rng(11)
    for it in range(40):
        sc = helpers.rand_layered_translucent_scene(rng)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), it


def test_fuzz_stroked_shapes_vs_oracle():
    """Random stroked (morph) shapes -- curves, rectilinear box strokes, round caps / joins, hairlines, reflected and off-frame
    placements -- through the whole product path against the oracle's pixels."""
    rng = np.random.default_rng(78)
    for it in range(120):
        sc = helpers.rand_stroked_scene(rng)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), it


def test_fuzz_bitmap_fills_vs_oracle():
    """Random bitmap-filled shapes (repeat / no-repeat, 20x minified to 30x magnified, rotated, reflected, partly off-frame, on a
    clear frame and over translucent solids): the shader uses pixman's integer sample positions, weights and sums, so the frame
    is bit-identical to the oracle's."""
    from helpers import rand_bitmap_scene
    rng = np.random.default_rng(4242)
    painted = 0
    for it in range(60):
        sc = rand_bitmap_scene(rng)
        ref = oracle_render(sc)
        assert diff_stats(product_render(sc), ref) == (0, 0), it
        painted += int((ref[..., 3] > 0).sum())
    assert painted > 50000


def test_fuzz_radial_gradients_vs_oracle():
    """Radial / focal gradient fills: exact 64-bit B and C of pixman's quadratic, the root in doubles (correctly rounded sqrt, no
    fused multiply-adds), the colour ramp in single precision -- the frame is bit-identical to the oracle's (which is bit-identical
    to libcairo's)."""
    from helpers import rand_radial_scene
    rng = np.random.default_rng(777)
    painted = 0
    for it in range(60):
        sc = rand_radial_scene(rng)
        ref = oracle_render(sc)
        assert diff_stats(product_render(sc), ref) == (0, 0), it
        painted += int((ref[..., 3] > 0).sum())
    assert painted > 50000


@pytest.mark.parametrize("case", helpers.SOAK_TIE_CASES)
def test_soak_regressions_tied_edges(case):
    """Scenes soak runs (tools/soak.py gpu) found: edges whose cells coincide at a pixel row's first sample row.  Their order in
    Cairo's list decides whether the row is converted analytically: two active edges keep the order of the last time the list was
    looked at while they differed (every sample row of a sampled pixel row, the first one of an analytic row -- reconstructed per
    row from the path's edges); a new edge goes before a tying active one when another new edge sorts between that edge's
    predecessor and the tie (Cairo's merge consumes its two lists in alternating runs); edges that arrive at the same sample row
    come out of Cairo's merge sort of the bucket, replayed for up to sixteen of them (long 300/171: a stroke cut by the frame's
    top edge starts twelve edges at sample row 0).  Whether an earlier row was sampled is itself
    decided with these rules when edges tie at its first sample row and at least one of them is new there (big 300/146: three
    edges of a round join start in one cell and leave it in the opposite order).  The last two are host-side findings of the
    oracle-vs-libcairo soak (tests/test_oracle_vs_cairo.py): the gradient translation fix that is skipped when the centre of the
    operation leaves 16.16, and a gradient with only transparent stops as a clear source.  mixed 777777/722 is the one scene of
    20 000 that the replay refused while it followed the history of two older coincident edges one level deep only (round 2's soak);
    it follows two levels now and the scene is exact."""
    from helpers import soak_scene
    sc = soak_scene(*case)
    assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), case


def test_tie_of_two_older_edges_decides_whether_the_row_before_was_sampled():
    """Soak finding (big 7000/2285, child 3; fixture written by tools/make_soak_fixture.py): three edges of a round join tie at the
    first sample row of a pixel row and leave it in another order, so Cairo samples that row -- and none of them is new there, so
    their order comes from the row before that (one level of history behind the history, tied_order_at<1>)."""
    import json
    sc = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "soak_big_7000_2285_child3.json")))
    ref = oracle_render(sc)
    assert (np.asarray(ref)[..., 3] > 0).sum() > 5000
    assert diff_stats(product_render(sc), ref) == (0, 0)


def test_rectilinear_stroke_outside_the_frame_leaves_the_surface_clear():
    """Soak finding of round 4 (mixed 7100/2196, children 0 and 1): an axis-parallel stroke that lies below the frame while its
    approximate extents (the miter reach) still touch it.  Cairo's box stroker hands over boxes that miss the operation's rectangle:
    nothing is drawn and the surface KEEPS its clear state, so the translucent fill that follows is composited with the SOURCE rule
    (0x7f rounding); the frame builder used to clip those boxes away first and then took "no boxes at all" for drawn (OVER, 0x80
    rounding: four pixels off by one)."""
    import json
    sc = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "soak_mixed_7100_2196_child0_1.json")))
    ref = oracle_render(sc)
    assert (np.asarray(ref)[..., 3] > 0).sum() > 500
    assert diff_stats(product_render(sc), ref) == (0, 0)


def test_tile_with_an_uncovered_path_row_is_not_a_full_cover():
    """Soak finding (large frames): a path whose bottom lies less than a sample row below a pixel boundary has a last pixel row with
    no active sample row at all.  A tile that the path covers completely in its other rows is then neither empty nor full although
    no single pixel of it is partial: it must take the accumulate-and-scan route, not the full-cover shortcut."""
    scenes = helpers.uncovered_path_row_scenes()
    assert len(scenes) == 8
    for key, sc in scenes:                  # bottoms at y = 242.026 (the case), 242.0, 242.48, opaque and translucent; two soak scenes
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), key


# ---- every internal route of the row/tile kernels gives the same pixels
@pytest.mark.parametrize("env", [{"SWFR_FAST_LIMIT": "0"}, {"SWFR_FAST_LIMIT": "3"}, {"SWFR_CHUNK_ROWS": "64"}, {"SWFR_CHUNK_ROWS": "16"}, {"SWFR_CHUNK_ROWS": "8"},
                                 {"SWFR_CHUNK_ROWS": "8", "SWFR_FAST_LIMIT": "3"},
                                 {"SWFR_CHUNK_ROWS": "32", "SWFR_FAST_LIMIT": "3"}, {"SWFR_STRIP_ORDER": "0"}, {"SWFR_FRAMES_IN_FLIGHT": "1"},
                                 {"SWFR_FRAMES_IN_FLIGHT": "4", "SWFR_CHUNK_ROWS": "16"}, {"SWFR_BATCH_FRAMES": "1"},
                                 {"SWFR_TILES_GRID": "7"}, {"SWFR_TILES_GRID": "300", "SWFR_STRIP_ORDER": "0"}])
def test_kernel_route_knobs_are_pixel_identical(env, monkeypatch):
    """SWFR_FAST_LIMIT sends rows with more active edges than the limit (0: every row) to the queued-row kernels (k2_rows_slow /
    k2_rows_huge) instead of the fast routine of k2_rows; SWFR_CHUNK_ROWS picks the pixel rows per k2_rows wavefront (8, 16, 32 or 64;
    by default the largest that still gives a thousand wavefronts); SWFR_STRIP_ORDER=0 launches the strips of k2_tiles row-major
    instead of heaviest first; SWFR_FRAMES_IN_FLIGHT is the number of frame sets (streams, intermediate buffers) consecutive
    frames rotate over; SWFR_BATCH_FRAMES=1 makes swfr_render_batch launch every frame by itself; SWFR_TILES_GRID is the number of
    k2_tiles wavefronts per launch (each paints slots k, k + grid, ... of the launch list with the next strips' records prefetched; by
    default one per strip for small frames and half as many as strips from 8 192 strips on).  Same bytes either way."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for name in ("config2_homestuck-beta-1", "translucent_stack", "evenodd_pentagram", "offframe_fill_stroke", "morph_128",
                 "stroke_curves", "morph_round_stroke_090"):
        sc = SC[name]
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), (env, name)


@pytest.mark.parametrize("env", [{"SWFR_GRAPHS": "1"}, {"SWFR_RESIDENT_BATCH": "1"}, {"SWFR_RESIDENT_BATCH": "2"}, {"SWFR_RESIDENT_BATCH": "4"}, {"SWFR_RESIDENT_BATCH": "2", "SWFR_FRAMES_IN_FLIGHT": "2"},
                                 {"SWFR_RESIDENT_BATCH": "1", "SWFR_EVENT_STRIDE": "1000"}, {"SWFR_EVENT_STRIDE": "1000"}])
def test_resident_frames_as_graph_launches_and_as_frames_per_launch(env, monkeypatch):
    """The ways swfr_render_resident can issue its frames -- every frame one hipGraphLaunch (SWFR_GRAPHS=1), one launch chain per frame
    (SWFR_RESIDENT_BATCH=1), or groups of frame sets as one launch per kernel (SWFR_RESIDENT_BATCH, default 2 for calls without per-kernel
    events: SWFR_EVENT_STRIDE larger than the call) -- render the same frames: the last of 7 (and of 2) equals the oracle, for a
    scene without and one with queued rows."""
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SWFR_EVENT_STRIDE", "1000000")
    for name in ("translucent_stack", "morph_round_stroke_090"):
        sc = SC[name]
        host = S.Renderer(sc["width"], sc["height"], device=api.DEVICE_HOST_ONLY)
        scene = host.build_frame(sc["stage"])
        host.close()
        r = S.Renderer(sc["width"], sc["height"])
        try:
            r.upload_edges(*scene)
            want = oracle_render(sc)
            for frames in (7, 2, 5):
                r.render_resident(frames)
                assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), (env, name, frames)
        finally:
            r.close()


# ---- BASELINE configs 3 and 4 at their full frame sizes (a few frames; the oracle needs seconds)
def test_config3_morph_1080p_vs_oracle():
    tag = fixture("homestuck-beta-29")
    b, mb = tag["bounds"], tag["morph_bounds"]
    x0, x1 = min(b["x_min"], mb["x_min"]), max(b["x_max"], mb["x_max"])
    y0, y1 = min(b["y_min"], mb["y_min"]), max(b["y_max"], mb["y_max"])
    sx, sy = 1920 * 20 / (x1 - x0), 1080 * 20 / (y1 - y0)
    for k in (0, 77, 255):
        sc = dict(width=1920, height=1080, stage={"children": [
            {"type": "morph-shape", "definition": tag, "ratio": k / 255, "matrix": scenarios._m(sx, sy, -x0 * sx, -y0 * sy)}]})
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), k


def test_config3_morph_256_ratios_1080p_as_one_batch():
    """BASELINE.json config 3 as the reference runs it (node-canvas-renderer.spec.ts:84-116: one render per ratio) but through
    swfr_render_batch: 256 ratios at 1920x1080 into one device tensor, groups of frames per kernel launch; a sample of the
    ratios against the oracle, and every frame against the per-frame path for one more."""
    import torch
    import swf_renderer_amd as S
    tag = fixture("homestuck-beta-29")
    b, mb = tag["bounds"], tag["morph_bounds"]
    x0, x1 = min(b["x_min"], mb["x_min"]), max(b["x_max"], mb["x_max"])
    y0, y1 = min(b["y_min"], mb["y_min"]), max(b["y_max"], mb["y_max"])
    sx, sy = 1920 * 20 / (x1 - x0), 1080 * 20 / (y1 - y0)
    stages = [{"children": [{"type": "morph-shape", "definition": tag, "ratio": k / 255, "matrix": scenarios._m(sx, sy, -x0 * sx, -y0 * sy)}]}
              for k in range(256)]
    r = S.Renderer(1920, 1080)
    out = torch.zeros((256, 1080, 1920, 4), dtype=torch.uint8, device="cuda")
    r.render_batch(stages, out.data_ptr(), 1080 * 1920 * 4)
    for k in (0, 63, 64, 77, 128, 255):                     # (63 / 64: the last frame of one launch group and the first of the next)
        got = out[k].cpu().numpy()
        assert diff_stats(got, oracle_render(dict(width=1920, height=1080, stage=stages[k]))) == (0, 0), k
    r.render(stages[200])
    assert (r.read_image(premultiplied=True) == out[200].cpu().numpy()).all()
    r.close()


def test_config4_textured_4k_vs_oracle():
    """Bitmap fill magnified to 3840x2160 (bilinear region of FILTER_GOOD): the HIP shader and the oracle both sample at
    pixman's integer 16.16 positions with its 7-bit weights, so the frames are identical; against libcairo that arithmetic is
    pinned at reduced size (cairo_bitmap_magnified.npz, tests/test_oracle_vs_cairo.py)."""
    tag = fixture("homestuck-beta-4")
    b = tag["bounds"]
    sx, sy = 3840 * 20 / (b["x_max"] - b["x_min"]), 2160 * 20 / (b["y_max"] - b["y_min"])
    sc = dict(width=3840, height=2160, bitmaps=[fixture("homestuck-beta-3.bitmap")], stage={"children": [
        {"type": "shape", "definition": tag, "matrix": scenarios._m(sx, sy, -b["x_min"] * sx, -b["y_min"] * sy)}]})
    assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0)


def test_config4_large_texture_4k_vs_oracle():
    """Config 4 with a texture that does not fit a cache (4096 x 4096, 64 MB, sampled about 1:1 over the 4K frame)."""
    from helpers import large_texture_scene
    sc = large_texture_scene()
    assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0)


# ---- full BASELINE sizes
_s_scene = helpers.synth_scene


def test_s1_4k_10k_edges_known_answer_and_properties():
    import swf_renderer_amd as S
    from swf_renderer_amd import synth, distributed as D
    W, H, fx, cols, (edges, paths, styles) = _s_scene(synth.S1)
    r = S.Renderer(W, H)
    r.render_edges(edges, paths, styles)
    img = r.read_image(premultiplied=True)
    kat = json.load(open(os.path.join(GOLD, "s1_kat.json")))
    rows = [hashlib.sha256(img[y:y + 16].tobytes()).hexdigest()[:16] for y in range(0, H, 16)]
    bad = [i for i, (a, b) in enumerate(zip(rows, kat["tile_row_sha256_16"])) if a != b]
    assert not bad, "tile rows differing from libcairo: %s" % bad[:10]
    assert hashlib.sha256(img.tobytes()).hexdigest() == synth.S1_SHA256_PREMUL     # libcairo known answer
    crops = np.load(os.path.join(GOLD, "cairo_s1_crops.npz"))
    for key in crops.files:
        x, y = map(int, key.split("_"))
        assert (img[y:y + 256, x:x + 256] == crops[key]).all(), key
    # idempotence: rendering the resident scene again gives the same bytes
    r.render_resident(3)
    assert (r.read_image(premultiplied=True) == img).all()
    # straight read-back equals the reference's un-premultiply rule applied on the host
    assert (r.read_image(premultiplied=False) == cr.unpremultiply(img)).all()
    r.close()
    # band sharding: two handles rendering interleaved tile-rows assemble to the same frame
    slabs = []
    for rank in range(2):
        rb = S.Renderer(W, H, band_index=rank, band_count=2)
        rb.render_edges(edges, paths, styles)
        slabs.append(D.extract_slab(rb.read_image(premultiplied=True), rank, 2))
        rb.close()
    assert (D.assemble(slabs, W, H) == img).all()


def test_s2_8k_100k_edges_vs_oracle():
    import swf_renderer_amd as S
    from swf_renderer_amd import synth
    W, H, fx, cols, (edges, paths, styles) = _s_scene(synth.S2)
    r = S.Renderer(W, H)
    r.render_edges(edges, paths, styles)
    img = r.read_image(premultiplied=True)
    # several frames in flight: two frames per kernel launch, the tile pass in its paired shape (two strips per wavefront, cost-ordered)
    r.render_resident(5)
    again = r.read_image(premultiplied=True)
    r.close()
    # the oracle closes polygons (close_path); the scene builder draws the reference's explicit final lineTo.
    # Both merge the same collinear vertices, so the pixels agree (checked for S1 against libcairo).
    assert diff_stats(img, _oracle_polys(fx, cols, W, H)) == (0, 0)
    assert (again == img).all()


def test_twenty_thousand_paths_in_three_tile_rows_vs_oracle():
    """k2_bin builds a tile-row's list in rounds of 16 384 paths and windows of 4 096 hits: here 20 000 small stars crowd a 640x48
    frame, so every tile-row's list takes two rounds and more than one window (S2's 10 000 paths: one round, one window)."""
    import swf_renderer_amd as S
    cfg = helpers.TWENTY_THOUSAND_PATHS
    W, H, fx, cols, (edges, paths, styles) = _s_scene(cfg)
    assert len(paths) > 16384
    r = S.Renderer(W, H)
    r.render_edges(edges, paths, styles)
    img = r.read_image(premultiplied=True)
    r.render_resident(3)                                                  # (the strips' launch order by the previous frame's costs)
    again = r.read_image(premultiplied=True)
    r.close()
    assert diff_stats(img, _oracle_polys(fx, cols, W, H)) == (0, 0)
    assert (again == img).all()


def test_s2_8k_sharded_over_eight_band_handles_vs_oracle():
    """BASELINE.json config 5 on one GPU: the 100k-edge 8K scene rasterized by eight handles, handle k taking the tile-rows
    t with t % 8 == k exactly as rank k of an 8-GPU node does; the eight slabs assembled by
    distributed.assemble equal the CPU oracle's frame."""
    import swf_renderer_amd as S
    from swf_renderer_amd import synth, distributed as D
    W, H, fx, cols, (edges, paths, styles) = _s_scene(synth.S2)
    slabs = []
    for rank in range(8):
        rb = S.Renderer(W, H, band_index=rank, band_count=8)
        rb.render_edges(edges, paths, styles)
        slabs.append(rb.band_slab())
        assert slabs[-1].shape == D.slab_shape(W, H, rank, 8)
        rb.close()
    assert diff_stats(D.assemble(slabs, W, H), _oracle_polys(fx, cols, W, H)) == (0, 0)


def test_s2_8k_eight_contiguous_block_handles_render_into_one_image():
    """The N>1 data path FramePipeline uses, on one GPU: eight handles with SWFR_FLAG_BANDS_CONTIGUOUS, handle k owning tile-rows
    [k*n, (k+1)*n), all rendering straight into ONE padded device image through swfr_set_targets + swfr_render_resident_async
    (no slab copy, no assembly pass).  The image equals the CPU oracle's frame; rows past the frame stay zero."""
    import torch
    import swf_renderer_amd as S
    from swf_renderer_amd import synth, distributed as D
    W, H, fx, cols, (edges, paths, styles) = _s_scene(synth.S2)
    world = 8
    hp = D.padded_height(H, world)
    image = torch.zeros((hp, W, 4), dtype=torch.uint8, device="cuda")
    handles = []
    for rank in range(world):
        rb = S.Renderer(W, H, band_index=rank, band_count=world, contiguous_bands=True)
        rb.set_targets([image.data_ptr()])
        rb.upload_edges(edges, paths, styles)
        assert rb.render_resident_async() == 0
        handles.append(rb)
    for rb in handles:
        rb.wait()
        rb.close()
    torch.cuda.synchronize()
    out = image.cpu().numpy()
    assert not out[H:].any()
    assert diff_stats(out[:H], _oracle_polys(fx, cols, W, H)) == (0, 0)


def test_frame_pipeline_over_rccl_single_rank():
    """FramePipeline on the real backend ("nccl" = RCCL) with the one rank this box has: set_targets, async frames on the handle's
    streams, torch's stream waiting for them, the in-place gather (send-to-self here) and the buffer-release events, eight steps
    over three buffers; the S1 frame equals the libcairo known answer; then RotatingPipeline on the same backend (block buffers, one
    all-to-all per group, five groups over two group buffers).  (N>1 ranks: tests/test_distributed.py, gloo.)"""
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "nccl_pipeline_worker.py")],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and b"PIPELINE_OK" in p.stdout, p.stdout.decode()[-3000:]


def test_block_targets_three_handles_render_into_block_buffers():
    """swfr_render_resident_group_to (what RotatingPipeline queues per group): every handle of a three-way split renders several
    frames into device buffers that hold ONLY its own block of tile-rows -- more buffers than the handle has frame sets -- and the blocks
    stacked in rank order are the oracle's frame, for every one of the frames."""
    import torch
    import swf_renderer_amd as S
    from swf_renderer_amd import api, distributed as D
    sc = SC["translucent_stack"]
    w, h = sc["width"], sc["height"]
    want = oracle_render(sc)
    host = S.Renderer(w, h, device=api.DEVICE_HOST_ONLY)
    scene = host.build_frame(sc["stage"])
    host.close()
    world, frames = 3, 6
    rows = D.block_rows(h, world) * D.TILE_H
    blocks = []
    for rank in range(world):
        rb = S.Renderer(w, h, band_index=rank, band_count=world, contiguous_bands=True)
        try:
            bufs = torch.zeros((frames, rows, w, 4), dtype=torch.uint8, device="cuda")
            rb.upload_edges(*scene)
            rb.render_resident(1)
            used = rb.render_resident_group_to([bufs[f].data_ptr() for f in range(frames)])
            assert used != 0
            rb.wait()
            torch.cuda.synchronize()
            blocks.append(bufs.cpu().numpy())
        finally:
            rb.close()
    for f in range(frames):
        img = np.concatenate([blocks[rank][f] for rank in range(world)], axis=0)[:h]
        assert diff_stats(img, want) == (0, 0), f


def test_contiguous_blocks_three_handles_ragged_height_and_slab_copy():
    """A frame whose tile-rows do not divide by the handle count (the last block is short, and one handle may own nothing):
    per-handle block slabs (swfr_copy_band_slab) stacked by distributed.assemble_blocks equal the oracle."""
    import swf_renderer_amd as S
    from swf_renderer_amd import distributed as D
    sc = SC["stroke_curves"]
    w, h = sc["width"], sc["height"]
    want = oracle_render(sc)
    for world in (3, 7, D.tile_rows(h) + 2):
        slabs = []
        for rank in range(world):
            rb = S.Renderer(w, h, band_index=rank, band_count=world, contiguous_bands=True)
            rb.render(sc["stage"])
            slab = rb.band_slab()
            full = np.zeros((D.block_rows(h, world) * 16, w, 4), dtype=np.uint8)
            full[:slab.shape[0]] = slab
            slabs.append(full)
            rb.close()
        assert diff_stats(D.assemble_blocks(slabs, w, h), want) == (0, 0), world


# ---- edge cases
def test_empty_ragged_and_tiny_frames():
    import swf_renderer_amd as S
    for (w, h) in [(1, 1), (63, 17), (65, 15), (130, 33)]:
        r = S.Renderer(w, h)
        r.render({"children": []})
        assert not r.read_image(premultiplied=True).any()
        tag = scenarios._poly_shape([(-200, -200), (w * 20 + 200, -200), (w * 20 + 200, h * 20 + 200), (-200, h * 20 + 200)],
                                    {"type": "solid", "color": scenarios._rgba(9, 8, 7)})
        sc = dict(width=w, height=h, stage={"children": [{"type": "shape", "definition": tag}]})
        r.render(sc["stage"])
        got = r.read_image(premultiplied=True)
        assert (got == np.array([9, 8, 7, 255], dtype=np.uint8)).all()
        tri = scenarios._poly_shape([(0, 0), (w * 20, h * 10), (0, h * 20)], {"type": "solid", "color": scenarios._rgba(200, 8, 7, 99)})
        sc = dict(width=w, height=h, stage={"children": [{"type": "shape", "definition": tri}]})
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0)
        r.close()


_comb = helpers.comb_shape


@pytest.mark.parametrize("teeth", [12, 40, 100, 140, 500, 1000, 1100, 3000])
def test_crowded_rows_vs_oracle(teeth):
    """Rows with 24 ... 6000 active edges of one path (a line of text outlines in one fill style looks like this): the crowded-row
    wavefronts (9..64 edges) and the workgroups of k_rows_huge (65..8192, every thread ranks up to eight edges) against the
    oracle, both fill rules; the teeth get narrower than a pixel.  1100 and 3000 teeth (2200 / 6000 edges active in every row, all
    of them starting at one sample row) were refused until round 3 raised the per-row capacity from 2048 to 8192."""
    if teeth > 1100 and os.environ.get("SWFR_EMULATOR"):
        pytest.skip("thousands of edges per row: quadratic work per row, hours on the emulator")
    for eo in (False, True):
        sc = helpers.crowded_rows_scene(teeth, eo)
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), (teeth, eo)


_comb_points = helpers.comb_points


def _multi_poly_shape(polys, fill):
    """DefineShape with several closed polygons in ONE fill style (one path for the scan converter)."""
    recs = []
    xs, ys = [], []
    for i, poly in enumerate(polys):
        p = [(int(x), int(y)) for x, y in poly]
        sc = {"type": "style-change", "move_to": {"x": p[0][0], "y": p[0][1]}}
        if i == 0:
            sc["left_fill"] = 1
        recs.append(sc)
        for k in range(1, len(p) + 1):
            a, b = p[k - 1], p[k % len(p)]
            recs.append({"type": "edge", "delta": {"x": b[0] - a[0], "y": b[1] - a[1]}})
        xs += [q[0] for q in p]; ys += [q[1] for q in p]
    return {"id": 1, "bounds": {"x_min": min(xs), "x_max": max(xs), "y_min": min(ys), "y_max": max(ys)},
            "shape": {"initial_styles": {"fill": [fill], "line": []}, "records": recs}}


@pytest.mark.parametrize("y_top", [0, -7, -300])
@pytest.mark.parametrize("teeth", [9, 13, 16])
def test_edges_arriving_together_at_the_frame_top_vs_oracle(teeth, y_top):
    """18 ... 32 edges of one path that all become active at sample row 0 because the frame's top edge clips them (round 1
    ordered at most sixteen such edges and silently fell back to path order beyond): the start ranks of k2_start_ranks replay
    Cairo's merge sort for any group size.  y_top = 0 puts the teeth's shared vertices exactly on the first sample row (pairs of
    edges coincide there), -7 twips a fraction of a pixel above it, -300 well outside."""
    for eo in (False, True):
        sc = helpers.frame_top_scene(teeth, y_top, eo)
        stats = {}
        assert diff_stats(product_render(sc, stats=stats), oracle_render(sc)) == (0, 0), (teeth, y_top, eo)
        assert stats["pairtest_limit"] == stats["start_group_limit"] == stats["history_limit"] == 0


def test_path_with_4k_edges_and_600_active_per_row_is_exact():
    """Seven stacked combs of 300 sub-pixel teeth in ONE path: 4200 edges, 600 of them active in every row, neighbouring edges
    half a pixel apart.  Every row goes through k2_rows_huge (77 crowded rows); the frame is rendered, not refused, and equals the
    oracle bit for bit (round 2 accepted either outcome; the outcome is pinned now, with the counters in the assertion message)."""
    import swf_renderer_amd as S
    polys = [_comb_points(300, 6000, 100, 100 + 260 * k, 100 + 260 * k + 220) for k in range(7)]
    tag = _multi_poly_shape(polys, {"type": "solid", "color": scenarios._rgba(10, 200, 120)})
    sc = dict(width=320, height=100, stage={"children": [{"type": "shape", "definition": tag}]})
    r = S.Renderer(sc["width"], sc["height"])
    try:
        r.render(sc["stage"])                                   # (a refusal would raise SwfrError here)
        st = r.stats()
        assert st["queued_rows"] == 77 and st["crowded_rows"] == 77, st
        assert st["pairtest_limit"] == st["start_group_limit"] == st["history_limit"] == 0, st
        assert diff_stats(r.read_image(premultiplied=True), oracle_render(sc)) == (0, 0), st
    finally:
        r.close()


def test_one_handle_alternating_plain_and_crowded_frames():
    """swfr_render launches the queued-row kernels (and their passes) the PREVIOUS frame needed and checks the frame's own counters
    afterwards: a frame that needed more is rendered again with everything.  One handle, frames alternating between scenes without
    queued rows, with crowded rows (9..64 active edges: k2_rows_slow), with rows beyond 64 (k2_rows_huge) and with coincident
    edges whose history spans several passes -- every frame equals the oracle."""
    import swf_renderer_amd as S
    w, h = 128, 100
    plain = {"children": [{"type": "shape", "definition": scenarios._poly_shape([(200, 200), (2200, 300), (1200, 1800)], {"type": "solid", "color": scenarios._rgba(9, 99, 199, 200)})}]}
    crowded = {"children": [{"type": "shape", "definition": _comb(12, 2000)}]}
    huge = {"children": [{"type": "shape", "definition": _comb(40, 2000)}]}
    order = [plain, crowded, plain, huge, crowded, plain, plain, huge, huge, plain]
    r = S.Renderer(w, h)
    try:
        for i, stage in enumerate(order):
            r.render(stage)
            want = oracle_render(dict(width=w, height=h, stage=stage))
            assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0), i
        st = r.stats()
        assert st["queued_rows"] > 0 and st["crowded_rows"] > 0
    finally:
        r.close()
    # the soak's tie scenes on one handle between plain frames (their rows need the list-order replay, some over several passes)
    from helpers import soak_scene
    for case in (("mixed", 23000, 196), ("big", 300, 146), ("long", 300, 171)):
        sc = soak_scene(*case)
        r = S.Renderer(sc["width"], sc["height"])
        try:
            for b in sc.get("bitmaps", []):
                r.add_bitmap(b)
            for stage in (plain, sc["stage"], plain, sc["stage"]):
                r.render(stage)
                assert diff_stats(r.read_image(premultiplied=True), oracle_render(dict(sc, stage=stage))) == (0, 0), case
        finally:
            r.close()


def test_frames_wider_than_a_cell_column_field():
    """Cells keep their column in 13 bits relative to the path's left edge: in a frame wider than 8192 px a path may lie anywhere
    (here: beyond column 9000); a single SOLID path wider than 8192 px is rasterized as one path per block of 8192 columns over the
    same edges (round 3; refused before) -- translucent, so that a seam or a doubled column would show -- and stays bit-exact, also
    on top of other paths, through swfr_render_batch and with the blocks' boundary inside an anti-aliased edge; so does a wide path
    with a radial gradient (its style stays anchored at the unsplit rectangle)."""
    import torch
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    w, h = helpers.WIDE_FRAME
    parts = helpers.wide_frame_parts()
    far, near, wide, wide_t, sliver = (parts[k] for k in ("far", "near", "wide", "wide_t", "sliver"))
    sc = dict(width=w, height=h, stage={"children": [{"type": "shape", "definition": near}, {"type": "shape", "definition": far}]})
    assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0)
    # a solid path wider than 8192 px, and a shallow edge crossing column 5 + 8192 (the block boundary of a path that starts at
    # x = 5) inside an anti-aliased span
    for kids in ([wide], [near, wide_t, far], [wide, sliver, wide_t]):
        sc = dict(width=w, height=h, stage={"children": [{"type": "shape", "definition": k} for k in kids]})
        assert diff_stats(product_render(sc), oracle_render(sc)) == (0, 0), len(kids)
    r = S.Renderer(w, h)
    try:
        stage = {"children": [{"type": "shape", "definition": wide}, {"type": "shape", "definition": sliver}]}
        want = oracle_render(dict(width=w, height=h, stage=stage))
        if not os.environ.get("SWFR_EMULATOR"):                  # (device tensors need the GPU)
            out = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda")
            r.render_batch([stage, stage], out.data_ptr(), h * w * 4)
            assert diff_stats(out[1].cpu().numpy(), want) == (0, 0)
        r.render_batch([stage, stage])                           # (the per-frame route)
        assert diff_stats(r.read_image(premultiplied=True), want) == (0, 0)
        # a wide path with a radial gradient: the blocks share the style, which stays anchored at the unsplit path's rectangle
        gstage = {"children": [{"type": "shape", "definition": near}, {"type": "shape", "definition": parts["wide_grad"]}]}
        r.render(gstage)
        assert diff_stats(r.read_image(premultiplied=True), oracle_render(dict(width=w, height=h, stage=gstage))) == (0, 0)
    finally:
        r.close()


def test_many_active_edges_fails_loudly_not_silently():
    import swf_renderer_amd as S
    from swf_renderer_amd import api
    # a comb with 4200 teeth: 8400 edges are active in every row, beyond the per-row capacity of 8192
    tag = _comb(4200, 6000)
    r = S.Renderer(320, 100)
    with pytest.raises(S.SwfrError) as e:
        r.render({"children": [{"type": "shape", "definition": tag}]})
    assert e.value.code == api.ERR_CAPACITY
    assert r.stats()["start_group_limit"] == 1                    # the refusal is counted, too
    r.close()
