"""shade_spread (raster_common.hip) and the non-pad branch of radial_of (renderer.cpp) against pixman's rule on random frames, where the
goldens of tests/test_spread_gpu.py hold seven matrices, four radii, two focal points and at most six stops.

The reference is tests/spread_model.py -- pixman's walker in Python integers and numpy.float32, no libcairo needed here -- composed into
a frame by tests/spread_fuzz.py: mul_un8(source, coverage) of one shape over a clear frame.  tests/test_spread_model.py pins that
composition, for a superset of the cases below, against live libcairo's whole frame with zero differing bytes.

a. test_random_frames: spread x gradient kind x antialias mode, 60 generated cases each (30 of 48 x 12 and 30 of 80 x 20, one handle per
   frame size): up to 16 stops, coincident stops, stops at 0 and 255, translucent colours, focal points of 1 to 249 epsilons, boxes on
   and off the pixel grid, slanted quadrilaterals, convex polygons, notched and stepped ones with two covered runs in a row.
b. The same cases forced through the instances 3 to 6 (a fifth each), and through render_batch with unlike frames -- several cases of
   both spreads and every kind per launch, mixed with a padded gradient and a plain frame: the other callers of shade_spread.
c. The aimed run-start scenes of tests/spread_scenes.py (4a of the change that added them: the device's rule is pinned, not changed).

What is asserted per frame: the device equals libcairo's rule (`truth`) on every pixel that is not a caveat pixel, and the documented
every-sample rule on the caveat pixels -- a covered run that begins exactly on a stop in an odd reflected period ("Gradient
spread modes") -- so no pixel is left unasserted; no capacity refusal.  A test whose caveat pixels exceed 0.1 % of its covered pixels
fails as vacuous.  In c the device equals the every-sample rule on the whole frame and differs from the libcairo golden at exactly the
model's caveat pixels -- the set -- and nowhere under REPEAT.

Observed on an MI355X: 26 passed in 4.3 s (the slowest test 0.3 s), 1 408 frame comparisons and 20 aimed ones, 0 differing pixels, 0
caveat pixels among the random frames' 140 846 covered ones; DESIGN.md ("Gradient spread modes") has the kernel mutations this file
catches.  Every test prints "spread fuzz ... frames N covered pixels P caveat pixels C".  Runs on an MI355X (-m gpu) and, every sixth case, under
tools/emu/run.py.
"""
import functools

import numpy as np
import pytest

import blend_scenes as bs
import device_routes as dr
import spread_fuzz as sf
import spread_scenes as ss
from device_routes import EMU
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)

pytestmark = pytest.mark.gpu
PER_SIZE = 30                                    # cases per frame size: 60 per spread, kind and antialias mode
MODES = [False, True]
MODE_IDS = ["antialiased", "aliased"]


@functools.lru_cache(maxsize=None)
def _cases(spread, kind, aliased, size):
    """[(case, expected)] -- computed once, shared by a and b, never written to"""
    return tuple((case, sf.expected(case)) for case in sf.cases(spread, kind, aliased, size, PER_SIZE)[::6 if EMU else 1])


class Tally:
    def __init__(self, what):
        self.what, self.frames, self.covered, self.caveat = what, 0, 0, 0

    def check(self, got, e, msg):
        """device == truth off the caveat pixels, == the every-sample rule on them"""
        off = (got != e["truth"]).any(-1) & ~e["caveat"]
        on = (got != e["every_sample"]).any(-1) & e["caveat"]
        self.frames += 1
        self.covered += int((e["alpha"] > 0).sum())
        self.caveat += int(e["caveat"].sum())
        if off.any() or on.any():
            print("spread fuzz", self.what, msg, "differing pixels", [(int(y), int(x)) for y, x in np.argwhere(off | on)][:8],
                  "device", got[off | on][:4].tolist(), "truth", e["truth"][off | on][:4].tolist())
        assert not off.any(), (self.what, msg, int(off.sum()), "pixels differ from libcairo's rule")
        assert not on.any(), (self.what, msg, int(on.sum()), "caveat pixels differ from the every-sample rule")

    def done(self):
        print("spread fuzz", self.what, "frames", self.frames, "covered pixels", self.covered, "caveat pixels", self.caveat)
        assert self.frames and self.covered
        assert self.caveat * 1000 <= self.covered, (self.what, "vacuous: caveat pixels above 0.1 % of the covered pixels", self.caveat, self.covered)


def _msg(case):
    return (case["spread"], case["kind"], "aliased" if case["aliased"] else "antialiased", case["width"], case["index"], case["shape"])


def _through_one_handle(tally, aliased, size, items):
    """every case of one frame size and antialias mode through one handle"""
    r = dr.handle(size[0], size[1], aliased)
    try:
        for case, e in items:
            r.render(case["scene"]["stage"])
            tally.check(r.read_image(premultiplied=True), e, _msg(case))
            dr.not_refused(r, _msg(case))
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- a. random frames
@pytest.mark.parametrize("aliased", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", ss.KINDS)
@pytest.mark.parametrize("spread", ss.SPREADS)
def test_random_frames(spread, kind, aliased, monkeypatch):
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    tally = Tally("render %s %s %s" % (spread, kind, MODE_IDS[aliased]))
    for size in sf.SIZES:
        _through_one_handle(tally, aliased, size, _cases(spread, kind, aliased, size))
    tally.done()


# ---------------------------------------------------------------------------------------------------------------- b. the other callers
@pytest.mark.parametrize("instance", ["3", "4", "5", "6"])
@pytest.mark.parametrize("spread", ss.SPREADS)
def test_random_frames_through_instance(spread, instance, monkeypatch):
    """the blend, layer, mask and fade instances shade through the same call: a fifth of a's cases forced through each"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)               # (read when a handle is created)
    tally = Tally("instance %s %s" % (instance, spread))
    for aliased in MODES:
        for size in sf.SIZES:
            items = [it for kind in ss.KINDS for it in _cases(spread, kind, aliased, size)[int(instance) % 5::5]]
            if EMU:                                                  # (a fifth of every sixth case is next to none: one of each kind)
                items = [_cases(spread, kind, aliased, size)[int(instance) % 5] for kind in ss.KINDS[int(instance) % 3:][:1]]
            _through_one_handle(tally, aliased, size, items)
    tally.done()


def _unlike_frames(aliased, size):
    """[(message, stage, expected, truth or None)] of one frame size: cases of both spreads and every kind, after every third a padded
    gradient (a case's box on whole pixels with its spread set to pad: the oracle's) or a plain frame (no gradient at all)"""
    from helpers import oracle_render
    W, H = size
    plain = dict(width=W, height=H, exact=True, stage={"children": bs._with_ground(dict(width=W, height=H))})
    if aliased:
        import frame_model as fm
        plain_want = fm.render(*dr.built_for_another_handle(plain, True), W, H, aliased=True)
    else:
        plain_want = oracle_render(plain)
    picked = [it for spread in ss.SPREADS for kind in ss.KINDS for it in _cases(spread, kind, aliased, size)[1::(3 if EMU else 8)]]
    boxes = [c for spread in ss.SPREADS for kind in ss.KINDS for c, _ in _cases(spread, kind, aliased, size)
             if c["shape"] == "box" and sf.piecewise(c["points"], False)]
    assert boxes
    frames = []
    for k, (case, e) in enumerate(picked):
        frames.append((_msg(case), case["scene"]["stage"], None, e))
        if k % 6 == 2:
            box = boxes[(k // 6) % len(boxes)]
            padded = ss.with_spread(box["scene"], "pad")
            frames.append((("padded",) + _msg(box), padded["stage"], oracle_render(padded), None))
        if k % 6 == 5:
            frames.append((("plain",), plain["stage"], plain_want, None))
    return frames


@pytest.mark.parametrize("aliased", MODES, ids=MODE_IDS)
def test_random_frames_through_render_batch_with_unlike_frames(aliased, monkeypatch):
    """one launch shades reflected, repeated and padded gradients and a plain frame side by side.  Into a device tensor where there is a
    device for it (every frame checked), and by the per-frame route (the last frame of a batch is what stays)"""
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    tally = Tally("batch %s" % MODE_IDS[aliased])
    for W, H in sf.SIZES:
        frames = _unlike_frames(aliased, (W, H))
        stages = [f[1] for f in frames]

        def check(got, k):
            msg, _, want, e = frames[k]
            if e is None:
                dr.zero(got, want, ("batch", aliased, k) + msg)
            else:
                tally.check(got, e, ("batch", k) + msg)
        r = dr.handle(W, H, aliased)
        try:
            if not EMU:                                              # (device tensors need the GPU)
                import torch
                out = torch.zeros((len(stages), H, W, 4), dtype=torch.uint8, device="cuda")
                r.render_batch(stages, out.data_ptr(), H * W * 4)
                got = out.cpu().numpy()
                for k in range(len(frames)):
                    check(got[k], k)
            for cut in sorted({1, 3, len(frames)} if EMU else {1, 2, 3, len(frames) // 2, len(frames) - 1, len(frames)}):
                if 0 < cut <= len(frames):
                    r.render_batch(stages[:cut])
                    check(r.read_image(premultiplied=True), cut - 1)
            dr.not_refused(r, ("batch", aliased, W))
        finally:
            r.close()
    tally.done()


# ---------------------------------------------------------------------------------------------------------------- c. the aimed scenes
@pytest.mark.parametrize("aliased", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spread", ss.SPREADS)
def test_run_start_scenes_follow_the_every_sample_rule(spread, aliased, monkeypatch):
    """The device's walker sees every sample of the rectangle from its left edge on; libcairo's sees the covered ones of a piece.  Where
    a covered run begins exactly on a stop in an odd reflected period the two are a whole colour apart at coincident stops: the
    device differs from the libcairo golden at exactly the model's caveat pixels, and under REPEAT nowhere."""
    monkeypatch.delenv("SWFR_TILES_SHADERS", raising=False)
    gold = np.load(ss.golden_path("cairo_spread_%s%s_runstart" % ("aliased_" if aliased else "", spread)))
    cases = ss.runstart_cases(spread, aliased)
    assert sorted(cases) == sorted(gold.files)
    total = 0
    for name, case in sorted(cases.items()):
        e = sf.expected(case)
        assert (e["truth"] == gold[name]).all(), (name, "the model no longer composes the golden")
        r = dr.handle(case["width"], case["height"], aliased)
        try:
            r.render(case["scene"]["stage"])
            got = r.read_image(premultiplied=True)
            dr.not_refused(r, name)
        finally:
            r.close()
        differs = (got != gold[name]).any(-1)
        where = [(int(y), int(x)) for y, x in np.argwhere(differs)]
        print("spread fuzz run start", spread, MODE_IDS[aliased], name, "pixels differing from libcairo", where, "caveat pixels", int(e["caveat"].sum()),
              "device", got[differs].tolist(), "libcairo", gold[name][differs].tolist())
        assert (got == e["every_sample"]).all(), (name, "the device left its every-sample rule")
        assert (differs == e["caveat"]).all(), (name, where)
        total += len(where)
    assert (total == 0) == (spread == "repeat"), (spread, total)
