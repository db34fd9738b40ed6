"""Workgroup stamps of the fused row launch (k2_rows_ahead_b) from a -DSWFR_TRACE build: two frame sets, one group; render_resident(6) is
prologue, fused, fused, plain.  Slot k of buffer 0 holds the stamps of the ahead workgroup blockIdx.x = k of the LAST fused launch (both
frames of a launch write the same slot: whichever wrote last), buffer 1 those of the row wavefronts of the last row launch (the plain one).
usage (GPU box): bash tools/build_variant.sh trace_ahead -DSWFR_TRACE && python tools/trace_wg_ahead.py [s1|s2]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SWFR_FRAMES_IN_FLIGHT"] = "2"
os.environ["SWFR_EVENT_STRIDE"] = "1000000"
import numpy as np
from swf_renderer_amd import api
LIB = os.path.join(ROOT, "build", "trace_ahead", "libswfr.so")
api.library_path = lambda: LIB
import swf_renderer_amd as S
from swf_renderer_amd import synth
which = sys.argv[1] if len(sys.argv) > 1 else "s1"
cfg = synth.S1 if which == "s1" else synth.S2
W, H = cfg["width"], cfg["height"]
pts, cols = synth.scene(**cfg)
host = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY)
scene = host.build_frame(api.stars_to_stage(pts, cols)); host.close()
r = S.Renderer(W, H)
r.upload_edges(*scene)
r.render_resident(10)
r.render_resident(6)
v = ctypes.c_uint32(0)
r.L.swfr_debug_copy(r.h, 3, ctypes.byref(v), 4)
print("%s: fused launches of the call: %d" % (which, v.value))
L = ctypes.CDLL(LIB)
buf = np.zeros((3, 32768, 8), dtype=np.uint32)
L.swfr_debug_trace.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
assert L.swfr_debug_trace(buf.ctypes.data, buf.nbytes) > 0
for k, name in enumerate(("ahead bin workgroups (last fused launch)", "row wavefronts (last, plain, row launch)")):
    b = buf[k]
    used = b[:, 7] != 0
    idx = np.nonzero(used)[0]
    b = b[used].astype(np.int64)
    if not len(b):
        print(name, ": none"); continue
    t0, t1 = b[:, 0].min(), b[:, 7].max()
    dur = (b[:, 7] - b[:, 0]) * 0.01
    print("%s: %d workgroups, span first entry -> last exit %.2f us; duration us p50 %.2f p90 %.2f max %.2f; entries spread over %.2f us" %
          (name, len(b), (t1 - t0) * 0.01, *np.percentile(dur, [50, 90]), dur.max(), (b[:, 0].max() - t0) * 0.01))
    if k == 0:
        o = idx < 8
        if o.any():
            print("   the eight ordering workgroups: entry %.2f..%.2f us after the first entry, duration max %.2f us, last exit at %.2f us" %
                  ((b[o, 0].min() - t0) * 0.01, (b[o, 0].max() - t0) * 0.01, dur[o].max(), (b[o, 7].max() - t0) * 0.01))
        print("   the other workgroups: duration p50 %.2f max %.2f us, last exit at %.2f us" % (np.percentile(dur[~o], 50), dur[~o].max(), (b[~o, 7].max() - t0) * 0.01))
r.close()
