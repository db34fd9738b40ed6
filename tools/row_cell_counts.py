"""Cells per row of the resident S1 frame (argv[1] = s2 for S2) from the row headers k2_rows wrote, by row mode: rows, cells, rows with
more than eight / sixteen cells (k2_tiles fetches sixteen per row in its first round, eight per further round).  Runs the kernels
of THIS tree on the CPU emulator (tools/emu/): the counts are the kernels' own, the emulator says nothing about time.
usage: python tools/row_cell_counts.py [s1|s2]        (a 4K frame: a few minutes)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import run as emu_run
emu_run.use_emulator()
import numpy as np
import swf_renderer_amd as S
from swf_renderer_amd import api, synth
which = sys.argv[1] if len(sys.argv) > 1 else "s1"
cfg = synth.S1 if which == "s1" else synth.S2
W, H = cfg["width"], cfg["height"]
pts, cols = synth.scene(**cfg)
host = S.Renderer(W, H, device=api.DEVICE_HOST_ONLY)
scene = host.build_frame(api.stars_to_stage(pts, cols)); host.close()
r = S.Renderer(W, H)
r.upload_edges(*scene)
r.render_resident(1)
buf = np.zeros((4000000, 2), np.uint32)                   # RowInfo2 {off, n | mode << 16}
n = r.L.swfr_debug_copy(r.h, 0, buf.ctypes.data, buf.nbytes)
r.close()
rows = buf[: n // 8]
mode, cnt = rows[:, 1] >> 16, (rows[:, 1] & 0xffff).astype(np.int64)
print("%s: row headers of the emulated frame (ROW_FULL = analytic rows, ROW_SUB = sampled rows)" % which)
for sel, name in ((mode == 1, "ROW_FULL"), (mode == 2, "ROW_SUB"), ((mode == 1) | (mode == 2), "both")):
    c = cnt[sel]
    print("  %-8s rows %7d  cells %8d  rows with > 8 cells %6d (%.1f %%)  with > 16 cells %6d  max %d" % (name, len(c), c.sum(), (c > 8).sum(), 100.0 * (c > 8).mean() if len(c) else 0.0, (c > 16).sum(), c.max() if len(c) else 0))
