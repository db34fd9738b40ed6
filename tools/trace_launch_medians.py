"""Per kernel and frames per launch (the grid's y), the median, p90 and mean duration of its launches in a rocprofv3 kernel_trace.csv,
and the launches per rendered frame of the whole process (a frame = one blockIdx.y of a k2_tiles launch).
usage: python tools/trace_launch_medians.py <kernel_trace.csv>"""
import collections
import csv
import sys

import numpy as np

rows = list(csv.DictReader(open(sys.argv[1])))
by = collections.defaultdict(list)
for r in rows:
    name = r["Kernel_Name"].split("(")[0].replace("swfr::", "").replace("void ", "")
    if not name.startswith("k2_"):
        continue
    by[(name, int(r["Grid_Size_Y"]))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
frames = 0
for (name, gy), v in sorted(by.items()):
    v = np.array(v)
    print("%-20s frames per launch %d: %4d launches, us p50 %.1f  p90 %.1f  mean %.1f" % (name, gy, len(v), np.percentile(v, 50), np.percentile(v, 90), v.mean()))
    if name.startswith("k2_tiles"):
        frames += gy * len(v)
launches = sum(len(v) for v in by.values())
print("launches %d, frames %d, launches per frame %.2f" % (launches, frames, launches / max(frames, 1)))
