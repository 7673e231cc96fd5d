#!/usr/bin/env python3
"""Per-launch-shape kernel times from a rocprofv3 --kernel-trace CSV: median / min / count per (kernel, grid X, grid Y),
for the kernels whose name contains PATTERN.
  python tools/kernel_shapes.py <kernel_trace.csv> [PATTERN]
e.g. PATTERN k_bispec: k_bispec_tile (grid X: 256 threads per tile, Y: 256-frame chunks), k_bispec_pzz, k_bispec_reduce, k_bispec_finish;
     PATTERN k_istft: k_istft (grid X: workgroups of 256 / T runs of frames, Y: records), k_istft_gather (bin-major input);
     PATTERN k_mtaper: k_mtaper (grid X: workgroups of 256 / T runs of frames or frame pairs, Y: taper blocks -- 1, or K for the
     eigenspectra), k_mtaper_combine (the weighted sum of the eigenspectra)."""
import collections
import csv
import sys

import numpy as np


def main():
    path = sys.argv[1]
    pat = sys.argv[2] if len(sys.argv) > 2 else ""
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        if pat not in r["Kernel_Name"]:
            continue
        k = (r["Kernel_Name"].split("(")[0], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]))
        d[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("%-34s %10s %6s %7s %10s %10s" % ("kernel", "grid X", "Y", "calls", "median us", "min us"))
    for k, v in sorted(d.items()):
        print("%-34s %10d %6d %7d %10.1f %10.1f" % (k[0], k[1], k[2], len(v), float(np.median(v)), min(v)))


if __name__ == "__main__":
    main()
