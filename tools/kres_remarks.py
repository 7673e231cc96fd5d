#!/usr/bin/env python3
"""One line per kernel from a hipcc -Rpass-analysis=kernel-resource-usage log: VGPRs, AGPRs, spilled VGPRs, scratch bytes per lane,
waves per SIMD.  usage: kres_remarks.py LOG [substring of the demangled name]"""
import re
import subprocess
import sys

log = open(sys.argv[1]).read()
pat = sys.argv[2] if len(sys.argv) > 2 else ""
seen = set()
for blk in re.split(r"remark: Function Name: ", log)[1:]:
    name = blk.split()[0]
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void sp::", "")
    if pat not in dem or dem in seen:
        continue
    seen.add(dem)

    def g(key):
        return int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
    print("%-58s VGPR %3d  AGPR %3d  spill %3d  scratch %4d  waves/SIMD %d" % (
        dem, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]")))
