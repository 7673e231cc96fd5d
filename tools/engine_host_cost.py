#!/usr/bin/env python3
"""Host overhead per call of pyfft_amd.engine in both calling modes: 2000 calls of engine.welch_psd on a device tensor of 4096 complex64
samples (nfft 256, hop 128) and the same on a numpy array, perf_counter around each loop with a torch.cuda.synchronize() before and
after it.  One line: label, microseconds per call on the device tensor and on the host array.

  python tools/engine_host_cost.py [TREE [LABEL]]

TREE (default: this repository) is where pyfft_amd is imported from, so that the Python files of another commit, unpacked elsewhere and
pointed at the same library with SP_LIB_PATH, can be timed in the same session: profiles/engine_host_cost.txt."""
import os
import sys
import time

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
label = sys.argv[2] if len(sys.argv) > 2 else root
sys.path.insert(0, root)
import numpy as np
import torch
from pyfft_amd import engine as E

assert os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))) == root, E.__file__
K, n, nfft, hop = 2000, 4096, 256, 128
nframes = (n - nfft) // hop + 1
rng = np.random.default_rng(0)
xh = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
xd = torch.from_numpy(xh).cuda()
win = np.hanning(nfft)
us = []
for x in (xd, xh):
    for _ in range(200):
        E.welch_psd(x, win, hop, nframes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        E.welch_psd(x, win, hop, nframes)
    torch.cuda.synchronize()
    us.append((time.perf_counter() - t0) / K * 1e6)
print("%s welch_psd us/call: device %.2f host %.2f" % (label, us[0], us[1]), flush=True)
