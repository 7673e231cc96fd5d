#!/usr/bin/env python3
"""Host overhead per call of pyfft_amd.engine in both calling modes: 2000 calls of engine.welch_psd on a device tensor of 4096 complex64
samples (nfft 256, hop 128) and the same on a numpy array, perf_counter around each loop with a torch.cuda.synchronize() before and
after it.  One line: label, microseconds per call on the device tensor and on the host array.

  python tools/engine_host_cost.py [TREE [LABEL [ENTRY]]]

ENTRY (default welch_psd) may also be cyclic (the same record and frames, 4 cycle frequencies, mean_value given so that it is one
library call), ssq (the same record and frames, T only), burg or ar_ls (the same segments, order 8; ar_ls with check=False, so that no
status is read back) or beamscan (31 eigen-models of order 8, one per frame, against 128 scan points).

TREE (default: this repository) is where pyfft_amd is imported from, so that the Python files of another commit, unpacked elsewhere and
pointed at the same library with SP_LIB_PATH, can be timed in the same session: profiles/engine_host_cost.txt."""
import os
import sys
import time

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
label = sys.argv[2] if len(sys.argv) > 2 else root
entry = sys.argv[3] if len(sys.argv) > 3 else "welch_psd"
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
dwin = np.gradient(win)
order, nk = 8, 128
Vh = np.linalg.qr(rng.standard_normal((nframes, order, order)) + 1j * rng.standard_normal((nframes, order, order)))[0]
wh = np.sort(rng.random((nframes, order)) + 0.1)[:, ::-1].copy()
eig = {True: (torch.from_numpy(Vh).cuda(), torch.from_numpy(wh).cuda()), False: (Vh, wh)}
pos, kv = np.arange(order) * 0.5, np.linspace(-0.5, 0.5, nk)
call = {"welch_psd": lambda x: E.welch_psd(x, win, hop, nframes),
        "cyclic": lambda x: E.cyclic(x, win, hop, nframes, [0.0, 0.05, 0.1, 0.25], mean_value=0.0),
        "ssq": lambda x: E.ssq(x, win, dwin, hop, 0, nframes),
        "burg": lambda x: E.burg(x, nfft, hop, 0, nframes, order),
        "ar_ls": lambda x: E.ar_ls(x, nfft, hop, 0, nframes, order, check=False),
        "beamscan": lambda x: E.beamscan(*eig[torch.is_tensor(x)], pos, kv)}[entry]
us = []
for x in (xd, xh):
    for _ in range(200):
        call(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        call(x)
    torch.cuda.synchronize()
    us.append((time.perf_counter() - t0) / K * 1e6)
print("%s %s us/call: device %.2f host %.2f" % (label, entry, us[0], us[1]), flush=True)
