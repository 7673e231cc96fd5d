#!/usr/bin/env python3
"""Inverse STFT (sp_istft) against the forward sp_stft of the same shape, which moves the same bytes the other way: one JSON line
per shape, device-resident input and output, frame-major spectra.
  sustained_ms  back-to-back calls between one pair of HIP events, per call
  isolated_ms   median of single calls, each between its own events with a device synchronise before it
  bytes         spectra + samples (8 (nfft/2+1) M + 4 n real, 8 nfft M + 8 n complex); tb_s = bytes / sustained time
  ratio         inverse / forward sustained time; halo = extra frames the inverse transforms, (q - 1) / fpg of the default partition
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/istft_bench.py [--reps 20] > profiles/r07_istft_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, complex, nfft, hop, log2 samples)
SHAPES = [("cfg3", False, 2048, 512, 26), ("n1024-ov50", False, 1024, 512, 26), ("n1024-ov75", False, 1024, 256, 26),
          ("n4096-ov50", False, 4096, 2048, 26), ("n4096-ov75", False, 4096, 1024, 26),
          ("n1024-ov50", True, 1024, 512, 25), ("n1024-ov75", True, 1024, 256, 25),
          ("n4096-ov50", True, 4096, 2048, 25), ("n4096-ov75", True, 4096, 1024, 25)]


def measure(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    sustained = a.elapsed_time(b) / reps
    iso = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        iso.append(a.elapsed_time(b))
    return sustained, float(np.median(iso))


def one(idx, warmup, reps):
    import torch
    from pyfft_amd import engine as E
    name, cplx, nfft, hop, lg = SHAPES[idx]
    n = 1 << lg
    M = (n - nfft) // hop + 1
    g = torch.Generator(device="cuda").manual_seed(idx)
    x = torch.randn(n, device="cuda", generator=g)
    if cplx:
        x = torch.complex(x, torch.randn(n, device="cuda", generator=g))
    win = np.hanning(nfft + 1)[:-1]
    sided = E.SIDED_RAW if cplx else E.SIDED_HALF
    amp = 1.0 / float(np.sum(win))
    Z, _ = E.stft_frames(x, win, hop, M, detrend=False, sided=sided, amp_scale=amp)
    y = E.istft_frames(Z, win, hop, sided=sided)
    torch.cuda.synchronize()
    L = (M - 1) * hop + nfft
    err = float((y[nfft:L - nfft] - x[nfft:L - nfft]).abs().max() / x.abs().max())
    fwd = measure(lambda: E.stft_frames(x, win, hop, M, detrend=False, sided=sided, amp_scale=amp), warmup, reps)
    inv = measure(lambda: E.istft_frames(Z, win, hop, sided=sided), warmup, reps)
    nbytes = 8.0 * Z.numel() + (8.0 if cplx else 4.0) * L
    print(json.dumps({"shape": name, "dtype": "complex64" if cplx else "float32", "nfft": nfft, "hop": hop, "nsig": n, "frames": M,
                      "bytes": nbytes, "round_trip_err": float("%.3g" % err),
                      "fwd_sustained_ms": round(fwd[0], 4), "fwd_isolated_ms": round(fwd[1], 4),
                      "inv_sustained_ms": round(inv[0], 4), "inv_isolated_ms": round(inv[1], 4),
                      "ratio": round(inv[0] / fwd[0], 3), "inv_tb_s": round(nbytes / inv[0] * 1e-9, 3),
                      "fwd_tb_s": round(nbytes / fwd[0] * 1e-9, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
    args = ap.parse_args()
    if args.one >= 0:
        return one(args.one, args.warmup, args.reps)
    for i in range(len(SHAPES)):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(i), "--reps", str(args.reps), "--warmup",
                             str(args.warmup)], timeout=args.limit).returncode
        if rc != 0:
            sys.exit("shape %s failed (exit %d): stopping" % (SHAPES[i][0], rc))


if __name__ == "__main__":
    main()
