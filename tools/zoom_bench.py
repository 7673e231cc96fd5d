#!/usr/bin/env python3
"""Zoom PSD (sp_zoom_welch) against the Welch PSD of the same record at the same nperseg and hop (sp_welch_psd): the cost of a band
at a chosen spacing against the cost of the whole FFT grid.  Device-resident input; one JSON line per shape.
  welch_ms, welch2_ms  engine.welch_psd, sustained, timed twice in the same process around the zoom call (their difference: the spread)
  zoom_ms              engine.zoom_welch, sustained (back-to-back calls between one pair of HIP events, per call)
  *_iso_ms             median of single calls, each between its own events with a device synchronise before it
  kernel_ms            k_zoom alone (library profiling events; fused shapes only)
  L                    the two transforms per frame are L-point, L = next_pow2(nperseg + m - 1); Welch does one nperseg-point transform
Shapes: fused ones (L <= 8192) and the reference's long segment, 116 508 points, against the long Welch.
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/zoom_bench.py [--reps 10] > profiles/r09_zoom_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


# (complex, nperseg, hop, m, log2 nsig)
SHAPES = [(c, n, h, m, 24) for c in (False, True) for n, m in ((256, 200), (1024, 1000), (4096, 1024), (4096, 4096), (1000, 300))
          for h in (n // 2, n)] + [(False, 116508, 58254, 1000, 22), (True, 116508, 58254, 1000, 22), (False, 116508, 58254, 8192, 22)]


def one(idx, warmup, reps):
    import torch
    from pyfft_amd import engine as E
    from pyfft_amd.zoom import zoom_plan
    cplx, nperseg, hop, m, lg = SHAPES[idx]
    n = 1 << lg
    g = torch.Generator(device="cuda").manual_seed(idx)
    x = torch.randn(n, device="cuda", generator=g) + 0.5
    if cplx:
        x = torch.complex(x, torch.randn(n, device="cuda", generator=g))
    p = zoom_plan(n, cplx, [0.10, 0.12], m, fs=1.0, nperseg=nperseg, noverlap=nperseg - hop, detrend="constant", return_onesided=False)
    M, win = p["nframes"], p["window"]

    def welch():
        return E.welch_psd(x, win, hop, M, detrend=True, sided=E.SIDED_RAW, scale=p["scale"])

    def zoom():
        return E.zoom_welch(x, win, hop, M, m, p["start"], p["step"], detrend="mean", scale=p["scale"])[0]

    welch(), zoom()
    torch.cuda.synchronize()
    w1 = measure(welch, warmup, reps)
    z = measure(zoom, warmup, reps)
    w2 = measure(welch, warmup, reps)
    L = 1 << max(9, (nperseg + m - 2).bit_length())
    kernel_ms = None
    if L <= 8192:
        E.profile_enable(True)
        zoom()
        kernel_ms = round(E.profile_last_ms(), 4)
        E.profile_enable(False)
    wm = min(w1[0], w2[0])
    print(json.dumps({"dtype": "complex64" if cplx else "float32", "nperseg": nperseg, "hop": hop, "m": m, "L": L, "nsig": n, "frames": M,
                      "path": "fused" if L <= 8192 else "long", "welch_ms": round(w1[0], 4), "welch2_ms": round(w2[0], 4),
                      "welch_spread": round(abs(w1[0] - w2[0]) / wm, 4), "zoom_ms": round(z[0], 4), "zoom_over_welch": round(z[0] / wm, 3),
                      "welch_iso_ms": round(min(w1[1], w2[1]), 4), "zoom_iso_ms": round(z[1], 4), "kernel_ms": kernel_ms,
                      "frames_per_s": float("%.4g" % (M / (z[0] * 1e-3)))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
    args = ap.parse_args()
    if args.one >= 0:
        return one(args.one, args.warmup, args.reps)
    for i in range(len(SHAPES)):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(i), "--reps", str(args.reps), "--warmup",
                             str(args.warmup)], timeout=args.limit).returncode
        if rc != 0:
            sys.exit("shape %s failed (exit %d): stopping" % (SHAPES[i], rc))


if __name__ == "__main__":
    main()
