#!/usr/bin/env python3
"""Multitaper spectra (sp_multitaper) in one pass against what a caller could do before: K calls of engine.welch_psd (PSD) or
engine.welch_csd (cross) with sqrt(c_k) v_k as the window, device-resident input, results summed on the device.  One JSON line per
shape and estimator (psd / cross).
  base_ms, base2_ms  the K-call baseline, timed twice in the same process around the fused call (their difference is the spread)
  fused_ms           engine.multitaper, sustained (back-to-back calls between one pair of HIP events, per call)
  *_iso_ms           median of single calls, each between its own events with a device synchronise before it
  kernel_ms          k_mtaper alone (library profiling events)
  transforms, tf_s   complex transforms of nfft points per call and per second of kernel time
  valu_share, lds_share   kernel time the fp32 flops (5 n log2 n per transform + windowing + accumulation) and the LDS traffic of the
                     workgroup transform's exchanges (16 n bytes per exchange: write + read of complex64) would take at peak
                     (157.3 Tflop/s fp32 vector, 256 CUs x 128 B/clk x 2.4 GHz LDS), as a share of kernel_ms
  max_rel_dev        the fused result against the baseline's, max |a - b| / max |b|
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/mtaper_bench.py [--reps 10] > profiles/r08_mtaper_bench.txt"""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (complex, nfft, hop, K)
SHAPES = [(c, n, h, k) for c in (False, True) for n in (1024, 4096) for h in (n // 2, n) for k in (3, 7)]
PEAK_FLOPS, PEAK_LDS = 157.3e12, 256 * 128 * 2.4e9


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


def exchanges(nfft):
    """LDS exchanges of one workgroup transform: radix-16 register stages, one exchange between consecutive stages."""
    return max(0, math.ceil(math.log2(nfft) / 4) - 1)


def one(idx, warmup, reps):
    import torch
    from pyfft_amd import engine as E
    from pyfft_amd.multitaper import multitaper_plan
    cplx, nfft, hop, K = SHAPES[idx]
    n = 1 << (25 if cplx else 26)
    g = torch.Generator(device="cuda").manual_seed(idx)
    x, y = torch.randn(n, device="cuda", generator=g) + 0.5, torch.randn(n, device="cuda", generator=g) - 0.25
    if cplx:
        x = torch.complex(x, torch.randn(n, device="cuda", generator=g))
        y = torch.complex(y, torch.randn(n, device="cuda", generator=g))
    p = multitaper_plan(n, cplx, fs=1.0, nfft=nfft, noverlap=nfft - hop, NW=4.0, Kmax=K)
    M = p["nframes"]
    rows = p["tapers"] / np.sqrt(p["energy"])[:, None] * np.sqrt(p["weights"])[:, None]
    sided = E.SIDED_RAW

    def base_psd():
        acc = E.welch_psd(x, rows[0], hop, M, detrend=True, sided=sided)
        for k in range(1, K):
            acc += E.welch_psd(x, rows[k], hop, M, detrend=True, sided=sided)
        return acc

    def base_cross():
        a = list(E.welch_csd(x, y, rows[0], hop, M, detrend=True, sided=sided))
        for k in range(1, K):
            for u, v in zip(a, E.welch_csd(x, y, rows[k], hop, M, detrend=True, sided=sided)):
                u += v
        return a

    def fused_psd():
        return E.multitaper(x, rows, hop, M, detrend=True)[0]

    def fused_cross():
        return E.multitaper(x, rows, hop, M, y=y, detrend=True)[:3]

    nb = nfft if cplx else nfft // 2 + 1
    for est, base, fused in (("psd", base_psd, fused_psd), ("cross", base_cross, fused_cross)):
        ref, got = base(), fused()
        torch.cuda.synchronize()
        if est == "psd":
            dev = float((got - ref[:nb]).abs().max() / ref.abs().max())
        else:
            dev = max(float((gq - rq.reshape(-1)[:nb]).abs().max() / rq.abs().max()) for gq, rq in zip(got, ref))
        b1 = measure(base, warmup, reps)
        fu = measure(fused, warmup, reps)
        b2 = measure(base, warmup, reps)
        E.profile_enable(True)
        fused()
        kernel_ms = E.profile_last_ms()
        E.profile_enable(False)
        # complex transforms per call: the PSD of a real record packs two frames, the real cross pair packs x + i y
        tf = K * ((M + 1) // 2 if (est == "psd" and not cplx) else (M if (est == "psd" or not cplx) else 2 * M))
        flops = tf * (5.0 * nfft * math.log2(nfft) + 2.0 * nfft + (3.0 if est == "psd" else 11.0) * nfft)
        lds = tf * 16.0 * nfft * (exchanges(nfft) + (1 if (est == "cross" and not cplx) else 0))
        base_ms = min(b1[0], b2[0])
        print(json.dumps({"est": est, "dtype": "complex64" if cplx else "float32", "nfft": nfft, "hop": hop, "K": K, "nsig": n,
                          "frames": M, "base_ms": round(b1[0], 4), "base2_ms": round(b2[0], 4),
                          "base_spread": round(abs(b1[0] - b2[0]) / base_ms, 4), "fused_ms": round(fu[0], 4),
                          "speedup": round(base_ms / fu[0], 3), "base_iso_ms": round(min(b1[1], b2[1]), 4),
                          "fused_iso_ms": round(fu[1], 4), "kernel_ms": round(kernel_ms, 4), "transforms": tf,
                          "tf_s": float("%.4g" % (tf / (kernel_ms * 1e-3))),
                          "valu_share": round(flops / PEAK_FLOPS / (kernel_ms * 1e-3), 3),
                          "lds_share": round(lds / PEAK_LDS / (kernel_ms * 1e-3), 3), "max_rel_dev": float("%.3g" % dev)}), flush=True)


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
