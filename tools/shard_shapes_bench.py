#!/usr/bin/env python3
"""Sharded Welch PSD at the shapes of the generic one-pass kernel (k_welch_opx), on ONE GPU in one process: the sharded form
of a world of one (sp_welch_export of the whole stream + sp_welch_apply) against one sp_welch_psd call of the same shape
(which runs its own mean pass there).  Device-resident float32 / complex64 input, median of --reps timed calls after --warmup,
CUDA events around each call.  Algorithmic bytes: one read of the samples; the share is of 8 TB/s.
    python tools/shard_shapes_bench.py [--log2n 27] > profiles/r05_shard_shapes.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("complex64", 4096, 1351), ("complex64", 2048, 675), ("float32", 2981, 992), ("float32", 4096, 1388)]


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    import torch
    from pyfft_amd import engine as E
    from pyfft_amd import _ffi
    from oracle import cpu_ref as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="", help="comma-separated shape indices")
    args = ap.parse_args()
    _ffi.init()
    n = 1 << args.log2n
    gen = torch.Generator(device="cuda").manual_seed(1)
    print("# sharded Welch (export + apply, world 1) vs sp_welch_psd, one GPU, %d samples, ms (median / min of %d)" % (n, args.reps))
    print("%-10s %5s %5s %8s | %8s %8s | %8s %8s | %6s | %6s %6s" % ("dtype", "nfft", "hop", "frames", "exp+app", "min", "psd", "min",
                                                                    "ratio", "GB/s", "%8TB/s"))
    only = {int(s) for s in args.only.split(",") if s}
    for i, (dt, nfft, hop) in enumerate(SHAPES):
        if only and i not in only:
            continue
        if dt == "complex64":
            x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=gen) + torch.tensor([0.3, -0.1], device="cuda"))
        else:
            x = torch.randn(n, device="cuda", generator=gen) + 0.3
        M = (n - nfft) // hop + 1
        win = O.windows("Blackman-Harris", nwins=nfft)

        def sharded():
            st = E.welch_export(x, win, hop, M, nmean=n)
            return E.welch_apply(st, win, M, sided=E.SIDED_ONE, scale=1.0)

        def single():
            return E.welch_psd(x, win, hop, M, detrend=True, sided=E.SIDED_ONE, scale=1.0)

        a = sharded()
        kname = E.profile_last_kernel()
        b = single()
        err = float(torch.max(torch.abs(a - b) / (2e-4 * torch.abs(b) + 1e-6 * b.max())).item())
        # interleaved: A B A B ... per round of reps
        ts_a, ts_b = [], []
        for _ in range(3):
            ts_a.append(timed(sharded, args.warmup, args.reps // 3))
            ts_b.append(timed(single, args.warmup, args.reps // 3))
        ta, tamin = float(np.median([t[0] for t in ts_a])), min(t[1] for t in ts_a)
        tb, tbmin = float(np.median([t[0] for t in ts_b])), min(t[1] for t in ts_b)
        nbytes = n * x.element_size()
        gbs = nbytes / (ta * 1e-3) / 1e9
        print("%-10s %5d %5d %8d | %8.4f %8.4f | %8.4f %8.4f | %6.3f | %6.0f %6.1f   (parity %.2f of tol; kernel %s)" % (
            dt, nfft, hop, M, ta, tamin, tb, tbmin, ta / tb, gbs, 100.0 * gbs / 8000.0, err, kname))
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
