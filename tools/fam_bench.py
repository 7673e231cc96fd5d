#!/usr/bin/env python3
"""The FFT accumulation method (engine.fam, k_fam) on a device-resident real record, one JSON line per shape.  The first shape is the
blind search the feature is for: nchan 256, hop 64, blocks of P = 8192 frames, 2 blocks (1 048 768 samples: 2^20 + 192, what two blocks
reach), all pairs with f >= 0 and alpha >= 0 (16 384 pairs of 2Q = 2048 bins); the second a shorter channelizer with more blocks.
  fam_ms          engine.fam (S and both powers): the median of --reps isolated calls after --warmup calls, *_spread = (max - min) / median
  stft_ms         engine.stft_frames(bin_major=True) of the same frames alone: the channelizer the call contains
  kernel_ms       the pair kernel alone (the library's own event pair around its last launch), and its share of the estimate
                  DESIGN section 4 gives: npairs nblocks 16 P bytes read from the scratch
  composed_ms     the same plane from engine.stft_frames(bin_major=True), torch products and torch.fft, pair rows in groups of one k;
                  asserted equal to the call within the allowance of tests/fam_ref.py (4 F32_DEV of the largest sqrt(Pw_k Pw_l) plus 1e-6
                  of the largest cell)
  cyclic_ms       engine.cyclic (S only) over 1024 cycle frequencies at nperseg = nchan and the same hop and frames;
                  cyclic_extrapolated_ms = cyclic_ms x (alpha bins of the plane / 1024): what scanning the plane's alpha grid would cost,
                  EXTRAPOLATED, not run
Times are the calls' (host launch included).  No counter was collected.
    python tools/fam_bench.py [--reps 7] > profiles/fam_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(256, 64, 8192, 2), (64, 16, 2048, 32)]          # nchan, hop, P, nblocks


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    iso = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        iso.append(a.elapsed_time(b))
    med = float(np.median(iso))
    return med, (max(iso) - min(iso)) / med


def composed(E, x, a, hop, g, nblocks, pairs, nchan, P):
    """S [npairs, 2Q] complex64 and Pw [nchan] float64 from materialised frames"""
    import torch
    Z, _ = E.stft_frames(x, a, hop, nblocks * P, detrend=False, sided=E.SIDED_RAW, bin_major=True)
    gt = torch.as_tensor(np.tile(g, nblocks), device=Z.device)
    twoQ = P * hop // nchan
    Q = twoQ // 2
    S = torch.empty((pairs.shape[0], twoQ), dtype=torch.complex64, device=Z.device)
    j = torch.arange(twoQ, device=Z.device)
    ks = pairs[:, 0]
    for k in np.unique(ks):
        rows = np.nonzero(ks == k)[0]
        ls = torch.as_tensor(pairs[rows, 1].astype(np.int64), device=Z.device)
        prod = (gt * Z[int(k)])[None, :] * Z[ls].conj()
        T = torch.fft.fft(prod.reshape(len(rows), nblocks, P), dim=-1).sum(dim=1)
        col = (j[None, :] - Q + (int(k) - ls)[:, None] * twoQ) % P
        S[torch.as_tensor(rows, device=Z.device)] = torch.gather(T, 1, col)
    Pw = (gt.double()[None, :] * (Z.real.double() ** 2 + Z.imag.double() ** 2)).sum(-1)
    return S, Pw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=-1, help="one shape by index")
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    import torch
    import fam_ref as R
    from pyfft_amd import engine as E, fam as F
    for idx, (nchan, hop, P, nblocks) in enumerate(SHAPES):
        if args.only >= 0 and idx != args.only:
            continue
        nframes = nblocks * P
        nsig = (nframes - 1) * hop + nchan
        gen = torch.Generator(device="cuda").manual_seed(1)
        t = torch.arange(nsig, device="cuda", dtype=torch.float64)
        x = ((1 + 0.8 * torch.cos(2 * np.pi * R.NU_AM * t + 0.3)).float() * torch.randn(nsig, device="cuda", generator=gen)).contiguous()
        a, g = R.hamming(nchan).astype(np.float32), R.hamming(P).astype(np.float32)
        pairs = F.fam_pairs(nchan, real=True)
        twoQ = P * hop // nchan

        def run():
            return E.fam(x, a, hop, g, nblocks, pairs, detrend=False)

        tk = timed(run, args.warmup, args.reps)
        E.profile_enable(True)
        kms = []
        for _ in range(max(args.reps // 2, 3)):
            E.fam(x, a, hop, g, nblocks, pairs, detrend=False, Pw=False)
            torch.cuda.synchronize()
            assert E.profile_last_kernel() == "k_fam"
            kms.append(E.profile_last_ms())
        E.profile_enable(False)
        kernel_ms = float(np.median(kms))
        ts = timed(lambda: E.stft_frames(x, a, hop, nframes, detrend=False, sided=E.SIDED_RAW, bin_major=True), 1, max(args.reps // 2, 3))
        p = E.fam_plan(nchan, hop, P, nblocks, pairs.shape[0])
        read_bytes = pairs.shape[0] * nblocks * 16 * P
        signed = np.where(pairs < nchan // 2, pairs, pairs - nchan).astype(np.int64)
        alpha_bins = int(np.unique(signed[:, 0] - signed[:, 1]).size) * twoQ      # the distinct diagonals' strips
        out = {"nsig": nsig, "nchan": nchan, "hop": hop, "P": P, "nblocks": nblocks, "npairs": int(pairs.shape[0]), "Q": p["Q"],
               "cells": int(pairs.shape[0]) * twoQ, "passes": p["passes"], "workgroups": p["workgroups"], "scratch_MiB": round(p["scratch"] / 2 ** 20, 1),
               "fam_ms": round(tk[0], 3), "fam_spread": round(tk[1], 3), "stft_ms": round(ts[0], 3), "stft_spread": round(ts[1], 3),
               "kernel_ms": round(kernel_ms, 3), "kernel_read_GB": round(read_bytes / 1e9, 2), "kernel_read_TBps": round(read_bytes / kernel_ms / 1e9, 2),
               "pair_transforms_per_s": round(pairs.shape[0] * nblocks / kernel_ms * 1e3)}
        if not args.no_baselines:
            S, Pwx, _ = run()
            tc = timed(lambda: composed(E, x, a, hop, g, nblocks, pairs, nchan, P), 1, 1)
            Sc, Pwc = composed(E, x, a, hop, g, nblocks, pairs, nchan, P)
            kk, ll = (torch.as_tensor(pairs[:, i].astype(np.int64), device="cuda") for i in (0, 1))
            scale_s = float(torch.sqrt(Pwc[kk] * Pwc[ll]).max())
            bound = R.ALLOWANCE * scale_s + R.ABS_TERM * float(Sc.abs().max())
            worst = max(float((S - Sc).abs().max()) / bound,
                        float((Pwx.double() - Pwc).abs().max()) / ((R.ALLOWANCE + R.ABS_TERM) * float(Pwc.max())))
            assert worst <= 1.0, ("the composition and the call differ", idx, worst)
            del S, Sc
            torch.cuda.empty_cache()
            A = 1024
            nu = (np.arange(A) + 1) / (P * hop)
            w = R.hamming(nchan)
            ty = timed(lambda: E.cyclic(x, w, hop, nframes, nu, detrend=False, Pp=False, Pm=False), 1, 3)
            out.update({"composed_ms": round(tc[0], 1), "composed_over_fam": round(tc[0] / tk[0], 1), "composed_worst_of_allowance": round(worst, 3),
                        "cyclic_1024_ms": round(ty[0], 3), "alpha_bins": alpha_bins,
                        "cyclic_extrapolated_ms": round(ty[0] * alpha_bins / A, 1),
                        "cyclic_extrapolated_over_fam": round(ty[0] * alpha_bins / A / tk[0], 1)})
        print(json.dumps(out), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
