#!/usr/bin/env python3
"""The type-2 NUFFT (engine.nufft2, k_nufft2) of device-resident records against the type-1 transform of the same shape IN THE SAME
RUN, one JSON line per shape: N = 2^20 samples against M = 2^20 and 2^16 modes, each with 1 and 8 rows, on a time-sorted and on a
shuffled record; then one line for the band-limited fit (nufft.nufft_fit) of 2^20 jittered samples by 2^18 + 1 modes.
  type2_ms      engine.nufft2: the median of --reps isolated calls after --warmup calls, *_spread = (max - min) / median
  interp_ms     k_nufft2_interp alone, between two events around its launch (the library's profile hooks), the median over the same calls
  transform_ms  the same transform alone: engine.fft of [rows, nf] complex64 on the device, the same code path
  rest_ms       type2_ms - interp_ms - transform_ms: k_nufft_prep, the check of the modes, scan and fill, k_nufft2_place, the status
                read-back and the host's launches
  type1_ms      engine.nufft1 of the same times, rows and grid, timed the same way; type2_over_type1 is the ratio of the two medians
  composed      the same values composed from torch in float64 (phases reduced by rounding, cos and sin, a matmul over chunks of
                modes) at the first `composed_samples` samples of the record, asserted equal to nufft2's within the tests' allowance
                (tests/nufft2_ref.py); composed_of_allowance is the worst cell's share of it
  fit           nufft_fit with rtol 1e-6: fit_ms the whole call (right-hand side, Toeplitz column, iterations, the residual's nufft2),
                setup_ms the same call with maxiter = 0, ms_per_iteration their difference over the iterations, and floor_ms the two
                transforms of 2^20 points an iteration cannot do without (engine.fft and engine.ifft of one row, timed alone)
Times are the calls' (host launches and read-backs included).  No counter was collected.  No figure here is a gate.
    python tools/nufft2_bench.py [--reps 20] > profiles/nufft2_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(20, lm, rows, order) for lm in (20, 16) for rows in (1, 8) for order in ("sorted", "shuffled")]
COMPOSED_SAMPLES = 64
MODE_CHUNK = 1 << 18


def timed(fn, warmup, reps, after=None):
    import torch
    for _ in range(warmup):
        fn()
    iso, extra = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        iso.append(a.elapsed_time(b))
        if after:
            extra.append(after())
    med = float(np.median(iso))
    return med, (max(iso) - min(iso)) / med, (float(np.median(extra)) if extra else None)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def record(N, seed):
    """an uneven clock (jittered, 20 % dropped before N samples are kept), in time order; float64"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(np.arange(int(N * 1.25)) + 0.3 * rng.standard_normal(int(N * 1.25)), N, replace=False)) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=int, default=-1, help="one shape by index")
    ap.add_argument("--no-fit", action="store_true")
    args = ap.parse_args()
    import torch
    import nufft2_ref as R2
    from pyfft_amd import engine as E, nufft as NU
    for idx, (ln, lm, rows, order) in enumerate(SHAPES):
        if args.only >= 0 and idx != args.only:
            continue
        N, M = 1 << ln, 1 << lm
        rng = np.random.default_rng(1000 + idx)
        t = record(N, lm)
        if order == "shuffled":
            t = t[rng.permutation(N)]
        t_ref = float(t.min())
        f0, df = 0.5, 399.5 / (M - 1)                  # up to the Nyquist frequency of the mean rate (800 per unit of t)
        F = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))).astype(np.complex64)
        c = (rng.standard_normal((rows, N)) + 1j * rng.standard_normal((rows, N))).astype(np.complex64)
        td, Fd, cd = (torch.as_tensor(a, device="cuda") for a in (t, F, c))

        def run2():
            return E.nufft2(td, Fd, f0, df, t_ref=t_ref)

        E.profile_enable(True)
        t2 = timed(run2, args.warmup, args.reps, after=E.profile_last_ms)
        assert E.profile_last_kernel() == "k_nufft2_interp"
        E.profile_enable(False)
        t1 = timed(lambda: E.nufft1(td, cd, f0, df, M, t_ref=t_ref), args.warmup, args.reps)
        plan = E.nufft2_plan(N, M, rows)
        g = torch.zeros((rows, plan["nf"]), dtype=torch.complex64, device="cuda")
        tt = timed(lambda: E.fft(g), args.warmup, args.reps)
        del g
        # the composition at the first samples of the record
        got = run2()[:, :COMPOSED_SAMPLES].to(torch.complex128)
        tau = (td[:COMPOSED_SAMPLES] - t_ref)[:, None]
        ref = torch.zeros((rows, COMPOSED_SAMPLES), dtype=torch.complex128, device="cuda")
        for m0 in range(0, M, MODE_CHUNK):
            m = torch.arange(m0, min(M, m0 + MODE_CHUNK), device="cuda", dtype=torch.float64)
            p = tau * (f0 + df * m)[None, :]
            p -= torch.round(p)
            p *= 2 * np.pi
            ref += Fd[:, m0:m0 + MODE_CHUNK].to(torch.complex128) @ torch.complex(torch.cos(p), torch.sin(p)).T
            del p
        used = float(((got - ref).abs() / Fd.abs().double().sum(dim=-1, keepdim=True)).max()) / R2.ALLOWANCE2
        out = {"N": N, "M": M, "rows": rows, "order": order, "nf": plan["nf"], "tiles": plan["tiles"], "passes": plan["passes"],
               "type2_ms": round(t2[0], 3), "type2_spread": round(t2[1], 3), "interp_ms": round(t2[2], 3), "transform_ms": round(tt[0], 3),
               "rest_ms": round(t2[0] - t2[2] - tt[0], 3), "type1_ms": round(t1[0], 3), "type1_spread": round(t1[1], 3),
               "type2_over_type1": round(t2[0] / t1[0], 2), "composed_samples": COMPOSED_SAMPLES, "composed_of_allowance": round(used, 3)}
        print(json.dumps(out), flush=True)
        assert used <= 1.0, used
        del td, Fd, cd
        torch.cuda.empty_cache()
    if args.only >= 0 or args.no_fit:
        return
    N, K = 1 << 20, 1 << 17
    M = 2 * K + 1
    rng = np.random.default_rng(77)
    h = 1e-3
    t = (np.arange(N) + rng.uniform(-0.45, 0.45, N)) * h
    period = N * h
    f0, df = -K / period, 1.0 / period
    y = sum(a * np.cos(2 * np.pi * k / period * t + ph) for k, a, ph in ((37, 1.0, 0.3), (4001, 0.5, 1.0), (100003, 0.25, 2.0)))
    y = (y + 0.1 * rng.standard_normal(N)).astype(np.float32)
    td, yd = torch.as_tensor(t, device="cuda"), torch.as_tensor(y, device="cuda")
    note("the fit: N %d, M %d" % (N, M))
    fit = NU.nufft_fit(td, yd, f0, df, M, t_ref=0.0)
    tfit = timed(lambda: NU.nufft_fit(td, yd, f0, df, M, t_ref=0.0), 1, max(3, args.reps // 4))
    tset = timed(lambda: NU.nufft_fit(td, yd, f0, df, M, t_ref=0.0, maxiter=0), 1, max(3, args.reps // 4))
    L = 1
    while L < 2 * M:
        L *= 2
    g = torch.zeros((1, L), dtype=torch.complex64, device="cuda")
    tfl = timed(lambda: E.ifft(E.fft(g)), args.warmup, args.reps)
    print(json.dumps({"fit": True, "N": N, "M": M, "circulant": L, "iterations": fit.iterations, "converged": fit.converged,
                      "residual": round(float(fit.residual), 5), "fit_ms": round(tfit[0], 3), "fit_spread": round(tfit[1], 3),
                      "setup_ms": round(tset[0], 3), "ms_per_iteration": round((tfit[0] - tset[0]) / max(1, fit.iterations), 3),
                      "floor_ms": round(tfl[0], 3), "floor_spread": round(tfl[1], 3)}), flush=True)


if __name__ == "__main__":
    main()
