#!/usr/bin/env python3
"""The fast Lomb-Scargle sums (engine.lomb_sums_grid: three type-1 NUFFTs, k_nufft) of device-resident records against the direct
sums (engine.lomb_sums, k_lomb) IN THE SAME RUN, one JSON line per shape: N = 2^17 samples against M = 2^17 frequencies, 2^20 against
2^20 and 2^20 against 2^16, each with 1 and 8 rows (equal weights); then one line per row count with the N = M at which the two paths
cross.
  fast_ms       engine.lomb_sums_grid: the median of --reps isolated calls after --warmup calls, *_spread = (max - min) / median
  spread_ms     k_nufft_spread of the 1 + rows rows alone, between two events around its launch (the library's profile hooks)
  transform_ms  the same transforms alone: engine.fft of [1 + rows, nf] and of [1, nf] complex64 on the device, the same code path
  rest_ms       fast_ms - spread_ms - transform_ms: the record's preparation (k_lomb_prep), k_nufft_prep, the shifts, scan and fill,
                the one-row spread of A2, the picks, two status read-backs and the host's launches.  The per-kernel split of this
                remainder comes from a kernel trace of one shape (profiles/nufft_kernel_resources.txt), not from this tool
  direct_ms     engine.lomb_sums of the same record at the same frequencies, the median of --direct-reps calls after one
  direct_over_fast, and the worst cell of the fast sums against the direct ones: common relative to 1 (the sum of w32), rows relative
                to their row's sum of |wy32|, as a share of the tests' allowance (tests/nufft_ref.py)
  composed_ms   the same sums composed from torch on the device as tools/lomb_bench.py composes them (float64 phases, torch.sin and
                torch.cos, matmuls), over the first composed_freqs frequencies only (it takes seconds), asserted equal to the fast
                sums within the allowance; composed_over_fast compares it with that share of fast_ms
  crossing      N = M = 2^k for k = --cross-lo .. --cross-hi, both paths timed: the first N M from which the fast path is the faster
                one and stays so.  LOMB_FAST_MIN_PAIRS (launch.h) is taken from these lines
Times are the calls' (host launches and read-backs included).  No counter was collected.
    python tools/nufft_bench.py [--reps 20] > profiles/nufft_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(ln, lm, rows) for ln, lm in ((17, 17), (20, 20), (20, 16)) for rows in (1, 8)]
BLOCK_ELEMS = 1 << 26               # cells of one frequency block of the composition: 512 MiB per float64 array
COMPOSED_PAIRS = 1 << 31            # the composition is timed over at most so many (sample, frequency) pairs


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


def record(N, rows, seed):
    """an uneven clock (jittered, 20 % dropped before N samples are kept), a line per row over noise; float64 t, float32 y"""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.choice(np.arange(int(N * 1.25)) + 0.3 * rng.standard_normal(int(N * 1.25)), N, replace=False)) * 1e-3
    y = np.stack([np.sin(2 * np.pi * (37.0 + 11.0 * r) * t + r) + rng.standard_normal(N) + 0.5 for r in range(rows)]).astype(np.float32)
    return t, y


def worst_share(fast, direct, yd, mean, N):
    """the worst cell of the fast sums against the direct ones, as a share of the tests' allowance"""
    import nufft_ref as R
    cm = float((fast.common - direct.common).abs().max())                        # sum of w32 = 1
    scale = ((yd.double() - mean[:, None]).abs().sum(dim=-1) / N)[:, None, None]   # sum of |wy32_r|
    rw = float(((fast.rows - direct.rows).abs() / scale).max())
    return max(cm, rw) / R.ALLOWANCE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--direct-reps", type=int, default=3)
    ap.add_argument("--only", type=int, default=-1, help="one shape by index")
    ap.add_argument("--no-baselines", action="store_true", help="the fast path alone (for a kernel trace)")
    ap.add_argument("--cross-lo", type=int, default=8)
    ap.add_argument("--cross-hi", type=int, default=17)
    args = ap.parse_args()
    import torch
    from pyfft_amd import engine as E
    for idx, (ln, lm, rows) in enumerate(SHAPES):
        if args.only >= 0 and idx != args.only:
            continue
        N, M = 1 << ln, 1 << lm
        t, y = record(N, rows, idx)
        f0, df = 0.5, 399.5 / (M - 1)                  # up to the Nyquist frequency of the mean rate (800 per unit of t)
        f = f0 + df * np.arange(M)
        td, yd = torch.as_tensor(t, device="cuda"), torch.as_tensor(y, device="cuda")
        mean_d = yd.double().mean(dim=-1)
        mean = mean_d.cpu().numpy()

        def run_fast():
            return E.lomb_sums_grid(td, yd, f0, df, M, mean_value=mean)

        E.profile_enable(True)
        tf = timed(run_fast, args.warmup, args.reps, after=E.profile_last_ms)
        assert E.profile_last_kernel() == "k_nufft_spread"
        E.profile_enable(False)
        plan = E.nufft_plan(N, M, rows + 1)
        nf = plan["nf"]
        g1, g2 = (torch.zeros((r, nf), dtype=torch.complex64, device="cuda") for r in (rows + 1, 1))
        tt = timed(lambda: (E.fft(g1), E.fft(g2)), args.warmup, args.reps)
        del g1, g2
        out = {"N": N, "M": M, "rows": rows, "nf": nf, "tiles": plan["tiles"], "passes": plan["passes"], "fast_ms": round(tf[0], 3),
               "fast_spread": round(tf[1], 3), "spread_ms": round(tf[2], 3), "transform_ms": round(tt[0], 3),
               "rest_ms": round(tf[0] - tf[2] - tt[0], 3),
               "lds_adds_per_s": round(float(N) * (rows + 1) * 16 / tf[2] * 1e3, 0)}
        if not args.no_baselines:
            def run_direct():
                return E.lomb_sums(td, yd, f, mean_value=mean)

            note("shape %d: the direct sums" % idx)
            tdir = timed(run_direct, 1, args.direct_reps)
            used = worst_share(run_fast(), run_direct(), yd, mean_d, N)
            out.update({"direct_ms": round(tdir[0], 3), "direct_spread": round(tdir[1], 3), "direct_over_fast": round(tdir[0] / tf[0], 1),
                        "fast_against_direct_of_allowance": round(used, 3)})
            # the composition, as tools/lomb_bench.py has it
            wn = torch.full((N,), 1.0 / N, dtype=torch.float64, device="cuda")
            d = yd.double() - mean_d[:, None]
            Wm = torch.cat([wn[:, None], (wn[None, :] * d).T], dim=1).contiguous()          # [N, 1 + rows]
            fd = torch.as_tensor(f, device="cuda")
            tp = td - td[0]
            mb = max(1, BLOCK_ELEMS // N)
            Mc = min(M, COMPOSED_PAIRS // N)

            def run_composed():
                cm, rw = [], []
                for m0 in range(0, Mc, mb):
                    p = fd[m0:min(m0 + mb, Mc), None] * tp[None, :]
                    p -= torch.round(p)
                    p *= 2 * np.pi
                    c, s = torch.cos(p), torch.sin(p)
                    del p
                    A = torch.cat([c, s]) @ Wm
                    B = torch.cat([c * c - s * s, 2 * c * s]) @ wn
                    k = c.shape[0]
                    cm.append(torch.stack([A[:k, 0], A[k:, 0], B[:k], B[k:]], dim=-1))
                    rw.append(torch.stack([A[:k, 1:].T, A[k:, 1:].T], dim=-1))
                    del c, s, A, B
                return torch.cat(cm), torch.cat(rw, dim=1)

            note("shape %d: the composition over %d frequencies" % (idx, Mc))
            tc = timed(run_composed, 1, 1)
            cm, rw = run_composed()
            fast = run_fast()
            comp = E.LombSums(cm, rw, fast.totals, mean, fast.t_ref, N)
            part = E.LombSums(fast.common[:Mc], fast.rows[:, :Mc], fast.totals, mean, fast.t_ref, N)
            used_c = worst_share(part, comp, yd, mean_d, N)
            out.update({"composed_freqs": Mc, "composed_ms": round(tc[0], 3), "composed_over_fast": round(tc[0] / (tf[0] * Mc / M), 1),
                        "fast_against_composed_of_allowance": round(used_c, 3)})
            del cm, rw, Wm, d
        print(json.dumps(out), flush=True)
        if not args.no_baselines:
            assert used_c <= 1.0 and used <= 1.0, (used_c, used)
        del td, yd
        torch.cuda.empty_cache()
    if args.only >= 0 or args.no_baselines:
        return
    for rows in (1, 8):
        line, cross = [], None
        for k in range(args.cross_lo, args.cross_hi + 1):
            N = M = 1 << k
            t, y = record(N, rows, 100 + k)
            f0, df = 0.5, 399.5 / (M - 1)
            f = f0 + df * np.arange(M)
            td, yd = torch.as_tensor(t, device="cuda"), torch.as_tensor(y, device="cuda")
            mean = yd.double().mean(dim=-1).cpu().numpy()
            a = timed(lambda: E.lomb_sums_grid(td, yd, f0, df, M, mean_value=mean), args.warmup, args.reps)[0]
            b = timed(lambda: E.lomb_sums(td, yd, f, mean_value=mean), args.warmup, args.reps)[0]
            line.append({"log2_N": k, "fast_ms": round(a, 3), "direct_ms": round(b, 3)})
            if a <= b and cross is None:
                cross = N * M
            if a > b:
                cross = None
        print(json.dumps({"crossing": True, "rows": rows, "N_equals_M": line, "fast_from_pairs": cross,
                          "fast_min_pairs_in_use": E.nufft_plan(1 << 10, 1 << 10)["fast_min_pairs"]}), flush=True)


if __name__ == "__main__":
    main()
