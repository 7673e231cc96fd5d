#!/usr/bin/env python3
"""Lomb-Scargle periodograms (engine.lomb, k_lomb) of device-resident records against two baselines, one JSON line per shape:
N = 2^17 samples against M = 2^17 frequencies and N = 2^20 against M = 2^16, 1 and 8 rows, weights on and off (floating mean,
'normalize'), and last one line for scipy on the host:
  lomb_ms       engine.lomb: the median of --reps isolated calls after --warmup calls, *_spread = (max - min) / median over them
  kernel_ms     k_lomb_sums alone, between two events around its launch (the library's profile hooks), the median of as many calls
  pairs_per_s   N M / lomb_ms; kernel_pairs_per_s the same over kernel_ms
  estimate      the issue-cost estimate: per sample a wave issues v_sin_f32 and v_cos_f32 at 8 cycles each and `other` further vector
                instructions (counted in the compiled loop: 3 float64, 1 conversion, 4 float32 and 2 + R packed FMAs, and one more
                for the loop's register moves and address arithmetic: 3 v_mov_b32 + 1 v_add_u32 per 4 samples at R = 1) taken at 4
                cycles each; 64 pairs per SIMD take est_cycles, and the device's SIMDs at its clock give est_pairs_per_s;
                kernel_over_estimate = kernel_pairs_per_s / est_pairs_per_s
  composed_ms   the same sums composed from torch on the device: float64 phases f (t - t0) reduced by their rounded value, torch.sin and
                torch.cos, e(2 phi) from them, and two matmuls against the weights and the weighted rows, in frequency blocks that
                fit memory; finished by the float64 closed form of tests/lomb_ref.py and asserted equal to the kernel's result within
                the tests' allowance.  The median of --base-reps calls after one.  It takes seconds, so at 2^36 pairs it runs over the
                first composed_freqs = 2^34 / N frequencies only, and composed_over_lomb compares it with that share of lomb_ms
  scipy_ms      scipy.signal.lombscargle on the host at N = M = 2^13, one call, against engine.lomb of the same host arrays
Times are the calls' (host launch, the record's preparation and the finish step included).  No counter was collected.
    python tools/lomb_bench.py [--reps 20] > profiles/lomb_bench.txt"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(ln, lm, rows, wt) for ln, lm in ((17, 17), (20, 16)) for rows in (1, 8) for wt in (False, True)]
BLOCK_ELEMS = 1 << 26               # cells of one frequency block of the composition: 512 MiB per float64 array
COMPOSED_PAIRS = 1 << 34           # the composition is timed over at most so many (sample, frequency) pairs
SCIPY_LOG2 = 13


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
    """an uneven clock (jittered, 20 % dropped before N samples are kept), a line per row over noise; float64 t, w, float32 y"""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.choice(np.arange(int(N * 1.25)) + 0.3 * rng.standard_normal(int(N * 1.25)), N, replace=False)) * 1e-3
    y = np.stack([np.sin(2 * np.pi * (37.0 + 11.0 * r) * t + r) + rng.standard_normal(N) + 0.5 for r in range(rows)]).astype(np.float32)
    w = rng.uniform(0.5, 1.5, N)
    return t, y, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--base-reps", type=int, default=2)
    ap.add_argument("--first", type=int, default=0, help="skip the shapes before this index")
    ap.add_argument("--only", type=int, default=-1, help="one shape by index")
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    import torch
    import lomb_ref as R
    from pyfft_amd import engine as E
    props = torch.cuda.get_device_properties(0)
    ncu, clock_hz = props.multi_processor_count, float(getattr(props, "clock_rate", 2400000)) * 1e3
    for idx, (ln, lm, rows, wt) in enumerate(SHAPES):
        if (args.only >= 0 and idx != args.only) or idx < args.first:
            continue
        N, M = 1 << ln, 1 << lm
        t, y, w = record(N, rows, idx)
        f = np.linspace(0.5, 400.0, M)                 # up to the Nyquist frequency of the mean rate (800 per unit of t)
        td, yd, wd = (torch.as_tensor(a, device="cuda") for a in (t, y, w))
        wdd = wd if wt else None
        mean = yd.double().mean(dim=-1).cpu().numpy()

        def run_lomb():
            return E.lomb(td, yd, f, weights=wdd, mean_value=mean)

        E.profile_enable(True)
        tk = timed(run_lomb, args.warmup, args.reps, after=E.profile_last_ms)
        assert E.profile_last_kernel() == "k_lomb_sums"
        E.profile_enable(False)
        plan = E.lomb_plan(N, M, rows)
        R_ = plan["rows_per_group"]
        other = 3 + 1 + 4 + (2 + R_) + 1          # float64, conversion, float32, packed FMAs, loop overhead
        est_cycles = 16 + 4 * other
        est_rate = ncu * 4 * clock_hz * 64.0 / est_cycles
        pairs = float(N) * M * (-(-rows // R_))
        out = {"N": N, "M": M, "rows": rows, "weights": wt, "rows_per_group": R_, "split": plan["split"], "passes": plan["passes"],
               "workgroups": plan["workgroups"], "lomb_ms": round(tk[0], 3), "lomb_spread": round(tk[1], 3), "kernel_ms": round(tk[2], 3),
               "pairs_per_s": round(pairs / tk[0] * 1e3, 0), "kernel_pairs_per_s": round(pairs / tk[2] * 1e3, 0),
               "est_cycles_per_64_pairs": est_cycles, "est_pairs_per_s": round(est_rate, 0), "cus": ncu, "clock_hz": clock_hz,
               "kernel_over_estimate": round(pairs / tk[2] * 1e3 / est_rate, 3)}
        if not args.no_baselines:
            wn = (wd if wt else torch.ones_like(wd))
            wn = wn / wn.sum()
            d = yd.double() - torch.as_tensor(mean, device="cuda")[:, None]
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
                    A = torch.cat([c, s]) @ Wm                                               # [2 mb, 1 + rows]
                    B = torch.cat([c * c - s * s, 2 * c * s]) @ wn
                    k = c.shape[0]
                    cm.append(torch.stack([A[:k, 0], A[k:, 0], B[:k], B[k:]], dim=-1))
                    rw.append(torch.stack([A[:k, 1:].T, A[k:, 1:].T], dim=-1))
                    del c, s, A, B
                return torch.cat(cm), torch.cat(rw, dim=1)

            note("shape %d: the composition over %d frequencies" % (idx, Mc))
            tc = timed(run_composed, 1, args.base_reps)
            note("shape %d: composed in %.0f ms" % (idx, tc[0]))
            cm, rw = (a.cpu().numpy() for a in run_composed())
            totals = np.empty(1 + 2 * rows)
            totals[0] = 1.0
            totals[1::2], totals[2::2] = (wn[None, :] * d).sum(dim=-1).cpu().numpy(), (wn[None, :] * d * d).sum(dim=-1).cpu().numpy()
            ref = R.finish(cm, rw, totals, mean, f[:Mc], N, float(t[0]), True, "normalize")
            with contextlib.redirect_stdout(sys.stderr):
                used = R.assert_within(run_lomb().cpu().numpy()[:, :Mc], ref, "shape %d against the composition" % idx)
            out.update({"composed_freqs": Mc, "composed_ms": round(tc[0], 3), "composed_spread": round(tc[1], 3),
                        "composed_over_lomb": round(tc[0] / (tk[0] * Mc / M), 1), "composed_worst_cell_of_allowance": round(used, 3),
                        "composed_block_freqs": mb})
            del cm, rw, Wm, d
        print(json.dumps(out), flush=True)
        del td, yd, wd
        torch.cuda.empty_cache()
    if args.only < 0 and not args.no_baselines:
        note("scipy on the host")
        import scipy.signal as ss
        N = M = 1 << SCIPY_LOG2
        t, y, w = record(N, 1, 99)
        f = np.linspace(0.5, 400.0, M)
        y64 = y[0].astype(np.float64)
        t0 = time.perf_counter()
        ref = ss.lombscargle(t, y64, 2 * np.pi * f, normalize=True, floating_mean=True)
        scipy_ms = (time.perf_counter() - t0) * 1e3
        E.lomb(t, y[0], f)
        t0 = time.perf_counter()
        got = E.lomb(t, y[0], f)
        lomb_ms = (time.perf_counter() - t0) * 1e3
        with contextlib.redirect_stdout(sys.stderr):
            used = R.assert_within(got[None], ref[None], "host arrays against scipy")
        print(json.dumps({"N": N, "M": M, "rows": 1, "weights": False, "memory": "host", "scipy_ms": round(scipy_ms, 1),
                          "lomb_ms": round(lomb_ms, 3), "scipy_over_lomb": round(scipy_ms / lomb_ms, 0),
                          "scipy_worst_cell_of_allowance": round(used, 3)}), flush=True)


if __name__ == "__main__":
    main()
