#!/usr/bin/env python3
"""Wavelet bispectrum (engine.wbic, k_wbic_tile) of device-resident records of 2^20 samples, one JSON line per shape: S = 128 and 256
rows (k = 8 .. 8 + S - 1 at df = 1/1600, Morlet-6: M = 949, L = 4096), the auto form of a float32 record and the cross form of three,
one block over the record and disjoint blocks of 4096 samples:
  wbic_ms       engine.wbic: the median of --reps isolated calls after --warmup calls, *_spread = (max - min) / median over them
  cwt_ms        engine.cwt (W materialised) of the same records and scales, one call per distinct record: the floor, since the call
                contains these transforms
  composed_ms   (--composed shapes) the same sums from torch: engine.cwt of every record, then per chunk of time and per row i the
                products X[i] Y[j] conj(Z[m]) in complex64 and their sums in float64; asserted equal to the call within the parity
                bound of tests/wbic_ref.py (|dB| <= 1e-4 A + 1e-6 max A)
  pair_samples  valid (i, j) pairs (both halves of the auto form) x samples of all blocks; Gps_call = pair_samples / wbic_ms,
                Gps_contraction = pair_samples / (wbic_ms - cwt_ms): the contraction with its reductions, what the call adds to the floor
Times are the calls' (host launch included).  No counter was collected: the share of any peak is not measured here.
    python tools/wbic_bench.py [--reps 7] > profiles/wbic_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOG2N, DF, K_LO, BLOCK = 20, 1.0 / 1600, 8, 4096
SHAPES = [(S, kind, blocks) for S in (128, 256) for kind in ("auto", "cross") for blocks in (False, True)]


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


def composed(E, recs, sc, L, M, k_lo, block, nblocks):
    """B, D, P, A of every block from materialised transforms: products in complex64, sums in float64"""
    import torch
    Ws = [E.cwt(r, sc, "morlet", 6.0, L, M)["W"] for r in recs]
    X, Y, Z = (Ws[0], Ws[0], Ws[0]) if len(Ws) == 1 else Ws
    S = X.shape[0]
    dev = X.device
    B = torch.full((nblocks, S, S), float("nan"), dtype=torch.complex128, device=dev)
    D = torch.full((nblocks, S, S), float("nan"), dtype=torch.float64, device=dev)
    A = torch.full((nblocks, S, S), float("nan"), dtype=torch.float64, device=dev)
    P = torch.zeros((nblocks, S), dtype=torch.float64, device=dev)
    piece = min(block, 16384)
    for b in range(nblocks):
        B[b][~torch.isnan(B[b].real)] = 0
        for c0 in range(b * block, (b + 1) * block, piece):
            c1 = min(c0 + piece, (b + 1) * block)
            x, y, z = X[:, c0:c1], Y[:, c0:c1], Z[:, c0:c1]
            az = z.abs()
            P[b] += (az.double() ** 2).sum(-1)
            for i in range(S - k_lo):
                nj = S - k_lo - i
                prod = x[i][None, :] * y[:nj]
                zm = z[i + k_lo:i + k_lo + nj]
                sums = ((prod * zm.conj()).to(torch.complex128).sum(-1), (prod.abs().double() ** 2).sum(-1),
                        (prod.abs() * az[i + k_lo:i + k_lo + nj]).double().sum(-1))
                for dst, v in zip((B, D, A), sums):
                    dst[b, i, :nj] = v if c0 == b * block else dst[b, i, :nj] + v
    return B / block, D / block, P / block, A / block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=-1, help="one shape by index")
    ap.add_argument("--log2n", type=int, default=LOG2N)
    ap.add_argument("--composed", type=int, default=128, help="the composition is run for shapes of up to so many rows (0: never)")
    args = ap.parse_args()
    import torch
    import wbic_ref as R
    from pyfft_amd import engine as E, wavelet as W
    nsig = 1 << args.log2n
    gen = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(nsig, device="cuda", dtype=torch.float64)
    recs3 = []
    for r in range(3):
        v = 0.5 * torch.randn(nsig, device="cuda", generator=gen)
        for k, a in ((17 + r, 1.0), (40, 0.8), (57 + r, 0.6)):
            v = v + a * torch.cos(2 * np.pi * DF * k * t + 0.3 * r).float()
        recs3.append(v.contiguous())
    for idx, (S, kind, blocks) in enumerate(SHAPES):
        if args.only >= 0 and idx != args.only:
            continue
        sc = R.grid_scales(DF, K_LO, K_LO + S - 1)
        plan = W.cwt_plan(nsig, 1.0, wavelet=W.Morlet(6.0), scales=sc)
        assert plan["fused"].all()
        L, M = plan["L"], plan["M"]
        recs = recs3 if kind == "cross" else recs3[:1]
        block = BLOCK if blocks else nsig
        nblocks = nsig // block
        y, z = (recs[1], recs[2]) if kind == "cross" else (None, None)

        def run():
            return E.wbic(recs[0], sc, K_LO, "morlet", 6.0, L, M, 0, block, block, nblocks, y=y, z=z)

        def run_cwt():
            for r in recs:
                E.cwt(r, sc, "morlet", 6.0, L, M)

        tk = timed(run, args.warmup, args.reps)
        tf = timed(run_cwt, 1, max(args.reps // 2, 3))
        p = E.wbic_plan(nsig, S, K_LO, L, M, 0, block, block, nblocks, len(recs), kind == "auto")
        pairs = sum(max(S - K_LO - i, 0) for i in range(S))
        ps = pairs * nsig
        out = {"nsig": nsig, "S": S, "kind": kind, "block": block, "nblocks": nblocks, "L": L, "M": M, "passes": p["passes"],
               "groups": p["groups"], "tiles": p["tiles"], "workgroups": p["workgroups"], "scratch_MiB": round(p["scratch"] / 2 ** 20, 1),
               "wbic_ms": round(tk[0], 3), "wbic_spread": round(tk[1], 3), "cwt_ms": round(tf[0], 3), "cwt_spread": round(tf[1], 3),
               "wbic_over_cwt": round(tk[0] / tf[0], 2), "pair_samples": ps, "Gps_call": round(ps / tk[0] / 1e6, 1),
               "Gps_contraction": round(ps / max(tk[0] - tf[0], 1e-3) / 1e6, 1)}
        if S <= args.composed:
            res = run()
            tc = timed(lambda: composed(E, recs, sc, L, M, K_LO, block, nblocks), 0, 1)
            Bc, Dc, Pc, Ac = (v.cpu().numpy() for v in composed(E, recs, sc, L, M, K_LO, block, nblocks))
            B = res["B"].cpu().numpy()
            ok = ~np.isnan(Bc)
            worst = max(float(np.max(np.abs(B[b][ok[b]] - Bc[b][ok[b]]) / R.parity_bound(Ac[b])[ok[b]])) for b in range(nblocks))
            assert worst <= 1.0, ("the composition and the call differ", idx, worst)
            out.update({"composed_ms": round(tc[0], 1), "composed_over_wbic": round(tc[0] / tk[0], 1), "composed_worst_of_bound": round(worst, 4)})
            del Bc, Dc, Pc, Ac, res
        print(json.dumps(out), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
