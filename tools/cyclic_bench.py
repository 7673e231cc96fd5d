#!/usr/bin/env python3
"""Spectral correlation (engine.cyclic, k_cyclic) of a device-resident record of 2^22 samples against two baselines, one JSON line per
shape: float32 rows (mirrored form, one transform per frame and cycle frequency), complex64 rows in the conjugate form (mirrored) and in
the plain form (two transforms), n 256 / hop 64 and n 1024 / hop 256, A = 64 and 1024 cycle frequencies at the cyclic resolution:
  cyclic_ms     engine.cyclic, S, Pp and Pm: the median of --reps isolated calls after --warmup calls, *_spread = (max - min) / median
                over them (20 calls after 3: at A = 64 a call takes 1.5 .. 3 ms, and five calls spread by up to 15 %)
  composed_ms   (A = 64) what the package offered before: per cycle frequency torch mixes the record on the device into x e(+nu/2 t) and
                y e(-nu/2 t), then engine.welch_csd of the pair.  Asserted equal to the kernel within the allowance of
                tests/cyclic_ref.py, so that the two sides do equal work
  floor_ms      (A = 64) A calls of engine.welch_psd over the same frames: one transform per (frame, cycle frequency) and nothing else
  transforms    frames x A x transforms per (frame, A); Gxf_per_s = transforms / cyclic_ms
The baselines take --base-reps calls after one (a composed call takes 28 .. 43 ms).  All cases run in one process in the same order.  Times
are the calls' (host launch included).  No counter was collected: the share of any peak is not measured here.
    python tools/cyclic_bench.py [--reps 20] > profiles/cyclic_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOG2N = 22
SHAPES = [(kind, n, A) for kind in ("real", "conj", "plain") for n in (256, 1024) for A in (64, 1024)]
A_COMPARED = 64


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--base-reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=-1, help="one shape by index")
    ap.add_argument("--log2n", type=int, default=LOG2N)
    args = ap.parse_args()
    import torch
    import cyclic_ref as R
    from pyfft_amd import engine as E
    nsig = 1 << args.log2n
    gen = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(nsig, device="cuda", dtype=torch.float64)
    env = (1 + 0.8 * torch.cos(2 * np.pi * R.NU_AM * t + 0.3)).to(torch.float32)
    xr = (env * torch.randn(nsig, device="cuda", generator=gen)).contiguous()
    xc = (env * torch.view_as_complex(torch.randn((nsig, 2), device="cuda", generator=gen))).contiguous()
    for idx, (kind, n, A) in enumerate(SHAPES):
        if args.only >= 0 and idx != args.only:
            continue
        hop = n // 4
        nframes = (nsig - n) // hop + 1
        x = xr if kind == "real" else xc
        conj = kind == "conj"
        nu = np.arange(A) / float(nsig) * 16 + (R.NU_AM - 8 * 16 / float(nsig))     # a scan around the modulation rate, off every grid
        w = R.hann(n)
        scale = 1.0 / nframes

        def run_cyclic():
            return E.cyclic(x, w, hop, nframes, nu, conj=conj, detrend=False, scale=scale)

        tk = timed(run_cyclic, args.warmup, args.reps)
        plan = E.cyclic_plan(n, hop, nframes, A, cplx=kind != "real", conj=conj)
        out = {"nsig": nsig, "kind": kind, "n": n, "hop": hop, "frames": nframes, "A": A, "fpg": plan["fpg"], "workgroups": plan["workgroups"],
               "passes": plan["passes"], "transforms_per_frame_alpha": plan["transforms"],
               "cyclic_ms": round(tk[0], 3), "cyclic_spread": round(tk[1], 3),
               "transforms": nframes * A * plan["transforms"], "Gxf_per_s": round(nframes * A * plan["transforms"] / tk[0] / 1e6, 2)}
        if A == A_COMPARED:
            tt = t.to(torch.float64)
            xx = x.to(torch.complex64)
            xm = torch.conj(xx) if conj else xx

            def mixed(v, sign, nuv):
                ph = torch.remainder(sign * 0.5 * nuv * tt, 1.0) * (2 * np.pi)
                return (v * torch.polar(torch.ones_like(ph), ph).to(torch.complex64)).contiguous()

            def run_composed():
                res = []
                for nuv in nu:
                    res.append(E.welch_csd(mixed(xm, 1.0, float(nuv)), mixed(xx, -1.0, float(nuv)), w, hop, nframes, detrend=False,
                                           sided=E.SIDED_RAW, scale=1.0))
                return res

            def run_floor():
                for _ in nu:
                    E.welch_psd(x, w, hop, nframes, detrend=False, sided=E.SIDED_RAW, scale=1.0)

            tc = timed(run_composed, 1, args.base_reps)
            tf = timed(run_floor, 1, args.base_reps)
            S, Pp, Pm = (o.cpu().numpy() for o in run_cyclic())
            res = run_composed()
            ref = (np.stack([r[2][0].cpu().numpy() for r in res]), np.stack([r[1][0].cpu().numpy() for r in res]),
                   np.stack([r[0].cpu().numpy() for r in res]))
            bd = R.bounds(ref)
            worst = max(float(np.max(np.abs(g - r) / b)) for g, r, b in zip((S, Pp, Pm), ref, bd))
            # the composition mixes with float64 phases of a float64 product nu t, exact to about 1e-9 turn at 2^22 samples; both sides
            # are held to the allowance of tests/cyclic_ref.py
            assert worst <= 1.0, ("the composition and the kernel differ", idx, worst)
            out.update({"composed_ms": round(tc[0], 3), "composed_spread": round(tc[1], 3), "composed_over_cyclic": round(tc[0] / tk[0], 2),
                        "composed_worst_cell_of_allowance": round(worst, 3), "floor_ms": round(tf[0], 3), "floor_spread": round(tf[1], 3),
                        "cyclic_over_floor": round(tk[0] / tf[0], 2)})
            del res, ref
        print(json.dumps(out), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
