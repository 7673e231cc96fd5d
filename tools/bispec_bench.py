#!/usr/bin/env python3
"""Bispectrum (sp_bispectrum) at the issue's shapes: one JSON line per shape.
  call_ms      whole call (detrend pass, spectra, contraction, reductions, finish), device-resident input and output: median of
               --reps warm calls between HIP events
  tile_ms      the contraction kernel k_bispec_tile alone (library profiling events; SP_BISPEC_MIB is raised so that the
               shape runs as one frame chunk and the figure covers every frame)
  pair_frames  valid (i, j) pairs computed (j <= i for the auto case) x frames; pair-frames/s from tile_ms
  valu_unpacked / valu_packed: tile_ms's share of the fp32 VALU bound, 10 lane-operations per pair and frame, at 64 (unpacked)
               or 128 (v_pk_fma_f32) lane-operations per CU and clock, at clock_mhz (the clock the run held when the runtime
               reports it, else 2400)
  cpu_s        numpy float64 on --cpu-frames frames (spectra + contraction), scaled to all frames
    python tools/bispec_bench.py [--reps 20] > profiles/r06_bispec_bench.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, dtype, nfft, log2 samples, cross)
SHAPES = [("real-auto", "float32", 512, 24, False), ("real-auto", "float32", 1024, 24, False),
          ("real-auto", "float32", 2048, 24, False), ("real-cross", "float32", 1024, 24, True),
          ("complex-auto", "complex64", 1024, 23, False)]


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
    return float(np.median(ts))


def clock_mhz():
    import torch
    try:
        return float(torch.cuda.clock_rate(0))
    except Exception:
        return None


def pair_count(nfft, cplx, cross):
    from pyfft_amd.bispectrum import valid_region
    ok = valid_region(nfft, cplx)
    return int(ok.sum()) if cross else int(np.tril(ok).sum())


def main():
    import torch
    from pyfft_amd import engine as E, _ffi
    from test_host_bispectrum import oracle_spectra, oracle_sums
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-frames", type=int, default=256)
    ap.add_argument("--only", default="", help="comma-separated shape indices")
    args = ap.parse_args()
    _ffi.init()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    only = {int(s) for s in args.only.split(",") if s}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for k, (name, dt, nfft, lg, cross) in enumerate(SHAPES):
        if only and k not in only:
            continue
        n = 1 << lg
        cplx = dt == "complex64"
        hop = nfft // 2
        M = 1 + (n - nfft) // hop
        win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)

        def sig():
            if cplx:
                return torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=gen))
            return torch.randn(n, device="cuda", generator=gen)
        x = sig()
        y, z = (sig(), sig()) if cross else (None, None)

        def call():
            return E.bispectrum(x, win, hop, M, y=y, z=z, detrend=True)
        os.environ.pop("SP_BISPEC_MIB", None)
        call_ms = timed(call, args.warmup, args.reps)
        mhz0 = clock_mhz()
        os.environ["SP_BISPEC_MIB"] = "4096"
        E.profile_enable(True)
        tiles = []
        for _ in range(args.warmup + args.reps):
            call()
            torch.cuda.synchronize()
            tiles.append(E.profile_last_ms())
        E.profile_enable(False)
        os.environ.pop("SP_BISPEC_MIB", None)
        tile_ms = float(np.median(tiles[args.warmup:]))
        mhz = clock_mhz() or mhz0
        clk = (mhz or 2400.0) * 1e6
        pairs = pair_count(nfft, cplx, cross)
        pf = pairs * M
        lane_ops = 10.0 * pf
        t_unp = lane_ops / (ncu * 64 * clk)
        t_pk = lane_ops / (ncu * 128 * clk)
        # numpy float64 over a frame subset, scaled
        xs = x.cpu().numpy()
        mf = min(args.cpu_frames, M)
        t0 = time.perf_counter()
        X = oracle_spectra(xs, win, nfft, hop, mf, 1)
        Y = X if y is None else oracle_spectra(y.cpu().numpy(), win, nfft, hop, mf, 1)
        Z = X if z is None else oracle_spectra(z.cpu().numpy(), win, nfft, hop, mf, 1)
        oracle_sums(X, Y, Z, nfft // 2 if cplx else 0)
        cpu_s = (time.perf_counter() - t0) * M / mf
        print(json.dumps({"shape": name, "dtype": dt, "nfft": nfft, "nsig": n, "hop": hop, "frames": M, "pairs": pairs,
                          "call_ms": round(call_ms, 4), "tile_ms": round(tile_ms, 4),
                          "pair_frames_per_s": float("%.4g" % (pf / (tile_ms * 1e-3))),
                          "valu_unpacked": round(t_unp * 1e3 / tile_ms, 3), "valu_packed": round(t_pk * 1e3 / tile_ms, 3),
                          "bound_unpacked_ms": round(t_unp * 1e3, 4), "clock_mhz": mhz, "cpu_s": round(cpu_s, 2),
                          "cpu_frames": mf}), flush=True)
        del x, y, z
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
