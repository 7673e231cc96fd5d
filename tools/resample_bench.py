#!/usr/bin/env python3
"""The rational resampler (sp_upfirdn) through resample.resample_poly at scipy's default filter: device-resident rows of 2^26 samples,
real and complex, at the ratios 3/2, 2/3, 160/147, 4/1 and 1/4.  One JSON line per shape.
      ms, iso_ms      sustained (back-to-back calls between one pair of HIP events, per call); median of single synchronised calls
      kernel_ms       k_upfirdn alone (library profiling events)
      gbytes_s        (bytes read once + bytes written once) / sustained time
      of_streaming    that rate over the 3.8 TB/s the streaming kernels of this library reach (the roof of tools/ddc_bench.py)
      of_hbm          and over the 8 TB/s of the memory
      macs_per_output taps per phase, ceil(ntaps / up); tmacs_s the real-tap MACs per second they amount to
  At 1/4 the existing decimator runs on the same record with the same taps (engine.ddc(x, 0.0, 4, h), complex64 out whatever the input):
      ddc_ms, ddc_kernel_ms, upfirdn_over_ddc (sustained)
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/resample_bench.py [--reps 10] > profiles/resample_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                                         # noqa: E402

STREAMING, HBM = 3.8e12, 8.0e12                                              # bytes per second
LOG2N = 26
SHAPES = [(c, up, down) for c in (False, True) for up, down in ((3, 2), (2, 3), (160, 147), (4, 1), (1, 4))]


def one(idx, warmup, reps):
    import torch
    from pyfft_amd import engine as E, resample as RS
    cplx, up, down = SHAPES[idx]
    n = 1 << LOG2N
    g = torch.Generator(device="cuda").manual_seed(idx)
    x = torch.randn(n, device="cuda", generator=g) + 0.5
    if cplx:
        x = torch.complex(x, torch.randn(n, device="cuda", generator=g))
    plan = RS.resample_plan(n, up, down, cplx=cplx)
    ntaps = plan["taps"].size + plan["pre"]

    def run():
        return RS.resample_poly(x, up, down)

    def kernel_ms(fn):
        E.profile_enable(True)
        fn()
        ms = round(E.profile_last_ms(), 4)
        E.profile_enable(False)
        return ms

    y = run()
    torch.cuda.synchronize()
    assert y.shape == (plan["nout"],) and y.dtype == x.dtype
    ms, iso = measure(run, warmup, reps)
    es = 8 if cplx else 4
    nbytes = es * (n + plan["nout"])
    macs = -(-ntaps // up)
    rec = {"kind": "resample_poly", "dtype": "complex64" if cplx else "float32", "up": up, "down": down, "ntaps": int(ntaps),
           "nsig": n, "nout": plan["nout"], "tile": plan["tile"], "workgroups": plan["workgroups"], "ms": round(ms, 4),
           "iso_ms": round(iso, 4), "kernel_ms": kernel_ms(run), "bytes": int(nbytes),
           "gbytes_s": float("%.4g" % (nbytes / (ms * 1e-3) / 1e9)), "of_streaming": round(nbytes / (ms * 1e-3) / STREAMING, 4),
           "of_hbm": round(nbytes / (ms * 1e-3) / HBM, 4), "macs_per_output": macs,
           "tmacs_s": float("%.4g" % (macs * plan["nout"] * (2 if cplx else 1) / (ms * 1e-3) / 1e12))}
    if (up, down) == (1, 4):
        h = plan["taps"]

        def ddc():
            return E.ddc(x, 0.0, 4, h)

        ddc()
        torch.cuda.synchronize()
        dms, _ = measure(ddc, warmup, reps)
        rec.update(ddc_ms=round(dms, 4), ddc_kernel_ms=kernel_ms(ddc), upfirdn_over_ddc=round(ms / dms, 3))
    print(json.dumps(rec), flush=True)


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
