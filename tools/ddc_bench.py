#!/usr/bin/env python3
"""The digital down-converter (sp_ddc) alone, and the band PSD built on it against the chirp-z zoom PSD over the same band at the same
resolution.  Device-resident input; one JSON line per shape.
  kind "ddc":   baseband.ddc of a 2^24-sample record at the plan's default filters (atten 90 dB, width 0.2), q = 8, 64 and 256 (two stages)
      ms, iso_ms      sustained (back-to-back calls between one pair of HIP events, per call); median of single synchronised calls
      kernel_ms       k_ddc alone (library profiling events; single-stage shapes only)
      gsamples_s      input samples per second of the sustained figure
      roof_fraction   (bytes read once + bytes written once) / sustained time, over the streaming roof of 3.8 TB/s
      macs_per_sample taps / q of every stage, referred to the input rate
  kind "band":  baseband.band_psd (nperseg at the rate fs / q) against zoom.zoom_psd with nperseg q times as long and m = the bins
      band_psd keeps, both over fc +- (1 - width) fs / (2 q), hop = nperseg / 2, two-sided
      band_ms, zoom_ms, zoom_over_band   sustained, and their ratio
  The last shapes are the reference's long segment: zoom nperseg = 116 508 (the multi-pass chirp-z) against band nperseg = 1821 at q = 64
  and 455 at q = 256.
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/ddc_bench.py [--reps 10] > profiles/r10_ddc_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                                         # noqa: E402

ROOF = 3.8e12                                                                # bytes per second, streaming
LOG2N = 24
# ("ddc", complex, q) and ("band", complex, q, band nperseg, zoom nperseg, log2 nsig)
SHAPES = ([("ddc", c, q) for c in (False, True) for q in (8, 64, 256)] +
          [("band", c, q, n, q * n, 24) for c in (False, True) for q, n in ((8, 512), (8, 1024), (64, 64), (64, 128))] +
          [("band", False, 64, 1821, 116508, 22), ("band", True, 64, 1821, 116508, 22), ("band", False, 256, 455, 116508, 22)])


def record(n, cplx, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, device="cuda", generator=g) + 0.5
    return torch.complex(x, torch.randn(n, device="cuda", generator=g)) if cplx else x


def one_ddc(idx, warmup, reps):
    import torch
    from pyfft_amd import engine as E, baseband as BB
    _, cplx, q = SHAPES[idx]
    n = 1 << LOG2N
    x = record(n, cplx, idx)
    stages = BB.ddc_plan(q)

    def run():
        return BB.ddc(x, 0.11, q)

    run()
    torch.cuda.synchronize()
    ms, iso = measure(run, warmup, reps)
    kernel_ms = None
    if len(stages) == 1:
        E.profile_enable(True)
        run()
        kernel_ms = round(E.profile_last_ms(), 4)
        E.profile_enable(False)
    nbytes, macs, rate = 0.0, 0.0, 1.0
    for i, (qi, h) in enumerate(stages):
        nbytes += n * rate * ((8 if cplx or i else 4) + 8.0 / qi)
        macs += rate * h.size / qi
        rate /= qi
    print(json.dumps({"kind": "ddc", "dtype": "complex64" if cplx else "float32", "q": q, "stages": [[qi, int(h.size)] for qi, h in stages],
                      "nsig": n, "ms": round(ms, 4), "iso_ms": round(iso, 4), "kernel_ms": kernel_ms,
                      "gsamples_s": float("%.4g" % (n / (ms * 1e-3) / 1e9)), "bytes": int(nbytes),
                      "roof_fraction": round(nbytes / (ms * 1e-3) / ROOF, 4), "macs_per_sample": round(macs, 2)}), flush=True)


def one_band(idx, warmup, reps):
    import torch
    from pyfft_amd import baseband as BB, zoom as ZM
    _, cplx, q, nb, nz, lg = SHAPES[idx]
    n = 1 << lg
    x = record(n, cplx, idx)
    fc, width = 0.11, 0.2
    p = BB.band_plan(n, cplx, fc, q, nperseg=nb, return_onesided=False)
    m = int(p["freq"].size)
    half = (1.0 - width) / (2.0 * q)

    def band():
        return BB.band_psd(x, fc, q, nperseg=nb, return_onesided=False)[1]

    def zoom():
        return ZM.zoom_psd(x, [fc - half, fc + half], m, nperseg=nz, return_onesided=False)[1]

    band(), zoom()
    torch.cuda.synchronize()
    b1 = measure(band, warmup, reps)
    z = measure(zoom, warmup, reps)
    b2 = measure(band, warmup, reps)
    bm = min(b1[0], b2[0])
    print(json.dumps({"kind": "band", "dtype": "complex64" if cplx else "float32", "q": q, "band_nperseg": nb, "zoom_nperseg": nz, "m": m,
                      "nsig": n, "band_frames": p["nframes"], "zoom_frames": 1 + (n - nz) // (nz - nz // 2), "band_ms": round(b1[0], 4),
                      "band2_ms": round(b2[0], 4), "band_spread": round(abs(b1[0] - b2[0]) / bm, 4), "zoom_ms": round(z[0], 4),
                      "zoom_over_band": round(z[0] / bm, 3), "band_iso_ms": round(min(b1[1], b2[1]), 4), "zoom_iso_ms": round(z[1], 4)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
    args = ap.parse_args()
    if args.one >= 0:
        return (one_ddc if SHAPES[args.one][0] == "ddc" else one_band)(args.one, args.warmup, args.reps)
    for i in range(len(SHAPES)):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(i), "--reps", str(args.reps), "--warmup",
                             str(args.warmup)], timeout=args.limit).returncode
        if rc != 0:
            sys.exit("shape %s failed (exit %d): stopping" % (SHAPES[i], rc))


if __name__ == "__main__":
    main()
