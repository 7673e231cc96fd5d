#!/usr/bin/env python3
"""The polyphase filter-bank channelizer (sp_pfb) on a device-resident complex64 record of 2^26 samples; one JSON line per shape
(M, P, D): M = 1024 and 4096 channels, P = 4 and 8 taps per channel, hop D = M and 3 M / 4, phase "time".
      ms, iso_ms         engine.pfb, frames: sustained (back-to-back calls between one pair of HIP events, per call); median of single
                         synchronised calls.  ms is the smaller of two sustained runs taken before and after the STFT's; spread = their
                         relative difference
      gbytes_s           (input bytes + output bytes) / ms
      stft_ms            engine.stft_frames at nfft = M (Hann), the same hop and input: the same output volume from 1 / P of the reads
                         and multiply-adds
      pfb_over_stft      ms / stft_ms
      power_ms           engine.pfb(power=True): the accumulated channel powers, no frames written
      frames_reduce_ms   frames mode followed by the reduction a caller would run on them (mean over the frames of |X|^2, torch, on the
                         device): what power_ms has to beat
      notreg_ms          frames with SP_PFB_TREG=0 (the taps re-read from the table every frame) where the register-held form applies
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/pfb_bench.py [--reps 10] > profiles/pfb_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                                         # noqa: E402

LOG2N = 26
SHAPES = [(M, P, D) for M in (1024, 4096) for P in (4, 8) for D in (M, 3 * M // 4)]


def one(idx, warmup, reps):
    import numpy as np
    import torch
    from pyfft_amd import engine as E, channelizer as CH
    M, P, D = SHAPES[idx]
    n = 1 << LOG2N
    g = torch.Generator(device="cuda").manual_seed(idx)
    x = torch.complex(torch.randn(n, device="cuda", generator=g) + 0.5, torch.randn(n, device="cuda", generator=g))
    p = CH.pfb_plan(n, True, M, P, D)
    h, nf, r0 = p["h"], p["nframes"], p["r0"]
    win = np.hanning(M + 1)[:M]
    nf_stft = (n - M) // D + 1

    def frames():
        return E.pfb(x, h, M, D, 0, nf, 1, r0)

    def power():
        return E.pfb(x, h, M, D, 0, nf, 1, r0, power=True)

    def frames_reduce():
        X = frames()
        return (X.real * X.real + X.imag * X.imag).mean(dim=0, dtype=torch.float64)

    def stft():
        return E.stft_frames(x, win, D, nf_stft, detrend=False, sided=E.SIDED_RAW)[0]

    frames(), power(), stft()
    torch.cuda.synchronize()
    a = measure(frames, warmup, reps)
    s = measure(stft, warmup, reps)
    b = measure(frames, warmup, reps)
    pw = measure(power, warmup, reps)
    fr = measure(frames_reduce, warmup, reps)
    ms = min(a[0], b[0])
    notreg = None
    if P <= 4 and D % M == 0:
        os.environ["SP_PFB_TREG"] = "0"
        notreg = round(measure(frames, warmup, reps)[0], 4)
        del os.environ["SP_PFB_TREG"]
    nbytes = 8 * n + 8 * nf * M
    print(json.dumps({"M": M, "P": P, "hop": D, "nsig": n, "nframes": nf, "ms": round(ms, 4), "spread": round(abs(a[0] - b[0]) / ms, 4),
                      "iso_ms": round(min(a[1], b[1]), 4), "bytes": nbytes, "gbytes_s": float("%.4g" % (nbytes / (ms * 1e-3) / 1e9)),
                      "stft_ms": round(s[0], 4), "stft_frames": nf_stft, "pfb_over_stft": round(ms / s[0], 3),
                      "power_ms": round(pw[0], 4), "frames_reduce_ms": round(fr[0], 4), "notreg_ms": notreg}), flush=True)


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
