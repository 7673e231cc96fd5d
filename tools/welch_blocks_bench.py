#!/usr/bin/env python3
"""Time-resolved Welch spectra (sp_welch_blocks: running PSD, CSD of a pair in blocks of navg frames) against the composed route that
existed before it: engine.stft_frames of both records (complex64 spectrograms in memory), then the block means of |X|^2, |Y|^2 and
conj(X) Y with torch on the device.  Device-resident input, 2^26 real float32 samples per record (2^25 complex64 for the complex case),
hop = nfft / 2, Hann, every frame's own mean removed; one JSON line per shape: nfft 256 / 1024 / 4096 with navg 8 and step 8 (disjoint
blocks: the kernel writes the outputs) and step 2 (overlapping blocks: run sums of 2 frames, then k_block_sum), and one complex case.
  fused_ms, fused2_ms    engine.welch_blocks, sustained: back-to-back calls between one pair of HIP events, as many as fill about
                         --window seconds (fused_reps); the two routes are timed twice in alternation, fused, composed, fused,
                         composed, and fused_spread is the difference of the two over their mean; fused_iso_ms: isolated calls, the median
  kernel_ms              k_welch_blocks alone (library profiling events)
  composed_ms, composed2_ms  the two stft_frames calls and the torch block means, likewise (composed_reps, composed_spread, composed_iso_ms)
  ratio                  mean of the composed timings / mean of the fused timings: above 1, the fused call is faster
  bytes_fused/composed   running_plan's byte counts (samples a frame loads, run sums or spectrograms written and read, outputs)
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/welch_blocks_bench.py [--reps 10] > profiles/welch_blocks_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                      # noqa: E402

# (complex, nfft, navg, step, log2 nsig)
SHAPES = [(False, n, 8, s, 26) for n in (256, 1024, 4096) for s in (8, 2)] + [(True, 1024, 8, 8, 25)]


def measure_window(fn, n):
    """ms per call over n back-to-back calls between one pair of HIP events."""
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def one(idx, warmup, reps, window):
    import numpy as np
    import torch
    from pyfft_amd import engine as E
    from pyfft_amd.running import running_plan
    cplx, nfft, navg, step, lg = SHAPES[idx]
    hop, n = nfft // 2, 1 << lg
    g = torch.Generator(device="cuda").manual_seed(idx)

    def noise(m):
        v = torch.randn(m, device="cuda", generator=g)
        return torch.complex(v, torch.randn(m, device="cuda", generator=g)) if cplx else v
    s = noise(n + 3)
    x = (s[3:] + 0.3 * noise(n) + 1.5).contiguous()
    y = (s[:n] + 0.3 * noise(n) - 0.7).contiguous()
    del s
    M = 1 + (n - nfft) // hop
    nblocks = (M - navg) // step + 1
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)).astype(np.float32)
    scale = 1.0 / float(np.sum(win.astype(np.float64) ** 2))
    plan = running_plan(n, nfft, nfft - hop, navg, step, nch=1, cplx=cplx)
    sided = E.SIDED_RAW if cplx else E.SIDED_HALF

    def fused():
        return E.welch_blocks(x, win, hop, M, navg, step, y=y, detrend=True, scale=scale)

    def block_mean(v):
        return v.unfold(0, navg, step).mean(dim=-1)

    def composed():
        X = E.stft_frames(x, win, hop, M, detrend="segmean", sided=sided)[0]
        Y = E.stft_frames(y, win, hop, M, detrend="segmean", sided=sided)[0]
        pxx = block_mean(X.real * X.real + X.imag * X.imag) * scale
        pyy = block_mean(Y.real * Y.real + Y.imag * Y.imag) * scale
        pxy = block_mean(X.conj() * Y) * scale
        return pxx, pyy, pxy

    a, b = fused(), composed()
    torch.cuda.synchronize()
    # the two routes compute the same thing: worst difference over every bin of every block, relative to the block's largest bin
    diff = max(float(((p - q).abs().amax(dim=1) / q.abs().amax(dim=1)).max()) for p, q in zip(a, b))
    assert tuple(a[0].shape) == (nblocks, plan["nf"]) and diff < 1e-4, diff
    del a, b
    # both routes twice, in alternation; every sustained window is sized to about `window` seconds from a first estimate
    def timed(fn):
        est = measure(fn, warmup, 5)[0]
        n = max(reps, min(20000, int(window * 1e3 / est) + 1))
        return measure_window(fn, n), n
    (f1, nf), (c1, nc) = timed(fused), timed(composed)
    (f2, _), (c2, _) = timed(fused), timed(composed)
    iso_f, iso_c = measure(fused, warmup, reps)[1], measure(composed, warmup, reps)[1]
    E.profile_enable(True)
    fused()
    k = E.profile_last_ms()
    E.profile_enable(False)
    fm, cm = 0.5 * (f1 + f2), 0.5 * (c1 + c2)
    out = {"dtype": "complex64" if cplx else "float32", "nfft": nfft, "hop": hop, "navg": navg, "step": step, "nsig": n, "frames": M,
           "blocks": nblocks, "q": plan["q"], "runs": plan["runs"], "workgroups": plan["workgroups"], "scratch_bytes": plan["scratch"],
           "fused_ms": round(f1, 4), "fused2_ms": round(f2, 4), "fused_iso_ms": round(iso_f, 4), "kernel_ms": round(k, 4),
           "fused_spread": round(abs(f1 - f2) / fm, 4), "fused_reps": nf, "composed_ms": round(c1, 4), "composed2_ms": round(c2, 4),
           "composed_iso_ms": round(iso_c, 4), "composed_spread": round(abs(c1 - c2) / cm, 4), "composed_reps": nc,
           "ratio": round(cm / fm, 3), "bytes_fused": plan["bytes_fused"], "bytes_composed": plan["bytes_composed"],
           "max_rel_diff": float("%.3g" % diff), "frames_per_s": float("%.4g" % (M / (fm * 1e-3)))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per sustained timing")
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=150, help="seconds per shape")
    args = ap.parse_args()
    if args.one >= 0:
        return one(args.one, args.warmup, args.reps, args.window)
    for i in range(len(SHAPES)):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(i), "--reps", str(args.reps), "--warmup",
                             str(args.warmup), "--window", str(args.window)], timeout=args.limit).returncode
        if rc != 0:
            sys.exit("shape %s failed (exit %d): stopping" % (SHAPES[i], rc))


if __name__ == "__main__":
    main()
