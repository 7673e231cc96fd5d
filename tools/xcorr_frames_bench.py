#!/usr/bin/env python3
"""Short-time cross-correlation (sp_xcorr_frames) of a 2^26-sample real pair, its three outputs one at a time, against the Welch cross
spectrum of the same records at nfft = L and the same hop (sp_welch_csd): the yardstick reads the same samples and does ONE real-pair
transform per frame where this kernel does two (forward and inverse).  Device-resident input; one JSON line per shape.
  avg_ms, peak_ms, frames_ms   engine.xcorr_frames with that output alone, sustained (back-to-back calls between one pair of HIP events)
  *_kernel_ms                  k_xcorr_frames alone (library profiling events)
  csd_ms, csd2_ms              engine.welch_csd, sustained, timed before and after (their difference: the spread)
  read_bytes                   both records once (a hop of half a window re-reads the other half from cache)
  *_bytes                      read_bytes plus what that output writes; *_roofline_ms = bytes / 8 TB/s, the HBM peak
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/xcorr_frames_bench.py [--reps 10] > profiles/xcorr_frames_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                      # noqa: E402

HBM_PEAK = 8.0e12
LOG2N = 26
# (nav, maxlag); hop = nav / 2
SHAPES = [(1024, 128), (1024, 1023), (4096, 128), (4096, 4095)]


def one(idx, warmup, reps):
    import numpy as np
    import torch
    from pyfft_amd import engine as E
    from pyfft_amd.ccf import ccf_plan
    nav, maxlag = SHAPES[idx]
    hop, n = nav // 2, 1 << LOG2N
    g = torch.Generator(device="cuda").manual_seed(idx)
    s = torch.randn(n + 5, device="cuda", generator=g)
    x = (s[5:] + 0.3 * torch.randn(n, device="cuda", generator=g) + 1.5).contiguous()
    y = (s[:n] + 0.3 * torch.randn(n, device="cuda", generator=g) - 0.7).contiguous()
    del s
    plan = ccf_plan(nav, maxlag)
    L, nl = plan["L"], plan["nlags"]
    M = 1 + (n - nav) // hop
    Mc = 1 + (n - L) // hop
    ones = np.ones(L, dtype=np.float32)

    def csd():
        return E.welch_csd(x, y, ones, hop, Mc, detrend=True, sided=E.SIDED_ONE)

    def xc(**want):
        return lambda: E.xcorr_frames(x, y, nav, hop, M, maxlag, **want)

    runs = {"avg": xc(avg=True), "peak": xc(peak=True), "frames": xc(frames=True)}
    csd()
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    c1 = measure(csd, warmup, reps)
    out = {"dtype": "float32", "nav": nav, "hop": hop, "maxlag": maxlag, "L": L, "nsig": n, "frames": M, "csd_frames": Mc}
    read = 2 * 4 * n
    wrote = {"avg": 8 * nl, "peak": 8 * M, "frames": 4 * nl * M}
    for name, fn in runs.items():
        t = measure(fn, warmup, reps)
        E.profile_enable(True)
        fn()
        k = E.profile_last_ms()
        E.profile_enable(False)
        out.update({name + "_ms": round(t[0], 4), name + "_iso_ms": round(t[1], 4), name + "_kernel_ms": round(k, 4),
                    name + "_bytes": read + wrote[name], name + "_roofline_ms": round((read + wrote[name]) / HBM_PEAK * 1e3, 4)})
    c2 = measure(csd, warmup, reps)
    cm = min(c1[0], c2[0])
    out.update({"read_bytes": read, "csd_ms": round(c1[0], 4), "csd2_ms": round(c2[0], 4), "csd_spread": round(abs(c1[0] - c2[0]) / cm, 4),
                "avg_over_csd": round(out["avg_ms"] / cm, 3), "peak_over_csd": round(out["peak_ms"] / cm, 3),
                "frames_over_csd": round(out["frames_ms"] / cm, 3), "frames_per_s_peak": float("%.4g" % (M / (out["peak_ms"] * 1e-3)))})
    print(json.dumps(out), flush=True)


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
