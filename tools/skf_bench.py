#!/usr/bin/env python3
"""Two-point wavenumber-frequency spectrum (sp_skf) of a 2^26-sample real pair against the Welch cross spectrum of the same records at
the same nfft and hop (sp_welch_csd): the yardstick reads the same samples and does the same ONE real-pair transform per frame; this
kernel adds an atan2, a histogram in LDS and, where the band's cells do not fit one tile, a repeat of the transforms per tile.
Device-resident input; one JSON line per shape: nfft 256 and 1024 with nk 65 over a quarter band and the full band, and nfft 4096 over
the full band with nk 128, the many-tiles case.
  skf_ms, skf_iso_ms     engine.skf, sustained (back-to-back calls between one pair of HIP events) and isolated
  skf_kernel_ms          k_skf alone (library profiling events)
  csd_ms, csd2_ms        engine.welch_csd, sustained, timed before and after (their difference: the spread)
  tiles, transforms      skf_plan: frequency tiles and transforms per frame
  bytes                  both records once per tile plus the float32 partials and the table; roofline_ms = bytes / 8 TB/s, the HBM peak
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/skf_bench.py [--reps 10] > profiles/skf_bench.txt"""
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
# (nfft, nk, b0, nb); hop = nfft / 2
SHAPES = [(256, 65, 16, 32), (256, 65, 0, 129), (1024, 65, 64, 128), (1024, 65, 0, 513), (4096, 128, 0, 2049)]


def one(idx, warmup, reps):
    import numpy as np
    import torch
    from pyfft_amd import engine as E
    from pyfft_amd.wavenumber import skf_plan
    nfft, nk, b0, nb = SHAPES[idx]
    hop, n = nfft // 2, 1 << LOG2N
    g = torch.Generator(device="cuda").manual_seed(idx)
    s = torch.randn(n + 3, device="cuda", generator=g)
    x = (s[3:] + 0.3 * torch.randn(n, device="cuda", generator=g) + 1.5).contiguous()
    y = (s[:n] + 0.3 * torch.randn(n, device="cuda", generator=g) - 0.7).contiguous()
    del s
    plan = skf_plan(nfft, nk, nb=nb)
    M = 1 + (n - nfft) // hop
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)).astype(np.float32)

    def csd():
        return E.welch_csd(x, y, win, hop, M, detrend=True, sided=E.SIDED_ONE)

    def skf():
        return E.skf(x, y, nfft, hop, M, b0, nb, nk, win=win, segmean=True, scale=1.0)

    csd()
    skf()
    torch.cuda.synchronize()
    c1 = measure(csd, warmup, reps)
    t = measure(skf, warmup, reps)
    E.profile_enable(True)
    skf()
    k = E.profile_last_ms()
    E.profile_enable(False)
    c2 = measure(csd, warmup, reps)
    cm = min(c1[0], c2[0])
    read = 2 * 4 * n * plan["tiles"]
    out = {"dtype": "float32", "nfft": nfft, "hop": hop, "nk": nk, "b0": b0, "nb": nb, "nsig": n, "frames": M, "tiles": plan["tiles"],
           "tile_bins": plan["tile_bins"], "lds_bytes": plan["lds_bytes"], "transforms": plan["transforms"],
           "skf_ms": round(t[0], 4), "skf_iso_ms": round(t[1], 4), "skf_kernel_ms": round(k, 4), "read_bytes": read,
           "roofline_ms": round(read / HBM_PEAK * 1e3, 4), "csd_ms": round(c1[0], 4), "csd2_ms": round(c2[0], 4),
           "csd_spread": round(abs(c1[0] - c2[0]) / cm, 4), "skf_over_csd": round(t[0] / cm, 3),
           "frames_per_s": float("%.4g" % (M / (t[0] * 1e-3)))}
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
