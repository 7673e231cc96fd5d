#!/usr/bin/env python3
"""Wavelet coherence and cross-wavelet transform of two 2^22-sample real records, Morlet w0 = 6, dj = 1/12 over the scales 4 .. 300 samples
(and 4 .. 50), against what the same commit composes from the pieces it had before.  Device-resident input; one JSON line per shape.
  wct_ms            wavelet.wct, every scale fused: k_wct_time, then k_wct_scale (sustained: back-to-back calls between one pair of HIP
                    events, *_calls of them)
  time_kernel_ms, scale_kernel_ms   the two kernels alone (library profiling events, one isolated launch each)
  wct_composed_ms   the same scales forced through the whole-record path of wavelet.wct (engine.fft / multiply / engine.ifft for Wx, Wy and
                    for the Gaussian, a chunk of scales at a time), timed before and after the fused calls: their difference is the spread
  xwt_ms            wavelet.xwt, fused: Wx conj(Wy) without Wx or Wy in memory
  xwt_composed_ms   two wavelet.cwt calls (k_cwt) and an elementwise multiply
  *_bytes           the records once plus what is written; transforms_per_s = frames x scales x 6 (and the two forward ones per frame and
                    scale chunk) / the time kernel's time
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/wct_bench.py [--reps 5] > profiles/wct_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                      # noqa: E402

LOG2N = 22
DJ = 1.0 / 12
# (smallest, largest scale in samples)
SHAPES = [(4.0, 300.0), (4.0, 50.0)]


def one(idx, warmup, reps):
    import numpy as np
    import torch
    from pyfft_amd import engine as E, wavelet as WV
    smin, smax = SHAPES[idx]
    n = 1 << LOG2N
    scales = smin * 2.0 ** (np.arange(int(np.log2(smax / smin) / DJ) + 1) * DJ)
    plan = WV.wct_plan(n, dj=DJ, scales=scales)
    assert plan["fused"].all()
    S, L, Mw, Mg = len(scales), plan["L"], plan["Mw"], plan["Mg"]
    g = torch.Generator(device="cuda").manual_seed(idx)
    x = torch.randn(n, device="cuda", generator=g)
    y = 0.5 * x + torch.randn(n, device="cuda", generator=g)
    taps = WV.scale_window(DJ)

    def timed(fn):
        """windows of about `reps` tenths of a second: the repetitions follow from a first estimate"""
        est = measure(fn, warmup, 2)[0]
        r = int(min(max(100.0 * reps / max(est, 1e-3), 3), 2000))
        return measure(fn, 1, r) + (r,)

    def kernel_ms(fn):
        E.profile_enable(True)
        out = fn()
        torch.cuda.synchronize()
        k = E.profile_last_ms()
        E.profile_enable(False)
        return k, out

    def fused():
        return WV.wct(x, y, dj=DJ, scales=scales)[0]

    def composed():
        keep = WV.FUSED_MAX_MARGIN
        WV.FUSED_MAX_MARGIN = -1                          # no scale fuses: every row takes the whole-record path
        try:
            return WV.wct(x, y, dj=DJ, scales=scales)[0]
        finally:
            WV.FUSED_MAX_MARGIN = keep

    def xwt_fused():
        return WV.xwt(x, y, scales=scales)[0]

    def xwt_composed():
        return WV.cwt(x, scales=scales)[0] * WV.cwt(y, scales=scales)[0].conj()

    c1 = timed(composed)
    tf = timed(fused)
    kt, T = kernel_ms(lambda: E.wct_time(x, y, scales, "morlet", 6.0, L, Mw, Mg))
    ks, _ = kernel_ms(lambda: E.wct_scale(T, taps))
    del T
    c2 = timed(composed)
    xf = timed(xwt_fused)
    xc = timed(xwt_composed)
    pw = WV.cwt_plan(n, scales=scales)
    kx, _ = kernel_ms(lambda: E.wct_time(x, y, scales, "morlet", 6.0, pw["L"], pw["M"], 0, xwt=True))
    p = E.wct_plan(n, S, L, Mw, Mg)
    cm = min(c1[0], c2[0])
    nchunks = -(-S // p["chunk"])
    out = {"dtype": "float32", "nsig": n, "scales": S, "smin": smin, "smax": float(scales[-1]), "dj": DJ, "ntaps": len(taps), "L": L, "Mw": Mw,
           "Mg": Mg, "hop": plan["hop"], "frames": plan["frames"], "chunk": p["chunk"], "workgroups": p["workgroups"], "lds_bytes": p["lds_bytes"],
           "wct_ms": round(tf[0], 4), "wct_iso_ms": round(tf[1], 4), "wct_calls": tf[2], "time_kernel_ms": round(kt, 4),
           "scale_kernel_ms": round(ks, 4), "wct_composed_ms": round(c1[0], 4), "wct_composed2_ms": round(c2[0], 4), "wct_composed_calls": c1[2],
           "composed_spread": round(abs(c1[0] - c2[0]) / cm, 4), "composed_over_fused": round(cm / tf[0], 3),
           "time_bytes": 8 * n + 16 * S * n, "scale_bytes": 16 * S * n + 8 * S * n,
           "time_store_TBps": round(16 * S * n / (kt * 1e-3) / 1e12, 3), "scale_TBps": round(24 * S * n / (ks * 1e-3) / 1e12, 3),
           "transforms_per_s": float("%.4g" % (plan["frames"] * (6 * S + 2 * nchunks) / (kt * 1e-3))),
           "xwt_ms": round(xf[0], 4), "xwt_calls": xf[2], "xwt_kernel_ms": round(kx, 4), "xwt_L": pw["L"], "xwt_M": pw["M"],
           "xwt_composed_ms": round(xc[0], 4), "xwt_composed_calls": xc[2], "xwt_composed_over_fused": round(xc[0] / xf[0], 3),
           "xwt_store_TBps": round(8 * S * n / (kx * 1e-3) / 1e12, 3)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="tenths of a second per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=200, help="seconds per shape")
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
