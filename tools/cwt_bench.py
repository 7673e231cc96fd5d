#!/usr/bin/env python3
"""Continuous wavelet transform (sp_cwt) of a 2^22-sample real record, Morlet w0 = 6, dj = 1/12 over the scales 4 .. 600 samples, its
outputs one at a time, against the composed whole-record path on the same commit over the same scales (engine.fft of the record
zero-padded to 2^23, a broadcast multiply with the filter rows, batched engine.ifft, a chunk of scales at a time).  Device-resident
input; one JSON line per shape.
  w_ms, gws_ms, recon_ms     engine.cwt with that output alone, sustained (back-to-back calls between one pair of HIP events, *_calls
                             of them: windows of about half a second)
  *_kernel_ms                k_cwt alone (library profiling events)
  composed_ms, composed2_ms  the composed path forming W, timed before and after (their difference: the spread)
  *_bytes                    the record once plus what that output writes; w_store_TBps = the W bytes / the kernel's time
The shapes differ in the scale range, which sets the margin and with it L and hop.
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/cwt_bench.py [--reps 5] > profiles/cwt_bench.txt"""
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
SHAPES = [(4.0, 600.0), (4.0, 50.0), (4.0, 200.0)]


def one(idx, warmup, reps):
    import numpy as np
    import torch
    from pyfft_amd import engine as E, wavelet as WV
    smin, smax = SHAPES[idx]
    n = 1 << LOG2N
    wv = WV.Morlet(6.0)
    scales = smin * 2.0 ** (np.arange(int(np.log2(smax / smin) / DJ) + 1) * DJ)
    plan = WV.cwt_plan(n, scales=scales)
    assert plan["fused"].all()
    S, L, M = len(scales), plan["L"], plan["M"]
    g = torch.Generator(device="cuda").manual_seed(idx)
    x = torch.randn(n, device="cuda", generator=g)
    wr = WV.recon_weights(wv, scales, 1.0, DJ)

    def composed():
        out = None
        for _, _, Wc in WV._composed_chunks(x, wv, scales, 2 * n):
            out = Wc
        return out

    def cw(**want):
        return lambda: E.cwt(x, scales, "morlet", 6.0, L, M, **want)

    def timed(fn):
        """windows of about `reps` tenths of a second: the repetitions follow from a first estimate"""
        est = measure(fn, warmup, 2)[0]
        r = int(min(max(100.0 * reps / max(est, 1e-3), 3), 2000))
        return measure(fn, 1, r) + (r,)

    runs = {"w": cw(W=True), "gws": cw(W=False, gws=True), "recon": cw(W=False, recon=wr)}
    c1 = timed(composed)
    out = {"dtype": "float32", "nsig": n, "scales": S, "smin": smin, "smax": float(scales[-1]), "dj": DJ, "L": L, "M": M, "hop": plan["hop"],
           "frames": plan["frames"]}
    wrote = {"w": 8 * S * n, "gws": 8 * S, "recon": 8 * n}
    for name, fn in runs.items():
        p = E.cwt_plan(n, S, L, M, W=name == "w", gws=name == "gws", recon=name == "recon")
        t = timed(fn)
        E.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        k = E.profile_last_ms()
        E.profile_enable(False)
        out.update({name + "_ms": round(t[0], 4), name + "_iso_ms": round(t[1], 4), name + "_kernel_ms": round(k, 4), name + "_calls": t[2],
                    name + "_bytes": 4 * n + wrote[name], name + "_chunk": p["chunk"], name + "_workgroups": p["workgroups"]})
    c2 = timed(composed)
    cm = min(c1[0], c2[0])
    out.update({"composed_ms": round(c1[0], 4), "composed2_ms": round(c2[0], 4), "composed_calls": c1[2], "composed_spread": round(abs(c1[0] - c2[0]) / cm, 4),
                "composed_over_w": round(cm / out["w_ms"], 3), "w_over_gws": round(out["w_ms"] / out["gws_ms"], 3),
                "w_over_recon": round(out["w_ms"] / out["recon_ms"], 3),
                "w_store_TBps": round(wrote["w"] / (out["w_kernel_ms"] * 1e-3) / 1e12, 3),
                "transforms_per_s_gws": float("%.4g" % (plan["frames"] * (S + out["gws_workgroups"] * max(1, 4096 // L) / plan["frames"])
                                                        / (out["gws_kernel_ms"] * 1e-3)))})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="tenths of a second per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=150, help="seconds per shape")
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
