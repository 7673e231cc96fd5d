#!/usr/bin/env python3
"""The synchrosqueezed STFT (engine.ssq, k_ssq) of device-resident real records against the plain STFT of the same frames
(engine.stft_frames) at the same nperseg and hop.  One JSON line per shape and record; every shape is timed on a noise-like record,
on a clean tone at the same threshold (rel = 1e-3, which leaves a tone a handful of used cells per frame) and on that tone at rel = 0
("tone0"): every cell of the frame is used and nearly all of them add to one address of the LDS accumulator, the contention case.
  T_ms, P_ms        engine.ssq with T alone, with P alone (sustained: back-to-back calls between one pair of HIP events; *_iso_ms: the
                    median of isolated calls); *_kernel_ms: k_ssq alone (library profiling events, one isolated launch)
  modes_ms          engine.ssq_bands, two bands, without forming T
  stft_ms           engine.stft_frames (one-sided complex spectra) of the same frames
  *_over_stft       the time over stft_ms times the transforms per frame ssq_plan reports (1 for a real record's T, P or modes)
  written           bytes of the output; T_store_TBps = written / T_kernel_ms
Every case runs in a process of its own under a time limit; the first failure ends the run.
    python tools/ssq_bench.py [--reps 3] > profiles/ssq_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                      # noqa: E402

# (log2 nsig, nperseg, hop, bins of the band or None for all)
SHAPES = [(20, 256, 1, None), (20, 256, 1, 32), (20, 1024, 1, None), (20, 1024, 1, 32), (24, 4096, 1024, None)]
RECORDS = ("noise", "tone", "tone0")


def one(idx, warmup, reps):
    import numpy as np
    import torch
    from pyfft_amd import engine as E, reassign as RA
    log2n, n, hop, band = SHAPES[idx // len(RECORDS)]
    kind = RECORDS[idx % len(RECORDS)]
    nsig = 1 << log2n
    nframes = (nsig - n) // hop + 1
    f_tone = 0.2 + 0.25 / n                                   # between two bins
    b0 = 0 if band is None else int(f_tone * n) - band // 2
    nb = n // 2 + 1 if band is None else band
    g = torch.Generator(device="cuda").manual_seed(idx)
    if kind == "noise":
        x = torch.randn(nsig, device="cuda", generator=g)
    else:
        x = torch.cos(2 * np.pi * f_tone * torch.arange(nsig, device="cuda", dtype=torch.float64)).float()
    h, dh, _ = RA.reassignment_windows("hann", n)
    edges = np.array([[b0 + 0.25 * nb, b0 + 0.5 * nb], [b0 + 0.5 * nb, b0 + 0.75 * nb]])
    rel = 0.0 if kind == "tone0" else 1e-3

    def timed(fn):
        """windows of about `reps` tenths of a second: the repetitions follow from a first estimate"""
        est = measure(fn, warmup, 2)[0]
        r = int(min(max(100.0 * reps / max(est, 1e-3), 3), 2000))
        return measure(fn, 1, r) + (r,)

    def kernel_ms(fn):
        E.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        k = E.profile_last_ms()
        E.profile_enable(False)
        return k

    def run_T():
        return E.ssq(x, h, dh, hop, 0, nframes, b0=b0, nb=nb, rel=rel)[0]

    def run_P():
        return E.ssq(x, h, dh, hop, 0, nframes, b0=b0, nb=nb, T=False, P=True, rel=rel)[1]

    def run_modes():
        return E.ssq_bands(x, h, dh, hop, 0, nframes, edges, rel=rel)

    def run_stft():
        return E.stft_frames(x, h, hop, nframes, detrend=False)

    s1 = timed(run_stft)
    tT, tP, tM = timed(run_T), timed(run_P), timed(run_modes)
    kT, kP, kM = kernel_ms(run_T), kernel_ms(run_P), kernel_ms(run_modes)
    s2 = timed(run_stft)
    st = min(s1[0], s2[0])
    plan = E.ssq_plan(n, nframes, nb=nb)
    assert plan["fits"] and plan["transforms"] == 1
    out = {"dtype": "float32", "record": kind, "nsig": nsig, "nperseg": n, "hop": hop, "frames": nframes, "b0": b0, "nb": nb, "rel": rel,
           "fpr": plan["fpr"], "workgroups": plan["workgroups"], "lds_bytes": plan["lds_bytes"], "transforms": plan["transforms"],
           "lds_bytes_P": E.ssq_plan(n, nframes, nb=nb, T=False, P=True)["lds_bytes"],
           "T_ms": round(tT[0], 4), "T_iso_ms": round(tT[1], 4), "T_calls": tT[2], "T_kernel_ms": round(kT, 4),
           "P_ms": round(tP[0], 4), "P_iso_ms": round(tP[1], 4), "P_kernel_ms": round(kP, 4),
           "modes_ms": round(tM[0], 4), "modes_iso_ms": round(tM[1], 4), "modes_kernel_ms": round(kM, 4),
           "stft_ms": round(s1[0], 4), "stft2_ms": round(s2[0], 4), "stft_spread": round(abs(s1[0] - s2[0]) / st, 4), "stft_calls": s1[2],
           "T_over_stft": round(tT[0] / (st * plan["transforms"]), 3), "P_over_stft": round(tP[0] / (st * plan["transforms"]), 3),
           "modes_over_stft": round(tM[0] / (st * plan["transforms"]), 3),
           "written": 8 * nframes * nb, "T_store_TBps": round(8 * nframes * nb / (kT * 1e-3) / 1e12, 3),
           "transformed_samples_per_s": float("%.4g" % (nframes * n / (kT * 1e-3)))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="tenths of a second per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=120, help="seconds per case")
    args = ap.parse_args()
    if args.one >= 0:
        return one(args.one, args.warmup, args.reps)
    for i in range(len(SHAPES) * len(RECORDS)):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(i), "--reps", str(args.reps), "--warmup",
                             str(args.warmup)], timeout=args.limit).returncode
        if rc != 0:
            sys.exit("case %d (%s, %s) failed (exit %d): stopping" % (i, SHAPES[i // len(RECORDS)], RECORDS[i % len(RECORDS)], rc))


if __name__ == "__main__":
    main()
