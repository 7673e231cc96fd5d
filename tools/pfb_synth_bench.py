#!/usr/bin/env python3
"""The polyphase synthesis bank (sp_pfb_synth) on device-resident frame-major frames of a 2^26-sample record; one JSON line per shape
(M, P, hop, input): M = 1024 and 4096 channels, P = 4 and 8 taps per channel, hop = M / 2 and 3 M / 4, two-sided (complex record) and
one-sided (real record) frames, phase "time", the geometry of pfb_plan(center=False).
      ms, iso_ms         engine.pfb_synth on the default path: sustained (back-to-back calls between one pair of HIP events, per call);
                         median of single synchronised calls.  ms is the smaller of two sustained runs taken before and after the
                         analysis'; spread = their relative difference
      path               the path the default rule took (the library's last kernel name); groups = transform groups of a workgroup
                         that own a ring on the fused path, of fpw (engine.pfb_synth_plan: the library's own figures)
      fused_ms           SP_PFBS_PATH=fused (null where not even one ring fits the LDS)
      composed_ms        SP_PFBS_PATH=composed
      binmajor_ms        the default path on bin-major frames (what channelize returns and synthesize passes on): the transposition into
                         scratch included
      gbytes_s           (frame bytes + output bytes) / ms
      halo_cost          (fpg + halo) / fpg of the default run length on the fused path
      pfb_ms             engine.pfb producing the same frames from the record at the same shape: the same bytes the other way
      synth_over_pfb     ms / pfb_ms
Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/pfb_synth_bench.py [--reps 10] > profiles/pfb_synth_bench.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.zoom_bench import measure                                         # noqa: E402

LOG2N = 26
SHAPES = [(M, P, D, cplx) for cplx in (True, False) for M in (1024, 4096) for P in (4, 8) for D in (M // 2, 3 * M // 4)]

def one(idx, warmup, reps):
    import torch
    from pyfft_amd import engine as E, channelizer as CH
    M, P, D, cplx = SHAPES[idx]
    n = 1 << LOG2N
    gen = torch.Generator(device="cuda").manual_seed(idx)
    x = torch.randn(n, device="cuda", generator=gen) + 0.5
    if cplx:
        x = torch.complex(x, torch.randn(n, device="cuda", generator=gen))
    p = CH.pfb_plan(n, cplx, M, P, D)
    h, nf, r0 = p["h"], p["nframes"], p["r0"]
    g = CH.pfb_dual(h, M, D)[0]
    X = E.pfb(x, h, M, D, 0, nf, 1, r0)
    nout = (nf - 1) * D + M * P

    def synth():
        return E.pfb_synth(X, g, M, D, 0, nout, 1, r0, onesided=not cplx)

    def analysis():
        return E.pfb(x, h, M, D, 0, nf, 1, r0)

    synth(), analysis()
    torch.cuda.synchronize()
    E.profile_enable(True)
    synth()
    path = E.profile_last_kernel()
    E.profile_enable(False)
    a = measure(synth, warmup, reps)
    f = measure(analysis, warmup, reps)
    b = measure(synth, warmup, reps)
    ms = min(a[0], b[0])
    plan = E.pfb_synth_plan(M, M * P, D, nf, onesided=not cplx)       # the library's own default route and run length
    ag, fpw, fpg, halo = plan["groups"], plan["fpw"], plan["fpg"], plan["halo"]
    forced = {}
    for name in ("fused", "composed"):
        if name == "fused" and ag < 1:
            forced[name] = None
            continue
        os.environ["SP_PFBS_PATH"] = name
        synth()
        forced[name] = round(measure(synth, warmup, reps)[0], 4)
        del os.environ["SP_PFBS_PATH"]
    Xb = X.transpose(-1, -2).contiguous()

    def synth_binmajor():
        return E.pfb_synth(Xb, g, M, D, 0, nout, 1, r0, onesided=not cplx, in_major=1)

    synth_binmajor()
    bm = measure(synth_binmajor, warmup, reps)
    nbytes = X.numel() * 8 + nout * (8 if cplx else 4)
    print(json.dumps({"M": M, "P": P, "hop": D, "input": "two-sided" if cplx else "one-sided", "nframes": nf, "nout": nout,
                      "ms": round(ms, 4), "spread": round(abs(a[0] - b[0]) / ms, 4), "iso_ms": round(min(a[1], b[1]), 4), "path": path,
                      "groups": ag, "fpw": fpw, "fused_ms": forced["fused"], "composed_ms": forced["composed"],
                      "binmajor_ms": round(bm[0], 4), "bytes": nbytes,
                      "gbytes_s": float("%.4g" % (nbytes / (ms * 1e-3) / 1e9)), "halo_cost": round((fpg + halo) / fpg, 4),
                      "pfb_ms": round(f[0], 4), "synth_over_pfb": round(ms / f[0], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", type=int, default=-1)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
    ap.add_argument("--budget", type=int, default=0, help="seconds for the whole run: no shape is started that could overrun it (0: none)")
    args = ap.parse_args()
    if args.one >= 0:
        return one(args.one, args.warmup, args.reps)
    t0 = time.monotonic()
    for i in range(len(SHAPES)):
        if args.budget > 0 and time.monotonic() - t0 + args.limit > args.budget:
            sys.exit("out of time before shape %s: stopping" % (SHAPES[i],))
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(i), "--reps", str(args.reps), "--warmup",
                             str(args.warmup)], timeout=args.limit).returncode
        if rc != 0:
            sys.exit("shape %s failed (exit %d): stopping" % (SHAPES[i], rc))


if __name__ == "__main__":
    main()
