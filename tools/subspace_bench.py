"""Subspace spectrograms of a long device-resident record: where the time of covmat -> eigh -> pseudospectrum goes.

One JSON line per shape (segments of n = 256 / 1024 at half overlap, matrix orders m = 16 / 32 / 64, forward-backward, float32 samples,
signal dimension 4, n // 2 + 1 bins):
  call_ms      pyfft_amd.subspace_spectrogram of the whole record (events around the call, median of --reps)
  covmat_ms    engine.covmat alone; cov_row_ms: k_cov_row alone, between two events around its launch (the library's profile hooks; the
               last pass's where there are several: covmat_passes)
  eigh_ms      engine.eigh of those matrices alone (check=False: no read-back)
  pseudo_ms    engine.pseudospectrum of those eigendecompositions; pseudo_kernel_ms: k_pseudo alone
  ls_ms        engine.ar_ls (the modified covariance fit of order m - 1) of the same segments: covmat into scratch and k_ls_chol
  composed_ms  the same matrices of --composed segments from torch in float64 (unfold, one batched matmul, the fold), and
               composed_of_bound: the worst element of the call's matrices against them as a share of the derived bound of
               tests/subspace_ref.py (4 (n + 2 m) 2^-53 of the mean power, plus the mean's own rounding): asserted <= 1
No ratio is a gate: the figures record where the time goes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(n, m) for n in (256, 1024) for m in (16, 32, 64)]


def timed(fn, warmup, reps, after=None):
    import torch
    for _ in range(warmup):
        fn()
    iso, extra = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        iso.append(a.elapsed_time(b))
        if after:
            extra.append(after())
    med = float(np.median(iso))
    return med, (max(iso) - min(iso)) / med, (float(np.median(extra)) if extra else None)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def covmat_torch(seg, m, fb):
    """C [S, m, m] complex128 of the detrended segments seg [S, n] float64: the snapshots by unfold, X'X / N in one batched matmul"""
    import torch
    X = torch.flip(seg.unfold(1, m, 1), dims=(2,)).to(torch.complex128)          # X[s, t, j] = seg[s, t + m - 1 - j]
    C = torch.matmul(X.conj().transpose(1, 2), X) / X.shape[1]
    if fb:
        C = 0.5 * (C + torch.flip(C, dims=(1, 2)).conj())
    return C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--composed", type=int, default=1024)
    ap.add_argument("--only", type=int, default=-1)
    args = ap.parse_args()
    import torch
    import subspace_ref as R
    import pyfft_amd
    from pyfft_amd import engine as E
    N = 1 << args.log2n
    rng = np.random.default_rng(3)
    t = np.arange(N)
    x = (np.cos(2 * np.pi * 0.11 * t) + 0.5 * np.cos(2 * np.pi * 0.123 * t + 1.0) + 0.2 * rng.standard_normal(N) + 0.3).astype(np.float32)
    xd = torch.as_tensor(x, device="cuda")
    p = 4
    for i, (n, m) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        hop = n // 2
        nframes = (N - n) // hop + 1
        bins = n // 2 + 1
        plan = E.sub_plan("covmat", n, m, 1, nframes)
        out = dict(n=n, m=m, p=p, dtype="float32", samples=N, segments=nframes, bins=bins, tiles=plan["tiles"], workgroups=plan["workgroups"],
                   lds_bytes=plan["lds_bytes"])
        call = lambda: pyfft_amd.subspace_spectrogram(xd, p, n, m=m, nfft=n)
        out["call_ms"], out["call_spread"], _ = timed(call, args.warmup, args.reps)
        E.profile_enable(True)
        cm = lambda: E.covmat(xd, n, hop, 0, nframes, m)
        out["covmat_ms"], out["covmat_spread"], out["cov_row_ms"] = timed(cm, args.warmup, args.reps, E.profile_last_ms)
        assert E.profile_last_kernel() == "k_cov_row"
        out["covmat_passes"] = E.last_passes(E.SUB_PASSES)
        C = cm()
        E.profile_enable(False)
        eg = lambda: E.eigh(C, check=False)
        out["eigh_ms"], out["eigh_spread"], _ = timed(eg, args.warmup, args.reps)
        w, V, _ = eg()
        E.profile_enable(True)
        ps = lambda: E.pseudospectrum(V, w, p, bins, 0.0, 1.0 / n)
        out["pseudo_ms"], out["pseudo_spread"], out["pseudo_kernel_ms"] = timed(ps, args.warmup, args.reps, E.profile_last_ms)
        assert E.profile_last_kernel() == "k_pseudo"
        E.profile_enable(False)
        ls = lambda: E.ar_ls(xd, n, hop, 0, nframes, m - 1, fb=True, check=False)
        out["ls_ms"], out["ls_spread"], _ = timed(ls, args.warmup, args.reps)
        out["ls_passes"] = E.last_passes(E.SUB_PASSES)
        S = min(args.composed, nframes)
        idx = (torch.arange(S, device="cuda") * hop)[:, None] + torch.arange(n, device="cuda")[None, :]
        raw = xd[idx].to(torch.float64)
        seg = raw - raw.mean(dim=1, keepdim=True)
        comp = lambda: covmat_torch(seg, m, True)
        out["composed_segments"] = S
        out["composed_ms"], _, _ = timed(comp, 1, 3)
        ref, got, segh, rawh = comp().cpu().numpy(), C[:S].cpu().numpy(), seg.cpu().numpy(), raw.cpu().numpy()
        share = max(float(np.max(np.abs(got[s] - ref[s]))) / R.covmat_bound(segh[s], m, R.mean_rounding(rawh[s])) for s in range(S))
        out["composed_of_bound"] = share
        assert share <= 1.0, out
        del C, w, V
        note("shape %d: %s" % (i, out))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
