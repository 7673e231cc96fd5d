"""Conditioned spectral analysis of a batch of device-resident Hermitian matrices: what k_cond costs beside the eigensolver and beside the
same quantities composed from torch.linalg.

One JSON line per shape (matrices x order, the inputs half of the channels; the first shape once without and once with the precision
matrix P), appended to stdout:
  call_ms        mimo.cond (events around the call, median of --reps, check=False: no read-back); spread = (max - min) / median
  kernel_ms      k_cond alone, between two events around its launch (the library's profile hooks)
  eigh_ms        engine.eigh of the same batch (check=False), in the same run, for scale
  torch_ms       H, Gc, mcoh, piv (and P) composed from torch.linalg.cholesky and solve_triangular in complex128 on the device
  of_bound       the worst output of the call against the longdouble definition as a share of the derived bound of tests/cond_ref.py,
                 over --check matrices spread over the batch: asserted <= 1; torch_of_bound the same for the composition, asserted <= 1
No ratio is a gate: the figures record where the time goes, and whether matrices of order <= 16 would deserve a form of their own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(2049, 64, False), (2049, 64, True), (513, 16, True), (129, 8, True), (65536, 4, True)]


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


def matrices(nb, n, seed):
    """nb Hermitian positive definite matrices of order n on the device, exactly Hermitian"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(nb, n, 3 * n, generator=g, device="cuda", dtype=torch.float64) + 1j * torch.randn(nb, n, 3 * n, generator=g, device="cuda", dtype=torch.float64)
    G = A @ A.conj().transpose(1, 2) / (3 * n)
    return (G + G.conj().transpose(1, 2)) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--only", type=int, default=-1)
    args = ap.parse_args()
    import torch
    import cond_ref as R
    from pyfft_amd import engine as E, mimo as M
    for i, (nb, n, withP) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        q = n // 2
        want = R.WANT if withP else R.WANT[:4]
        G = matrices(nb, n, 5 + n)
        out = dict(matrices=nb, n=n, q=q, want="".join(w[0] for w in want), plan=M.cond_plan(n, q, nb, want))
        out["eigh_ms"], out["eigh_spread"], _ = timed(lambda: E.eigh(G, check=False), args.warmup, args.reps)
        E.profile_enable(True)
        call = lambda: M.cond(G, q, want=want, check=False)
        out["call_ms"], out["call_spread"], out["kernel_ms"] = timed(call, args.warmup, args.reps, E.profile_last_ms)
        assert E.profile_last_kernel() == "k_cond"
        E.profile_enable(False)
        res = call()
        assert not bool(res.status.any())
        eye = torch.eye(n, dtype=torch.complex128, device="cuda").expand(nb, n, n)

        def composed():
            L = torch.linalg.cholesky(G)
            Lxx, Lyx, Lyy = L[:, :q, :q], L[:, q:, :q], L[:, q:, q:]
            o = dict(H=torch.linalg.solve_triangular(Lxx, Lyx, upper=False, left=False), Gc=Lyy @ Lyy.conj().transpose(1, 2),
                     mcoh=(Lyx.real ** 2 + Lyx.imag ** 2).sum(-1) / torch.diagonal(G, dim1=1, dim2=2).real[:, q:],
                     piv=torch.diagonal(L, dim1=1, dim2=2).real ** 2)
            if withP:
                W = torch.linalg.solve_triangular(L, eye, upper=False)
                o["P"] = W.conj().transpose(1, 2) @ W
            return o
        out["torch_ms"], _, _ = timed(composed, args.warmup, args.reps)
        comp = composed()
        share = tshare = 0.0
        pick = np.unique(np.linspace(0, nb - 1, args.check).astype(int))
        Gh = G[torch.as_tensor(pick, device="cuda")].cpu().numpy()
        for j, s in enumerate(pick):
            ref = R.ref_cond(Gh[j], q)
            bd = R.bound_of(ref)
            share = max(share, max(R.share_of({k: [getattr(res, k)[s].cpu().numpy()] for k in want}, [ref], [bd], want).values()))
            tshare = max(tshare, max(R.share_of({k: [comp[k][s].cpu().numpy()] for k in want}, [ref], [bd], want).values()))
        out["checked_matrices"], out["of_bound"], out["torch_of_bound"] = int(len(pick)), share, tshare
        assert share <= 1.0 and tshare <= 1.0, out
        del G, res, comp, eye
        note("shape %d: %s" % (i, out))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
