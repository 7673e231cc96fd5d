"""The array scan of a batch of device-resident eigendecompositions: what k_beam costs beside the eigensolver and a torch composition.

One JSON line per shape (models x sensors x steering vectors; the first shape under each of the four methods, MUSIC and EV at p = 2, the
others under Capon), appended to stdout:
  call_ms        engine.beamscan (events around the call, median of --reps); spread = (max - min) / median
  kernel_ms      k_beam alone, between two events around its launch (the library's profile hooks)
  eigh_ms        engine.eigh of the same batch of matrices (check=False: no read-back), in the same run
  torch_ms       the same contraction composed from torch in complex128 on the device, abs(conj(A) @ V) ** 2 @ g, the steering matrix A
                 and the weights g given (their making is not timed)
  of_bound       the worst output of the call against that composition as a share of the derived bound of tests/beam_ref.py, over
                 --check models spread over the batch: asserted <= 1
  gfma_per_s     4 m (m - first) multiply-adds per (model, steering vector) over kernel_ms: the achieved float64 FMA rate, the sincospi
                 of the steering tile not counted
No ratio is a gate: the figures record where the time goes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(2049, 64, 1024, me) for me in ("bartlett", "capon", "music", "ev")] + [(513, 16, 256, "capon"), (129, 8, 4096, "capon")]
P = 2


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


def matrices(nb, m, seed):
    """nb Hermitian positive definite matrices of order m on the device: two plane waves whose strength varies over the batch, and noise"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(nb, m, 3 * m, generator=g, device="cuda", dtype=torch.float64) + 1j * torch.randn(nb, m, 3 * m, generator=g, device="cuda", dtype=torch.float64)
    A[:, :, :2] *= 10.0
    return A @ A.conj().transpose(1, 2) / (3 * m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--only", type=int, default=-1)
    args = ap.parse_args()
    import torch
    import beam_ref as R
    from pyfft_amd import engine as E
    for i, (nb, m, nk, method) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        rng = np.random.default_rng(7)
        pos = np.arange(m) + 0.3 * rng.uniform(-1, 1, m)
        kv = np.linspace(-0.5, 0.5, nk)
        loading = 1e-3 if method == "capon" else 0.0
        G = matrices(nb, m, 5 + m)
        eg = lambda: E.eigh(G, check=False)
        out = dict(models=nb, m=m, nk=nk, method=method, p=P, plan=E.beam_plan(m, nk, nb, method, P))
        out["eigh_ms"], out["eigh_spread"], _ = timed(eg, args.warmup, args.reps)
        w, V, _ = eg()
        E.profile_enable(True)
        call = lambda: E.beamscan(V, w, pos, kv, method, P, loading, None, True)
        out["call_ms"], out["call_spread"], out["kernel_ms"] = timed(call, args.warmup, args.reps, E.profile_last_ms)
        assert E.profile_last_kernel() == "k_beam"
        E.profile_enable(False)
        got, st = call()
        assert not bool(st.any())
        k0 = R.first_vector(method, P)
        out["gfma_per_s"] = 4.0 * m * (m - k0) * nb * nk / (out["kernel_ms"] * 1e-3) / 1e9
        # the same contraction from torch
        Ad = torch.as_tensor(R.steer_def(pos, kv), device="cuda")                                        # [nk, m]
        wh = w.cpu().numpy()
        gd = torch.as_tensor(np.stack([R.weights_def(wh[s], method, P, loading)[0] for s in range(nb)]), device="cuda")    # [nb, m - k0]
        Vn = V[:, :, k0:].contiguous()

        def composed():
            D = (torch.abs(torch.matmul(Ad.conj(), Vn)) ** 2 @ gd[:, :, None])[:, :, 0]
            return D / (m * m) if method == "bartlett" else torch.where(D > 0, 1.0 / D, torch.zeros_like(D))
        out["torch_ms"], _, _ = timed(composed, 1, 3)
        ref, gh, Vh = composed().cpu().numpy(), got.cpu().numpy(), V.cpu().numpy()
        share = 0.0
        for s in np.unique(np.linspace(0, nb - 1, args.check).astype(int)):
            share = max(share, float(np.max(np.abs(gh[s] - ref[s]) / R.beam_bound(Vh[s], wh[s], pos, kv, method, P, loading))))
        out["checked_models"], out["of_bound"] = int(min(args.check, nb)), share
        assert share <= 1.0, out
        del G, w, V, Vn, Ad, gd
        note("shape %d: %s" % (i, out))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
