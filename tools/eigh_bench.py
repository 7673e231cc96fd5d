#!/usr/bin/env python3
"""The batched Hermitian eigensolver (sp_eigh) on device-resident random CSD matrices of 4n frames, one JSON line per shape:
batch 2049 x n 64 (the cfg5 matrix at nfft 4096) with all vectors and with none, 513 x 16, 129 x 8.
  eigh_ms, eigh_iso_ms   engine.eigh(check=False), sustained (back-to-back calls between one pair of HIP events) and isolated
  eigh_kernel_ms         k_eigh alone (library profiling events)
  sweeps_max, _mean      Jacobi sweeps used over the batch
  resid_tol, orth_tol    the worst residual and orthogonality over the batch in units of tol(n) = 4 n 30 eps (with vectors)
  numpy_host_ms          numpy.linalg.eigh (eigvalsh without vectors) over the same batch on the host, plus copy_ms, the device-to-host
                         copy of the matrices: how these numbers were had before sp_eigh
  torch_ms / torch_error torch.linalg.eigh (eigvalsh) on the device if it runs there, else the text of its exception
  plan                   sp_eigh_plan: padded order, LDS bytes, workgroups per CU, grid
No ratio is asserted.  Every shape runs in a process of its own under a time limit; the first failure ends the run.
    python tools/eigh_bench.py [--reps 10] > profiles/eigh_bench.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.zoom_bench import measure                      # noqa: E402

# (batch, n, vectors)
SHAPES = [(2049, 64, True), (2049, 64, False), (513, 16, True), (129, 8, True)]


def one(idx, warmup, reps):
    import numpy as np
    import torch
    from pyfft_amd import engine as E
    from pyfft_amd.spod import spod_plan
    import eigh_ref as R
    batch, n, vec = SHAPES[idx]
    g = torch.Generator(device="cuda").manual_seed(idx)
    X = torch.randn((batch, n, 4 * n, 2), device="cuda", dtype=torch.float64, generator=g)
    X = torch.view_as_complex(X)
    A = (X @ X.conj().transpose(1, 2) / (4 * n)).contiguous()
    del X
    nvec = n if vec else 0

    def run():
        return E.eigh(A, nvec=nvec, check=False)

    w, V, sw = run()
    torch.cuda.synchronize()
    sweeps = sw.cpu().numpy()
    out = {"batch": batch, "n": n, "nvec": nvec, "plan": spod_plan(n, nvec, batch), "sweeps_max": int(sweeps.max()),
           "sweeps_mean": round(float(sweeps.mean()), 2)}
    t0 = time.perf_counter()
    Ah = A.cpu().numpy()
    out["copy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    if vec:
        L = R.limits(Ah, w.cpu().numpy(), V.cpu().numpy(), sweeps)
        out["resid_tol"], out["orth_tol"] = round(L["resid"] / R.tol(n), 4), round(L["orth"] / R.tol(n), 4)
    else:
        ref = np.linalg.eigvalsh(Ah)[:, ::-1]
        out["eig_tol"] = round(float(np.max(np.abs(w.cpu().numpy() - ref) / np.abs(ref).max(axis=1, keepdims=True))) / R.tol(n), 4)
    t = measure(run, warmup, reps)
    E.profile_enable(True)
    run()
    k = E.profile_last_ms()
    E.profile_enable(False)
    out.update(eigh_ms=round(t[0], 4), eigh_iso_ms=round(t[1], 4), eigh_kernel_ms=round(k, 4))
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        np.linalg.eigh(Ah) if vec else np.linalg.eigvalsh(Ah)
        host.append((time.perf_counter() - t0) * 1e3)
    out["numpy_host_ms"] = round(min(host), 3)
    print(json.dumps(out), file=sys.stderr, flush=True)       # kept should torch's solver not come back within the limit
    try:
        fn = (lambda: torch.linalg.eigh(A)) if vec else (lambda: torch.linalg.eigvalsh(A))
        fn()
        torch.cuda.synchronize()
        out["torch_ms"] = round(measure(fn, 1, 3)[0], 4)
    except Exception as ex:                                  # no device eigensolver in this build of torch: say so
        out["torch_error"] = ("%s: %s" % (type(ex).__name__, ex))[:300]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
