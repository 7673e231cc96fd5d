#!/usr/bin/env python3
"""Autoregressive spectrograms (pyfft_amd.ar_spectrogram: engine.burg or engine.yule, then engine.ar_psd) of a device-resident record of
2^24 samples, one JSON line per shape: segments of n = 256 / 1024 / 4096 at half overlap, orders 16 / 64, float32 and complex64.
  call_ms      ar_spectrogram: the median of --reps isolated calls after --warmup calls, *_spread = (max - min) / median
  fit_ms       engine.burg of the same frames alone (the scan for values that are not finite and its read-back included)
  burg_ms      k_burg alone, between two events around its launch (the library's profile hooks); per_order_us = burg_ms / p: the
               latency of one order over all segments in flight, what the kernel is bound by (a chain of two wave sums, a barrier in
               the workgroup form, and the update)
  yule_ms      engine.yule of the same frames, the whole call: k_ar_scan and its read-back, k_ar_mean, k_ar_lags, k_levinson; lags_ms is
               k_ar_lags alone between the profile events (the last pass's: yule_passes says how many there were); the other kernels
               of the call are not timed alone
  psd_ms       engine.ar_psd of the fitted models (n / 2 + 1 or n bins), the whole call; psd_kernel_ms k_ar_psd alone between the events
  stft_ms      engine.stft_frames of the same frames with a rectangular window: the floor of reading the samples once and transforming
  composed     the same Burg fit composed from torch in float64 on the device (p steps of elementwise products and sums over [segments,
               n]), at the first --composed segments; composed_ms its time.  The allowance is formed as the tests form theirs
               (tests/burg_ref.py), at THIS shape: composed_restated is what the same composition with float32 state and products and
               float64 sums is off by from the float64 one (the worst of P per bin, k, a, E_m over the segments), composed_allowance
               4 x that, asserted <= 2e-4; composed_off what the kernel's models are off by and composed_of_allowance its share,
               asserted <= 1.  yule_composed_*: the same for the Yule-Walker fit (p + 1 lag products and sums, then p Levinson steps)
  form         0 the wave form of k_burg, 1 the workgroup form (SP_BURG_FORM in the environment forces one: profiles/burg_variants.txt)
Times are the calls' (host launches and read-backs included).  No counter was collected.  No figure here is a gate.
    python tools/burg_bench.py [--reps 10] > profiles/burg_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(n, p, cplx) for n in (256, 1024, 4096) for p in (16, 64) for cplx in (False, True)]


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


def burg_torch(seg, p, f32=False):
    """burg_def over the rows of seg [S, n] (float64 or complex128, detrended) -> a [S, p + 1], E [S, p + 1], k [S, p]; f32: the kernel's
    split as tests/burg_ref.py restates it (f, b and the products float32, the sums, k, a and E float64)"""
    import torch
    S, n = seg.shape
    st = {torch.float64: torch.float32, torch.complex128: torch.complex64}[seg.dtype] if f32 else seg.dtype
    f, b = seg.to(st).clone(), seg.to(st).clone()
    a = torch.zeros(S, p + 1, dtype=seg.dtype, device=seg.device)
    a[:, 0] = 1
    E = torch.zeros(S, p + 1, dtype=torch.float64, device=seg.device)
    k = torch.zeros(S, p, dtype=seg.dtype, device=seg.device)
    E[:, 0] = (seg.abs() ** 2).mean(dim=1)
    for m in range(1, p + 1):
        fm, bm = f[:, m:], b[:, m - 1:n - 1]
        num = (fm * bm.conj()).to(seg.dtype).sum(dim=1)
        den = (fm.abs() ** 2 + bm.abs() ** 2).to(torch.float64).sum(dim=1)
        km = torch.where(den > 0, -2 * num / den, torch.zeros_like(num))
        k[:, m - 1] = km
        ks = km.to(st)
        fn, bn = fm + ks[:, None] * bm, bm + ks.conj()[:, None] * fm
        f, b = f.clone(), b.clone()
        f[:, m:], b[:, m:] = fn, bn
        a[:, 1:m] = a[:, 1:m] + km[:, None] * torch.flip(a[:, 1:m].conj(), dims=(1,))
        a[:, m] = km
        E[:, m] = E[:, m - 1] * (1 - km.abs() ** 2)
    return a, E, k


def yule_torch(seg, p, f32=False):
    """yule_def over the rows of seg [S, n]: the biased lags, then Levinson-Durbin, in float64 -> a, E, k; f32: float32 samples and
    products, float64 sums"""
    import torch
    S, n = seg.shape
    v = seg.to({torch.float64: torch.float32, torch.complex128: torch.complex64}[seg.dtype]) if f32 else seg
    r = torch.stack([(v[:, l:] * v[:, :n - l].conj()).to(seg.dtype).sum(dim=1) for l in range(p + 1)], dim=1) / n
    a = torch.zeros(S, p + 1, dtype=seg.dtype, device=seg.device)
    a[:, 0] = 1
    E = torch.zeros(S, p + 1, dtype=torch.float64, device=seg.device)
    k = torch.zeros(S, p, dtype=seg.dtype, device=seg.device)
    E[:, 0] = r[:, 0].real.clamp_min(0)
    for m in range(1, p + 1):
        acc = (a[:, :m] * torch.flip(r[:, 1:m + 1], dims=(1,))).sum(dim=1)
        Em = E[:, m - 1].to(seg.dtype)
        km = torch.where(E[:, m - 1] > 0, -acc / Em, torch.zeros_like(acc))
        k[:, m - 1] = km
        a[:, 1:m] = a[:, 1:m] + km[:, None] * torch.flip(a[:, 1:m].conj(), dims=(1,))
        a[:, m] = km
        E[:, m] = (E[:, m - 1] * (1 - km.abs() ** 2)).clamp_min(0)
    return a, E, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--composed", type=int, default=1024)
    ap.add_argument("--only", type=int, default=-1)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--variants", action="store_true", help="both forms of k_burg at n = 128 .. 1024 instead: profiles/burg_variants.txt")
    args = ap.parse_args()
    import torch
    import burg_ref as R
    import pyfft_amd
    from pyfft_amd import engine as E
    N = 1 << args.log2n
    rng = np.random.default_rng(3)
    if args.variants:
        # both forms of k_burg on either side of where they meet: the kernel alone, per segment length, order and dtype
        w = rng.standard_normal(N).astype(np.float32)
        xr = np.convolve(w, [1.0, 0.9, 0.5, 0.2], mode="same").astype(np.float32)
        E.profile_enable(True)
        for cplx in (False, True):
            xd = torch.as_tensor((xr + 1j * np.roll(xr, 7)).astype(np.complex64) if cplx else xr, device="cuda")
            for n in (128, 256, 512, 1024):
                for p in (16, 64):
                    hop = n // 2
                    nframes = (N - n) // hop + 1
                    out = dict(n=n, order=p, dtype="complex64" if cplx else "float32", segments=nframes)
                    for form, key in ((1, "wave"), (2, "workgroup")):
                        os.environ["SP_BURG_FORM"] = str(form)
                        plan = E.ar_plan("burg", n, p, 1, nframes, cplx)
                        assert plan["form"] == form - 1
                        _, _, ms = timed(lambda: E.burg(xd, n, hop, 0, nframes, p), args.warmup, args.reps, E.profile_last_ms)
                        out[key + "_ms"], out[key + "_per_order_us"], out[key + "_threads"] = ms, 1e3 * ms / p, plan["threads"] // plan["segs_per_wg"]
                    del os.environ["SP_BURG_FORM"]
                    out["workgroup_over_wave"] = out["workgroup_ms"] / out["wave_ms"]
                    print(json.dumps(out), flush=True)
        return
    for i, (n, p, cplx) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        w = rng.standard_normal(N).astype(np.float32)
        x = np.convolve(w, [1.0, 0.9, 0.5, 0.2], mode="same").astype(np.float32)            # coloured noise: every |k| well below 1
        if cplx:
            x = (x + 1j * np.roll(x, 7)).astype(np.complex64) * np.exp(2j * np.pi * 0.07 * np.arange(N)).astype(np.complex64)
        xd = torch.as_tensor(x, device="cuda")
        hop = n // 2
        nframes = (N - n) // hop + 1
        m = n if cplx else n // 2 + 1
        plan = E.ar_plan("burg", n, p, 1, nframes, cplx)
        out = dict(n=n, order=p, dtype="complex64" if cplx else "float32", samples=N, segments=nframes, bins=m, form=plan["form"],
                   samples_per_lane=plan["samples"], workgroups=plan["workgroups"], lds_bytes=plan["lds_bytes"])
        call = lambda: pyfft_amd.ar_spectrogram(xd, p, n, fs=1.0)
        out["call_ms"], out["call_spread"], _ = timed(call, args.warmup, args.reps)
        E.profile_enable(True)
        fit = lambda: E.burg(xd, n, hop, 0, nframes, p)
        out["fit_ms"], out["fit_spread"], out["burg_ms"] = timed(fit, args.warmup, args.reps, E.profile_last_ms)
        assert E.profile_last_kernel() == "k_burg"
        out["per_order_us"] = 1e3 * out["burg_ms"] / p
        yl = lambda: E.yule(xd, n, hop, 0, nframes, p)
        out["yule_ms"], out["yule_spread"], out["lags_ms"] = timed(yl, args.warmup, args.reps, E.profile_last_ms)
        out["yule_passes"] = E.last_passes(E.AR_PASSES)                  # lags_ms is the last pass's kernel: the whole of it at one pass
        a, e, k = fit()
        ev = e[..., -1].contiguous()
        psd = lambda: E.ar_psd(a, ev, m, 0.0, 1.0 / n)
        out["psd_ms"], out["psd_spread"], out["psd_kernel_ms"] = timed(psd, args.warmup, args.reps, E.profile_last_ms)
        assert E.profile_last_kernel() == "k_ar_psd"
        E.profile_enable(False)
        if not args.no_baselines:
            win = np.ones(n, dtype=np.float32)
            st = lambda: E.stft_frames(xd, win, hop, nframes, detrend=3)
            out["stft_ms"], out["stft_spread"], _ = timed(st, args.warmup, args.reps)
            S = min(args.composed, nframes)
            idx = (torch.arange(S, device="cuda") * hop)[:, None] + torch.arange(n, device="cuda")[None, :]
            seg = xd[idx].to(torch.complex128 if cplx else torch.float64)
            seg = seg - seg.mean(dim=1, keepdim=True)
            comp = lambda: burg_torch(seg, p)
            out["composed_segments"] = S
            out["composed_ms"], _, _ = timed(comp, 1, 3)
            compy = lambda: yule_torch(seg, p)
            out["yule_composed_ms"], _, _ = timed(compy, 1, 3)
            host = lambda vs: tuple(v[:S].cpu().numpy()[None] for v in vs)
            for key, fn, got in (("composed", burg_torch, (a, e, k)), ("yule_composed", yule_torch, yl())):
                ref = host(fn(seg, p))
                restated = max(R.deviations(host(fn(seg, p, True)), ref))
                out[key + "_restated"] = restated
                out[key + "_allowance"] = R.MARGIN * restated
                out[key + "_off"] = max(R.deviations(host(got), ref))
                out[key + "_of_allowance"] = out[key + "_off"] / out[key + "_allowance"]
                assert out[key + "_allowance"] <= R.PARITY and out[key + "_of_allowance"] <= 1.0, out
        note("shape %d: %s" % (i, out))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
