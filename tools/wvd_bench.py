#!/usr/bin/env python3
"""The smoothed pseudo Wigner-Ville distribution (engine.wvd, k_wvd) of a device-resident complex record of 2^20 samples against two
baselines, one JSON line per shape (nfft 256 / 1024 with a Hamming lag window of nfft/2 - 1 taps, hop 1 / 16, a time window of 1 or 33
taps, the full band or 32 bins, auto or cross):
  stft_ms       engine.stft_frames of the same record at the same nfft, hop and (but for the last nfft / hop) column count, two-sided
                complex spectra: what a linear map of the same size costs
  composed_ms   the same distribution composed from what the package had: the lag products and the smoothing with torch on the device
                (in chunks of columns, so that K fits), then engine.fft of K and the band cut out.  It is asserted equal to the kernel
                within the allowance of tests/wvd_ref.py, so the two sides do equal work
  wvd_ms        engine.wvd: the median of isolated calls, *_spread = (max - min) / median over them; wvd_kernel_ms: k_wvd alone (library
                profiling events, one isolated launch)
  macs          complex multiply-adds of the products and the smoothing as the kernel forms them (auto: the lags 0 .. Lh)
  written       bytes of W; store_TBps = written / wvd_kernel_ms; valu_fraction = 8 flops per MAC / wvd_kernel_ms over the fp32 vector
                peak of the device (2 flops x 128 lanes x CUs x 2.4 GHz)
All cases run in one process in the same order: stft, kernel, composed, stft again (stft_spread is between the two).
    python tools/wvd_bench.py [--reps 5] > profiles/wvd_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOG2N = 20
CLOCK_HZ = 2.4e9                         # the MI355X's peak engine clock
SHAPES = [(nfft, hop, ng, band, cross) for nfft in (256, 1024) for hop in (1, 16) for ng in (1, 33) for band in (None, 32)
          for cross in (False, True)]


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    iso = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        iso.append(a.elapsed_time(b))
    med = float(np.median(iso))
    return med, (max(iso) - min(iso)) / med


def composed(torch, E, x, y, h, g, hop, ntimes, nfft, b0, nb, scale, chunk):
    """W [ntimes, nb] from torch products and smoothing, then engine.fft; columns n = j hop, the record zero outside itself"""
    Lh, Lg = h.numel() // 2, g.numel() // 2
    pad = Lh + Lg
    auto = y is None
    y = x if auto else y
    zp, yp = (torch.nn.functional.pad(torch.view_as_real(a), (0, 0, pad, pad + hop * chunk)) for a in (x, y))
    zp, yp = torch.view_as_complex(zp), torch.view_as_complex(yp)
    tau = (torch.arange(-Lh, Lh + 1, device=x.device) % nfft)
    out = []
    for j0 in range(0, ntimes, chunk):
        nj = min(chunk, ntimes - j0)
        m0 = j0 * hop                                        # zp index of the sample n_j0 - Lg - Lh
        M = (nj - 1) * hop + 2 * Lg + 1                      # the times m = n - Lg .. of the chunk
        A = zp[m0:m0 + M + 2 * Lh].unfold(0, 2 * Lh + 1, 1)   # [M, nh]: z[m + tau]
        B = yp[m0:m0 + M + 2 * Lh].unfold(0, 2 * Lh + 1, 1).flip(-1)   # y[m - tau]
        if Lg == 0:
            P = A[::hop] * torch.conj(B[::hop]) * g[0]
        else:
            Pm = A * torch.conj(B)                           # [M, nh]
            P = g[0] * Pm[0:(nj - 1) * hop + 1:hop]
            for mu in range(1, 2 * Lg + 1):                  # one strided pass over the products per tap
                P += g[mu] * Pm[mu:mu + (nj - 1) * hop + 1:hop]
            del Pm
        img = torch.zeros((nj, nfft), dtype=torch.complex64, device=x.device)
        img[:, tau] = P * h
        Wc = E.fft(img)
        cols = (b0 + torch.arange(nb, device=x.device)) % nfft
        Wc = Wc[:, cols] * scale
        out.append(Wc.real.contiguous() if auto else Wc)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", type=int, default=-1, help="one shape by index")
    ap.add_argument("--log2n", type=int, default=LOG2N)
    args = ap.parse_args()
    import torch
    import wvd_ref as R
    from pyfft_amd import engine as E
    nsig = 1 << args.log2n
    gen = torch.Generator(device="cuda").manual_seed(1)
    n = torch.arange(nsig, device="cuda", dtype=torch.float64)
    chirp = torch.exp(2j * np.pi * (0.02 * n + 0.09 * n * n / nsig)).to(torch.complex64)
    x = (2.0 * chirp + torch.view_as_complex(torch.randn((nsig, 2), device="cuda", generator=gen))).contiguous()
    y = (1.5 * torch.roll(chirp, 3) + torch.view_as_complex(torch.randn((nsig, 2), device="cuda", generator=gen))).contiguous()
    props = torch.cuda.get_device_properties(0)
    peak = 2.0 * 128 * props.multi_processor_count * CLOCK_HZ      # fp32 vector flops per second: 157.3e12 with 256 CUs
    for idx, (nfft, hop, ng, band, cross) in enumerate(SHAPES):
        if args.only >= 0 and idx != args.only:
            continue
        nh = nfft // 2 - 1
        h, g = R.hamming(nh), R.hamming(ng)
        h, g = (h / h[nh // 2]).astype(np.float32), (g / g.sum()).astype(np.float32)
        ntimes = (nsig - 1) // hop + 1
        b0, nb = (0, nfft) if band is None else (nfft // 8, band)
        yy = y if cross else None
        win = torch.ones(nfft, device="cuda").cpu().numpy()
        nframes = (nsig - nfft) // hop + 1

        def run_wvd():
            return E.wvd(x, h, g, hop, 0, ntimes, nfft, y=yy, b0=b0, nb=nb, scale=1.0 / nfft)

        hd, gd = torch.as_tensor(h, device="cuda"), torch.as_tensor(g, device="cuda")
        chunk = max(1, (1 << 24) // nfft // (hop if ng > 1 else 1))        # columns of a composed chunk: K and the products of a chunk stay below 1 GiB

        def run_composed():
            return composed(torch, E, x, yy, hd, gd, hop, ntimes, nfft, b0, nb, 1.0 / nfft, chunk)

        def run_stft():
            return E.stft_frames(x, win, hop, nframes, detrend=False, sided=E.SIDED_TWO)

        s1 = timed(run_stft, args.warmup, args.reps)
        tw = timed(run_wvd, args.warmup, args.reps)
        E.profile_enable(True)
        W = run_wvd()
        torch.cuda.synchronize()
        kms = E.profile_last_ms()
        E.profile_enable(False)
        tc = timed(run_composed, 1, 2)
        ref = run_composed()
        big = torch.amax(torch.abs(ref), dim=-1, keepdim=True)
        bound = R.ALLOWANCE * big + R.ABS_TERM * torch.amax(big)
        worst = float(torch.amax(torch.abs(W - ref) / bound))
        # a few columns of both against the float64 restatement, so that a difference names its side
        xh, yh = x.cpu().numpy(), (yy.cpu().numpy() if cross else None)
        bins = (b0 + np.arange(nb)) % nfft
        for j in (0, 1, ntimes // 2, ntimes // 2 + 1, ntimes - 1):
            col = R.wvd_ref(xh, h, g, hop, j * hop, 1, nfft, y=yh, scale=1.0 / nfft)[0][bins]
            col = col if cross else col.real
            for side, got in (("kernel", W[j]), ("composed", ref[j])):
                e = float(np.max(np.abs(got.cpu().numpy() - col)) / (R.ALLOWANCE * np.max(np.abs(col)) + R.ABS_TERM * float(torch.amax(big))))
                assert e <= 1.0, ("%s: column %d is off the float64 reference" % (side, j), idx, e)
        assert worst <= 1.0, ("the composed path and the kernel differ", idx, worst)
        del ref, W
        s2 = timed(run_stft, 0, args.reps)
        st = min(s1[0], s2[0])
        plan = E.wvd_plan(nfft, nh, ng, hop, ntimes, cross=cross, nb=nb)
        macs = ntimes * ng * (nh if cross else nh // 2 + 1)
        written = ntimes * nb * (8 if cross else 4)
        out = {"nsig": nsig, "nfft": nfft, "nh": nh, "ng": ng, "hop": hop, "columns": ntimes, "b0": b0, "nb": nb, "cross": cross,
               "cpr": plan["cpr"], "workgroups": plan["workgroups"], "lds_bytes": plan["lds_bytes"],
               "wvd_ms": round(tw[0], 4), "wvd_spread": round(tw[1], 3), "wvd_kernel_ms": round(kms, 4),
               "composed_ms": round(tc[0], 3), "composed_spread": round(tc[1], 3), "composed_over_wvd": round(tc[0] / tw[0], 2),
               "composed_worst_cell_of_allowance": round(worst, 3),
               "stft_ms": round(s1[0], 4), "stft2_ms": round(s2[0], 4), "stft_spread": round(abs(s1[0] - s2[0]) / st, 3),
               "stft_frames": nframes, "wvd_over_stft": round(tw[0] / st, 2),
               "macs": macs, "written": written, "store_TBps": round(written / (kms * 1e-3) / 1e12, 3),
               "valu_fraction": round(8.0 * macs / (kms * 1e-3) / peak, 3)}
        print(json.dumps(out), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
