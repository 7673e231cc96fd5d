"""The discrete wavelet transforms on device-resident data: one JSON line per shape.

Shapes: 2^14 rows x 1024 samples, db4, full depth (7 levels), 'periodization' and 'symmetric', float32, and 'periodization' complex64
(the row form: one launch); one record of 2^26 samples, db4, 8 levels, 'symmetric' (the tile form); the MODWT of 2^22 samples, 10 levels.
Per shape:
  fwd_ms / inv_ms    engine.dwt / idwt (modwt / imodwt) between two events, median of --reps, and their spread
  floor_ms           the bytes the transform must move (the rows read once, every coefficient written once: 2 n elements; MODWT:
                     (levels + 2) n) at the 6.0 TB/s this part streams; fwd_of_floor = floor_ms / fwd_ms
  composed_ms        the same coefficients from what the library had before: per level a device-padded copy (one gather through the
                     mode's index map) and engine.upfirdn(h, xe, 1, 2) per filter (MODWT: the dilated filter at 1 / 1), in the same run;
                     ratio = composed_ms / fwd_ms
  share_ours / share_composed   both results against the float64 reference of tests/dwt_ref.py as the worst share of its running bound,
                     on rows (or a window of the record) the reference can afford: asserted <= 1
No ratio is a gate."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM = 6.0e12


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


def share(got, ref, bound, tiny):
    return float(np.max(np.abs(got.astype(ref.dtype) - ref) / (bound + tiny)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=-1)
    ap.add_argument("--log2rows", type=int, default=14)
    ap.add_argument("--log2long", type=int, default=26)
    ap.add_argument("--log2modwt", type=int, default=22)
    args = ap.parse_args()
    import torch
    import dwt_ref as R
    from pyfft_amd import engine as E, _dwt_mod as D
    dl, dh, rl, rh = D.wavelet_filters("db4")
    L = 8
    rng = np.random.default_rng(5)
    case = 0

    def emit(out):
        print(json.dumps(out), flush=True)

    def pad_index(n, mode, dev):
        """the gather that extends a level of n samples so that upfirdn(h, xe, 1, 2) from m0 on gives its coefficients -> (idx, m0, zero mask)"""
        c = L // 2 if mode == "periodization" else 1
        P = L - 1 if (c + L - 1) % 2 == 0 else L
        K = R.coeff_len(n, L, mode)
        idx = R.ext_index(np.arange(-P, 2 * K + c), n, mode)
        return torch.as_tensor(np.maximum(idx, 0), device=dev), (c + P) // 2, K

    def composed_dwt(x, mode, levels):
        """[cA_J | cD_J | .. | cD_1] from gathers and upfirdn calls"""
        parts, a = [], x
        for _ in range(levels):
            idx, m0, K = pads[int(a.shape[-1])]
            xe = a[..., idx]
            parts.insert(0, E.upfirdn(xe, dh, 1, 2, m0, K))
            a = E.upfirdn(xe, dl, 1, 2, m0, K)
        return torch.cat([a] + parts, dim=-1)

    # ---- many short rows: the row form ----
    rows, n = 1 << args.log2rows, 1024
    levels = D.dwt_max_level(n, L)
    for mode, cplx in (("periodization", False), ("symmetric", False), ("periodization", True)):
        case += 1
        if args.only >= 0 and args.only != case - 1:
            continue
        x = rng.standard_normal((rows, n)).astype(np.float32)
        if cplx:
            x = (x + 1j * rng.standard_normal((rows, n))).astype(np.complex64)
        xd = torch.as_tensor(x, device="cuda")
        el = 8 if cplx else 4
        plan = E.dwt_plan("dwt", n, L, mode, levels, rows, cplx)
        lens = E.dwt_layout(n, L, mode, levels)[0]
        pads = {m: pad_index(m, mode, "cuda") for m in lens[:-1]}
        out = dict(shape="rows", rows=rows, n=n, wavelet="db4", levels=levels, mode=mode, dtype="complex64" if cplx else "float32", form=plan["form"],
                   lds_bytes=plan["lds_bytes"], workgroups=plan["workgroups"], launches=plan["launches"])
        out["fwd_ms"], out["fwd_spread"] = timed(lambda: E.dwt(xd, dl, dh, mode, levels), args.warmup, args.reps)
        c = E.dwt(xd, dl, dh, mode, levels)
        out["inv_ms"], out["inv_spread"] = timed(lambda: E.idwt(c, n, rl, rh, mode, levels), args.warmup, args.reps)
        out["tile_form_ms"], _ = timed(lambda: E.dwt(xd, dl, dh, mode, levels, "tile"), args.warmup, args.reps)
        out["composed_ms"], out["composed_spread"] = timed(lambda: composed_dwt(xd, mode, levels), 1, 3)
        out["floor_ms"] = 1e3 * (rows * (n + c.shape[-1]) * el) / STREAM
        out["fwd_of_floor"], out["ratio"] = out["floor_ms"] / out["fwd_ms"], out["composed_ms"] / out["fwd_ms"]
        k = 64
        ref, b = R.wavedec(x[:k].astype(np.complex128 if cplx else np.float64), dl, dh, mode, levels, B=0.0)
        ref, b = np.concatenate(ref, axis=-1), np.concatenate(b, axis=-1)
        out["share_ours"] = share(c[:k].cpu().numpy(), ref, b, R.TINY)
        out["share_composed"] = share(composed_dwt(xd, mode, levels)[:k].cpu().numpy(), ref, b, R.TINY)
        back, bb = R.waverec([c[:k].cpu().numpy()[..., o:o + ln].astype(ref.dtype) for ln, o in plan["entries"]], n, rl, rh, mode, bounds=[np.zeros(1)] * (levels + 1))
        out["share_inverse"] = share(E.idwt(c, n, rl, rh, mode, levels)[:k].cpu().numpy(), back, bb, R.TINY)
        assert max(out["share_ours"], out["share_composed"], out["share_inverse"]) <= 1.0, out
        emit(out)
        del xd, c

    # ---- one long record: the tile form ----
    case += 1
    if args.only < 0 or args.only == case - 1:
        n, levels, mode = 1 << args.log2long, 8, "symmetric"
        x = rng.standard_normal(n).astype(np.float32)
        xd = torch.as_tensor(x, device="cuda")
        plan = E.dwt_plan("dwt", n, L, mode, levels, 1)
        lens = E.dwt_layout(n, L, mode, levels)[0]
        pads = {m: pad_index(m, mode, "cuda") for m in lens[:-1]}
        out = dict(shape="long", rows=1, n=n, wavelet="db4", levels=levels, mode=mode, dtype="float32", form=plan["form"], lds_bytes=plan["lds_bytes"],
                   workgroups=plan["workgroups"], launches=plan["launches"], scratch_bytes=plan["scratch_bytes"])
        out["fwd_ms"], out["fwd_spread"] = timed(lambda: E.dwt(xd, dl, dh, mode, levels), args.warmup, args.reps)
        c = E.dwt(xd, dl, dh, mode, levels)
        out["inv_ms"], out["inv_spread"] = timed(lambda: E.idwt(c, n, rl, rh, mode, levels), args.warmup, args.reps)
        out["composed_ms"], out["composed_spread"] = timed(lambda: composed_dwt(xd, mode, levels), 1, 3)
        out["floor_ms"] = 1e3 * ((n + c.shape[-1]) * 4) / STREAM
        out["moved_ms"] = 1e3 * (sum(lens[j - 1] + 2 * lens[j] for j in range(1, levels + 1)) * 4) / STREAM      # what a launch per level moves
        out["fwd_of_floor"], out["fwd_of_moved"], out["ratio"] = out["floor_ms"] / out["fwd_ms"], out["moved_ms"] / out["fwd_ms"], out["composed_ms"] / out["fwd_ms"]
        win = min(n, (1 << 18) + (1 << 12))                                  # the left end of the record: level j's first 2^18 / 2^j coefficients see no more of it
        ref, b = R.wavedec(x[None, :win].astype(np.float64), dl, dh, mode, levels, B=0.0)
        comp = composed_dwt(xd, mode, levels)
        so = sc = 0.0
        for e, (ln, o) in enumerate(plan["entries"]):
            j = levels if e == 0 else levels - e + 1
            keep = min(ln, (1 << 18) >> j) if win < n else ln
            so = max(so, share(c[o:o + keep].cpu().numpy()[None], ref[e][:, :keep], b[e][:, :keep], R.TINY))
            sc = max(sc, share(comp[o:o + keep].cpu().numpy()[None], ref[e][:, :keep], b[e][:, :keep], R.TINY))
        out["share_ours"], out["share_composed"] = so, sc
        assert max(so, sc) <= 1.0, out
        assert float(torch.max(torch.abs(E.idwt(c, n, rl, rh, mode, levels) - xd))) <= 1e-4
        emit(out)
        del xd, c, comp

    # ---- the MODWT ----
    case += 1
    if args.only < 0 or args.only == case - 1:
        n, levels = 1 << args.log2modwt, 10
        x = rng.standard_normal(n).astype(np.float32)
        xd = torch.as_tensor(x, device="cuda")
        plan = E.dwt_plan("modwt", n, L, None, levels, 1)
        g, h = R.modwt_filters(rl, rh)
        dil, idxs = [], []
        for j in range(1, levels + 1):
            s = 1 << (j - 1)
            gd, hd = np.zeros((L - 1) * s + 1), np.zeros((L - 1) * s + 1)
            gd[::s], hd[::s] = g, h
            dil.append((gd, hd))
            idxs.append(torch.as_tensor(np.mod(np.arange(-(L - 1) * s, n), n), device="cuda"))

        def composed_modwt():
            a, planes = xd, []
            for j in range(levels):
                xe = a[idxs[j]]
                m0 = (L - 1) << j
                planes.append(E.upfirdn(xe, dil[j][1], 1, 1, m0, n))
                a = E.upfirdn(xe, dil[j][0], 1, 1, m0, n)
            return torch.stack(planes + [a])
        out = dict(shape="modwt", rows=1, n=n, wavelet="db4", levels=levels, dtype="float32", form=plan["form"], workgroups=plan["workgroups"], launches=plan["launches"],
                   scratch_bytes=plan["scratch_bytes"])
        out["fwd_ms"], out["fwd_spread"] = timed(lambda: E.modwt(xd, rl, rh, levels), args.warmup, args.reps)
        W = E.modwt(xd, rl, rh, levels)
        out["inv_ms"], out["inv_spread"] = timed(lambda: E.imodwt(W, rl, rh), args.warmup, args.reps)
        out["composed_ms"], out["composed_spread"] = timed(composed_modwt, 1, 3)
        out["floor_ms"] = 1e3 * ((levels + 2) * n * 4) / STREAM
        out["moved_ms"] = 1e3 * (3 * levels * n * 4) / STREAM
        out["fwd_of_floor"], out["fwd_of_moved"], out["ratio"] = out["floor_ms"] / out["fwd_ms"], out["moved_ms"] / out["fwd_ms"], out["composed_ms"] / out["fwd_ms"]
        lo_t, hi_t, skip = n // 2 - 8192, n // 2 + (1 << 16), ((1 << levels) - 1) * (L - 1)     # a window in the middle: past `skip` samples its circular ends are not seen
        ref, b = R.modwt(x[None, lo_t:hi_t].astype(np.float64), rl, rh, levels, B=0.0)
        comp = composed_modwt()
        out["share_ours"] = share(W[:, lo_t + skip:hi_t].cpu().numpy()[:, None], ref[..., skip:], b[..., skip:], R.TINY)
        out["share_composed"] = share(comp[:, lo_t + skip:hi_t].cpu().numpy()[:, None], ref[..., skip:], b[..., skip:], R.TINY)
        assert max(out["share_ours"], out["share_composed"]) <= 1.0, out
        assert float(torch.max(torch.abs(E.imodwt(W, rl, rh) - xd))) <= 1e-4
        emit(out)


if __name__ == "__main__":
    main()
