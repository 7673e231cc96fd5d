"""The synchrosqueezed STFT and the reassignment fields on the GPU (k_ssq, k_ssq_sum, sp_ssq / sp_ssq_bands / sp_ssq_sum, engine.ssq /
ssq_bands / ssq_sum, pyfft_amd.reassign) against the float64 reference of tests/ssq_ref.py.

The cases are ssq_ref.CASES: n = 32 (128 transform groups per workgroup), 256, 2048, 4096 (one group per workgroup) and 8192 (real
records only), hops 1, 37 and n / 4, first = 0 and -n / 2, 37 frames, real and complex records, the full band and a band that drops
targets; a three-row batch with x_ld > nsig.  The threshold is ssq_ref.REL of the frame's largest cell.

Tolerances.  Per cell of T and P:  |got - ref| <= 2e-4 |ref| + 1e-6 (the frame's largest cell) + the sum of |Xc| (of |X_h|^2 for P)
over the unsure coefficients that may enter or leave the cell; 2e-4 and 1e-6 are the project's float32 figures of
test_gpu_kernels.py.  Cells that no sure or unsure coefficient reaches are exactly 0.  The frame sums are held to 2e-4 of themselves
and 1e-6 of the frame's largest cell; added to that is only what can enter or leave a frame's sum (ssq_ref.squeeze's `edge`): a
coefficient within DELTA_T of the threshold, and an unsure coefficient of whose candidate targets some are kept and some dropped (the
band's ends; bins 0 and n / 2 of a real record).  An unsure coefficient that moves between two kept bins does not count; over the
table one frame of one case has such an allowance.  IF and GD are checked at the sure used cells with the reference's own allowance
KAPPA d1 (d1 with th in place of dh for GD); NaN exactly where the reference has NaN, except at unsure threshold cells.

Measured on an MI355X over the table: cells without an unsure coefficient within 0.8e-7 .. 3.8e-6 of the frame's largest cell, frame
sums within 1.1e-7 .. 4.9e-6, IF at 0.02 .. 0.20 and GD at 0.004 .. 0.06 of their allowance, the band sums within 2.2e-7 .. 6.2e-7 of
the frame's largest cell (3.9e-3 where an unsure coefficient sits on an edge, inside its slack), issq_stft(ssq_stft(x)) - x at
2.1e-5 (real) and 1.4e-7 (complex) of max |x|, ssq_extract against the same bands of Tx at 2.4e-7 of the mode's modulus."""
import functools
import math

import numpy as np
import pytest

import ssq_ref as R
from pyfft_amd import _ffi, engine as E, reassign as RA

pytestmark = pytest.mark.gpu
IDS = [R.case_id(c) for c in R.CASES]


@pytest.fixture(scope="module")
def torch():
    import torch
    _ffi.init()
    return torch


@functools.lru_cache(maxsize=None)
def case_of(i):
    """-> (case, x, (h, dh, th), cells, squeeze): computed once and shared, read-only"""
    cs = R.CASES[i]
    x = R.make_signal(cs)
    w = R.hann_windows(cs["n"])
    c = R.cells(x, *w, cs["hop"], cs["first"], R.NFRAMES, rel=R.REL)
    b0, nb = cs["band"] if cs["band"] else (0, None)
    sq = R.squeeze(c, b0, nb)
    for v in (c["khat"], sq["T"], sq["P"]):
        v.setflags(write=False)
    return cs, x, w, c, sq


def run(cs, x, w, **kw):
    b0, nb = cs["band"] if cs["band"] else (0, None)
    return E.ssq(x, w[0], w[1], cs["hop"], cs["first"], R.NFRAMES, b0=b0, nb=nb, rel=R.REL, **kw)


def check_cells(got, ref, slack, reach, what):
    big = np.maximum(np.max(np.abs(ref), axis=1, keepdims=True), 1e-300)
    err = np.abs(got.astype(ref.dtype) - ref)
    tol = 2e-4 * np.abs(ref) + 1e-6 * big + slack
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print("%s: worst cell at %.3g of its allowance; largest error without a slack %.3g of the frame's largest"
          % (what, worst, float(np.max(np.where(slack == 0, err, 0) / big))))
    assert np.all(err <= tol), what
    assert np.all(got[reach == 0] == 0), what + ": a cell nothing reaches is not exactly 0"


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_squeeze_against_reference(torch, i):
    cs, x, w, c, sq = case_of(i)
    T = run(cs, x, w)[0]
    P = run(cs, x, w, T=False, P=True)[1]
    assert T.dtype == np.complex64 and P.dtype == np.float32 and T.shape == P.shape == sq["T"].shape
    assert R.unsure_share(c, sq) <= 0.02
    check_cells(T, sq["T"], sq["slackT"], sq["reach"], "T")
    check_cells(P, sq["P"], sq["slackP"], sq["reach"], "P")
    # the frame sums do not depend on where anything lands; only a coefficient at the threshold, or an unsure one of whose candidate
    # targets some are kept and some dropped (the band's ends; 0 and n / 2 of a real record), may enter or leave them
    edge = sq["edge"]
    big = np.maximum(np.max(np.abs(sq["T"]), axis=1), 1e-300)
    want = sq["T"].sum(axis=1)
    err = np.abs(T.astype(np.complex128).sum(axis=1) - want)
    print("frame sums: %.3g of the largest cell" % float(np.max(err / big)))
    assert np.all(err <= 2e-4 * np.abs(want) + 1e-6 * big + edge)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_fields_against_reference(torch, i):
    cs, x, w, c, sq = case_of(i)
    _, _, IF, GD = run(cs, x, w, T=False, IF=True, GD=True, th=w[2])
    n, b0, nb = cs["n"], sq["b0"], sq["nb"]
    src = (b0 + np.arange(nb)) % n
    assert src.max() < c["nsrc"]
    sure, unsure = sq["sure"][:, src], sq["unsure"][:, src]
    kh, gd, d1, d1t = (c[k][:, src] for k in ("khat", "gd", "d1", "d1t"))
    eif = np.abs(IF - kh)[sure] / (R.KAPPA * d1[sure])
    egd = np.abs(GD - gd)[sure] / (R.KAPPA * d1t[sure])
    print("IF at %.3g, GD at %.3g of the allowance KAPPA d1 (%d sure cells)" % (eif.max(), egd.max(), int(sure.sum())))
    assert np.all(np.isfinite(IF[sure])) and np.all(np.isfinite(GD[sure]))
    assert eif.max() <= 1 and egd.max() <= 1
    dead = ~c["used"][:, src] & ~unsure
    assert np.all(np.isnan(IF[dead])) and np.all(np.isnan(GD[dead]))
    assert np.all(np.isnan(IF) == np.isnan(GD))


@pytest.mark.parametrize("i", [4, 6, 9], ids=[IDS[j] for j in (4, 6, 9)])
def test_segment_mean(torch, i):
    """segmean: the frame's own mean (over its n values, the zeros outside the record included) removed before the windows; groups of
    16, 128 and 512 threads (the last two reduce across waves)."""
    cs, x, w, _, _ = case_of(i)
    x = x + np.asarray(0.7 - (0.2j if cs["cplx"] else 0), dtype=x.dtype)
    c = R.cells(x, *w, cs["hop"], cs["first"], R.NFRAMES, rel=R.REL, segmean=True)
    b0, nb = cs["band"] if cs["band"] else (0, None)
    sq = R.squeeze(c, b0, nb)
    assert R.unsure_share(c, sq) <= 0.02
    T = run(cs, x, w, segmean=True)[0]
    check_cells(T, sq["T"], sq["slackT"], sq["reach"], "T with segmean")
    plain = R.squeeze(R.cells(x, *w, cs["hop"], cs["first"], R.NFRAMES, rel=R.REL), b0, nb)
    assert np.max(np.abs(plain["T"] - sq["T"])) > 1e-3 * np.max(np.abs(sq["T"]))          # the offset is seen without it
    assert np.array_equal(T, run(cs, torch.as_tensor(x, device="cuda"), w, segmean=True)[0].cpu().numpy())


def test_bin_centred_tone_is_one_cell(torch):
    n, hop, nframes = 256, 5, 37
    t = np.arange(nframes * hop + n)
    x = np.exp(2j * math.pi * 40 * t / n).astype(np.complex64)
    h, dh, th = R.hann_windows(n)
    T = E.ssq(x, h, dh, hop, 0, nframes, rel=1e-3)[0]
    want = n * h[n // 2] * x[np.arange(nframes) * hop + n // 2]
    assert np.all(np.abs(T[:, 40] - want) <= 2e-4 * np.abs(want))
    rest = T.copy()
    rest[:, 40] = 0
    assert np.all(rest == 0)


@pytest.mark.parametrize("i", [1, 4, 6, 9], ids=[IDS[j] for j in (1, 4, 6, 9)])
def test_bitwise_reproducible(torch, i, monkeypatch):
    cs, x, w, c, sq = case_of(i)
    both = E.ssq_lds_bytes(cs["cplx"], cs["n"], sq["nb"], True, True) <= E.SSQ_LDS_MAX      # T and P from one call where they fit
    assert both == (cs["n"] in (256, 2048))
    a, b = run(cs, x, w, P=both), run(cs, x, w, P=both)
    assert np.array_equal(a[0], b[0]) and (a[1] is None or np.array_equal(a[1], b[1]))
    edges = np.array([[c["nsrc"] * 0.2, c["nsrc"] * 0.45], [c["nsrc"] * 0.55, c["nsrc"] * 0.8]])
    bands = E.ssq_bands(x, w[0], w[1], cs["hop"], cs["first"], R.NFRAMES, edges, rel=R.REL)
    for fpg in ("3", "5", "37"):
        monkeypatch.setenv("SP_SSQ_FPG", fpg)
        assert E.ssq_plan(cs["n"], R.NFRAMES, cplx=cs["cplx"], nb=sq["nb"])["fpr"] == int(fpg)
        assert np.array_equal(run(cs, x, w)[0], a[0]), fpg
        assert np.array_equal(E.ssq_bands(x, w[0], w[1], cs["hop"], cs["first"], R.NFRAMES, edges, rel=R.REL), bands), fpg
    monkeypatch.delenv("SP_SSQ_FPG")
    # device-resident on a side stream, and a slice at an odd element offset
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd = torch.as_tensor(x, device="cuda")
        d = run(cs, xd, w, P=both)
        buf = torch.zeros(x.shape[0] + 3, dtype=xd.dtype, device="cuda")
        buf[3:] = xd
        o = run(cs, buf[3:], w)
    side.synchronize()
    assert isinstance(d[0], torch.Tensor) and d[0].is_cuda and d[2] is None
    assert np.array_equal(d[0].cpu().numpy(), a[0]) and (a[1] is None or np.array_equal(d[1].cpu().numpy(), a[1]))
    assert np.array_equal(o[0].cpu().numpy(), a[0])


def test_batch_of_strided_rows(torch):
    cs, x, w, c, sq = case_of(4)
    nsig = x.shape[0]
    rows = np.stack([x, x[::-1], 0.5 * x]).astype(np.float32)
    buf = torch.full((3, nsig + 5), 7.0, dtype=torch.float32, device="cuda")
    buf[:, :nsig] = torch.as_tensor(rows, device="cuda")
    view = buf[:, :nsig]
    assert view.stride(0) == nsig + 5
    T = run(cs, view, w)[0].cpu().numpy()
    host = run(cs, rows, w)[0]
    assert T.shape == (3,) + sq["T"].shape and np.array_equal(T, host)
    assert np.array_equal(T[0], run(cs, x, w)[0]) and np.array_equal(T[1], run(cs, np.ascontiguousarray(x[::-1]), w)[0])
    modes = E.ssq_bands(view, w[0], w[1], cs["hop"], cs["first"], R.NFRAMES, [(10.0, 40.0)], rel=R.REL).cpu().numpy()
    assert modes.shape == (3, 1, R.NFRAMES)
    assert np.array_equal(modes[0], E.ssq_bands(x, w[0], w[1], cs["hop"], cs["first"], R.NFRAMES, [(10.0, 40.0)], rel=R.REL))


@pytest.mark.parametrize("i", [2, 5, 6, 8, 10], ids=[IDS[j] for j in (2, 5, 6, 8, 10)])
def test_band_sums_against_reference(torch, i):
    """ssq_bands (the un-rounded khat against float32 edges) and ssq_sum over the device's own T, against the reference's band sums.
    The edges of ssq_bands sit on half-integers, so both sum the same cells up to the unsure ones."""
    cs, x, w, c, sq = case_of(i)
    n, b0, nb = cs["n"], sq["b0"], sq["nb"]
    lo = b0 + nb // 5
    m = np.array([[lo, lo + nb // 4], [lo + nb // 3, lo + nb // 2 + 7]])                 # absolute target bins, inside the band, no wrap
    assert m.max() < (n if cs["cplx"] else n // 2 + 1) and m.max() < b0 + nb
    per_frame = np.repeat(m[:, None, :].astype(np.float64), R.NFRAMES, axis=1)
    per_frame[:, ::2, :] += 3                                                            # a band that moves with the frame
    for edges_m in (m.astype(np.float64), per_frame):
        edges = edges_m - 0.5
        want, slack = R.band_sums(c, edges)
        big = np.max(c["mag"], axis=1)
        got = E.ssq_bands(x, w[0], w[1], cs["hop"], cs["first"], R.NFRAMES, edges, rel=R.REL)
        err = np.abs(got - want)
        print("ssq_bands: %.3g of the largest cell" % float(np.max(err / big)))
        assert np.all(err <= 2e-4 * np.abs(want) + 1e-6 * big + slack)
        T = run(cs, x, w)[0]
        summed = E.ssq_sum(T, n, edges_m, b0=b0)
        assert np.all(np.abs(summed - want) <= 2e-4 * np.abs(want) + 1e-6 * big + slack)
        # ssq_sum is a plain sum of the T it is given
        e3 = edges_m if edges_m.ndim == 3 else np.repeat(edges_m[:, None, :], R.NFRAMES, axis=1)
        for b in range(2):
            for g in (0, 17, 36):
                j0, j1 = int(e3[b, g, 0]) - b0, int(e3[b, g, 1]) - b0
                plain = T[g, j0:j1].astype(np.complex128).sum()
                assert abs(summed[b, g] - plain) <= 1e-5 * np.sum(np.abs(T[g, j0:j1])) + 1e-30


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_way_back(torch, cplx):
    n, nsig = 256, 1500
    t = np.arange(nsig)
    # no content near the bins 0 and n / 2: what a real record squeezes below 0 or above n / 2 is dropped, not mirrored
    x = np.cos(2 * math.pi * (0.12 * t + 0.08 / nsig * t * t)) + 0.5 * np.cos(2 * math.pi * 0.37 * t)
    if cplx:
        x = x + 1j * np.sin(2 * math.pi * 0.21 * t)
    x = x.astype(np.complex64 if cplx else np.float32)
    f, tt, Tx = RA.ssq_stft(x, window="hann", nperseg=n, threshold=0.0)
    assert Tx.shape == ((n if cplx else n // 2 + 1), nsig) and np.array_equal(tt, t)
    back = RA.issq_stft(Tx, "hann", n, onesided=not cplx)
    err = float(np.max(np.abs(back - x)))
    print("issq_stft(ssq_stft(x)) - x: %.3g of max |x|" % (err / float(np.max(np.abs(x)))))
    assert err <= 2e-4 * float(np.max(np.abs(x)))
    if cplx:
        # bands of a complex record below 0 and across 0: the bins are taken modulo n
        full, tiny = np.asarray(back), 1e-5 * float(np.max(np.abs(x)))
        neg = RA.issq_stft(Tx, "hann", n, band=(-0.5, -1.0 / n), onesided=False)
        pos = RA.issq_stft(Tx, "hann", n, band=(0.0, 0.5 - 1.0 / n), onesided=False)
        across = RA.issq_stft(Tx, "hann", n, band=(-0.5, 0.5 - 1.0 / n), onesided=False)
        assert np.max(np.abs(neg)) > 0.1 and np.max(np.abs(neg + pos - full)) <= tiny and np.max(np.abs(across - full)) <= tiny
    if not cplx:
        # a ridge +- a half-width per frame: the mode from the band kernel against the same band of Tx (half-integer edges in bins)
        ridge = np.rint((0.12 + 0.16 / nsig * t) * n)
        c = R.cells(x, *R.hann_windows(n), 1, -n // 2, nsig)
        bands = np.stack([np.stack([ridge - 6.5, ridge + 6.5], axis=-1), np.stack([round(0.37 * n) - 5.5 + 0 * t, round(0.37 * n) + 5.5 + 0 * t], axis=-1)]) / n
        modes = RA.ssq_extract(x, bands, nperseg=n, threshold=0.0)
        assert modes.shape == (2, nsig) and modes.dtype == np.float32
        bins = np.arange(n // 2 + 1)[:, None]
        for b in range(2):
            inside = (bins >= bands[b, :, 0] * n) & (bins < bands[b, :, 1] * n)
            # 2 Re of a complex sum: the float32 figure applies to the sum's modulus, not to its real part near a zero crossing
            want = 2 * np.sum(np.where(inside, Tx, 0), axis=0) / (n * 1.0)
            _, slack = R.band_sums(c, bands[b:b + 1] * n)
            err = np.abs(modes[b] - want.real)
            print("ssq_extract against the band of Tx: %.3g of the mode's modulus" % float(np.max(err / np.abs(want))))
            assert np.all(err <= 2e-4 * np.abs(want) + 1e-6 * np.max(np.abs(x)) + 2 * slack[0] / n)
        mid = slice(n, nsig - n)
        assert np.max(np.abs(modes[1][mid] - 0.5 * np.cos(2 * math.pi * 0.37 * t[mid]))) < 0.02


def test_sum_wraps_with_the_band(torch):
    """A complex T over a band that wraps past bin n - 1: ssq_sum compares the edges with the bin modulo n."""
    cs, x, w, c, sq = case_of(3)
    n, (b0, nb) = cs["n"], cs["band"]
    assert cs["cplx"] and b0 + nb > n
    T = run(cs, x, w)[0]
    bins = (b0 + np.arange(nb)) % n
    got = E.ssq_sum(T, n, [(240.0, 256.0), (0.0, 20.0), (250.0, 251.0)], b0=b0)
    for b, (lo, hi) in enumerate(((240, 256), (0, 20), (250, 251))):
        sel = (bins >= lo) & (bins < hi)
        assert sel.sum() == hi - lo
        want = T[:, sel].astype(np.complex128).sum(axis=1)
        assert np.all(np.abs(got[b] - want) <= 1e-5 * np.sum(np.abs(T[:, sel]), axis=1) + 1e-30)


def test_other_entries_are_untouched(torch):
    rng = np.random.default_rng(9)
    x = rng.standard_normal(5000).astype(np.float32)
    win = np.hanning(256)
    a = E.stft_frames(x, win, 64, 70)
    RA.ssq_stft(x, nperseg=256, hop=64)
    RA.squeezed_spectrogram(x, nperseg=256, hop=64)
    RA.reassignment_fields(x, nperseg=256, hop=64)
    RA.ssq_extract(x, [(0.1, 0.2)], nperseg=256, hop=64)
    b = E.stft_frames(x, win, 64, 70)
    assert a[0].shape == (70, 128) and np.array_equal(a[0], b[0])


def test_public_shapes_and_scaling(torch):
    import scipy.signal as ss
    fs, n, hop = 1000.0, 256, 32
    t = np.arange(4000) / fs
    x = (1.5 * np.cos(2 * math.pi * 125.0 * t)).astype(np.float32)
    f, tt, P = RA.squeezed_spectrogram(x, fs=fs, nperseg=n, hop=hop, boundary=None)
    fr, tr, S = ss.spectrogram(x, fs=fs, window="hann", nperseg=n, noverlap=n - hop, scaling="spectrum", mode="psd", detrend=False)
    assert P.shape == S.shape and np.allclose(f, fr) and np.allclose(tt, tr)
    # the squeeze moves power, it does not make or lose any: the rms^2 of the line times the window's noise bandwidth, 1.5 bins
    assert np.all(np.abs(S.sum(axis=0) - P.sum(axis=0)) < 2e-3) and np.all(np.abs(S.sum(axis=0) - 1.5 * 1.125) < 2e-3)
    assert np.all(P[32] > 0.99 * P.sum(axis=0))
    f, tt, fh, th = RA.reassignment_fields(x, fs=fs, nperseg=n, hop=hop, boundary=None, threshold=1e-2, band=(100.0, 150.0))
    ok = np.isfinite(fh)
    assert ok.any() and np.all(np.abs(fh[ok] - 125.0) < 0.05) and fh.shape == th.shape == (len(f), len(tt))
    # a stationary line: every cell's group delay is its frame's centre, held in float64 (a float32 could not keep hop 1 apart at 2^20)
    assert th.dtype == np.float64 and np.all(np.abs(th[ok] - np.broadcast_to(tt, th.shape)[ok]) < 0.05 / fs)
    xd = torch.as_tensor(x, device="cuda")
    d = RA.ssq_stft(xd, fs=fs, nperseg=n, hop=hop)[2]
    assert isinstance(d, torch.Tensor) and np.array_equal(d.cpu().numpy(), RA.ssq_stft(x, fs=fs, nperseg=n, hop=hop)[2])
    # device tensors in, device tensors out, the same numbers
    Pd = RA.squeezed_spectrogram(xd, fs=fs, nperseg=n, hop=hop, boundary=None)[2]
    fd, td = RA.reassignment_fields(xd, fs=fs, nperseg=n, hop=hop, boundary=None, threshold=1e-2, band=(100.0, 150.0))[2:]
    assert Pd.is_cuda and fd.is_cuda and np.allclose(Pd.cpu().numpy(), P, rtol=1e-6, atol=0)
    assert np.allclose(fd.cpu().numpy(), fh, rtol=1e-6, equal_nan=True) and np.allclose(td.cpu().numpy(), th, rtol=1e-6, equal_nan=True)
    md = RA.ssq_extract(xd, [(100.0, 150.0)], fs=fs, nperseg=n, hop=hop)
    assert md.is_cuda and np.array_equal(md.cpu().numpy(), RA.ssq_extract(x, [(100.0, 150.0)], fs=fs, nperseg=n, hop=hop))
