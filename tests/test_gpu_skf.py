"""The two-point wavenumber-frequency spectrum S(k, f) on the MI355X against the float64 oracle of tests/test_host_skf.py.  A histogram
is discontinuous, so a cell is held between the oracle's `lower` (the samples whose phase, with its float32 error, lies surely in the
bin) and `upper` (every unsure sample added to every bin it may land in), with the Welch PSD bounds of tests/test_gpu_kernels.py on
top: lower (1 - 2e-4) - 1e-6 max <= S <= upper (1 + 2e-4) + 1e-6 max in every cell.  The row sums do not depend on where a sample
lands: they agree with the float64 Welch mean PSD at rtol 2e-4, atol 1e-6 max.  Cells that `upper` leaves empty are exactly 0."""
import math

import numpy as np
import pytest

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E, _wavenumber_mod as WN                       # noqa: E402
from test_host_skf import (SHAPES, SHAPE_IDS, CASES, CASE_IDS, POWERS, shape_case, skf_ref, welch_mean_psd, hann,   # noqa: E402
                           exact_pair, bandlimited_pair, make_pair)


def within(S, ref, rows, what):
    """S against (hist, lower, upper, unsure) and the row sums `rows`."""
    hist, lower, upper, _ = ref
    top = float(hist.max())
    assert S.shape == hist.shape and S.dtype == np.float64, what
    under = float(np.max(lower * (1 - 2e-4) - 1e-6 * top - S))
    over = float(np.max(S - upper * (1 + 2e-4) - 1e-6 * top))
    moved = float(np.sum(np.abs(S - hist)) / np.sum(hist))
    print("%s: below lower by %.3g, above upper by %.3g of the largest cell; %.3g of the power sits in another cell than the oracle's"
          % (what, under / top, over / top, moved))
    assert under <= 0 and over <= 0, what
    assert np.all(S[upper == 0] == 0), what
    np.testing.assert_allclose(S.sum(axis=1), rows, rtol=2e-4, atol=1e-6 * float(rows.max()), err_msg=what)


def run(k, nframes, power="mean"):
    nfft, hop, nk, (b0, nb), _ = SHAPES[k]
    x, y, win, scale, _, _ = shape_case(k, nframes)
    return E.skf(x, y, nfft, hop, nframes, b0, nb, nk, win=win, segmean=True, cross=power == "cross", scale=scale)


@pytest.mark.parametrize("k,nframes", CASES, ids=CASE_IDS)
def test_accuracy(k, nframes):
    _, _, _, _, ref, psd = shape_case(k, nframes)
    for pw in POWERS:
        S = run(k, nframes, pw)
        within(S, ref[pw], psd if pw == "mean" else ref[pw][0].sum(axis=1), "%s %s" % (CASE_IDS[CASES.index((k, nframes))], pw))


def test_exact_case():
    """Pins the sign and the bin map: y[n] = x[n - 1] puts the whole power of the odd bin f into cell f // 2 + 16 of 32."""
    x, y = exact_pair()
    S = E.skf(x, y, 64, 64, 8, 0, 33, 32, win=None, segmean=False, scale=1.0)
    top = S.max()
    assert abs(top - 32.0 ** 2) <= 2e-4 * 32.0 ** 2
    odd = np.arange(1, 32, 2)
    for f in odd:
        j = f // 2 + 16
        assert abs(S[f, j] - 32.0 ** 2) <= 2e-4 * 32.0 ** 2, f
        assert np.all(np.delete(S[f], j) <= 1e-6 * top), f
    Sw = E.skf(y, x, 64, 64, 8, 0, 33, 32, win=None, segmean=False, scale=1.0)
    np.testing.assert_allclose(Sw[odd], S[odd][:, ::-1], rtol=2e-4, atol=1e-6 * top)
    assert np.array_equal(np.argmax(Sw[odd], axis=1), 31 - (odd // 2 + 16))


@pytest.mark.parametrize("k,fpg", [(2, 3), (3, 5), (6, 37), (0, 5)], ids=lambda v: str(v))
def test_runs_of_frames(k, fpg, monkeypatch):
    """SP_SKF_FPG: runs of 3, 5 and 37 frames, the last partly past the end (3 and 5 do not divide 37, and a run is not a whole
    number of rounds of the workgroup's groups): the result stays within the bounds."""
    nframes = 37
    _, _, _, _, ref, psd = shape_case(k, nframes)
    monkeypatch.setenv("SP_SKF_FPG", str(fpg))
    S = run(k, nframes)
    monkeypatch.delenv("SP_SKF_FPG")
    within(S, ref["mean"], psd, "%s in runs of %d" % (SHAPE_IDS[k], fpg))


@pytest.mark.parametrize("k,cells,tiles,nframes", [(2, 64 * 64, 2, 3000), (4, 63 * 48, 7, 37)], ids=lambda v: str(v))
def test_tiles_keep_the_bits(k, cells, tiles, nframes, monkeypatch):
    """SP_SKF_CELLS forces several frequency tiles at small shapes: every cell sees the same additions in the same order, so the
    table is bitwise the untiled one at the same frames per run."""
    nfft, _, nk, (_, nb), cplx = SHAPES[k]
    _, _, _, _, ref, psd = shape_case(k, nframes)
    assert WN.skf_plan(nfft, nk, nb=nb, cplx=cplx, cells=0)["tiles"] == 1
    for fpg in (16, 37):
        monkeypatch.setenv("SP_SKF_FPG", str(fpg))
        monkeypatch.delenv("SP_SKF_CELLS", raising=False)
        one = run(k, nframes)
        monkeypatch.setenv("SP_SKF_CELLS", str(cells))
        assert WN.skf_plan(nfft, nk, nb=nb, cplx=cplx)["tiles"] == tiles
        out = np.zeros(4, dtype=np.int64)
        assert _ffi.lib().sp_skf_plan(int(cplx), nfft, nb, nk, _ffi.ptr(out)) == 0 and out[0] == tiles
        many = run(k, nframes)
        monkeypatch.delenv("SP_SKF_CELLS")
        monkeypatch.delenv("SP_SKF_FPG")
        assert np.array_equal(one, many)
        within(many, ref["mean"], psd, "%s in %d tiles, runs of %d" % (SHAPE_IDS[k], tiles, fpg))


@pytest.mark.parametrize("k", [2, 3, 6], ids=[SHAPE_IDS[k] for k in (2, 3, 6)])
def test_reproducible_and_resident(k):
    import torch
    nfft, hop, nk, (b0, nb), cplx = SHAPES[k]
    nframes = 37
    x, y, win, scale, _, _ = shape_case(k, nframes)
    a, b = run(k, nframes, "cross"), run(k, nframes, "cross")
    assert np.array_equal(a, b)
    xt, yt = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d = E.skf(xt, yt, nfft, hop, nframes, b0, nb, nk, win=win, segmean=True, cross=True, scale=scale)
    s.synchronize()
    assert d.is_cuda and d.device == xt.device and d.dtype == torch.float64 and np.array_equal(d.cpu().numpy(), a)
    # the public function on device tensors: S stays on the device, the axes are host arrays
    f, kk, S = WN.skf(xt, yt, 1.0, 1.0, nperseg=nfft, noverlap=nfft - hop, nk=nk, power="cross")
    torch.cuda.synchronize()
    assert S.is_cuda and S.dtype == torch.float64 and isinstance(f, np.ndarray) and isinstance(kk, np.ndarray)
    f2, k2, S2 = WN.skf(x, y, 1.0, 1.0, nperseg=nfft, noverlap=nfft - hop, nk=nk, power="cross")
    assert np.array_equal(S.cpu().numpy(), S2) and np.array_equal(f, f2) and np.array_equal(kk, k2)


def test_public_skf():
    """skf on arrays against the oracle scaled on the host: the one-sided doubling, the fftshift-ed complex axis, a band through zero."""
    fs, dx, nfft, hop, nk, nframes = 250.0, 0.02, 256, 128, 33, 40
    nsig = (nframes - 1) * hop + nfft + 50                                      # a trailing partial segment is dropped
    w = hann(nfft)
    kref = (np.arange(nk) + 0.5 - 0.5 * nk) * 2 * math.pi / (nk * dx)
    # real input, every bin but DC and Nyquist compared through the bounds (there the phase sits on a bin edge); their row sums too
    x, y = make_pair(nsig, False, 61, d=3)
    f, k, S = WN.skf(x, y, fs, dx, nperseg=nfft, nk=nk)
    np.testing.assert_allclose(f, np.fft.rfftfreq(nfft, 1 / fs))
    np.testing.assert_allclose(k, kref)
    scale = 1.0 / (fs * np.sum(w * w))
    ref = tuple(2.0 * t for t in skf_ref(x, y, nfft, hop, nframes, nk, 1, 127, w, True, "mean", scale)[:3]) + (0.0,)
    psd = welch_mean_psd(x, y, nfft, hop, nframes, 0, 129, w, True, scale) * np.r_[1.0, np.full(127, 2.0), 1.0]
    assert S.shape == (129, nk)
    within(S[1:128], ref, psd[1:128], "real, one-sided")
    np.testing.assert_allclose(S.sum(axis=1), psd, rtol=2e-4, atol=1e-6 * psd.max())
    # 'spectrum' scaling, a tuple window, no detrend, the cross power, a band
    w2 = np.kaiser(nfft + 1, 6.0)[:-1]
    x0, y0 = (x - np.float32(1.5)).astype(np.float32), (y + np.float32(0.7)).astype(np.float32)
    f, _, S = WN.skf(x0, y0, fs, dx, nperseg=nfft, noverlap=nfft - 100, window=("kaiser", 6.0), nk=nk, band=(20.0, 60.0), detrend=False,
                     power="cross", scaling="spectrum")
    lo, hi = int(math.ceil(20.0 * nfft / fs)), int(math.floor(60.0 * nfft / fs))
    nfr = 1 + (nsig - nfft) // 100
    np.testing.assert_allclose(f, np.arange(lo, hi + 1) * fs / nfft)
    r = skf_ref(x0, y0, nfft, 100, nfr, nk, lo, hi - lo + 1, w2, False, "cross", 1.0 / np.sum(w2) ** 2)
    within(S, tuple(2.0 * t for t in r[:3]) + (0.0,), 2.0 * r[0].sum(axis=1), "real, a band, spectrum scaling, cross")
    # complex input: the fftshift-ed axis, and a band that runs through zero
    xc, yc = make_pair(nsig, True, 62, d=3)
    f, _, S = WN.skf(xc, yc, fs, dx, nperseg=nfft, nk=nk)
    np.testing.assert_allclose(f, np.fft.fftshift(np.fft.fftfreq(nfft, 1 / fs)))
    r = skf_ref(xc, yc, nfft, hop, nframes, nk, nfft // 2, nfft, w, True, "mean", scale)
    within(S, r, welch_mean_psd(xc, yc, nfft, hop, nframes, nfft // 2, nfft, w, True, scale), "complex, two-sided")
    f, _, Sb = WN.skf(xc, yc, fs, dx, nperseg=nfft, nk=nk, band=(-30.0, 12.0))
    keep = (np.fft.fftshift(np.fft.fftfreq(nfft, 1 / fs)) >= -30.0) & (np.fft.fftshift(np.fft.fftfreq(nfft, 1 / fs)) <= 12.0)
    assert f[0] < 0 < f[-1] and Sb.shape == (int(keep.sum()), nk)
    assert np.array_equal(Sb, S[keep])                                          # the same additions in the same order: the same bits


def test_dispersion():
    """The band-limited pair: kbar(f) dx within half a bin width, pi / nk, of 2 pi f 2.3 / fs on 0.03 .. 0.15 (the oracle: 0.17 bins)."""
    fs, dx, nfft, hop, nframes, nk = 2.0e6, 5e-3, 256, 100, 500, 65
    x, y = bandlimited_pair((nframes - 1) * hop + nfft)
    f, kbar, sig, P = WN.dispersion(x, y, fs, dx, nperseg=nfft, noverlap=nfft - hop, nk=nk)
    assert f.shape == kbar.shape == sig.shape == P.shape == (nfft // 2 + 1,)
    use = (f >= 0.03 * fs) & (f <= 0.15 * fs)
    err = np.abs(kbar * dx - 2 * math.pi * f * 2.3 / fs)[use]
    print("kbar dx off by at most %.3f bins; sigma_k dx %.3f .. %.3f rad" % (err.max() * nk / (2 * math.pi), (sig * dx)[use].min(),
                                                                            (sig * dx)[use].max()))
    assert err.max() <= math.pi / nk
    f2, k, S = WN.skf(x, y, fs, dx, nperseg=nfft, noverlap=nfft - hop, nk=nk)
    m = WN.skf_moments(k, S)
    assert np.array_equal(m["kbar"], kbar) and np.array_equal(m["sigma_k"], sig) and np.array_equal(m["P"], P) and np.array_equal(f, f2)
    assert np.all(P[use] > 1e2 * P[f > 0.2 * fs].max())


def test_raw_abi_refusals():
    """Every refusal returns < 0, names the entry point and leaves a poisoned s_out alone; the library works afterwards."""
    _ffi.init()
    lib = _ffi.lib()
    nsig, nfft, hop, nframes, nk, b0, nb = 1000, 64, 32, 20, 16, 1, 31
    x, y = make_pair(nsig, False, 51, d=3)
    xc = np.zeros(nsig, dtype=np.complex64)
    w = hann(nfft).astype(np.float32)
    out = np.full((nb, nk), -3.5, dtype=np.float64)
    good = dict(x=_ffi.ptr(x), y=_ffi.ptr(y), dtype=_ffi.DTYPE_F32, nsig=nsig, win=_ffi.ptr(w), nfft=nfft, hop=hop, nframes=nframes,
                detrend=_ffi.DETREND_SEGMEAN, power=_ffi.SKF_MEAN, b0=b0, nb=nb, nk=nk, scale=1.0, s_out=_ffi.ptr(out), mem=0)
    cgood = dict(good, x=_ffi.ptr(xc), y=_ffi.ptr(xc), dtype=_ffi.DTYPE_C64)
    bad = [dict(nfft=16, win=None), dict(nfft=8192, nsig=1 << 20, win=None), dict(nfft=48, win=None), dict(nfft=0, win=None),
           dict(nfft=-64, win=None), dict(nk=1), dict(nk=0), dict(nk=-4), dict(nk=1025), dict(nb=0), dict(nb=-1), dict(b0=-1),
           dict(b0=2, nb=32), dict(b0=33, nb=1), dict(b0=0, nb=34), dict(b0=1 << 30, nb=1 << 30), dict(hop=0), dict(hop=-3),
           dict(nframes=0), dict(nframes=-1), dict(nframes=31), dict(nsig=63), dict(nframes=1 << 40), dict(dtype=2), dict(dtype=-1),
           dict(detrend=_ffi.DETREND_MEAN), dict(detrend=_ffi.DETREND_LINEAR), dict(detrend=_ffi.DETREND_SEGLINEAR), dict(detrend=9),
           dict(power=2), dict(power=-1), dict(scale=float("nan")), dict(scale=float("inf")), dict(x=None), dict(y=None),
           dict(s_out=None)]
    cbad = [dict(b0=64, nb=1), dict(b0=-1, nb=4), dict(b0=0, nb=65)]
    for base, changes in ((good, bad), (cgood, cbad)):
        for change in changes:
            args = dict(base, **change)
            rc = lib.sp_skf(*args.values())
            msg = (lib.sp_last_error() or b"").decode()
            assert rc < 0 and "sp_skf" in msg, (change, rc, msg)
            assert np.all(out == -3.5), change
    assert lib.sp_skf(*good.values()) == 0
    scale = 1.0
    ref = skf_ref(x, y, nfft, hop, nframes, nk, b0, nb, w, True, "mean", scale)
    within(out, ref, welch_mean_psd(x, y, nfft, hop, nframes, b0, nb, w, True, scale), "the good call after the refusals")
    # a complex band through zero over all 64 bins is accepted
    outc = np.full((64, nk), -3.5, dtype=np.float64)
    assert lib.sp_skf(*dict(cgood, b0=40, nb=64, s_out=_ffi.ptr(outc)).values()) == 0 and not np.any(outc)
