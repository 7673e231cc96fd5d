"""The short-time cross-correlation on the MI355X against the float64 oracle of tests/test_host_xcorr_frames.py (the definition's direct
lag sums; the spectral form in float64 where the weighting is spectral).  Inputs: the same noise sequence shifted by d = 5 samples plus
independent noise and different offsets, rounded to float32 first; the oracle reads the rounded values.
Bounds: frames and avg within 1e-4 of the largest |ref| (the project's bound for ccf and for the two-transform czt path); avg against the
float64 mean of the frames output 1e-6 of its maximum (fp32 run sums of at most a few dozen frames, float64 across the runs); the peak's
lag exactly and its fraction to 2e-3 (a lag error of 1e-4 top over a curvature of at least 0.1 top) on the frames whose top stands clear."""
import numpy as np
import pytest

from conftest import have_gpu, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E, _ccf_mod as CC                              # noqa: E402
from test_host_xcorr_frames import (SHAPES, SHAPE_IDS, shape_case, xcorr_frames_ref, peak_ref, make_pair, frames_of,   # noqa: E402
                                    xc_len)

BETA = 1e-2


def close(got, ref, what, tol=1e-4):
    err = float(np.max(np.abs(np.asarray(got, dtype=ref.dtype) - ref)) / np.max(np.abs(ref)))
    print("%s: max err / max |ref| = %.3g" % (what, err))
    assert got.shape == ref.shape and err <= tol, what


def run_all(x, y, shape, nframes, **kw):
    nw, maxlag, hop, _ = shape
    fr, av, pk = E.xcorr_frames(x, y, nw, hop, nframes, maxlag, frames=True, avg=True, peak=True, **kw)
    assert fr.shape == (nframes, 2 * maxlag + 1) and av.shape == (2 * maxlag + 1,) and pk.shape == (nframes, 2)
    assert fr.dtype == (np.complex64 if shape[3] else np.float32) and av.dtype == (np.complex128 if shape[3] else np.float64)
    return fr, av, pk


def check_avg_is_mean_of_frames(fr, av, what):
    m = fr.astype(av.dtype).mean(axis=0)
    err = float(np.max(np.abs(av - m)) / np.max(np.abs(m)))
    print("%s: avg against the float64 mean of the frames %.3g" % (what, err))
    assert err <= 1e-6, what


CASES = [(k, nf) for k in range(len(SHAPES)) for nf in (1, 37)] + [(2, 3000)]
CASE_IDS = ["%s-%dfr" % (SHAPE_IDS[k], nf) for k, nf in CASES]


@pytest.mark.parametrize("k,nframes", CASES, ids=CASE_IDS)
def test_accuracy(k, nframes):
    """coeff, raw and the regularised PHAT at every shape: all three outputs from one launch."""
    shape = SHAPES[k]
    nw, maxlag, hop, _ = shape
    x, y, raw, En = shape_case(k, nframes)
    for what, kw, ref in (("coeff", dict(), raw / En[:, None]), ("raw", dict(coeff=False), raw),
                          ("phat", dict(beta=BETA), None)):
        if ref is None:
            ref = xcorr_frames_ref(x, y, nw, hop, nframes, maxlag, beta=BETA)
        fr, av, pk = run_all(x, y, shape, nframes, **kw)
        close(fr, ref, what + " frames")
        close(av, ref.mean(axis=0), what + " avg")
        check_avg_is_mean_of_frames(fr, av, what)
        # each output alone is the same launch with the other two switched off: the same bits
        f1, _, _ = E.xcorr_frames(x, y, nw, hop, nframes, maxlag, frames=True, **kw)
        _, a1, _ = E.xcorr_frames(x, y, nw, hop, nframes, maxlag, avg=True, **kw)
        _, _, p1 = E.xcorr_frames(x, y, nw, hop, nframes, maxlag, peak=True, **kw)
        assert np.array_equal(f1, fr) and np.array_equal(a1, av) and np.array_equal(p1, pk, equal_nan=True)


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_taper_and_weight(k):
    """A Hann taper, a band table on the cross spectrum, and no mean removal: the outputs agree with each other and with the oracle."""
    shape = SHAPES[k]
    nw, maxlag, hop, _ = shape
    nframes = 37
    x, y, _, _ = shape_case(k, nframes)
    L = xc_len(nw, maxlag)
    w = np.hanning(nw).astype(np.float32)
    band = CC.band_weight(L, 1.0, (0.05, 0.3))
    assert 0 < band.sum() < L
    # without the mean removal the records go in with their offsets taken off (and rounded again): the bound is the one of the rest
    x0, y0 = (x - x.dtype.type(1.5)).astype(x.dtype), (y + y.dtype.type(0.7)).astype(y.dtype)
    for what, kw in (("hann", dict(win=w)), ("band", dict(weight=band)), ("band phat", dict(weight=band, beta=BETA)),
                     ("hann band nomean", dict(win=w, weight=band, segmean=False))):
        xs, ys = (x0, y0) if "nomean" in what else (x, y)
        fr, av, _ = run_all(xs, ys, shape, nframes, **kw)
        check_avg_is_mean_of_frames(fr, av, what)
        if "band" in what or nw <= 1000:                       # (the direct sums of a tapered 4096-sample window are slow: the spectral ones)
            close(fr, xcorr_frames_ref(xs, ys, nw, hop, nframes, maxlag, L=L, **kw), what + " frames")


@pytest.mark.parametrize("k,nframes,fpg", [(2, 3000, 7), (3, 37, 5), (5, 37, 3), (6, 37, 4), (8, 37, 6), (0, 37, 37)],
                         ids=lambda v: str(v))
def test_runs_of_frames(k, nframes, fpg, monkeypatch):
    """Several frames per transform group (SP_XCF_FPG), with a last run that is partly past the end: a frame's lags and peak keep
    their bits however the frames are dealt out; the average, summed in float32 along a run, stays within the bound."""
    shape = SHAPES[k]
    nw, maxlag, hop, _ = shape
    x, y, raw, En = shape_case(k, nframes)
    ref = raw / En[:, None]
    for kw in (dict(), dict(beta=BETA)):
        monkeypatch.delenv("SP_XCF_FPG", raising=False)
        f0, a0, p0 = run_all(x, y, shape, nframes, **kw)
        monkeypatch.setenv("SP_XCF_FPG", str(fpg))
        f1, a1, p1 = run_all(x, y, shape, nframes, **kw)
        _, a2, _ = E.xcorr_frames(x, y, nw, hop, nframes, maxlag, avg=True, **kw)
        monkeypatch.delenv("SP_XCF_FPG")
        assert np.array_equal(f1, f0) and np.array_equal(p1, p0) and np.array_equal(a2, a1)
        check_avg_is_mean_of_frames(f1, a1, "runs of %d" % fpg)
        if not kw:
            close(a1, ref.mean(axis=0), "avg over runs of %d" % fpg)


def check_track(pk, ref, maxlag, what):
    l, dl, h, gap, curv = peak_ref(ref, maxlag)
    top = np.abs(ref).max(axis=1) if np.iscomplexobj(ref) else ref.max(axis=1)
    use = (gap > 1e-3 * top) & (curv >= 0.1 * top)
    print("%s: %d of %d frames left out, lags %d .. %d, smallest curvature / top %.3g" % (what, int(np.sum(~use)), use.size, l.min(), l.max(),
                                                                                       float(np.min(curv / top))))
    assert np.sum(~use) <= 0.01 * use.size, what
    # the kernel returns l* + delta, so l* is read back as its nearest integer.  That is exact while |delta| stays clear of 1/2 by more
    # than the tolerance of delta; on these inputs every compared frame does (asserted), so l* is compared exactly on all of them
    assert not np.any((np.abs(dl) > 0.5 - 4e-3)[use]), what
    gl = np.rint(pk[:, 0].astype(np.float64))
    pos_err = np.abs(pk[:, 0].astype(np.float64) - (l + dl))[use]
    print("%s: worst position error %.3g, worst height error / top %.3g" % (what, float(pos_err.max()),
                                                                         float(np.max(np.abs(pk[:, 1] - h)[use] / top[use]))))
    assert np.all((gl == l)[use]), what
    assert np.all(pos_err <= 2e-3), what
    # |dh| <= |dq| + |qm - qp| |d delta| / 4 + |delta| |d(qm - qp)| / 4 <= (1e-4 + 2 * 2e-3 / 4 + 2e-4 / 8) top
    assert np.all(np.abs(pk[:, 1] - h)[use] <= 1.2e-3 * top[use]), what
    return l, dl, use


@pytest.mark.parametrize("k,nframes", [(k, 37) for k in range(2, len(SHAPES))] + [(2, 3000)],
                         ids=["%s-%dfr" % (SHAPE_IDS[k], 37) for k in range(2, len(SHAPES))] + [SHAPE_IDS[2] + "-3000fr"])
def test_peak_track(k, nframes):
    shape = SHAPES[k]
    nw, maxlag, hop, _ = shape
    x, y, raw, En = shape_case(k, nframes)
    for what, kw, ref in (("coeff", dict(), raw / En[:, None]), ("phat", dict(beta=BETA), None)):
        if ref is None:
            ref = xcorr_frames_ref(x, y, nw, hop, nframes, maxlag, beta=BETA)
        _, _, pk = E.xcorr_frames(x, y, nw, hop, nframes, maxlag, peak=True, **kw)
        l, _, use = check_track(pk, ref, maxlag, what)
        if maxlag >= 5 and nw >= 64:
            assert np.all(l[use] == -5)


def band_limited_pair(nsig, delay, seed):
    """Noise confined to 0.02 .. 0.2 cycles per sample, and the same delayed by a fractional number of samples (a phase ramp), plus
    independent noise: x leads y by `delay`."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(nsig)
    S = (rng.standard_normal(f.size) + 1j * rng.standard_normal(f.size)) * ((f >= 0.02) & (f <= 0.2))
    y = np.fft.irfft(S, nsig)
    x = np.fft.irfft(S * np.exp(2j * np.pi * f * delay), nsig)
    sd = y.std()
    x = x / sd + 0.05 * rng.standard_normal(nsig) + 1.5
    y = y / sd + 0.05 * rng.standard_normal(nsig) - 0.7
    return _ffi.as_samples(x), _ffi.as_samples(y)


def test_fractional_delay_track():
    nw, hop, maxlag, nframes, fs = 256, 100, 40, 500, 2.0e6
    x, y = band_limited_pair((nframes - 1) * hop + nw, 5.3, 31)
    ref = xcorr_frames_ref(x, y, nw, hop, nframes, maxlag)
    _, _, pk = E.xcorr_frames(x, y, nw, hop, nframes, maxlag, peak=True)
    l, dl, use = check_track(pk, ref, maxlag, "band-limited, delay 5.3")
    med_ref, med = float(np.median((l + dl)[use])), float(np.median(pk[use, 0]))
    print("median position: oracle %.4f, device %.4f" % (med_ref, med))
    # the three-point parabola on a peak this wide is biased by a few hundredths of a sample; 0.1 is a loose ceiling for it
    assert abs(med_ref + 5.3) <= 0.1 and abs(med - med_ref) <= 2e-3
    t, delay, height = CC.delay_track(x, y, fs, nw, hop=hop, maxlag=maxlag)
    assert t.shape == delay.shape == height.shape == (nframes,)
    np.testing.assert_array_equal(delay, -pk[:, 0].astype(np.float64) / fs)
    np.testing.assert_array_equal(height, pk[:, 1].astype(np.float64))
    np.testing.assert_allclose(t, (np.arange(nframes) * hop + 0.5 * (nw - 1)) / fs)
    assert abs(np.median(delay) * fs - 5.3) <= 0.1                             # x leads: a positive delay in tau's convention


def test_drop_in():
    g = load_golden("ccf")
    for a, b, co in ((g["x1"], g["x2"], g["co"]), (g["x3"], g["x4"], g["co2"])):
        n = a.size
        tau, t, fr = CC.ccf_frames(a, b, 250.0, n)
        assert fr.shape == (1, 2 * n - 1) and t.shape == (1,)
        close(fr[0], co.astype(np.float64), "one window over the golden record of %d" % n)
        tau_ref, _ = CC.ccf(a, b, 250.0)
        np.testing.assert_array_equal(tau, tau_ref)
    # ccf_sh = the mean of the per-window ccf formula
    x, y = make_pair(5000, False, 41)
    nav, hop, fs = 300, 120, 1.0e3
    tau, csh = CC.ccf_sh(x, y, fs, nav, hop=hop)
    nfr = 1 + (5000 - nav) // hop
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    ref = np.zeros(2 * nav - 1)
    for gq in range(nfr):
        a, b = xd[gq * hop:gq * hop + nav], yd[gq * hop:gq * hop + nav]
        ref += np.correlate(a - a.mean(), b - b.mean(), "full") / (nav * a.std() * b.std())
    ref /= nfr
    assert csh.dtype == np.float64
    close(csh, ref, "ccf_sh against the mean of the windows' ccf")
    tau_ref, _ = CC.ccf(x[:nav], y[:nav], fs)
    np.testing.assert_array_equal(tau, tau_ref)
    # the default hop is nav, a trailing partial window is dropped; the other norms are raw scaled per lag
    _, c1 = CC.ccf_sh(x, y, fs, nav, maxlag=20)
    _, c2 = CC.ccf_sh(x[:(5000 // nav) * nav], y[:(5000 // nav) * nav], fs, nav, hop=nav, maxlag=20)
    assert np.array_equal(c1, c2)
    _, raw = CC.ccf_sh(x, y, fs, nav, maxlag=20, norm="raw")
    _, bia = CC.ccf_sh(x, y, fs, nav, maxlag=20, norm="biased")
    _, unb = CC.ccf_sh(x, y, fs, nav, maxlag=20, norm="unbiased")
    np.testing.assert_allclose(bia, raw / nav, rtol=1e-14)
    np.testing.assert_allclose(unb, raw / (nav - np.abs(np.arange(-20, 21))), rtol=1e-14)
    # band= is the 0 / 1 weight
    _, cb = CC.ccf_sh(x, y, fs, nav, maxlag=20, band=(50.0, 200.0))
    _, cw = CC.ccf_sh(x, y, fs, nav, maxlag=20, weight=CC.band_weight(CC.ccf_plan(nav, 20)["L"], fs, (50.0, 200.0)))
    assert np.array_equal(cb, cw)


@pytest.mark.parametrize("k", [3, 4, 8], ids=[SHAPE_IDS[k] for k in (3, 4, 8)])
def test_reproducible_and_resident(k):
    import torch
    shape = SHAPES[k]
    nw, maxlag, hop, cplx = shape
    nframes = 37
    x, y, _, _ = shape_case(k, nframes)
    a = run_all(x, y, shape, nframes, beta=BETA)
    b = run_all(x, y, shape, nframes, beta=BETA)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    xt, yt = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d = E.xcorr_frames(xt, yt, nw, hop, nframes, maxlag, beta=BETA, frames=True, avg=True, peak=True)
    s.synchronize()
    for u, v in zip(a, d):
        assert v.is_cuda and v.device == xt.device and np.array_equal(v.cpu().numpy(), u)
    assert d[0].dtype == (torch.complex64 if cplx else torch.float32) and d[1].dtype == (torch.complex128 if cplx else torch.float64)
    # the public functions on device tensors
    tau, csh = CC.ccf_sh(xt, yt, 10.0, nw, hop=hop, maxlag=maxlag, phat=BETA)
    t, delay, height = CC.delay_track(xt, yt, 10.0, nw, hop=hop, maxlag=maxlag, phat=BETA)
    torch.cuda.synchronize()
    assert csh.is_cuda and delay.is_cuda and height.is_cuda and isinstance(tau, np.ndarray) and isinstance(t, np.ndarray)
    assert np.array_equal(csh.cpu().numpy(), a[1]) and np.array_equal(height.cpu().numpy(), a[2][:, 1])
    np.testing.assert_allclose(delay.cpu().numpy(), -a[2][:, 0] / 10.0, rtol=1e-6)


def test_raw_abi_refusals():
    """Every refusal returns < 0, names the entry point and leaves poisoned outputs alone; the library works afterwards."""
    _ffi.init()
    lib = _ffi.lib()
    nsig, nw, hop, nframes, maxlag = 1000, 64, 32, 20, 63
    x, y = make_pair(nsig, False, 51)
    w = np.hanning(nw).astype(np.float32)
    nl = 2 * maxlag + 1
    fr = np.full((nframes, nl), 7.25, dtype=np.float32)
    av = np.full(nl, -3.5, dtype=np.float64)
    pk = np.full((nframes, 2), 11.0, dtype=np.float32)
    uneven = np.ones(128, dtype=np.float32)              # L = 128; W[3] != W[125]: refused for a real pair
    uneven[3] = 2.0
    good = dict(x=_ffi.ptr(x), y=_ffi.ptr(y), dtype=_ffi.DTYPE_F32, nsig=nsig, win=_ffi.ptr(w), nw=nw, hop=hop, nframes=nframes,
                maxlag=maxlag, detrend=_ffi.DETREND_SEGMEAN, norm=_ffi.XC_COEFF, beta=0.0, weight=None, frames=_ffi.ptr(fr),
                avg=_ffi.ptr(av), peak=_ffi.ptr(pk), mem=0)
    bad = [dict(nw=1, maxlag=0), dict(nw=0, maxlag=0), dict(maxlag=-1), dict(maxlag=64), dict(nw=4097, maxlag=4096, nsig=1 << 20, win=None),
           dict(nw=8192, maxlag=1, nsig=1 << 20, win=None), dict(hop=0), dict(hop=-3), dict(nframes=0), dict(nframes=-1),
           dict(nframes=31), dict(nsig=63), dict(nframes=1 << 40), dict(dtype=2), dict(dtype=-1), dict(detrend=_ffi.DETREND_MEAN),
           dict(detrend=_ffi.DETREND_LINEAR), dict(detrend=_ffi.DETREND_SEGLINEAR), dict(detrend=9), dict(norm=2), dict(norm=-1),
           dict(beta=-1e-3), dict(beta=float("nan")), dict(beta=float("inf")), dict(beta=1e-2, norm=_ffi.XC_RAW),
           dict(frames=None, avg=None, peak=None), dict(x=None), dict(y=None), dict(weight=_ffi.ptr(uneven))]
    for change in bad:
        args = dict(good, **change)
        rc = lib.sp_xcorr_frames(*args.values())
        msg = (lib.sp_last_error() or b"").decode()
        assert rc < 0 and "sp_xcorr_frames" in msg, (change, rc, msg)
        assert np.all(fr == 7.25) and np.all(av == -3.5) and np.all(pk == 11.0), change
    assert lib.sp_xcorr_frames(*good.values()) == 0
    ref = xcorr_frames_ref(x, y, nw, hop, nframes, maxlag, win=w)
    close(fr, ref, "the good call after the refusals")
    close(av, ref.mean(axis=0), "its avg")
    assert not np.any(pk == 11.0)
    # one output at a time leaves the others alone
    fr[:] = 7.25
    pk[:] = 11.0
    assert lib.sp_xcorr_frames(*dict(good, frames=None, peak=None).values()) == 0
    assert np.all(fr == 7.25) and np.all(pk == 11.0)
    assert lib.sp_xcorr_frames_len(nw, maxlag) == 128
