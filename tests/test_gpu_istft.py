"""GPU parity of the inverse STFT (sp_istft through engine.istft_frames / spectrogram.istft / fftanal.scipy_istft).

Reference: scipy.signal.istft in float64, fed the same complex64-rounded spectra.  Bound: max|y - ref| <= 1e-4 max|ref|, the
bound the forward STFT and the Hilbert frames are held to (test_stft_golden_f32, test_hilbert_rows); a float32 emulation of
the definition stays at or below 2e-6 on every shape here, so a structural defect (a frame dropped at a run seam, a wrong edge
envelope, a halo off by one) shows as 1e-2 or worse.  Every test prints the figure it asserts."""
import os
import warnings

import numpy as np
import pytest
import scipy.signal as ss

pytestmark = pytest.mark.gpu

TOL = 1e-4
WINDOWS = ["hann", "hamming", "blackman", ("tukey", 0.5), "boxcar"]
SHAPES = [(32, 8), (256, 64), (1024, 512), (1024, 256), (4096, 1024), (8192, 2048), (1000, 250), (3640, 910), (777, 111)]


@pytest.fixture(scope="module")
def E():
    from pyfft_amd import engine
    from pyfft_amd import _ffi
    _ffi.init()
    return engine


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def record(n, cplx, seed, nch=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nch, n)) + 3.0
    if cplx:
        x = x + 1j * (rng.standard_normal((nch, n)) - 3.0)
    return x[0] if nch == 1 else x


def spectra(x, win, nfft, hop, cplx, boundary):
    """scipy's forward STFT in float64, rounded to complex64: Zxx[..., nfreq, nseg]."""
    _, _, Z = ss.stft(x, window=win, nperseg=nfft, noverlap=nfft - hop, return_onesided=not cplx,
                      boundary="zeros" if boundary else None, padded=boundary)
    return Z.astype(np.complex64)


def scipy_inverse(Z, win, nfft, hop, cplx, boundary):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ss.istft(Z.astype(np.complex128), window=win, nperseg=nfft, noverlap=nfft - hop, input_onesided=not cplx,
                        boundary=boundary)[1]


def ours(Z, win, nfft, hop, cplx, boundary):
    from pyfft_amd import spectrogram
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return spectrogram.istft(Z, window=win, nperseg=nfft, noverlap=nfft - hop, input_onesided=not cplx, boundary=boundary)[1]


def nola(win, nfft, hop):
    return ss.check_NOLA(win, nfft, nfft - hop)


def envelope(win, nfft, hop, nseg):
    env = np.zeros((nseg - 1) * hop + nfft)
    for g in range(nseg):
        env[g * hop:g * hop + nfft] += win ** 2
    return env


def check_against_scipy(label, got, ref, win, nfft, hop, boundary):
    """boundary=True: every sample.  boundary=False: the samples whose envelope is at least 1e-3 of its maximum (where the window
    goes to zero at the ends the quotient amplifies float32 rounding by 1/w); the excluded ones are at most 4 % and lie within
    nfft of either end; samples scipy does not divide (env <= 1e-10) are compared with the absolute tolerance."""
    scale = np.max(np.abs(ref))
    err = np.abs(got - ref)
    if boundary:
        worst = float(np.max(err) / scale)
        print("%s: max rel err %.3e" % (label, worst))
        assert worst <= TOL
        return worst
    nseg = (ref.shape[-1] - nfft) // hop + 1
    env = envelope(win, nfft, hop, nseg)
    keep = env >= 1e-3 * env.max()
    tiny = env <= 1e-10
    excl = ~keep & ~tiny
    idx = np.nonzero(excl)[0]
    frac = idx.size / env.size
    worst = float(np.max(err[..., keep]) / scale)
    worst_tiny = float(np.max(err[..., tiny]) / scale) if tiny.any() else 0.0
    print("%s: max rel err %.3e on kept samples, %.3e on undivided ones, %.2f %% excluded" % (label, worst, worst_tiny, 100 * frac))
    assert frac <= 0.04
    assert np.all((idx < nfft) | (idx >= env.size - nfft))
    assert worst <= TOL and worst_tiny <= TOL
    return worst


@pytest.mark.parametrize("nfft,hop", SHAPES)
@pytest.mark.parametrize("wname", WINDOWS, ids=lambda w: w if isinstance(w, str) else w[0])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("boundary", [True, False], ids=["boundary", "noboundary"])
def test_istft_matches_scipy(E, nfft, hop, wname, cplx, boundary):
    win = ss.get_window(wname, nfft)
    if not nola(win, nfft, hop):
        pytest.skip("window / hop fail scipy's check_NOLA")
    x = record(40 * hop + nfft + 37, cplx, nfft + hop)
    Z = spectra(x, win, nfft, hop, cplx, boundary)
    ref = scipy_inverse(Z, win, nfft, hop, cplx, boundary)
    got = ours(Z, win, nfft, hop, cplx, boundary)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    check_against_scipy("%s %d/%d" % (wname, nfft, hop), got, ref, win, nfft, hop, boundary)


@pytest.mark.parametrize("nfft,hop", SHAPES)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_istft_layouts_and_batch(E, nfft, hop, cplx):
    """Frame-major and bin-major input, one and three records: all against scipy, and the layouts agree bit for bit."""
    win = ss.get_window("hann", nfft)
    x = record(40 * hop + nfft + 37, cplx, 7 * nfft + hop, nch=3)
    Z = spectra(x, win, nfft, hop, cplx, True)                       # [3, nfreq, nseg]
    ref = scipy_inverse(Z, win, nfft, hop, cplx, True)
    sided = E.SIDED_RAW if cplx else E.SIDED_HALF
    nseg = Z.shape[-1]
    skip, nout = nfft // 2, (nseg - 1) * hop + nfft - 2 * (nfft // 2)
    y_bm = E.istft_frames(Z, win, hop, sided=sided, bin_major=True, skip=skip, nout=nout)
    y_fm = E.istft_frames(np.ascontiguousarray(np.swapaxes(Z, -1, -2)), win, hop, sided=sided, bin_major=False, skip=skip, nout=nout)
    y_1 = E.istft_frames(Z[1], win, hop, sided=sided, bin_major=True, skip=skip, nout=nout)
    assert y_bm.shape == ref.shape
    worst = relerr(y_bm, ref)
    print("layouts %d/%d: max rel err %.3e" % (nfft, hop, worst))
    assert worst <= TOL
    assert np.array_equal(y_bm, y_fm)
    assert np.array_equal(y_bm[1], y_1)


@pytest.mark.parametrize("nfft,hop,wname,nseg", [(64, 64, "boxcar", 41), (64, 1, "hann", 300), (256, 64, "hann", 1),
                                                  (256, 64, "hann", 2), (1024, 256, "hamming", 1), (1000, 250, "hamming", 2),
                                                  (64, 1, "hann", 5)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_istft_corner_shapes(E, nfft, hop, wname, nseg, cplx):
    """hop = nfft, hop = 1, one frame, two frames (the two ends of the envelope meet): against scipy, boundary=False so that
    every frame count is reachable; samples compared as in check_against_scipy."""
    win = ss.get_window(wname, nfft)
    rng = np.random.default_rng(nfft + nseg)
    nb = nfft if cplx else nfft // 2 + 1
    Z = (rng.standard_normal((nb, nseg)) + 1j * rng.standard_normal((nb, nseg))).astype(np.complex64)
    ref = scipy_inverse(Z, win, nfft, hop, cplx, False)
    got = ours(Z, win, nfft, hop, cplx, False)
    assert got.shape == ref.shape
    scale = np.max(np.abs(ref))
    env = envelope(win, nfft, hop, nseg)
    keep = (env >= 1e-3 * env.max()) | (env <= 1e-10)
    worst = float(np.max(np.abs(got - ref)[keep]) / scale)
    print("corner %s %d/%d x %d: max rel err %.3e" % (wname, nfft, hop, nseg, worst))
    assert worst <= TOL


def test_istft_long_record(E):
    """2^24 samples at nfft 4096, hop 1024: many runs per workgroup row, and the bin-major input is transposed in chunks."""
    nfft, hop, n = 4096, 1024, 1 << 24
    win = ss.get_window("hann", nfft)
    x = record(n, False, 5)
    Z = spectra(x, win, nfft, hop, False, True)
    ref = scipy_inverse(Z, win, nfft, hop, False, True)
    got = ours(Z, win, nfft, hop, False, True)
    worst = relerr(got, ref)
    print("long record: max rel err %.3e over %d samples" % (worst, ref.size))
    assert got.shape == ref.shape and worst <= TOL


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("nwins,overlap", [(1024, 0.5), (1000, 0.75), (4096, 0.75)])
def test_round_trip_through_own_forward(E, cplx, nwins, overlap):
    """x -> fftanal.scipy_stft -> scipy_istft returns x within 2e-4 max|x|: two stages, each held to 1e-4."""
    from pyfft_amd import fftanal
    n = 60 * nwins + 123
    x = record(n, cplx, nwins)
    t = np.arange(n) / 1.0e3
    ft = fftanal()
    ft.init(t, x, None, nwins=nwins, windowoverlap=overlap, windowfunction="hanning", onesided=not cplx, detrend=0, verbose=False)
    assert ft.nwins == nwins
    freq, tseg, Zxx = ft.scipy_stft()
    tt, back = ft.scipy_istft(Zxx)
    assert back.shape == x.shape and tt.shape == (n,)
    worst = relerr(back, x)
    print("round trip nwins %d (%s): max rel err %.3e" % (ft.nwins, "complex" if cplx else "real", worst))
    assert worst <= 2e-4
    _, back2 = ft.scipy_istft()
    assert np.array_equal(back, back2)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_masking_matches_scipy(E, cplx):
    """Zeroing the bins above a cut and inverting equals scipy's result on the same masked spectra."""
    nfft, hop = 1024, 256
    win = ss.get_window("hann", nfft)
    x = record(40 * hop + nfft + 37, cplx, 99)
    Z = spectra(x, win, nfft, hop, cplx, True)
    f = np.abs(np.fft.fftfreq(nfft)) if cplx else np.fft.rfftfreq(nfft)
    Z[f > 0.1, :] = 0
    ref = scipy_inverse(Z, win, nfft, hop, cplx, True)
    got = ours(Z, win, nfft, hop, cplx, True)
    worst = relerr(got, ref)
    print("masking: max rel err %.3e" % worst)
    assert worst <= TOL
    assert relerr(ref[:x.size], x) > 1e-2            # the mask did remove something


def test_determinism_tensor_and_stream(E):
    import torch
    nfft, hop = 1024, 256
    win = ss.get_window("hann", nfft)
    x = record(400 * hop + nfft, False, 3)
    Z = np.ascontiguousarray(spectra(x, win, nfft, hop, False, True).T)       # [nseg, nfreq]
    a = E.istft_frames(Z, win, hop)
    b = E.istft_frames(Z, win, hop)
    assert np.array_equal(a, b)
    zt = torch.from_numpy(Z).cuda()
    c = E.istft_frames(zt, win, hop)
    torch.cuda.synchronize()
    assert c.dtype == torch.float32 and np.array_equal(c.cpu().numpy(), a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d = E.istft_frames(zt, win, hop)
    s.synchronize()
    assert np.array_equal(d.cpu().numpy(), a)
    zc = torch.from_numpy(np.ascontiguousarray(Z.T)).cuda()
    e = E.istft_frames(zc, win, hop, bin_major=True)
    torch.cuda.synchronize()
    assert np.array_equal(e.cpu().numpy(), a)


@pytest.mark.parametrize("nfft,hop,cplx", [(1024, 256, False), (1024, 256, True), (1000, 250, False), (256, 32, False),
                                           (4096, 1024, False)])
def test_partition_independence(E, nfft, hop, cplx):
    """Run lengths from below q = nfft / hop to one run for everything, and the bin-major transpose in small chunks: every
    output sample is summed by one workgroup in frame order, so the results are identical, not merely close."""
    win = ss.get_window("hann", nfft)
    x = record(200 * hop + nfft, cplx, nfft)
    Z = spectra(x, win, nfft, hop, cplx, True)
    ref = scipy_inverse(Z, win, nfft, hop, cplx, True)
    outs = {}
    try:
        for fpg in (0, 1, 2, 3, 16, 100000):
            os.environ["SP_ISTFT_FPG"] = str(fpg)
            outs[fpg] = ours(Z, win, nfft, hop, cplx, True)
        os.environ["SP_ISTFT_FPG"] = "5"
        os.environ["SP_ISTFT_MIB"] = "1"
        outs["chunks"] = ours(Z, win, nfft, hop, cplx, True)
        if not cplx:
            os.environ.pop("SP_ISTFT_FPG")
            os.environ.pop("SP_ISTFT_MIB")
            os.environ["SP_NO_REALPAIR"] = "1"
            single = ours(Z, win, nfft, hop, cplx, True)
            print("one frame per transform: max rel err %.3e" % relerr(single, ref))
            assert relerr(single, ref) <= TOL
    finally:
        for k in ("SP_ISTFT_FPG", "SP_ISTFT_MIB", "SP_NO_REALPAIR"):
            os.environ.pop(k, None)
    for k, v in outs.items():
        print("fpg %s: max rel err %.3e" % (k, relerr(v, ref)))
        assert relerr(v, ref) <= TOL
        assert np.array_equal(v, outs[0])


def test_c_level_refusals(E):
    from pyfft_amd._ffi import lib, ptr, SIDED_HALF, SIDED_RAW
    nfft, hop, M = 256, 64, 10
    win = np.hanning(nfft).astype(np.float32)
    Z = np.zeros((M, nfft // 2 + 1), np.complex64)
    total = (M - 1) * hop + nfft
    y = np.full(total, 7.0, np.float32)

    def call(Zp=Z, sided=SIDED_HALF, major=0, nch=1, nframes=M, w=win, n=nfft, h=hop, skip=0, nout=total, yp=y):
        return lib().sp_istft(ptr(Zp), sided, major, nch, nframes, ptr(w), n, h, 1.0, skip, nout, ptr(yp), 0)

    bad = [dict(sided=1), dict(sided=2), dict(sided=0), dict(major=2), dict(h=0), dict(h=nfft + 1), dict(nframes=0), dict(nch=0),
           dict(skip=-1), dict(nout=0), dict(skip=1), dict(nout=total + 1), dict(n=1 << 14), dict(n=5000), dict(n=1),
           dict(Zp=None), dict(w=None), dict(yp=None)]
    for kw in bad:
        rc = call(**kw)
        msg = lib().sp_last_error().decode()
        assert rc < 0 and "sp_istft" in msg, (kw, rc, msg)
        assert np.all(y == 7.0), kw
    assert call() == 0 and np.all(y == 0.0)
    assert call(sided=SIDED_RAW, n=nfft // 2 + 1, h=32, nout=(M - 1) * 32 + nfft // 2 + 1,
                yp=np.zeros((M - 1) * 32 + nfft // 2 + 1, np.complex64)) == 0
