"""Multitaper PSD / CSD / coherence on the GPU against the weighted sum of K scipy.signal.welch / csd calls (the oracle of
tests/test_host_multitaper.py), anchors that do not go through that oracle, the chi-square variance law, a 2^24-sample record,
bitwise repeatability, device tensors, and the C entry's refusals.

Bounds are those of the Welch parity tests (tests/test_gpu_kernels.py): PSD and eigenspectra rtol 2e-4, atol 1e-6 max(ref); cross
spectra rtol 2e-4, atol 2e-6 max|ref|; coherence 2e-4 absolute.  Every bin is compared."""
import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
from pyfft_amd import _ffi, engine as E, multitaper as MT
from test_host_multitaper import detrended, make_signal, scipy_oracle

pytestmark = pytest.mark.gpu


def assert_psd(got, ref, what=""):
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-6 * np.max(ref), err_msg=what)


def assert_cross(got, ref, what=""):
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-6 * np.max(np.abs(ref)), err_msg=what)


def coherence_of(pxx, pyy, pxy):
    den = pxx * pyy
    return np.divide(np.abs(pxy) ** 2, den, out=np.zeros_like(den), where=den > 0)


def check_case(nfft, M, K, cplx, detrend, weights, full_hop, seed):
    hop = nfft if full_hop else nfft - nfft // 3
    nsig = (M - 1) * hop + nfft + hop // 3                       # a tail shorter than a hop is ignored
    x, y = make_signal(nsig, cplx, seed), make_signal(nsig, cplx, seed + 1)
    NW = 4.0 if nfft >= 64 else 1.5
    kw = dict(fs=250.0, nfft=nfft, noverlap=nfft - hop, NW=NW, Kmax=K, weights=weights, detrend=detrend)
    plan = MT.multitaper_plan(nsig, cplx, **kw)
    assert plan["nframes"] == M and plan["tapers"].shape[0] == K
    ref = scipy_oracle(x, y, plan, detrend)
    # weighted spectra in one pass (sqrt(c_k) inside the tapers), PSD alone and the cross pair
    f, pxx = pyfft_amd.multitaper_psd(x, **kw)
    np.testing.assert_array_equal(f, plan["freq"])
    assert_psd(pxx, ref["pxx"], "pxx")
    f, pxx, pyy, pxy = pyfft_amd.multitaper_spectra(x, y, **kw)
    assert_psd(pxx, ref["pxx"], "pxx (pair)")
    assert_psd(pyy, ref["pyy"], "pyy (pair)")
    assert_cross(pxy, ref["pxy"], "pxy")
    np.testing.assert_allclose(coherence_of(pxx, pyy, pxy), coherence_of(ref["pxx"], ref["pyy"], ref["pxy"]), rtol=0, atol=2e-4)
    # eigenspectra: one taper per grid row, weights applied in float64
    f, pxx_e, skx = pyfft_amd.multitaper_psd(x, return_eigenspectra=True, **kw)
    assert skx.shape == ref["skx"].shape
    for k in range(K):
        assert_psd(skx[k], ref["skx"][k], "skx[%d]" % k)
    assert_psd(pxx_e, ref["pxx"], "pxx from eigenspectra")
    np.testing.assert_allclose(pxx_e, plan["weights"] @ skx, rtol=1e-6, atol=0)
    f, pxx_e, pyy_e, pxy_e, skx, sky = pyfft_amd.multitaper_spectra(x, y, return_eigenspectra=True, **kw)
    for k in range(K):
        assert_psd(skx[k], ref["skx"][k], "skx[%d] (pair)" % k)
        assert_psd(sky[k], ref["sky"][k], "sky[%d] (pair)" % k)
    assert_psd(pxx_e, ref["pxx"])
    assert_psd(pyy_e, ref["pyy"])
    assert_cross(pxy_e, ref["pxy"], "pxy from the per-taper cross spectra")
    f, cxy = pyfft_amd.multitaper_coherence(x, y, **kw)
    np.testing.assert_allclose(cxy, coherence_of(ref["pxx"], ref["pyy"], ref["pxy"]), rtol=0, atol=2e-4)
    assert np.all(cxy >= 0) and np.all(cxy <= 1 + 1e-5)
    f, pxy_c = pyfft_amd.multitaper_csd(x, y, **kw)
    assert_cross(pxy_c, ref["pxy"])


# (nfft, frames, K, kind, detrend, weights, hop = nfft?): the grid of nfft x frames x K x kind x detrend x weights x hop, thinned so that
# every value of every axis occurs, odd and even K at power-of-two real shapes, and both kinds at a chirp-z length
GRID = [
    (8, 1, 1, "real", "none", "unity", False), (8, 300, 2, "cplx", "mean", "eigen", True), (8, 33, 2, "real", "linear", "unity", False),
    (64, 2, 5, "real", "mean", "eigen", False), (64, 300, 7, "cplx", "linear", "unity", False), (64, 33, 2, "real", "none", "eigen", True),
    (257, 33, 5, "real", "mean", "unity", False), (257, 2, 7, "cplx", "none", "eigen", True), (257, 1, 2, "real", "linear", "eigen", False),
    (1000, 300, 7, "real", "mean", "eigen", False), (1000, 2, 1, "cplx", "linear", "unity", True), (1000, 33, 5, "cplx", "mean", "unity", False),
    (1024, 33, 7, "real", "mean", "unity", False), (1024, 33, 2, "real", "linear", "eigen", True), (1024, 1, 5, "real", "none", "unity", False),
    (1024, 300, 5, "cplx", "mean", "eigen", False), (1024, 2, 1, "real", "mean", "unity", True), (1024, 2, 2, "cplx", "none", "unity", True),
    (2047, 2, 5, "real", "none", "unity", False), (2047, 33, 2, "cplx", "mean", "eigen", True), (2047, 1, 7, "real", "linear", "eigen", False),
    (4096, 300, 7, "real", "mean", "unity", False), (4096, 33, 2, "real", "none", "eigen", True), (4096, 2, 5, "cplx", "linear", "unity", False),
    (4096, 1, 1, "cplx", "mean", "eigen", True),
    (8192, 33, 5, "real", "mean", "eigen", False), (8192, 2, 2, "cplx", "mean", "unity", True), (8192, 1, 7, "real", "linear", "unity", False),
    (8192, 300, 1, "real", "none", "unity", True),
]


@pytest.mark.parametrize("nfft,M,K,kind,detrend,weights,full_hop", GRID)
def test_parity_with_scipy(nfft, M, K, kind, detrend, weights, full_hop):
    check_case(nfft, M, K, kind == "cplx", detrend, weights, full_hop, seed=nfft + 7 * M + K)


def test_explicit_weights_with_a_zero():
    nfft, nsig = 512, 512 * 20
    x, y = make_signal(nsig, False, 21), make_signal(nsig, False, 22)
    kw = dict(fs=1.0, nfft=nfft, noverlap=256, NW=3.0, Kmax=5, weights=[3.0, 0.0, 1.0, 2.5, 0.5], detrend="mean")
    plan = MT.multitaper_plan(nsig, False, **kw)
    ref = scipy_oracle(x, y, plan, "mean")
    f, pxx, pyy, pxy = pyfft_amd.multitaper_spectra(x, y, **kw)
    assert_psd(pxx, ref["pxx"])
    assert_psd(pyy, ref["pyy"])
    assert_cross(pxy, ref["pxy"])
    f, pxx_e, skx = pyfft_amd.multitaper_psd(x, return_eigenspectra=True, **kw)
    assert_psd(pxx_e, ref["pxx"])
    assert_psd(skx[1], ref["skx"][1], "the eigenspectrum of the taper of weight 0")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("nfft,noverlap", [(1024, 512), (1000, 0), (4096, 2048)])
def test_one_hann_taper_is_welch(cplx, nfft, noverlap):
    """K = 1 with a Hann row is scipy.signal.welch with that window, and the package's own Welch PSD."""
    nsig = nfft * 40 + 11
    x = make_signal(nsig, cplx, 31)
    win = ss.get_window("hann", nfft)
    f, pxx = pyfft_amd.multitaper_psd(x, fs=50.0, nfft=nfft, noverlap=noverlap, tapers=win[None, :], detrend="mean")
    xd = x - np.mean(x)
    fr, ref = ss.welch(xd, fs=50.0, window="hann", nperseg=nfft, noverlap=noverlap, detrend=False, return_onesided=not cplx,
                       scaling="density")
    np.testing.assert_array_equal(f, fr)
    assert_psd(pxx, ref)
    hop = nfft - noverlap
    M = 1 + (nsig - nfft) // hop
    own = E.welch_psd(x, win, hop, M, detrend=True, sided=E.SIDED_RAW, scale=1.0 / (50.0 * np.sum(win ** 2)))
    if not cplx:                                # bins 0 .. nfft/2 of the raw spectrum (the numpy rfft layout), then doubled
        own = own[:nfft // 2 + 1] * MT.multitaper_plan(nsig, False, nfft=nfft)["fold"]
    assert_psd(pxx, own)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("nfft", [256, 1000])
def test_self_coherence_and_bounds(cplx, nfft):
    nsig = nfft * 12
    x, y = make_signal(nsig, cplx, 41), make_signal(nsig, cplx, 42)
    f, pxx = pyfft_amd.multitaper_psd(x, nfft=nfft, noverlap=nfft // 2, NW=3.0)
    f, cxx = pyfft_amd.multitaper_coherence(x, x, nfft=nfft, noverlap=nfft // 2, NW=3.0)
    keep = pxx > 1e-12 * pxx.max()
    np.testing.assert_allclose(cxx[keep], 1.0, rtol=0, atol=1e-5)
    f, cxy = pyfft_amd.multitaper_coherence(x, y, nfft=nfft, noverlap=nfft // 2, NW=3.0)
    assert np.all(cxy >= 0) and np.all(cxy <= 1 + 1e-5)
    f, pxx_e, sk = pyfft_amd.multitaper_psd(x, nfft=nfft, noverlap=nfft // 2, NW=3.0, weights="eigen", return_eigenspectra=True)
    c = MT.multitaper_plan(nsig, cplx, nfft=nfft, noverlap=nfft // 2, NW=3.0, weights="eigen")["weights"]
    np.testing.assert_allclose(pxx_e, c @ sk, rtol=1e-6, atol=0)


@pytest.mark.parametrize("K", [1, 7])
def test_variance_follows_chi_square(K):
    """Pxx of white noise is chi-square with 2K degrees of freedom: K x (relative variance across 64 independent records), averaged
    over the interior bins, is 1 within 15 % (five times the scatter of a correct estimator over seeds)."""
    nfft, nrec = 1024, 64
    rng = np.random.default_rng(2024)
    P = np.array([pyfft_amd.multitaper_psd(rng.standard_normal(nfft), NW=4.0, Kmax=K)[1] for _ in range(nrec)])
    relvar = np.var(P, axis=0, ddof=1) / np.mean(P, axis=0) ** 2
    figure = K * float(np.mean(relvar[8:nfft // 2 - 8 + 1]))
    print("K = %d: K x mean relative variance = %.4f" % (K, figure))
    assert abs(figure - 1.0) <= 0.15


def test_long_record_and_bitwise_repeatability():
    """2^24 real samples, nfft 4096, 50 % overlap, K = 7: parity, and the same call twice agrees bit for bit."""
    nsig, nfft = 1 << 24, 4096
    x, y = make_signal(nsig, False, 51), make_signal(nsig, False, 52)
    kw = dict(fs=1000.0, nfft=nfft, noverlap=nfft // 2, NW=4.0, Kmax=7)
    plan = MT.multitaper_plan(nsig, False, **kw)
    ref = scipy_oracle(x, y, plan, "mean")
    a = pyfft_amd.multitaper_spectra(x, y, return_eigenspectra=True, **kw)
    b = pyfft_amd.multitaper_spectra(x, y, return_eigenspectra=True, **kw)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    f, pxx, pyy, pxy, skx, sky = a
    assert_psd(pxx, ref["pxx"])
    assert_psd(pyy, ref["pyy"])
    assert_cross(pxy, ref["pxy"])
    for k in range(7):
        assert_psd(skx[k], ref["skx"][k], "skx[%d]" % k)
        assert_psd(sky[k], ref["sky"][k], "sky[%d]" % k)
    c = pyfft_amd.multitaper_spectra(x, y, **kw)
    d = pyfft_amd.multitaper_spectra(x, y, **kw)
    for u, v in zip(c, d):
        np.testing.assert_array_equal(u, v)
    assert_psd(c[1], ref["pxx"])
    assert_psd(c[2], ref["pyy"])
    assert_cross(c[3], ref["pxy"])
    p1, p2 = pyfft_amd.multitaper_psd(x, **kw)[1], pyfft_amd.multitaper_psd(x, **kw)[1]
    np.testing.assert_array_equal(p1, p2)
    assert_psd(p1, ref["pxx"])


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_device_tensors_give_the_same_values(cplx):
    import torch
    nfft, nsig = 1024, 1024 * 50 + 100
    x, y = make_signal(nsig, cplx, 61), make_signal(nsig, cplx, 62)
    dt = torch.complex64 if cplx else torch.float32
    xt, yt = torch.as_tensor(x).to(dt).cuda(), torch.as_tensor(y).to(dt).cuda()
    kw = dict(fs=10.0, nfft=nfft, noverlap=512, NW=4.0, weights="eigen", detrend="linear")
    host = pyfft_amd.multitaper_spectra(x, y, return_eigenspectra=True, **kw)
    dev = pyfft_amd.multitaper_spectra(xt, yt, return_eigenspectra=True, **kw)
    np.testing.assert_array_equal(host[0], dev[0])
    for h, d in zip(host[1:], dev[1:]):
        assert isinstance(d, torch.Tensor) and d.is_cuda
        np.testing.assert_allclose(d.cpu().numpy(), h, rtol=1e-12, atol=0)
    fh, ch = pyfft_amd.multitaper_coherence(x, y, **kw)
    fd, cd = pyfft_amd.multitaper_coherence(xt, yt, **kw)
    np.testing.assert_allclose(cd.cpu().numpy(), ch, rtol=1e-12, atol=1e-15)
    ph, pd = pyfft_amd.multitaper_psd(x, **kw)[1], pyfft_amd.multitaper_psd(xt, **kw)[1]
    np.testing.assert_allclose(pd.cpu().numpy(), ph, rtol=1e-12, atol=0)


def test_c_entry_refusals():
    lib = _ffi.load_library()
    nsig, nfft = 4096, 256
    x = np.zeros(nsig, np.float32)
    tp = np.ones((33, nfft), np.float32)
    big = np.ones((1, 16384), np.float32)
    out = np.zeros(16384, np.float64)

    def call(tapers=tp, K=2, nfft=nfft, hop=128, nframes=4, nsig=nsig, dtype=0, detrend=1, weights=None, skx=None):
        return lib.sp_multitaper(_ffi.ptr(x), None, dtype, nsig, _ffi.ptr(tapers), K, nfft, hop, nframes, detrend, None, None,
                                 _ffi.ptr(weights), 1.0, _ffi.ptr(out), None, None, _ffi.ptr(skx), None, 0)
    bad = [dict(K=0), dict(K=33), dict(nfft=16384, tapers=big, K=1, nsig=1 << 15), dict(nfft=4100, tapers=big, K=1), dict(nfft=4),
           dict(hop=0), dict(nframes=0), dict(nframes=32), dict(nframes=31, hop=128, nsig=4095), dict(dtype=2), dict(detrend=3),
           dict(weights=np.array([1.0, -1.0]), skx=out), dict(weights=np.array([0.0, 0.0]), skx=out), dict(weights=np.array([1.0, 1.0]))]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert lib.sp_last_error(), kw
    assert call() == 0                                           # the same arguments, in range: accepted
