"""Host side of the short-time cross-correlation (ccf_sh, ccf_frames, delay_track): the float64 oracle from the definition's direct lag
sums, against np.correlate, against the zero-padded FFT form at the library's transform length, the real-pair identity the kernel
separates its two records with, the peak formula, the band tables, every Python-side refusal before the library loads, and the
declaration and binding of sp_xcorr_frames / sp_xcorr_frames_len.  No GPU needed.  tests/test_gpu_xcorr_frames.py imports the oracle,
the inputs and the shapes from here."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import pyfft_amd
from pyfft_amd import _ffi, _ccf_mod as CC         # (pyfft_amd.ccf is the function)
from test_host_multitaper import no_library        # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nav, maxlag, hop, complex): the transform lengths 32 .. 8192, a window that is no power of two, ragged hops
SHAPES = [(16, 15, 5, False), (24, 23, 7, False), (64, 63, 32, False), (100, 99, 37, False), (256, 64, 128, True),
          (1000, 999, 500, False), (3000, 200, 1500, True), (4096, 4095, 2048, False), (4096, 4095, 2048, True)]
SHAPE_L = [32, 64, 128, 256, 512, 2048, 4096, 8192, 8192]
SHAPE_IDS = ["%d-%d-%d-%s" % (n, m, h, "cplx" if c else "real") for n, m, h, c in SHAPES]


def xc_len(nw, maxlag):
    """L from the library's own sp_xcorr_frames_len where it is built (host only, no device), else from the Python plan."""
    L = CC.ccf_plan(nw, maxlag)["L"]
    if os.path.exists(_ffi.LIB_PATH):
        assert ctypes.CDLL(_ffi.LIB_PATH).sp_xcorr_frames_len(int(nw), int(maxlag)) == L
    return L


def make_pair(nsig, cplx, seed, d=5):
    """The same noise sequence shifted by d samples, plus independent noise and different offsets, rounded to what the device sees:
    x = s[n + d] + 0.3 noise + 1.5, y = s[n] + 0.3 noise - 0.7."""
    rng = np.random.default_rng(seed)

    def noise(n):
        return rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
    s = noise(nsig + d)
    x = s[d:] + 0.3 * noise(nsig) + 1.5
    y = s[:nsig] + 0.3 * noise(nsig) - 0.7
    return _ffi.as_samples(x), _ffi.as_samples(y)


def frames_of(x, nw, hop, nframes, win, segmean):
    """[nframes, nw] float64 / complex128: the windows, their own means removed, tapered."""
    x = np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    a = np.lib.stride_tricks.sliding_window_view(x, nw)[::hop][:nframes].copy()
    assert a.shape == (nframes, nw)
    if segmean:
        a -= a.mean(axis=1, keepdims=True)
    if win is not None:
        a *= np.asarray(win, dtype=np.float64)
    return a


def direct_lags(a, b, maxlag):
    """c[g, l + maxlag] = sum_n a[g, n + l] conj(b[g, n]): the lag sums as they are written, no transform."""
    nfr, nw = a.shape
    out = np.zeros((nfr, 2 * maxlag + 1), dtype=np.result_type(a, b))
    bc = np.conj(b)
    if 2 * maxlag + 1 <= 1024 or nfr > 64:
        for l in range(-maxlag, maxlag + 1):                                  # one lag at a time, all frames at once
            lo, hi = max(0, -l), min(nw, nw - l)
            out[:, l + maxlag] = np.sum(a[:, lo + l:hi + l] * bc[:, lo:hi], axis=1)
        return out
    cut = slice(nw - 1 - maxlag, nw + maxlag)
    for g in range(nfr):                                                      # np.correlate: the same sums in C, real parts at a time
        if np.iscomplexobj(out):
            ar, ai, br, bi = a[g].real, a[g].imag, b[g].real, b[g].imag
            re = np.correlate(ar, br, "full") + np.correlate(ai, bi, "full")
            im = np.correlate(ai, br, "full") - np.correlate(ar, bi, "full")
            out[g] = (re + 1j * im)[cut]
        else:
            out[g] = np.correlate(a[g], b[g], "full")[cut]
    return out


def spectral_lags(a, b, maxlag, L, E, coeff, beta, weight):
    """The definition's FFT form at the transform length L, float64."""
    S = np.fft.fft(a, L, axis=1) * np.conj(np.fft.fft(b, L, axis=1))
    W = np.ones(L) if weight is None else np.asarray(weight, dtype=np.float64)
    if beta > 0:
        den = np.abs(S) + beta * E[:, None]
        S = W * np.divide(S, den, out=np.zeros_like(S), where=den > 0)
    else:
        S = W * S
    c = np.fft.ifft(S, axis=1)
    if beta == 0 and coeff:
        c = np.divide(c, E[:, None], out=np.zeros_like(c), where=E[:, None] > 0)
    c = np.concatenate([c[:, L - maxlag:], c[:, :maxlag + 1]], axis=1)
    return c if np.iscomplexobj(a) else c.real


def xcorr_frames_ref(x, y, nw, hop, nframes, maxlag, win=None, segmean=True, coeff=True, beta=0.0, weight=None, L=None):
    """The float64 oracle of sp_xcorr_frames -> frames [nframes, 2 maxlag + 1].  Without a spectral weighting (beta = 0, weight None)
    the direct lag sums; with one, the definition is spectral and needs L."""
    a, b = frames_of(x, nw, hop, nframes, win, segmean), frames_of(y, nw, hop, nframes, win, segmean)
    E = np.sqrt(np.sum(np.abs(a) ** 2, axis=1) * np.sum(np.abs(b) ** 2, axis=1))
    if beta == 0 and weight is None:
        c = direct_lags(a, b, maxlag)
        return np.divide(c, E[:, None], out=np.zeros_like(c), where=E[:, None] > 0) if coeff else c
    return spectral_lags(a, b, maxlag, xc_len(nw, maxlag) if L is None else L, E, coeff, beta, weight)


def peak_ref(c, maxlag):
    """The peak formula on rows of lags -> (lstar, delta, height, gap, curvature): gap = the top minus the runner-up, curvature =
    |d| (0 at the ends of the lag range), both for choosing the frames a float32 result can be held to."""
    q = np.abs(c) if np.iscomplexobj(c) else np.asarray(c, dtype=np.float64)
    nfr = q.shape[0]
    i = np.argmax(q, axis=1)                                                  # the first maximum: the smallest lag
    rows = np.arange(nfr)
    top = q[rows, i]
    inner = (i > 0) & (i < 2 * maxlag)
    qm, qp = q[rows, np.maximum(i - 1, 0)], q[rows, np.minimum(i + 1, 2 * maxlag)]
    d = np.where(inner, qm - 2 * top + qp, 0.0)
    ok = inner & (d < 0)
    delta = np.where(ok, 0.5 * (qm - qp) / np.where(ok, d, 1.0), 0.0)
    height = top - 0.25 * (qm - qp) * delta
    masked = q.copy()
    masked[rows, i] = -np.inf
    gap = top - masked.max(axis=1) if q.shape[1] > 1 else top
    return i - maxlag, delta, height, gap, np.abs(d)


@functools.lru_cache(maxsize=None)
def shape_case(k, nframes, seed=7):
    """Inputs and the direct-sum references (coeff and raw) of shape k at a frame count, computed once and shared."""
    nw, maxlag, hop, cplx = SHAPES[k]
    x, y = make_pair((nframes - 1) * hop + nw + 3, cplx, seed + k)
    raw = xcorr_frames_ref(x, y, nw, hop, nframes, maxlag, coeff=False)
    a, b = frames_of(x, nw, hop, nframes, None, True), frames_of(y, nw, hop, nframes, None, True)
    E = np.sqrt(np.sum(np.abs(a) ** 2, axis=1) * np.sum(np.abs(b) ** 2, axis=1))
    for arr in (x, y, raw, E):
        arr.setflags(write=False)
    return x, y, raw, E


def test_exported():
    for name in ("ccf", "ccf_sh", "ccf_frames", "delay_track", "ccf_plan"):
        assert getattr(pyfft_amd, name) is getattr(CC, name)
    assert callable(pyfft_amd.engine.xcorr_frames)


@pytest.mark.parametrize("n", [16, 100, 777])
def test_one_window_equals_np_correlate(n):
    """One window of the oracle is the reference's ccf: correlate(a - mean, b - mean, 'full') / (n std std)."""
    x, y = make_pair(n, False, 3)
    x, y = x.astype(np.float64), y.astype(np.float64)
    got = xcorr_frames_ref(x, y, n, n, 1, n - 1)[0]
    ref = np.correlate(x - x.mean(), y - y.mean(), "full") / (n * x.std() * y.std())
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 1e-12
    if n >= 100:
        assert np.argmax(got) - (n - 1) == -5                                 # x[n] = s[n + 5] and y[n] = s[n]: a[n + l] meets b[n] at l = -5


def test_real_pair_identity():
    """With Z = FFT(a + i b), P = Z[k], Q = conj(Z[L - k]):  A conj(B) = Im(P conj Q) / 2 + i (|P|^2 - |Q|^2) / 4."""
    rng = np.random.default_rng(5)
    for L in (32, 64, 256):
        a, b = rng.standard_normal(L), rng.standard_normal(L)
        a[L // 2 + 3:] = 0
        b[L // 2 + 3:] = 0
        Z = np.fft.fft(a + 1j * b)
        P, Q = Z, np.conj(Z[(-np.arange(L)) % L])
        S = 0.5 * np.imag(P * np.conj(Q)) + 0.25j * (np.abs(P) ** 2 - np.abs(Q) ** 2)
        ref = np.fft.fft(a) * np.conj(np.fft.fft(b))
        assert np.max(np.abs(S - ref)) <= 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_fft_form_equals_direct_sums(k):
    nw, maxlag, hop, cplx = SHAPES[k]
    L = xc_len(nw, maxlag)
    assert L == SHAPE_L[k] == max(32, 1 << (nw + maxlag - 1).bit_length())
    x, y, raw, E = shape_case(k, 3)
    a, b = frames_of(x, nw, hop, 3, None, True), frames_of(y, nw, hop, 3, None, True)
    for coeff in (False, True):
        got = spectral_lags(a, b, maxlag, L, E, coeff, 0.0, None)
        ref = raw / E[:, None] if coeff else raw
        assert got.dtype == ref.dtype and np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref))
    # a taper, and no mean removal
    w = np.hanning(nw)
    ref = xcorr_frames_ref(x, y, nw, hop, 3, maxlag, win=w, segmean=False)
    a, b = frames_of(x, nw, hop, 3, w, False), frames_of(y, nw, hop, 3, w, False)
    E2 = np.sqrt(np.sum(np.abs(a) ** 2, axis=1) * np.sum(np.abs(b) ** 2, axis=1))
    assert np.max(np.abs(spectral_lags(a, b, maxlag, L, E2, True, 0.0, None) - ref)) <= 1e-11 * np.max(np.abs(ref))
    # an all-ones weight is no weight; the zero frame gives zero, PHAT or not
    np.testing.assert_allclose(xcorr_frames_ref(x, y, nw, hop, 3, maxlag, weight=np.ones(L)), raw / E[:, None], rtol=0,
                               atol=1e-11 * np.max(np.abs(raw / E[:, None])))
    z = np.zeros(nw + 2 * hop, dtype=x.dtype)
    assert not np.any(xcorr_frames_ref(z, z, nw, hop, 3, maxlag)) and not np.any(xcorr_frames_ref(z, z, nw, hop, 3, maxlag, beta=1e-2))


def test_len_function():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    f = ctypes.CDLL(_ffi.LIB_PATH).sp_xcorr_frames_len
    for (nw, maxlag, _, _), L in zip(SHAPES, SHAPE_L):
        assert f(nw, maxlag) == L
    assert f(2, 0) == 32 and f(2, 1) == 32 and f(17, 15) == 32 and f(17, 16) == 64 and f(4097, 4095) == 8192 and f(8192, 0) == 8192
    for nw, maxlag in ((1, 0), (0, 0), (16, -1), (16, 16), (4097, 4096), (8192, 1), (8193, 0)):
        assert f(nw, maxlag) < 0


def test_peak_formula():
    # an interior top: the vertex of the parabola through the three points
    c = np.array([[0.0, 1.0, 4.0, 3.0, 0.0]])
    l, dl, h, gap, curv = peak_ref(c, 2)
    d = 1.0 - 8.0 + 3.0
    assert l[0] == 0 and np.isclose(dl[0], 0.5 * (1.0 - 3.0) / d) and np.isclose(h[0], 4.0 - 0.25 * (1.0 - 3.0) * dl[0])
    assert np.isclose(gap[0], 1.0) and np.isclose(curv[0], 4.0)
    # a parabola sampled at the integers is recovered exactly
    ll = np.arange(-6, 7)
    l, dl, h, _, _ = peak_ref((3.0 - 0.2 * (ll - 1.3) ** 2)[None, :], 6)
    assert l[0] == 1 and np.isclose(l[0] + dl[0], 1.3) and np.isclose(h[0], 3.0)
    # the ends of the lag range: delta = 0, the height is the sample
    for row, want in (([5.0, 1.0, 0.0], -1), ([0.0, 1.0, 5.0], 1)):
        l, dl, h, _, _ = peak_ref(np.array([row]), 1)
        assert l[0] == want and dl[0] == 0.0 and h[0] == 5.0
    # a plateau: the smallest lag of the top; one that starts at the end of the range, or a flat row (d = 0 is not < 0): delta = 0
    l, dl, h, gap, _ = peak_ref(np.array([[2.0, 2.0, 2.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0, 1.0]]), 2)
    assert l[0] == -2 and l[1] == -2 and not np.any(dl) and h[0] == 2.0 and h[1] == 1.0 and not np.any(gap)
    # the left shoulder of a plateau inside the range has d < 0: delta follows the formula, towards the plateau
    l, dl, _, gap, _ = peak_ref(np.array([[0.0, 0.0, 2.0, 2.0, 0.0]]), 2)
    assert l[0] == 0 and np.isclose(dl[0], 0.5 * (0.0 - 2.0) / (0.0 - 4.0 + 2.0)) and gap[0] == 0.0
    # maxlag = 0: one lag
    l, dl, h, _, _ = peak_ref(np.array([[0.7]]), 0)
    assert l[0] == 0 and dl[0] == 0 and h[0] == 0.7
    # complex rows: the modulus
    l, dl, h, _, _ = peak_ref(np.array([[1j, -3.0, 2.0 + 0j]]), 1)
    assert l[0] == 0 and np.isclose(h[0], 3.0 - 0.25 * (1.0 - 2.0) * dl[0])


def test_band_tables_and_even_weight(no_library):
    L, fs = 64, 128.0
    W = CC.band_weight(L, fs, (10.0, 20.0))
    f = np.abs(np.fft.fftfreq(L, 1 / fs))
    assert W.dtype == np.float32 and W.shape == (L,)
    np.testing.assert_array_equal(W, ((f >= 10.0) & (f <= 20.0)).astype(np.float32))
    assert W[0] == 0 and W[5] == 1 and W[10] == 1 and W[11] == 0 and np.array_equal(W[1:], W[1:][::-1])
    assert CC.band_weight(L, fs, (0.0, fs)).all()
    for bad in ((5.0,), (20.0, 10.0), (-1.0, 5.0), (0.0, np.inf), 3.0):
        with pytest.raises(ValueError):
            CC.band_weight(L, fs, bad)
    x = np.zeros(200)
    odd = np.ones(128)
    odd[3] = 2.0
    with pytest.raises(ValueError) as ei:
        CC.ccf_sh(x, x, 1.0, 64, weight=odd)
    assert "even" in str(ei.value)
    # a complex pair may carry a one-sided weight: the check is for real input only, so this one gets as far as the library
    with pytest.raises(AssertionError):
        CC.ccf_sh(x + 0j, x + 0j, 1.0, 64, weight=odd)


def test_plan():
    p = CC.ccf_plan(1024, 128)
    assert p == dict(L=2048, nlags=257, transforms=2, read=8192, written=dict(frames=1028, avg=0, peak=8))
    p = CC.ccf_plan(100, cplx=True)
    assert p["L"] == 256 and p["nlags"] == 199 and p["transforms"] == 3 and p["read"] == 1600 and p["written"]["frames"] == 1592
    for (nw, maxlag, _, _), L in zip(SHAPES, SHAPE_L):
        assert CC.ccf_plan(nw, maxlag)["L"] == L


X200, C200 = np.zeros(200), np.zeros(200, complex)
REFUSALS = [
    (dict(nav=1), "nav must be at least 2"),
    (dict(maxlag=64), "maxlag"),
    (dict(maxlag=-1), "maxlag"),
    (dict(nav=300), "shorter than nav"),
    (dict(hop=0), "hop must be at least 1"),
    (dict(fs=0.0), "fs must be positive"),
    (dict(fs=np.inf), "fs must be positive"),
    (dict(x1=np.zeros((2, 100))), "one-dimensional"),
    (dict(x2=np.zeros(199)), "equal lengths"),
    (dict(x2=C200), "both be real or both be complex"),
    (dict(window=np.ones(63)), "window must be"),
    (dict(window=np.r_[np.nan, np.ones(63)]), "finite"),
    (dict(detrend="linear"), "detrend"),
    (dict(norm="power"), "norm must be one of"),
    (dict(phat=-1e-3), "phat"),
    (dict(phat=np.nan), "phat"),
    (dict(phat=1e-2, norm="raw"), "norm='coeff'"),
    (dict(phat=1e-2, norm="biased"), "norm='coeff'"),
    (dict(weight=np.ones(64)), "weight must hold L = 128"),
    (dict(weight=np.r_[np.inf, np.ones(127)]), "finite"),
    (dict(band=(30.0, 10.0)), "band"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_before_the_library(no_library, kw, text):
    kw = dict(kw)
    x1, x2, fs, nav = kw.pop("x1", X200), kw.pop("x2", X200), kw.pop("fs", 100.0), kw.pop("nav", 64)
    for fn in (CC.ccf_sh, CC.ccf_frames, CC.delay_track):
        with pytest.raises(ValueError) as ei:
            fn(x1, x2, fs, nav, **kw)
        assert text in str(ei.value) or (fn is CC.delay_track and kw.get("norm") == "biased")


def test_too_long_is_value_and_not_implemented(no_library):
    x = np.zeros(10000)
    for fn in (CC.ccf_sh, CC.ccf_frames, CC.delay_track):
        for nav, maxlag in ((4097, None), (8192, 1), (5000, 3193)):
            with pytest.raises(NotImplementedError) as ei:
                fn(x, x, 1.0, nav, maxlag=maxlag)
            assert isinstance(ei.value, ValueError) and "beyond one workgroup transform" in str(ei.value)
    with pytest.raises(NotImplementedError):
        CC.ccf_plan(8192, 1)
    for norm in ("biased", "unbiased"):
        with pytest.raises(ValueError) as ei:
            CC.delay_track(x, x, 1.0, 64, norm=norm)
        assert "delay_track" in str(ei.value)


def test_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("sp_xcorr_frames", 17), ("sp_xcorr_frames_len", 2)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt, "%s is not declared in include/spectral.h" % name
        nargs = len([a for a in mt.group(1).split(",") if a.strip()])
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs == want
        assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    assert re.search(r"#define SP_XC_RAW 0\b", hdr) and re.search(r"#define SP_XC_COEFF 1\b", hdr)
    assert (_ffi.XC_RAW, _ffi.XC_COEFF) == (0, 1)
