"""Host side of the digital down-converter and the band spectra: the float64 oracle ddc_ref (oscillator phases reduced modulo one turn
in exact rational arithmetic) against scipy.signal.resample_poly, the filter plans and their composite responses, every refusal that
comes before the library loads, and the declaration and binding of sp_ddc.  No GPU needed.  tests/test_gpu_baseband.py imports ddc_ref
and cascade_ref from here."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
from pyfft_amd import baseband as BB
from test_host_multitaper import make_signal, no_library        # noqa: F401  (no_library: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_turns(nu, n0, n):
    """(nu (n0 + i)) mod 1 in [-1/2, 1/2) for i < n, exact: nu is a dyadic rational a / b, and the integers a (n0 + i) mod b divide
    correctly rounded."""
    fr = Fraction(nu)
    a, b = fr.numerator, fr.denominator
    r = (a * n0) % b
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        out[i] = r / b
        r = (r + a) % b
    out[out >= 0.5] -= 1.0
    return out


def ddc_ref(x, nu, q, h, n0=0):
    """The definition along the last axis, float64: v[n] = x[n] exp(-2 pi i nu (n0 + n)), 0 outside the row;
    y[k] = sum_j h[j] v[k q + (T - 1) / 2 - j], k < ceil(n / q)."""
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, T = x.shape[-1], h.size
    assert T % 2 == 1
    v = x * np.exp(-2j * np.pi * exact_turns(nu, n0, n))
    rows = v.reshape(-1, n)
    nout = -(-n // q)
    pick = np.arange(nout) * q + (T - 1) // 2
    out = np.array([np.convolve(row, h)[pick] for row in rows])
    return out.reshape(x.shape[:-1] + (nout,))


def cascade_ref(x, nu, stages, n0=0):
    """ddc_ref stage by stage: the first mixes, the others only filter and decimate."""
    y = x
    for i, (qi, h) in enumerate(stages):
        y = ddc_ref(y, nu if i == 0 else 0.0, qi, h, n0 if i == 0 else 0)
    return y


def test_exported():
    for name in ("ddc", "ddc_plan", "band_stft", "band_psd", "band_csd", "band_coherence", "band_plan"):
        assert getattr(pyfft_amd, name) is getattr(BB, name)
    assert callable(pyfft_amd.engine.ddc) and callable(pyfft_amd.engine.ddc_tile)


@pytest.mark.parametrize("n,q,T", [(1000, 4, 33), (1001, 7, 57), (257, 16, 129), (64, 8, 65)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_ddc_ref_equals_resample_poly(n, q, T, cplx):
    x = make_signal(2 * n, cplx, 41).reshape(2, n)
    h = ss.firwin(T, 0.8 / q)
    nu, n0 = 1977.0 / 16384.0, 77                                               # dyadic: nu (n0 + n) and its reduction are exact in float64
    t = (nu * (n0 + np.arange(n))) % 1.0
    v = x * np.exp(-2j * np.pi * np.where(t >= 0.5, t - 1.0, t))
    ref = ss.resample_poly(v, 1, q, axis=-1, window=h)
    got = ddc_ref(x, nu, q, h, n0)
    assert got.shape == ref.shape == (2, -(-n // q))
    err = float(np.max(np.abs(got - ref)))
    print("n %d q %d T %d: max |ddc_ref - resample_poly| = %.3g" % (n, q, T, err))
    assert err <= 1e-14


def test_exact_turns():
    for nu in (0.25, 0.3 / 116508, -0.013, np.sqrt(2.0) - 1.0, 1e-9):
        for n0 in (0, (1 << 24) - 3, (1 << 31) + 5, (1 << 40) - 4096):
            got = exact_turns(nu, n0, 5)
            for i in range(5):
                t = (Fraction(nu) * (n0 + i)) % 1
                t = t - 1 if t >= Fraction(1, 2) else t
                assert abs(got[i] - float(t)) <= 2.3e-16                        # one rounding more than float(t): the shift by 1


def test_plan_stages():
    want = {1: [1], 2: [2], 8: [8], 64: [64], 256: [64, 4], 4096: [64, 64], 130: [26, 5], 63 * 64: [64, 63], 3 * 61: [61, 3]}
    for q, factors in want.items():
        st = BB.ddc_plan(q)
        assert [qi for qi, _ in st] == factors and int(np.prod(factors)) == q
        for _, h in st:
            assert h.dtype == np.float64 and h.size % 2 == 1 and h.size <= 4095
            np.testing.assert_allclose(h, h[::-1], rtol=0, atol=1e-15)          # linear phase
            np.testing.assert_allclose(h.sum(), 1.0, rtol=1e-12)
    # the tap counts of a single stage at the defaults
    assert [BB.ddc_plan(q)[0][1].size for q in (2, 8, 64)] == [117, 459, 3659]
    # the caller's own taps: one stage, kept as they are
    h = ss.firwin(33, 0.1)
    (q, got), = BB.ddc_plan(8, taps=h)
    assert q == 8 and got.dtype == np.float64 and np.array_equal(got, h)


def test_plan_refusals():
    for q in (67, 2 * 67, 64 * 71):
        with pytest.raises(NotImplementedError) as ei:
            BB.ddc_plan(q)
        assert isinstance(ei.value, ValueError) and "prime factor" in str(ei.value)
    for call, text in ((lambda: BB.ddc_plan(0), "positive integer"),
                       (lambda: BB.ddc_plan(-4), "positive integer"),
                       (lambda: BB.ddc_plan(2.5), "positive integer"),
                       (lambda: BB.ddc_plan(8, taps=np.ones(32)), "odd length"),
                       (lambda: BB.ddc_plan(8, taps=np.ones((3, 3))), "odd length"),
                       (lambda: BB.ddc_plan(8, taps=np.ones(33) * 1j), "real"),
                       (lambda: BB.ddc_plan(8, taps=np.r_[np.nan, np.ones(32)]), "finite"),
                       (lambda: BB.ddc_plan(8, width=0.0), "width"),
                       (lambda: BB.ddc_plan(8, width=1.0), "width"),
                       (lambda: BB.ddc_plan(8, width=-0.2), "width"),
                       (lambda: BB.ddc_plan(8, width=1.5), "width"),
                       (lambda: BB.ddc_plan(8, atten=0.0), "atten")):
        with pytest.raises(ValueError) as ei:
            call()
        assert text in str(ei.value)
    for call, text in ((lambda: BB.ddc_plan(64, width=0.05), "taps"),          # 14 633 taps as one stage
                       (lambda: BB.ddc_plan(128, taps=np.ones(33)), "one stage"),
                       (lambda: BB.ddc_plan(8, taps=np.ones(4097)), "beyond")):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert isinstance(ei.value, ValueError) and text in str(ei.value)


def composite_response(stages, per_band=1024):
    """|H| of the cascade at the original rate on N = q per_band points over the whole circle: stage i, running at the rate 1 / Q, is
    freqz over one period of ITS rate, repeated Q times."""
    q = int(np.prod([qi for qi, _ in stages]))
    N = q * per_band
    H = np.ones(N, dtype=np.complex128)
    Q = 1
    for qi, h in stages:
        _, Hi = ss.freqz(h, 1, worN=N // Q, whole=True)
        H *= np.tile(Hi, Q)
        Q *= qi
    return q, N, np.abs(H)


@pytest.mark.parametrize("q", [8, 64, 256, 4096])
def test_composite_response(q):
    """What aliases into the passband |f| <= (1 - width) / (2 q) is at most -(atten - 3) dB, component by component, and the passband
    ripples by at most 0.01 dB: the conditions.  Measured at atten = 90, width = 0.2 (worst alias / ripple): q = 8: -101.38 dB / 3.0e-4 dB;
    q = 64: -101.06 dB / 2.8e-4 dB; q = 256 (64 x 4): -88.20 dB / 1.0e-3 dB; q = 4096 (64 x 64): -90.71 dB / 3.1e-4 dB."""
    atten, width = 90.0, 0.2
    stages = BB.ddc_plan(q, atten, width)
    qq, N, A = composite_response(stages)
    assert qq == q
    k = np.arange(N)
    f = np.where(k < N // 2, k, k - N) / N                                     # the original frequency of every grid point
    fb = np.where(k % (N // q) < N // (2 * q), k % (N // q), k % (N // q) - N // q) / N    # where it lands after decimation
    fp = (1.0 - width) / (2.0 * q)
    into_pass = np.abs(fb) <= fp
    wanted = np.abs(f) <= fp
    assert np.count_nonzero(wanted) >= 800 and np.count_nonzero(into_pass) == q * np.count_nonzero(wanted)
    alias_db = 20 * np.log10(np.max(A[into_pass & ~wanted]))
    ripple_db = float(np.max(np.abs(20 * np.log10(A[wanted]))))
    print("q %d: stages %s, worst alias %.2f dB, passband ripple %.2g dB" % (q, [(qi, h.size) for qi, h in stages], alias_db, ripple_db))
    assert alias_db <= -(atten - 3.0)
    assert ripple_db <= 0.01


def test_declared_and_bound():
    from pyfft_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("sp_ddc", 12), ("sp_ddc_tile", 1)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt, "%s is not declared in include/spectral.h" % name
        nargs = len([a for a in mt.group(1).split(",") if a.strip()])
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs == want
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_tile_widths_are_exported():
    """Host only: a tile of K outputs consumes K q samples, between 2048 and 4096 of them."""
    from pyfft_amd import _ffi
    lib = _ffi.load_library()
    for q in range(1, 65):
        K = lib.sp_ddc_tile(q)
        assert K >= 64 and K % 8 == 0 and 2048 <= K * q <= 4096, (q, K)
    assert lib.sp_ddc_tile(0) == 0 and lib.sp_ddc_tile(65) == 0


def test_band_plan_axis_and_scaling():
    win = ss.get_window("hann", 256)
    p = BB.band_plan(1 << 16, False, 1000.0, 8, fs=8000.0, nperseg=256)
    grid = np.fft.fftshift(np.fft.fftfreq(256, 8 / 8000.0))
    kept = np.abs(grid) <= 0.8 * 8000.0 / 16
    np.testing.assert_array_equal(p["keep"], np.nonzero(kept)[0])
    np.testing.assert_allclose(p["freq"], 1000.0 + grid[kept], rtol=1e-14)
    assert p["freq"].dtype == np.float64 and p["hop"] == 128 and p["nframes"] == 1 + ((1 << 13) - 256) // 128
    np.testing.assert_allclose(p["scale"], 1.0 / (1000.0 * np.sum(win ** 2)), rtol=1e-13)
    assert p["onesided"] and p["fold"] == 2.0
    p = BB.band_plan(1 << 16, False, 100.0, 8, fs=8000.0, nperseg=256, scaling="spectrum", return_onesided=False, noverlap=0)
    np.testing.assert_allclose(p["scale"], 1.0 / np.sum(win) ** 2, rtol=1e-13)
    np.testing.assert_allclose(p["amp"], 1.0 / np.sum(win), rtol=1e-13)
    assert not p["onesided"] and p["fold"] == 1.0 and p["hop"] == 256
    assert not BB.band_plan(1 << 16, True, -100.0, 8, fs=8000.0)["onesided"]   # complex input: any band, nothing doubled


X64 = np.zeros(1 << 14)
ONE_SIDED = "a one-sided spectrum lives on [0, fs / 2]"
REFUSALS = [
    (dict(fc=300.0), ONE_SIDED),                                               # 300 - 0.8 * 8000 / 16 < 0
    (dict(fc=3700.0), ONE_SIDED),                                              # 3700 + 400 > fs / 2
    (dict(fc=-1000.0), ONE_SIDED),
    (dict(nperseg=0), "nperseg must be at least 1"),
    (dict(nperseg=5000), "one-workgroup transforms"),
    (dict(nperseg=16384), "one-workgroup transforms"),
    (dict(nperseg=4096), "shorter than nperseg"),                              # the baseband record has 2048 samples
    (dict(noverlap=256), "noverlap"),
    (dict(scaling="power"), "scaling"),
    (dict(fs=0.0), "fs must be positive"),
    (dict(fc=np.nan), "finite"),
    (dict(width=1.0), "width"),
    (dict(q=67, nperseg=64), "prime factor"),
    (dict(window=np.zeros(64)), "sums to zero"),
    (dict(x=np.zeros((2, 640))), "one-dimensional"),
    (dict(y=np.zeros(639)), "equal lengths"),
    (dict(y=np.zeros(1 << 14, complex)), "both be real or both be complex"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_band_refusals_before_the_library(no_library, kw, text):
    kw = dict(kw)
    x, y = kw.pop("x", X64), kw.pop("y", None)
    fc, q = kw.pop("fc", 1000.0), kw.pop("q", 8)
    kw.setdefault("fs", 8000.0)
    calls = [lambda: BB.band_csd(x, x if y is None else y, fc, q, **kw), lambda: BB.band_coherence(x, x if y is None else y, fc, q, **kw)]
    if y is None:
        calls += [lambda: BB.band_psd(x, fc, q, **kw), lambda: BB.band_stft(x, fc, q, **kw)]
    for call in calls:
        with pytest.raises(ValueError) as ei:
            call()
        assert text in str(ei.value)


def test_ddc_refusals_before_the_library(no_library):
    x = np.zeros(4096)
    for call, text in ((lambda: BB.ddc(x, 0.1, 256, n0=3), "not divisible"),
                       (lambda: BB.ddc(x, 0.1, 256, n0=64 * 5 + 1), "not divisible"),
                       (lambda: BB.ddc(x, 0.1, 8, taps=np.ones(33) * (1 + 1j)), "real"),
                       (lambda: BB.ddc(x, 0.1, 8, taps=np.ones(32)), "odd length"),
                       (lambda: BB.ddc(x, 0.1, 67), "prime factor"),
                       (lambda: BB.ddc(x, 0.1, 0), "positive integer"),
                       (lambda: BB.ddc(x, np.inf, 8), "finite"),
                       (lambda: BB.ddc(x, 0.1, 8, fs=-1.0), "fs must be positive"),
                       (lambda: BB.ddc(np.float64(1.0), 0.1, 8), "at least one axis"),
                       (lambda: BB.ddc(x, 0.1, 8, axis=1), "axis")):
        with pytest.raises(ValueError) as ei:
            call()
        assert text in str(ei.value)
    with pytest.raises(ValueError) as ei:
        pyfft_amd.engine.ddc(x, 0.1, 8, np.ones(33) * 1j)
    assert "real" in str(ei.value)
