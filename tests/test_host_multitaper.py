"""Host side of the multitaper estimator: the float64 oracle of the definition against scipy.signal.welch / csd / coherence, the
host plan (tapers, weights, frames, frequency axes), every refusal before the library loads, and the declaration / binding of
sp_multitaper.  No GPU needed.  tests/test_gpu_multitaper.py imports the signal maker and the oracles from here."""
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
from pyfft_amd import multitaper as MT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETRENDS = {"none": False, "mean": "constant", "linear": "linear"}


def make_signal(n, cplx, seed):
    """Seeded white noise + two sines 50 dB apart + an offset and a slope."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = rng.standard_normal(n) + 3.0 * np.sin(2 * np.pi * 0.11 * t + 0.3) + 3.0 * 10 ** (-50 / 20) * np.sin(2 * np.pi * 0.31 * t)
    x = x + 0.7 + 1.5e-5 * t
    if cplx:
        x = x + 1j * (rng.standard_normal(n) + 3.0 * np.cos(2 * np.pi * 0.11 * t + 0.3) - 0.4 + 0.9e-5 * t)
    return x


def detrended(x, mode):
    """The whole-record detrend, float64."""
    x = np.asarray(x, dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    return x if mode == "none" else ss.detrend(x, type=DETRENDS[mode])


def oracle(x, y, plan, detrend):
    """The definition, literally: frame loop, np.fft.fft, float64.  -> dict(pxx, pyy, pxy, skx, sky) in the output layout."""
    v, c, nfft, hop, M, fs = plan["tapers"], plan["weights"], plan["nfft"], plan["hop"], plan["nframes"], plan["fs"]
    cplx = np.iscomplexobj(x)
    xd = detrended(x, detrend)
    yd = None if y is None else detrended(y, detrend)
    K = v.shape[0]
    sx, sy, sxy = np.zeros((K, nfft)), np.zeros((K, nfft)), np.zeros((K, nfft), complex)
    for k in range(K):
        norm = 1.0 / (M * fs * np.sum(v[k] ** 2))
        for g in range(M):
            X = np.fft.fft(v[k] * xd[g * hop:g * hop + nfft])
            sx[k] += norm * np.abs(X) ** 2
            if yd is not None:
                Y = np.fft.fft(v[k] * yd[g * hop:g * hop + nfft])
                sy[k] += norm * np.abs(Y) ** 2
                sxy[k] += norm * np.conj(X) * Y
    if not cplx:
        nb = nfft // 2 + 1
        sx, sy, sxy = (a[:, :nb] * plan["fold"] for a in (sx, sy, sxy))
    out = dict(skx=sx, pxx=c @ sx)
    if yd is not None:
        out.update(sky=sy, pyy=c @ sy, pxy=c @ sxy)
    return out


def scipy_oracle(x, y, plan, detrend):
    """The c-weighted sum over k of K scipy.signal.welch / csd calls on the detrended record."""
    v, c, nfft, hop, fs = plan["tapers"], plan["weights"], plan["nfft"], plan["hop"], plan["fs"]
    kw = dict(fs=fs, nperseg=nfft, noverlap=nfft - hop, detrend=False, return_onesided=not np.iscomplexobj(x), scaling="density")
    xd = detrended(x, detrend)
    skx = np.array([ss.welch(xd, window=w, **kw)[1] for w in v])
    out = dict(skx=skx, pxx=c @ skx)
    if y is not None:
        yd = detrended(y, detrend)
        sky = np.array([ss.welch(yd, window=w, **kw)[1] for w in v])
        sxy = np.array([ss.csd(xd, yd, window=w, **kw)[1] for w in v])
        out.update(sky=sky, pyy=c @ sky, pxy=c @ sxy)
    return out


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the refusals must come first."""
    from pyfft_amd import _ffi

    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "load_library", boom)
    monkeypatch.setattr(_ffi, "init", boom)


def test_exported():
    for name in ("multitaper_psd", "multitaper_spectra", "multitaper_csd", "multitaper_coherence", "multitaper_plan"):
        assert getattr(pyfft_amd, name) is getattr(MT, name)
    assert callable(pyfft_amd.engine.multitaper)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("nfft,noverlap", [(64, 0), (64, 21), (101, 50), (256, 128), (257, 85)])
@pytest.mark.parametrize("weights", ["unity", "eigen", "explicit"])
def test_oracle_equals_weighted_scipy(cplx, nfft, noverlap, weights):
    nsig = 5 * nfft + 17
    x, y = make_signal(nsig, cplx, 3), make_signal(nsig, cplx, 4)
    K = 5
    w = np.array([3.0, 0.0, 1.0, 2.5, 0.5]) if weights == "explicit" else weights
    for detrend in ("none", "mean", "linear"):
        plan = MT.multitaper_plan(nsig, cplx, fs=250.0, nfft=nfft, noverlap=noverlap, NW=3.0, Kmax=K, weights=w, detrend=detrend)
        a, b = oracle(x, y, plan, detrend), scipy_oracle(x, y, plan, detrend)
        for key in ("pxx", "pyy", "skx", "sky"):
            np.testing.assert_allclose(a[key], b[key], rtol=1e-12, atol=1e-12 * b[key].max(), err_msg=key)
        np.testing.assert_allclose(a["pxy"], b["pxy"], rtol=1e-12, atol=1e-12 * np.abs(b["pxy"]).max())


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_oracle_coherence_one_taper_is_scipy(cplx):
    nfft, nsig = 128, 128 * 9
    x, y = make_signal(nsig, cplx, 5), make_signal(nsig, cplx, 6)
    win = ss.get_window("hann", nfft)
    plan = MT.multitaper_plan(nsig, cplx, fs=2.0, nfft=nfft, noverlap=64, tapers=win[None, :], detrend="mean")
    o = oracle(x, y, plan, "mean")
    cxy = np.abs(o["pxy"]) ** 2 / (o["pxx"] * o["pyy"])
    f, ref = ss.coherence(detrended(x, "mean"), detrended(y, "mean"), fs=2.0, window=win, nperseg=nfft, noverlap=64, detrend=False)
    np.testing.assert_allclose(cxy, ref, rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(plan["freq"], f)


def test_plan_defaults():
    p = MT.multitaper_plan(5000, False, fs=100.0, nfft=1000, noverlap=250)
    K = 7                                                   # int(2 NW) - 1 at NW = 4
    assert p["tapers"].shape == (K, 1000) and p["weights"].shape == (K,)
    np.testing.assert_allclose(p["tapers"] @ p["tapers"].T, np.eye(K), rtol=0, atol=1e-10)
    np.testing.assert_allclose(p["weights"], 1.0 / K)
    np.testing.assert_allclose(p["energy"], 1.0, rtol=1e-12)
    assert p["hop"] == 750 and p["nframes"] == 1 + (5000 - 1000) // 750 and p["detrend"] == 1
    np.testing.assert_array_equal(p["freq"], np.fft.rfftfreq(1000, 0.01))
    assert p["fold"][0] == 1 and p["fold"][-1] == 1 and np.all(p["fold"][1:-1] == 2)
    ref_v, ref_lam = ss.windows.dpss(1000, 4.0, K, sym=True, norm=2, return_ratios=True)
    np.testing.assert_array_equal(p["tapers"], ref_v)
    np.testing.assert_array_equal(p["eigenvalues"], ref_lam)


def test_plan_variants():
    p = MT.multitaper_plan(999, True, fs=8.0, nfft=333, noverlap=0, NW=2.5, weights="eigen", detrend="linear")
    assert p["tapers"].shape[0] == 4 and p["nframes"] == 3 and p["hop"] == 333 and p["detrend"] == 2
    np.testing.assert_array_equal(p["freq"], np.fft.fftfreq(333, 1 / 8.0))
    np.testing.assert_allclose(p["weights"], p["eigenvalues"] / p["eigenvalues"].sum(), rtol=1e-15)
    assert abs(p["weights"].sum() - 1) < 1e-15 and np.all(p["fold"] == 1)
    p = MT.multitaper_plan(333, False, nfft=333)                          # odd nfft: no Nyquist bin, the last bin is doubled
    assert p["fold"][0] == 1 and np.all(p["fold"][1:] == 2) and p["freq"].size == 167
    p = MT.multitaper_plan(4096, False)                                   # nfft=None: one segment over the whole record
    assert p["nfft"] == 4096 and p["nframes"] == 1 and p["hop"] == 4096
    p = MT.multitaper_plan(640, False, nfft=64, tapers=np.hanning(64), weights=[4.0])
    assert p["tapers"].shape == (1, 64) and p["weights"][0] == 1.0
    np.testing.assert_allclose(p["energy"], np.sum(np.hanning(64) ** 2))
    p = MT.multitaper_plan(640, False, nfft=64, NW=3, Kmax=4, weights=[1, 0, 1, 2])
    np.testing.assert_allclose(p["weights"], [0.25, 0, 0.25, 0.5])
    p = MT.multitaper_plan(1 << 20, False, nfft=8192, noverlap=4096, detrend="none")
    assert p["nframes"] == 255 and p["detrend"] == 0


X64, C64 = np.zeros(640), np.zeros(640, complex)
REFUSALS = [
    (dict(nfft=4), "at least 8"),
    (dict(x=np.zeros(20000), nfft=16384), "one workgroup transform"),
    (dict(x=np.zeros(20000), nfft=4097), "one workgroup transform"),
    (dict(x=np.zeros(20000)), "one workgroup transform"),                      # nfft=None: the whole record, same limit
    (dict(nfft=64, noverlap=64), "noverlap"),
    (dict(nfft=64, noverlap=-1), "noverlap"),
    (dict(nfft=1024), "shorter than nfft"),
    (dict(nfft=64, fs=0.0), "fs must be positive"),
    (dict(nfft=64, fs=-1.0), "fs must be positive"),
    (dict(nfft=64, detrend="segment"), "detrend"),
    (dict(nfft=64, NW=0.0), "NW"),
    (dict(nfft=64, NW=32.0), "NW"),
    (dict(nfft=64, NW=2.0, Kmax=5), "2 NW"),
    (dict(nfft=64, NW=0.4), "number of tapers"),                               # default K = int(0.8) - 1 < 1
    (dict(nfft=64, NW=4.0, Kmax=0), "number of tapers"),
    (dict(nfft=512, NW=20.0, Kmax=33), "number of tapers"),
    (dict(nfft=64, tapers=np.ones((33, 64))), "number of tapers"),
    (dict(nfft=64, tapers=np.ones((2, 63))), "[K, nfft]"),
    (dict(nfft=64, tapers=np.zeros((2, 64))), "identically zero"),
    (dict(nfft=64, weights=[1, 2]), "weights"),
    (dict(nfft=64, weights=[1, -1, 1, 1, 1, 1, 1]), "non-negative"),
    (dict(nfft=64, weights=[0] * 7), "not all zero"),
    (dict(nfft=64, weights=[np.nan] + [1] * 6), "finite"),
    (dict(nfft=64, weights="adaptive"), "weights"),
    (dict(nfft=64, weights="eigen", tapers=np.ones((2, 64))), "Slepian"),
    (dict(x=np.zeros((2, 640)), nfft=64), "one-dimensional"),
    (dict(y=np.zeros(639), nfft=64), "equal lengths"),
    (dict(y=C64, nfft=64), "both be real or both be complex"),
    (dict(y=np.zeros((640, 1)), nfft=64), "one-dimensional"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_before_the_library(no_library, kw, text):
    kw = dict(kw)
    x, y = kw.pop("x", X64), kw.pop("y", None)
    calls = [lambda: MT.multitaper_psd(x, **kw)] if y is None else []
    calls += [lambda: MT.multitaper_spectra(x, x if y is None else y, **kw),
              lambda: MT.multitaper_coherence(x, x if y is None else y, **kw),
              lambda: MT.multitaper_csd(x, x if y is None else y, **kw)]
    for call in calls:
        with pytest.raises(ValueError) as ei:
            call()
        assert text in str(ei.value)


def test_long_segment_is_not_implemented(no_library):
    with pytest.raises(NotImplementedError):
        MT.multitaper_psd(np.zeros(1 << 15), nfft=1 << 14)


def test_declared_and_bound():
    from pyfft_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    m = re.search(r"int sp_multitaper\(([^;]*)\);", hdr)
    assert m, "sp_multitaper is not declared in include/spectral.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert "sp_multitaper" in _ffi.SIGNATURES and len(_ffi.SIGNATURES["sp_multitaper"][1]) == nargs == 20
    if os.path.exists(_ffi.LIB_PATH):
        import ctypes
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "sp_multitaper")
