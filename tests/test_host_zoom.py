"""Host side of the chirp-z transform and the zoom spectra: the float64 oracles (the literal definition for czt, a frame loop for the
estimators) against scipy.signal.czt / zoom_fft / welch / csd, the host plan, every refusal before the library loads, the declaration
and binding of sp_czt / sp_zoom_welch / sp_czt_chirp, and the chirp table phases against exact integer arithmetic.  No GPU needed.
tests/test_gpu_zoom.py imports the oracles from here."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
from pyfft_amd import zoom as ZM
from test_host_multitaper import make_signal, detrended, no_library        # noqa: F401  (no_library: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETREND_NAME = {False: "none", "constant": "mean", "linear": "linear"}


def czt_oracle(x, m, start, step):
    """The definition, literally, along the last axis: X[k] = sum_j x[j] exp(-2 pi i (start + k step) j), float64."""
    x = np.asarray(x, dtype=np.complex128)
    j = np.arange(x.shape[-1], dtype=np.float64)
    out = np.empty(x.shape[:-1] + (m,), dtype=np.complex128)
    for k0 in range(0, m, 64):                                   # columns in blocks: the n x m phase matrix stays small
        f = start + np.arange(k0, min(k0 + 64, m)) * step
        out[..., k0:k0 + f.size] = x @ np.exp(-2j * np.pi * np.outer(j, f))
    return out


def zoom_oracle(x, y, plan, stft=False):
    """The frame loop: window, literal transform on the arc, sums in float64.  -> dict(pxx[, pyy, pxy]) in the output layout (folded
    for a one-sided plan), or with stft the frames Z [m, nframes]."""
    mode = {0: "none", 1: "mean", 2: "linear"}[plan["detrend"]]
    n, hop, M, m, w = plan["nperseg"], plan["hop"], plan["nframes"], plan["m"], plan["window"]
    xd = detrended(x, mode)
    yd = None if y is None else detrended(y, mode)
    # the frame loop: every frame windowed on its own, then all of them through the literal transform (one phase matrix for all)
    X = czt_oracle(np.array([w * xd[g * hop:g * hop + n] for g in range(M)]), m, plan["start"], plan["step"])
    Y = None if yd is None else czt_oracle(np.array([w * yd[g * hop:g * hop + n] for g in range(M)]), m, plan["start"], plan["step"])
    if stft:
        return plan["amp"] * X.T
    sc = plan["scale"] * plan["fold"] / M
    out = dict(pxx=sc * np.sum(np.abs(X) ** 2, axis=0))
    if yd is not None:
        out.update(pyy=sc * np.sum(np.abs(Y) ** 2, axis=0), pxy=sc * np.sum(np.conj(X) * Y, axis=0))
    return out


def test_exported():
    for name in ("czt", "zoom_fft", "zoom_stft", "zoom_psd", "zoom_csd", "zoom_coherence", "zoom_plan"):
        assert getattr(pyfft_amd, name) is getattr(ZM, name)
    assert callable(pyfft_amd.engine.czt) and callable(pyfft_amd.engine.zoom_welch)


@pytest.mark.parametrize("n,m", [(8, 5), (100, 37), (257, 300), (1000, 300)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_czt_oracle_equals_scipy(n, m, cplx):
    x = make_signal(3 * n, cplx, 11).reshape(3, n)
    start, step = 0.1037, 0.3 / m
    ref = ss.czt(x, m, w=np.exp(-2j * np.pi * step), a=np.exp(2j * np.pi * start))
    got = czt_oracle(x, m, start, step)
    assert np.max(np.abs(got - ref)) <= 1e-10 * np.max(np.abs(ref))
    fs = 250.0
    f1, f2 = 17.0, 43.5
    for endpoint in (False, True):
        st, sp_, freq = ZM._arc(f1, f2, m, fs, endpoint)
        ref = ss.zoom_fft(x, [f1, f2], m, fs=fs, endpoint=endpoint)
        got = czt_oracle(x, m, st, sp_)
        assert np.max(np.abs(got - ref)) <= 1e-10 * np.max(np.abs(ref))
        np.testing.assert_allclose(freq, np.linspace(f1, f2, m, endpoint=endpoint), rtol=1e-14, atol=1e-12)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_frame_loop_oracle_equals_scipy_zoom_fft(cplx):
    nsig, nperseg, m, fs = 2000, 300, 64, 8.0
    x = make_signal(nsig, cplx, 12)
    plan = ZM.zoom_plan(nsig, cplx, [0.5, 1.5], m, fs=fs, window="hann", nperseg=nperseg, noverlap=100, detrend="linear",
                        return_onesided=False)
    Z = zoom_oracle(x, None, plan, stft=True)
    xd = detrended(x, "linear")
    w, hop = plan["window"], plan["hop"]
    assert Z.shape == (m, plan["nframes"]) and plan["nframes"] == 1 + (nsig - nperseg) // 200
    for g in range(plan["nframes"]):
        ref = ss.zoom_fft(w * xd[g * hop:g * hop + nperseg], [0.5, 1.5], m, fs=fs) / w.sum()
        assert np.max(np.abs(Z[:, g] - ref)) <= 1e-10 * np.max(np.abs(ref))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("nperseg,noverlap,k0,m", [(128, 64, 3, 40), (128, 0, 0, 64), (100, 33, 7, 21), (256, 128, 100, 28)])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("detrend", [False, "constant", "linear"])
def test_oracle_on_fft_bins_equals_scipy_welch(cplx, nperseg, noverlap, k0, m, scaling, detrend):
    """An arc laid exactly on FFT bins (start = k0 / n, step = 1 / n) reproduces scipy.signal.welch / csd on those bins, with the
    one-sided doubling for real input."""
    nsig, fs = 9 * nperseg + 5, 250.0
    x, y = make_signal(nsig, cplx, 13), make_signal(nsig, cplx, 14)
    fn = [k0 * fs / nperseg, (k0 + m) * fs / nperseg]
    plan = ZM.zoom_plan(nsig, cplx, fn, m, fs=fs, window="hann", nperseg=nperseg, noverlap=noverlap, detrend=detrend, scaling=scaling)
    assert abs(plan["start"] - k0 / nperseg) < 1e-15 and abs(plan["step"] - 1.0 / nperseg) < 1e-17
    o = zoom_oracle(x, y, plan)
    xd, yd = detrended(x, DETREND_NAME[detrend]), detrended(y, DETREND_NAME[detrend])
    kw = dict(fs=fs, window="hann", nperseg=nperseg, noverlap=noverlap, detrend=False, scaling=scaling)
    f, pxx = ss.welch(xd, **kw)
    _, pyy = ss.welch(yd, **kw)
    _, pxy = ss.csd(xd, yd, **kw)
    sl = slice(k0, k0 + m)
    np.testing.assert_allclose(plan["freq"], f[sl], rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(o["pxx"], pxx[sl], rtol=1e-10, atol=1e-12 * pxx[sl].max())
    np.testing.assert_allclose(o["pyy"], pyy[sl], rtol=1e-10, atol=1e-12 * pyy[sl].max())
    np.testing.assert_allclose(o["pxy"], pxy[sl], rtol=1e-10, atol=1e-12 * np.abs(pxy[sl]).max())


def test_plan_axes_scaling_and_fold():
    win = ss.get_window("hann", 256)
    p = ZM.zoom_plan(5000, False, [10.0, 20.0], 100, fs=100.0)
    np.testing.assert_allclose(p["freq"], 10.0 + 0.1 * np.arange(100), rtol=1e-14)
    assert p["freq"].dtype == np.float64 and p["start"] == 0.1 and abs(p["step"] - 0.001) < 1e-18
    assert p["nperseg"] == 256 and p["hop"] == 128 and p["nframes"] == 1 + (5000 - 256) // 128 and p["detrend"] == 0
    np.testing.assert_allclose(p["window"], win, rtol=0, atol=1e-15)
    np.testing.assert_allclose(p["scale"], 1.0 / (100.0 * np.sum(win ** 2)), rtol=1e-13)
    np.testing.assert_allclose(p["amp"], 1.0 / np.sum(win), rtol=1e-13)
    assert p["onesided"] and np.all(p["fold"] == 2)
    p = ZM.zoom_plan(5000, False, [10.0, 20.0], 101, fs=100.0, endpoint=True, scaling="spectrum", detrend="constant", noverlap=0)
    np.testing.assert_allclose(p["freq"], np.linspace(10.0, 20.0, 101), rtol=1e-14)
    assert abs(p["step"] - 0.001) < 1e-18 and p["hop"] == 256 and p["detrend"] == 1
    np.testing.assert_allclose(p["scale"], 1.0 / np.sum(win) ** 2, rtol=1e-13)
    # the doubling rule: 0 < f < fs / 2 doubled, DC and Nyquist not; a scalar fn is the band [0, fn]
    p = ZM.zoom_plan(5000, False, 50.0, 4, fs=100.0, endpoint=True, detrend="linear")
    np.testing.assert_allclose(p["freq"], [0.0, 50.0 / 3, 100.0 / 3, 50.0])
    np.testing.assert_array_equal(p["fold"], [1, 2, 2, 1])
    assert p["detrend"] == 2 and p["start"] == 0.0
    # complex input, or return_onesided=False: nothing doubled, any band
    for cplx, onesided in ((True, True), (False, False)):
        p = ZM.zoom_plan(5000, cplx, [-30.0, 80.0], 64, fs=100.0, return_onesided=onesided)
        assert not p["onesided"] and np.all(p["fold"] == 1) and p["start"] == -0.3
    # an explicit window sets nperseg; a single frame
    p = ZM.zoom_plan(300, False, [1.0, 2.0], 8, fs=10.0, window=np.ones(300))
    assert p["nperseg"] == 300 and p["nframes"] == 1 and p["hop"] == 150
    np.testing.assert_allclose(p["scale"], 1.0 / (10.0 * 300))
    p = ZM.zoom_plan(1 << 20, False, [0.1, 0.2], 1000, nperseg=116508)
    assert p["nframes"] == 1 + ((1 << 20) - 116508) // 58254


X64, C64 = np.zeros(640), np.zeros(640, complex)
REFUSALS = [
    (dict(m=0), "m must be at least 1"),
    (dict(nperseg=0), "nperseg must be at least 1"),
    (dict(window=np.zeros((2, 64))), "one-dimensional"),
    (dict(window=np.zeros(64)), "sums to zero"),
    (dict(window=np.r_[np.nan, np.ones(63)]), "finite"),
    (dict(nperseg=1024), "shorter than nperseg"),
    (dict(nperseg=64, noverlap=64), "noverlap"),
    (dict(nperseg=64, noverlap=-1), "noverlap"),
    (dict(fs=0.0), "fs must be positive"),
    (dict(fs=-1.0), "fs must be positive"),
    (dict(fn=[0.1, 0.2, 0.3]), "scalar or a pair"),
    (dict(fn=[0.1, np.inf]), "finite"),
    (dict(fn=np.nan), "finite"),
    (dict(detrend="segment"), "detrend"),
    (dict(detrend=True), "detrend"),
    (dict(scaling="power"), "scaling"),
    (dict(fn=[0.1, 0.6]), "[0, fs / 2]"),                                      # real, one-sided: the band leaves [0, fs / 2]
    (dict(fn=[-0.1, 0.2]), "[0, fs / 2]"),
    (dict(x=np.zeros(1 << 17), nperseg=1 << 17, m=(1 << 26) - (1 << 17) + 2), "beyond the longest transform"),
    (dict(x=np.zeros((2, 640))), "one-dimensional"),
    (dict(y=np.zeros(639)), "equal lengths"),
    (dict(y=C64), "both be real or both be complex"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_before_the_library(no_library, kw, text):
    kw = dict(kw)
    x, y = kw.pop("x", X64), kw.pop("y", None)
    fn, m = kw.pop("fn", [0.1, 0.2]), kw.pop("m", 16)
    kw.setdefault("nperseg", 64)
    calls = [lambda: ZM.zoom_csd(x, x if y is None else y, fn, m, **kw), lambda: ZM.zoom_coherence(x, x if y is None else y, fn, m, **kw)]
    if y is None:
        calls.append(lambda: ZM.zoom_psd(x, fn, m, **kw))
        if not {"scaling"} & set(kw) and "[0, fs / 2]" not in text:
            calls.append(lambda: ZM.zoom_stft(x, fn, m, **kw))
    for call in calls:
        with pytest.raises(ValueError) as ei:
            call()
        assert text in str(ei.value)


def test_czt_refusals_before_the_library(no_library):
    x = np.zeros(64)
    for w, a in ((0.99 * np.exp(-0.1j), 1.0), (np.exp(-0.1j), 1.01), (1.0 + 1e-6, 1.0)):
        with pytest.raises(NotImplementedError) as ei:
            ZM.czt(x, 16, w, a)
        assert isinstance(ei.value, ValueError) and "unit circle" in str(ei.value)
    for call, text in ((lambda: ZM.czt(x, 0), "m must be at least 1"),
                       (lambda: ZM.czt(x, 16, complex(np.nan, 0)), "finite"),
                       (lambda: ZM.czt(np.zeros(0), 4), "at least one input sample"),
                       (lambda: ZM.czt(np.float64(1.0), 4), "at least one axis"),
                       (lambda: ZM.czt(x, 4, axis=2), "axis"),
                       (lambda: ZM.zoom_fft(x, [0.1, 0.2], 0), "m must be at least 1"),
                       (lambda: ZM.zoom_fft(x, [0.1, 0.2, 0.3], 8), "scalar or a pair"),
                       (lambda: ZM.zoom_fft(x, 0.5, 8, fs=0), "fs must be positive"),
                       (lambda: ZM.zoom_fft(x, np.inf, 8), "finite")):
        with pytest.raises(ValueError) as ei:
            call()
        assert text in str(ei.value)
    with pytest.raises(NotImplementedError):
        ZM.czt(x, 1 << 26)


def test_declared_and_bound():
    from pyfft_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("sp_czt", 10), ("sp_zoom_welch", 20), ("sp_czt_chirp", 5)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt, "%s is not declared in include/spectral.h" % name
        nargs = len([a for a in mt.group(1).split(",") if a.strip()])
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs == want
        if os.path.exists(_ffi.LIB_PATH):
            assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def exact_chirp(i, step, start):
    """(cos, sin) of exp(-2 pi i (start i + step i^2 / 2)) with the phase reduced modulo one turn in exact rational arithmetic."""
    t = (Fraction(start) * i + Fraction(step) * i * i / 2) % 1
    if t >= Fraction(1, 2):
        t -= 1
    a = -2.0 * math.pi * float(t)
    return math.cos(a), math.sin(a)


STEPS = [1.0 / 4096, 1.0 / (64 * 4096), 0.1, math.pi / 1e4, -0.013, 1e-9, 0.3 / 116508, math.sqrt(2.0) - 1.0]
STARTS = [0.0, 0.25, 0.123456789, -0.3]


@pytest.mark.parametrize("step", STEPS, ids=["%g" % s for s in STEPS])
def test_chirp_table_phases_are_exact(step):
    """Every table entry within 2e-7 absolute of the exactly reduced phasor: float32 rounding of a unit phasor plus the 1e-9-turn
    requirement (2 pi 1e-9 = 6.3e-9), at indices where a float64 product step * i^2 / 2 has lost its fractional bits."""
    from pyfft_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.skip("the library is not built")
    lib = _ffi.load_library()
    worst = 0.0
    for start in STARTS:
        for centre in (0, 1 << 13, 1 << 20, (1 << 25) - 4, -(1 << 25) + 1, (1 << 26) - 8):
            i0, count = centre - 5, 12
            cs = np.empty((count, 2), dtype=np.float32)
            assert lib.sp_czt_chirp(i0, count, step, start, _ffi.ptr(cs)) == 0
            ref = np.array([exact_chirp(i0 + c, step, start) for c in range(count)])
            worst = max(worst, float(np.max(np.abs(cs - ref))))
    print("step %r: worst table error %.3g" % (step, worst))
    assert worst <= 2e-7


def test_chirp_refusals():
    from pyfft_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.skip("the library is not built")
    lib = _ffi.load_library()
    cs = np.empty((4, 2), dtype=np.float32)
    for args in ((0, -1, 0.1, 0.0, _ffi.ptr(cs)), (0, 4, float("nan"), 0.0, _ffi.ptr(cs)), (0, 4, 0.1, float("inf"), _ffi.ptr(cs)),
                 (0, 4, 0.1, 0.0, None)):
        assert lib.sp_czt_chirp(*args) < 0
        assert b"sp_czt_chirp" in lib.sp_last_error()
