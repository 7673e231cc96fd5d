"""Autoregressive spectra without a GPU: the float64 restatements of tests/burg_ref.py against things outside this work (scipy's
Toeplitz solve and freqz, the closed form at order 1, the step-up, the poles, autocorrelation matching, a known AR(4)), the measured
float32 figures the GPU test's allowances rest on, the plan figures, the refusals of the C entries and of their Python front ends
before the library is loaded, the zero and constant records, the declared set of include/spectral_ar.h, and ar_plan.h under sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import burg_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, parametric as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definitions, anchored outside this work ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("w64", "w333c", "frames"))
def test_yule_def_against_the_toeplitz_solve(name):
    from scipy.linalg import solve_toeplitz
    c = R.shape_of(name)
    x = R.segment(R.signals(name)[0], c["n"], c["first"])
    p = c["p"]
    r = R.lags_def(x, p)
    a, Ev, k = R.levinson_def(r, p)
    sol = solve_toeplitz((r[:p], np.conj(r[:p])), -r[1:])
    assert np.max(np.abs(a[1:] - sol)) <= 1e-12 * np.sum(np.abs(sol))
    assert abs(Ev[-1] - (r[0] + np.sum(sol * np.conj(r[1:]))).real) <= 1e-12 * Ev[0]
    assert Ev[0] == r[0].real and np.all(np.abs(k) < 1)


def test_psd_def_against_freqz():
    from scipy.signal import freqz
    for name in ("w64", "w333c"):
        c = R.shape_of(name)
        a, Ev, _ = R.burg_def(R.segment(R.signals(name)[0], c["n"]), c["p"])
        w, h = freqz(1.0, a, worN=512, whole=True)
        ref = Ev[-1] * np.abs(h) ** 2                                  # freqz(1, a) is 1 / A
        got = R.psd_def(a, Ev[-1], 512, 0.0, 1.0 / 512)
        assert np.max(np.abs(got - ref) / ref) <= 1e-11
    a = np.array([1.0, -0.5, 0.25])
    assert np.array_equal(R.psd_def(a, 0.0, 5, 0.0, 0.1), np.zeros(5))
    # a far start: the phase is reduced before it is multiplied by j
    near, far = R.psd_def(a, 1.0, 7, 0.37, 0.01), R.psd_def(a, 1.0, 7, 1e6 + 0.37, 0.01)
    assert np.max(np.abs(far - near) / near) <= 1e-8                    # 1e6 + 0.37 itself is rounded to 1.2e-10


def test_burg_at_order_one_is_the_closed_form():
    for name in ("w65", "w333c"):
        x = R.segment(R.signals(name)[0], R.shape_of(name)["n"])
        a, Ev, k = R.burg_def(x, 1)
        k1 = -2 * np.sum(x[1:] * np.conj(x[:-1])) / np.sum(np.abs(x[1:]) ** 2 + np.abs(x[:-1]) ** 2)
        assert abs(k[0] - k1) <= 1e-15 and a[1] == k[0] and abs(Ev[1] - np.mean(np.abs(x) ** 2) * (1 - abs(k1) ** 2)) <= 1e-15 * Ev[0]


@pytest.mark.parametrize("method", ("burg", "yule"))
def test_stepup_gives_a_at_every_order_and_the_poles_lie_inside(method):
    for name in ("w1024", "g1100"):
        c = R.shape_of(name)
        x = R.segment(R.signals(name)[0], c["n"])
        fit = R.burg_def if method == "burg" else R.yule_def
        a, Ev, k = fit(x, c["p"])
        for order in range(c["p"] + 1):
            lower = fit(x, order)[0] if order else np.ones(1)
            assert np.max(np.abs(PM.ar_stepup(k, order) - lower)) <= 1e-12 * np.sum(np.abs(lower))
        assert np.array_equal(PM.ar_stepup(k), PM.ar_stepup(k, c["p"])) and np.max(np.abs(PM.ar_stepup(k) - a)) <= 1e-13 * np.sum(np.abs(a))
        assert np.max(np.abs(np.roots(a))) < 1
        f, d = PM.ar_poles(a, fs=2.0)
        assert f.shape == d.shape == (c["p"],) and np.all(d > 0) and np.all(np.abs(f) <= 1.0) and np.all(np.diff(f) >= 0)
    batch = np.stack([R.burg_def(R.segment(R.signals("frames")[r], 200, 13), 6)[2] for r in range(3)])
    assert PM.ar_stepup(batch).shape == (3, 7) and np.array_equal(PM.ar_stepup(batch)[1], PM.ar_stepup(batch[1]))


def test_yule_walker_matches_the_autocorrelation():
    """the all-pole model reproduces r[0 .. p], so the mean of P over the full circle is r[0].  On a grid of M bins the mean is the
    aliased sum over l of rho[l M] of the model's autocorrelation rho, which decays like R^|l| with R the largest pole radius:
    the tolerance is 2 R^M / (1 - R^M) of r[0] times the model's gain bound, and M is chosen to put that under 1e-9"""
    for name in ("w64", "w333c", "w1024"):
        c = R.shape_of(name)
        x = R.segment(R.signals(name)[0], c["n"])
        a, Ev, _ = R.yule_def(x, c["p"])
        Rmax = np.max(np.abs(np.roots(a)))
        M = int(np.ceil(np.log(1e-12) / np.log(Rmax)))
        P = R.psd_def(a, Ev[-1], M, 0.0, 1.0 / M)
        tol = 2 * Rmax ** M / (1 - Rmax ** M) * P.max() / Ev[0] + 1e-12
        assert tol <= 1e-9 and abs(P.mean() - Ev[0]) <= tol * Ev[0] + 1e-12 * P.max(), (name, M, P.mean(), Ev[0])


def test_a_known_ar4_is_recovered():
    """2^16 samples: the coefficients' standard error is about sqrt(1 / n) each (Kay, sec. 6.5: the covariance is sigma^2 R^-1 / n,
    whose diagonal is of order 1 / n for poles this far inside); five of them"""
    n = 1 << 16
    y, den = R.ar4(n)
    for fit in (R.burg_def, R.yule_def):
        a, Ev, k = fit(y - y.mean(), 4)
        assert np.max(np.abs(a - den)) <= 5.0 / np.sqrt(n), (a, den)
        assert abs(Ev[-1] - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert PM.ar_order(np.stack([R.burg_def(y - y.mean(), 12)[1]]), n, "mdl")[0] == 4
    for crit in ("aic", "aicc", "fpe"):
        assert 4 <= PM.ar_order(R.burg_def(y - y.mean(), 12)[1], n, crit) <= 12
    with pytest.raises(E.ArRefused):
        PM.ar_order(np.ones(5), 100, "bic")


# ---- the allowances --------------------------------------------------------------------------------------------------------------
def test_measured_deviations():
    """BURG_F32_DEV and YULE_F32_DEV: burg_def32 / yule_def32 against the float64 definitions over the GPU test's own cases"""
    for method, recorded, names in (("burg", R.BURG_F32_DEV, list(R.CASES)), ("yule", R.YULE_F32_DEV, list(R.CASES) + list(R.YULE_ONLY))):
        worst = (0.0, None)
        for name in names:
            c = R.shape_of(name)
            ref, f32 = R.reference(name, method), R.reference(name, method, True)
            d = R.deviations(f32, ref)
            margin = 1.0 - float(np.max(np.abs(ref[2])))
            print("  %-4s %-7s P %.2e k %.2e a %.2e E %.2e   1 - max|k| %.2e   %.1f dB" %
                  ((method, name) + d + (margin, R.dynamic_range_db(ref[0][0, 0], ref[1][0, 0, -1], c["cplx"]))))
            assert margin >= 1e-4
            worst = max(worst, (max(d), name))
        print("%s: float32 %.3e at %s, recorded %.3e" % ((method,) + worst + (recorded,)))
        assert 0.5 * recorded <= worst[0] <= recorded
    assert R.BURG_ALLOWANCE == R.MARGIN * R.BURG_F32_DEV and R.YULE_ALLOWANCE == R.MARGIN * R.YULE_F32_DEV and R.MARGIN == 4.0
    assert R.BURG_ALLOWANCE <= R.PARITY == 2e-4 and R.YULE_ALLOWANCE <= R.PARITY


def test_the_recorded_device_shares():
    """what tests/test_gpu_parametric.py used of its allowances on an MI355X"""
    assert 0 < R.BURG_DEVICE_SHARE <= 1 and 0 < R.YULE_DEVICE_SHARE <= 1


def test_zero_and_constant_records():
    for fit in (R.burg_def, R.yule_def):
        for f32 in (False, True):
            for x in (np.zeros(40), R.segment(np.full(40, 3.5, dtype=np.float32), 40), np.zeros(40, dtype=np.complex128)):
                a, Ev, k = fit(x, 5, f32)
                assert np.array_equal(a, np.eye(1, 6)[0]) and not Ev.any() and not k.any() and np.iscomplexobj(a) == np.iscomplexobj(x)
                assert np.array_equal(R.psd_def(a, Ev[-1], 9, 0.0, 0.1), np.zeros(9))


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.AR_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.AR_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


def plan_ref(method, cplx, n, p, segs, form=0, hook=0):
    """ar_plan.h restated: form, segments per workgroup, samples, LDS bytes, workgroups, passes, threads, tiles"""
    el = 16 if cplx else 8
    chunk = max(2048, -(-(-(-n // 1024)) // 2048) * 2048)
    tiles = -(-n // chunk)
    if method == 0:
        if n <= 1024 and form != 2:
            spl, nw = next(s for s in (1, 2, 4, 8, 16) if 64 * s >= n), 1
        else:
            spl, nw = (8, 4) if n <= 2048 else (16, 4) if n <= 4096 else (16, 8) if n <= 8192 else (16, 16)
        spw, threads = (4, 256) if nw == 1 else (1, 64 * nw)
        lds = spw * 2 * p * el + (2 * nw * (32 + el) if nw > 1 else 0)
        fit, kind, samples = 1 << 20, 0 if nw == 1 else 1, spl
    else:
        spw, threads, kind, samples = 1, 256, 2, chunk
        lds = (2048 + 256) * el // 2 + 2 * 256 * el
        fit = min(1 << 20, max(1, (256 << 20) // (tiles * (p + 1) * el)))
    if hook > 0:
        fit = min(fit, hook)
    spp = min(max(segs, 1), fit)
    passes = -(-segs // spp)
    wgs = sum(-(-min(spp, segs - s0) // spw) if method == 0 else min(spp, segs - s0) * tiles for s0 in range(0, segs, spp))
    return kind, spw, samples, lds, wgs, passes, threads, tiles


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_AR_SEGS", raising=False)
    monkeypatch.delenv("SP_BURG_FORM", raising=False)
    lib = _c_entry()
    out = np.zeros(8, dtype=np.int64)
    plan = lambda me, dt, n, p, b, f: (lib.sp_ar_plan(me, dt, n, p, b, f, _ffi.ptr(out)), tuple(int(v) for v in out))[1]
    shapes = [(0, 0, 64, 4, 1, 1), (0, 0, 65, 1, 1, 1), (0, 1, 333, 8, 1, 1), (0, 0, 1024, 16, 3, 5), (0, 0, 1025, 16, 1, 1), (0, 1, 4096, 64, 2, 2),
              (0, 1, 8192, 128, 1, 1), (0, 0, 16384, 256, 1, 1), (0, 1, 64, 3, 1, 11), (1, 0, 100003, 20, 1, 1), (1, 1, 64, 4, 3, 5),
              (1, 1, (1 << 31) - 1, 256, 100, 1), (1, 0, 3 * 2048 + 5, 9, 1, 1), (0, 0, 64, 4, 0, 5)]
    for me, dt, n, p, b, f in shapes:
        assert plan(me, dt, n, p, b, f) == plan_ref(me, dt, n, p, b * f), (me, dt, n, p, b, f)
    assert plan(0, 0, 1024, 16, 3, 5) == (0, 4, 16, 4 * 2 * 16 * 8, 4, 1, 256, 1) and plan(0, 0, 1025, 16, 1, 1) == (1, 1, 8, 2 * 16 * 8 + 2 * 4 * 40, 1, 1, 256, 1)
    assert plan(1, 0, 100003, 20, 1, 1) == (2, 1, 2048, 2304 * 4 + 4096, 49, 1, 256, 49)
    monkeypatch.setenv("SP_AR_SEGS", str(R.SEGS_HOOK))
    assert plan(0, 1, 64, 3, 1, 11) == plan_ref(0, 1, 64, 3, 11, hook=R.SEGS_HOOK) == (0, 4, 1, 4 * 2 * 3 * 16, 3, 2, 256, 1)
    monkeypatch.setenv("SP_AR_SEGS", "0")
    monkeypatch.setenv("SP_BURG_FORM", "2")
    assert plan(0, 0, 1024, 16, 1, 1) == plan_ref(0, 0, 1024, 16, 1, form=2) and plan(0, 0, 1024, 16, 1, 1)[0] == 1
    monkeypatch.setenv("SP_BURG_FORM", "1")
    assert plan(0, 0, 1024, 16, 1, 1)[0] == 0 and plan(0, 0, 1025, 16, 1, 1)[0] == 1
    monkeypatch.delenv("SP_BURG_FORM")
    d = E.ar_plan("burg", 333, 8, 2, 3, cplx=True)
    assert d == PM.ar_plan("burg", 333, 8, 2, 3, True) == pyfft_amd.ar_plan(0, 333, 8, 2, 3, True)
    assert tuple(d[k] for k in ("form", "segs_per_wg", "samples", "lds_bytes", "workgroups", "passes", "threads", "tiles")) == plan_ref(0, True, 333, 8, 6)
    assert d["lds_bytes"] <= 64 * 1024 and E.BURG_WAVE_MAX == R.CROSSOVER
    assert lib.sp_ar_plan(0, 0, 64, 4, 1, 1, None) < 0
    for bad in ((2, 0, 64, 4, 1, 1), (0, 2, 64, 4, 1, 1), (0, 0, 64, 0, 1, 1), (0, 0, 1024, 257, 1, 1), (0, 0, 64, 33, 1, 1), (0, 0, 16385, 4, 1, 1),
                (1, 0, 1 << 31, 4, 1, 1), (0, 0, 1, 1, 1, 1), (0, 0, 64, 4, -1, 1), (0, 0, 64, 4, 1, -1)):
        assert lib.sp_ar_plan(*bad, _ffi.ptr(out)) < 0, bad
    for bad in (("burg", 64, 0), ("burg", 64, 33), ("burg", 16385, 4), ("yule", 1 << 31, 4), ("burg", 1024, 257), (3, 64, 4), ("burg", 64, 4, -1)):
        with pytest.raises(E.ArRefused):
            E.ar_plan(*bad)


FIT_GOOD = dict(x=True, dtype=0, xld=400, nsig=400, batch=2, n=100, hop=50, first=10, nframes=3, order=5, detrend=3, mre=0.0, mim=0.0, a=True,
                e=True, k=True, old=6)
SENT = -12345.0
NAN, INF = float("nan"), float("inf")
FIT_REFUSALS = [(dict(dtype=2), "dtype"), (dict(order=0), "order must"), (dict(order=257, n=1000, nsig=2000, xld=2000), "order must"),
                (dict(order=51, old=60), "n / 2"), (dict(n=1), "n must"), (dict(hop=0), "hop"), (dict(first=-1), "first"), (dict(nframes=-1), "nframes"),
                (dict(batch=-1), "batch"), (dict(nframes=7), "reach outside"), (dict(first=301), "reach outside"), (dict(nsig=0), "nsig"),
                (dict(xld=399), "x_ld"), (dict(old=5), "out_ld"), (dict(detrend=1), "detrend"), (dict(detrend=0, mre=NAN), "mean"),
                (dict(detrend=0, mim=INF), "mean"), (dict(x=False), "x is"), (dict(a=False), "a is"), (dict(e=False), "evar is"), (dict(k=False), "k is")]


def _fit_call(lib, entry, **over):
    p = dict(FIT_GOOD, **over)
    x = np.ones(800, dtype=np.float32)
    a, e, k = (np.full(6 * 64, SENT) for _ in range(3))
    ptr = _ffi.ptr
    rc = getattr(lib, entry)(ptr(x) if p["x"] else None, p["dtype"], p["xld"], p["nsig"], p["batch"], p["n"], p["hop"], p["first"], p["nframes"],
                             p["order"], p["detrend"], p["mre"], p["mim"], ptr(a) if p["a"] else None, ptr(e) if p["e"] else None,
                             ptr(k) if p["k"] else None, p["old"], 0)
    return rc, (lib.sp_last_error() or b"").decode(), (a, e, k)


@pytest.mark.parametrize("entry", ("sp_burg", "sp_yule"))
@pytest.mark.parametrize("over,word", FIT_REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(FIT_REFUSALS)])
def test_c_refusals_of_the_fits(entry, over, word):
    rc, msg, outs = _fit_call(_c_entry(), entry, **over)
    assert rc == -1 and msg.startswith(entry + ": ") and word in msg, (rc, msg)
    assert all(np.all(o == SENT) for o in outs)


def test_burg_refuses_a_long_segment_and_nothing_to_do():
    lib = _c_entry()
    rc, msg, outs = _fit_call(lib, "sp_burg", n=16385, nsig=20000, xld=20000, nframes=1)
    assert rc == -1 and "16384" in msg
    for over in (dict(batch=0), dict(nframes=0)):
        rc, _, outs = _fit_call(lib, "sp_yule", **over)
        assert rc == 0 and all(np.all(o == SENT) for o in outs)


PSD_GOOD = dict(a=True, cplx=0, ald=6, e=True, eld=1, order=5, nm=3, m=20, start=0.0, step=0.01, scale=1.0, out64=0, P=True, pld=20)
PSD_REFUSALS = [(dict(order=-1), "order"), (dict(order=257, ald=300), "order"), (dict(ald=5), "a_ld"), (dict(eld=0), "e_ld"), (dict(m=0), "m ="),
                (dict(m=1 << 31, pld=1 << 31), "m ="), (dict(pld=19), "P_ld"), (dict(nm=-1), "nmodels"), (dict(nm=1 << 30, m=1000, pld=1000), "nmodels"),
                (dict(start=NAN), "finite"), (dict(step=INF), "finite"), (dict(scale=NAN), "finite"), (dict(a=False), "a is"), (dict(e=False), "e is"),
                (dict(P=False), "P is")]


@pytest.mark.parametrize("over,word", PSD_REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(PSD_REFUSALS)])
def test_c_refusals_of_the_spectrum(over, word):
    lib = _c_entry()
    p = dict(PSD_GOOD, **over)
    a, e, P = np.ones(64), np.ones(8), np.full(64, SENT, dtype=np.float32)
    ptr = _ffi.ptr
    rc = lib.sp_ar_psd(ptr(a) if p["a"] else None, p["cplx"], p["ald"], ptr(e) if p["e"] else None, p["eld"], p["order"], p["nm"], p["m"], p["start"],
                       p["step"], p["scale"], p["out64"], ptr(P) if p["P"] else None, p["pld"], 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc == -1 and msg.startswith("sp_ar_psd: ") and word in msg and np.all(P == np.float32(SENT)), (rc, msg)


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    x = np.ones(400, dtype=np.float32)
    xn = x.copy()
    xn[17] = np.nan
    a, e = np.ones((3, 6)), np.ones(3)
    bad = [lambda: E.burg(x, 100, 50, 0, 3, 0), lambda: E.burg(x, 100, 50, 0, 3, 51), lambda: E.burg(x, 100, 50, 0, 8, 5),
           lambda: E.burg(x, 100, 0, 0, 3, 5), lambda: E.burg(x, 100, 50, -1, 3, 5), lambda: E.burg(x, 100, 50, 0, -1, 5),
           lambda: E.burg(x, 1, 1, 0, 3, 1), lambda: E.burg(np.ones(20000, dtype=np.float32), 16385, 1, 0, 1, 5), lambda: E.burg(xn, 100, 50, 0, 3, 5),
           lambda: E.burg(x, 100, 50, 0, 3, 5, mean_value=np.nan), lambda: E.burg(x, 100, 50, 0, 3, 5, mean_value=1j),
           lambda: E.burg(x, 100, 50, 0, 3, 5, detrend="linear"), lambda: E.burg(x, 100, 50, 0, 3, 5, detrend="constant"),
           lambda: E.burg(x, 100, 50, 0, 3, 5, detrend=3), lambda: E.yule(x, 100, 50, 0, 3, 5, detrend=False, mean_value=0.5), lambda: E.burg(x, 1000, 1, 0, 1, 257),
           lambda: E.yule(x, 100, 50, 301, 1, 5), lambda: E.yule(xn, 100, 50, 0, 3, 5), lambda: E.yule(np.float32(1.0), 100, 50, 0, 3, 5),
           lambda: E.ar_psd(a, e[:2], 10, 0.0, 0.1), lambda: E.ar_psd(a, e, 0, 0.0, 0.1), lambda: E.ar_psd(a, e, 10, np.nan, 0.1),
           lambda: E.ar_psd(a, e, 10, 0.0, np.inf), lambda: E.ar_psd(a, e, 10, 0.0, 0.1, scale=np.nan), lambda: E.ar_psd(np.ones((2, 258)), e[:2], 10, 0.0, 0.1),
           lambda: E.ar_psd(a * np.nan, e, 10, 0.0, 0.1), lambda: E.ar_psd(np.float64(1.0), e, 10, 0.0, 0.1),
           lambda: PM.arburg(x, 201), lambda: PM.aryule(x[:1], 1), lambda: PM.pburg(x, 5, nfft=0), lambda: PM.pburg(x, 5, fs=0.0),
           lambda: PM.pyulear(x, 5, band=(0.3, 0.2), m=8), lambda: PM.pyulear(x, 5, band=(0.1, 0.2), m=1),
           lambda: PM.ar_spectrogram(x, 5, 100, method="covariance"), lambda: PM.ar_spectrogram(x, 5, 401), lambda: PM.ar_spectrogram(x, 5, 100, noverlap=100),
           lambda: PM.ar_spectrogram(x, 51, 100), lambda: PM.ar_psd(a, e, nfft=0), lambda: PM.ar_stepup(np.ones(4), 5), lambda: PM.ar_order(np.ones(5), 5),
           lambda: E.ar_plan("burg", 64, 33)]
    for i, fn in enumerate(bad):
        with pytest.raises(E.ArRefused) as exc:
            fn()
        assert isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError), i
    assert PM.ArRefused is E.ArRefused


def test_axes_and_units():
    f, m, start, step, dbl = PM._axis("t", 8, 4.0, True, None, None)
    assert np.array_equal(f, np.arange(5) * 0.5) and (m, start, step) == (5, 0.0, 0.125) and dbl == slice(1, 4)
    f, m, start, step, dbl = PM._axis("t", 7, 1.0, True, None, None)
    assert m == 4 and dbl == slice(1, 4)                                # an odd nfft has no Nyquist bin
    f, m, start, step, dbl = PM._axis("t", 8, 4.0, False, None, None)
    assert np.array_equal(f, np.fft.fftfreq(8, 0.25)) and m == 8 and dbl is None
    f, m, start, step, dbl = PM._axis("t", 8, 10.0, True, (0.0, 5.0), 11)
    assert np.allclose(f, np.arange(11) * 0.5) and (m, start) == (11, 0.0) and abs(step - 0.05) < 1e-17 and not dbl[0] and not dbl[-1] and dbl[1:-1].all()


def test_exported_declared_and_bound():
    for name in ("arburg", "aryule", "pburg", "pyulear", "ar_spectrogram", "ar_psd", "ar_order", "ar_stepup", "ar_poles", "ar_plan", "ArRefused"):
        assert getattr(pyfft_amd, name) is getattr(PM, name)
    for name in ("ArRefused", "ar_check", "burg", "yule", "ar_psd", "ar_plan"):
        assert hasattr(E, name)
    assert issubclass(E.ArRefused, ValueError) and issubclass(E.ArRefused, NotImplementedError)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_ar.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.AR_SIGNATURES) == {"sp_burg", "sp_yule", "sp_ar_psd", "sp_ar_plan"}
    assert len(_ffi.TABLES) == 6 and _ffi.MORE_TABLES[-1] is _ffi.AR_SIGNATURES and all(t is not _ffi.AR_SIGNATURES for t in _ffi.TABLES)
    for table in _ffi.TABLES + tuple(t for t in _ffi.MORE_TABLES if t is not _ffi.AR_SIGNATURES):
        assert not set(_ffi.AR_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_burg", 18), ("sp_yule", 18), ("sp_ar_psd", 15), ("sp_ar_plan", 7)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.AR_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.AR_SIGNATURES[name][1]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "spectral_ar.h":
            assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other))), other
    assert "spectral_ar.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert '#include "../../include/spectral_ar.h"' in open(os.path.join(ROOT, "pyfft_amd", "csrc", "spectral.hip")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "SP_AR_SEGS" in launch and "SP_BURG_FORM" in launch and "launch_burg" in launch and "profiles/burg_variants.txt" in launch
    ext = open(os.path.join(ROOT, "include", "spectral_ext.h")).read()
    assert "which = 7" in ext and "which = 6" in ext and "sp_burg" in ext and "which=7" in E.last_passes.__doc__
    assert _ffi.load_library().sp_last_passes(7) == 0 and E.AR_PASSES == 7
    kernel = open(os.path.join(ROOT, "pyfft_amd", "csrc", "k_burg.hip")).read()
    assert "atomic" not in kernel.split("#include")[1].lower().replace("__atomic_release", "").replace("__atomic_acquire", "") and "hipMemset" not in kernel


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """ar_plan.h is host-only arithmetic: built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run here as its own
    process -- the forms and slots of every length, the tiles up to 2^31 - 1 samples, the passes up to 2^40 segments, the refusals"""
    exe = str(tmp_path / "ar_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "pyfft_amd", "csrc"), os.path.join(ROOT, "tests", "ar_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ar plan ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
