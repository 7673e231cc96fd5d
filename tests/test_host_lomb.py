"""Lomb-Scargle spectra without a GPU: the float64 closed form of tests/lomb_ref.py against scipy.signal.lombscargle over all of its
options and against the FFT of an even clock, the measured float32 figure the GPU test's allowance rests on, the additivity of the sums,
the significance level on white noise, the frequency grid and the spectral window of an even clock, the refusals of the C entries and
of their Python front ends, the plan figures, and the declared set of include/spectral_uneven.h."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import lomb_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, lomb as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form", R.FORMS24, ids=[R.form_id(f) for f in R.FORMS24])
def test_closed_form_is_scipys_lombscargle(form):
    name = "n1000-m300"
    t, y, w, _ = R.signals(name)
    wt, fm, pc, nz = form
    f = R.freqs_of(name, form)
    ref = ss.lombscargle(np.array(t), np.array(y[0]), 2 * np.pi * f, precenter=pc, normalize=nz, weights=np.array(w) if wt else None,
                         floating_mean=fm)
    dev = R.deviation(R.reference(name, form), ref[None])
    print("%s: %.2e of the row maximum" % (R.form_id(form), dev))
    assert dev <= 1e-11


def test_even_clock_at_fft_bins_is_the_periodogram():
    rng = np.random.default_rng(2)
    N = 256
    y = rng.standard_normal(N) + 0.4
    k = np.arange(1, N // 2)                                # 0 and Nyquist left out: there sin or cos vanishes on the grid
    P = R.lomb_def(np.arange(N, dtype=np.float64), y, k / N, None, False, "power")
    ref = np.abs(np.fft.fft(y)[k]) ** 2 / N
    assert R.deviation(P, ref[None]) <= 1e-12


def test_float32_restatement_deviation():
    """the figure the GPU allowance rests on: lomb_def32 against lomb_def over the GPU test's cases"""
    worst, where = 0.0, None
    for name, form in R.CASES:
        dev = R.deviation(R.reference32(name, form), R.reference(name, form))
        print("  %-12s %-16s %.3e" % (name, R.form_id(form), dev))
        if dev > worst:
            worst, where = dev, (name, R.form_id(form))
    print("float32 restatement: %.3e at %s; recorded %.3e; allowance %.3e" % (worst, where, R.F32_DEV, R.ALLOWANCE))
    assert 0.5 * R.F32_DEV <= worst <= R.F32_DEV
    assert R.ALLOWANCE == R.MARGIN * R.F32_DEV and R.MARGIN == 4.0 and R.ALLOWANCE <= R.PARITY == 2e-4
    assert R.LOMB_SUB == E.LOMB_SUB == 256


def test_float32_restatement_below_one_over_span():
    """what the documents say about the bins under 1 / span, which ls_grid's default starts with: at 1 / (5 span) a floating-mean fit
    amplifies float32 rounding some 40 times (the sinusoid, the constant and the record's window are close to collinear)"""
    t, y, w, f = R.signals("n1000-m300")
    fl = np.concatenate([[0.002], f])                       # 1 / (5 span), then the case's own list
    y32 = R.front32(y[0], None, False, True)[None, :]
    worst = {}
    for nz in ("normalize", "amplitude"):
        a, b = R.lomb_def32(t, y32, fl, None, True, nz), R.lomb_def(t, y, fl, None, True, nz)
        err = np.abs(a - b)[0] / np.max(np.abs(b))
        worst[nz] = (float(err[0]), float(np.max(err[1:])))
        print("%s: %.2e of the row maximum at 1 / (5 span), %.2e from 1 / span on" % ((nz,) + worst[nz]))
    assert worst["amplitude"][1] <= R.F32_DEV and worst["normalize"][1] <= R.F32_DEV
    assert 10 * R.F32_DEV <= worst["amplitude"][0] <= 1e-4 and worst["normalize"][0] <= 1e-4


def test_sums_of_two_parts_add_up_to_the_wholes():
    t, y, w, f = R.signals("tails")
    mean, cut = y.mean(axis=-1), 333
    whole = R.sums_def(t, y, f, w, t[0], mean)
    a = R.sums_def(t[:cut], y[:, :cut], f, w[:cut], t[0], mean)
    b = R.sums_def(t[cut:], y[:, cut:], f, w[cut:], t[0], mean)
    sa, sb = w[:cut].sum() / w.sum(), w[cut:].sum() / w.sum()         # each part normalised its weights by its own sum
    for p, q, r in zip(a, b, whole):
        assert np.max(np.abs(sa * p + sb * q - r)) <= 1e-13 * np.max(np.abs(r))
    wrong = R.sums_def(t[cut:], y[:, cut:], f, w[cut:], t[cut], mean)         # an origin of its own does not add up
    assert np.max(np.abs(sa * a[1] + sb * wrong[1] - whole[1])) > 1e-3 * np.max(np.abs(whole[1]))


def test_level_on_white_noise():
    rng = np.random.default_rng(7)
    N, M, draws, p = 200, 400, 50, 0.05
    lvl = LS.ls_level(N, p)
    assert lvl == pytest.approx(1 - p ** (2.0 / (N - 3)), rel=1e-12)
    above = 0
    for _ in range(draws):
        t = np.sort(rng.uniform(0.0, 100.0, N))
        f = np.linspace(0.05, 0.9, M)                       # inside the Nyquist frequency of the mean rate, from 5 / span on
        z = ss.lombscargle(t, rng.standard_normal(N), 2 * np.pi * f, normalize=True, floating_mean=True)
        above += int(np.sum(z > lvl))
    share = above / float(draws * M)
    print("share of the normalised periodogram above the 5 %% level %.5f: %.4f" % (lvl, share))
    assert 0.035 <= share <= 0.065
    # over independent frequencies the level rises: 1 - (1 - p1)^nindep = p
    p1 = 1 - (1 - p) ** (1 / 50.0)
    assert LS.ls_level(N, p, nindep=50) == pytest.approx(1 - p1 ** (2.0 / (N - 3)), rel=1e-10) and LS.ls_level(N, p, 50) > lvl
    for bad in (lambda: LS.ls_level(3, 0.05), lambda: LS.ls_level(100, 0.0), lambda: LS.ls_level(100, 1.0), lambda: LS.ls_level(100, 0.05, 0.5)):
        with pytest.raises(E.LombRefused):
            bad()


def test_grid_and_the_spectral_window_of_an_even_clock():
    fs, N = 8.0, 160
    t = 3.0 + np.arange(N) / fs
    f = LS.ls_grid(t, oversample=5, nyquist_factor=1.0)
    span = t[-1] - t[0]
    assert f[0] == pytest.approx(1 / (5 * span)) and np.allclose(np.diff(f), f[0]) and f[-1] <= N / (2 * span) < f[-1] + f[0]
    assert LS.ls_grid(t, oversample=5, nyquist_factor=2.0).size in (2 * f.size, 2 * f.size + 1)
    for bad in (lambda: LS.ls_grid([1.0]), lambda: LS.ls_grid([2.0, 2.0]), lambda: LS.ls_grid(t, oversample=0), lambda: LS.ls_grid([[0.0, 1.0]])):
        with pytest.raises(E.LombRefused):
            bad()
    # the window's sums: peaks of height 1 at the multiples of the sample rate, and well below 1 between them
    fw = np.linspace(0.0, 2 * fs, 321)
    common, _, totals = R.sums_def(t, np.zeros((0, N)), fw, None, t[0], np.zeros(0))
    win = (common[:, 0] ** 2 + common[:, 1] ** 2) / totals[0] ** 2
    assert np.allclose(win[[0, 160, 320]], 1.0, atol=1e-12) and np.max(np.delete(win, [0, 1, 159, 160, 161, 319, 320])) < 0.5


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.UNEVEN_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.UNEVEN_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


GOOD = dict(t=True, w=True, y=True, y_ld=100, N=100, batch=2, t_ref=0.5, wnorm=0.0, f=(0.1, 0.2, 0.3), f_ptr=True, M=3, mean=(0.0, 0.0),
            fm=1, nz=1, P=True, common=True, rows=True, totals=True)
SENT = -12345.0


def _call(lib, entry, **over):
    p = dict(GOOD, **over)
    t, w = np.arange(400, dtype=np.float64), np.ones(400)
    y = np.ones(800, dtype=np.float32)
    f = np.array(list(p["f"]) + [0.0] * 8, dtype=np.float64)
    mean = np.array(list(p["mean"]) * 4, dtype=np.float64)
    P = np.full(64, SENT, dtype=np.float32)
    outs = [np.full(64, SENT, dtype=np.float64) for _ in range(3)]
    ptr = _ffi.ptr
    if entry == "sp_lomb":
        rc = lib.sp_lomb(ptr(t) if p["t"] else None, ptr(w) if p["w"] else None, ptr(y) if p["y"] else None, p["y_ld"], p["N"], p["batch"],
                         p["t_ref"], ptr(f) if p["f_ptr"] else None, p["M"], ptr(mean), p["fm"], p["nz"], ptr(P) if p["P"] else None, 0)
    elif entry == "sp_lomb_sums":
        rc = lib.sp_lomb_sums(ptr(t) if p["t"] else None, ptr(w) if p["w"] else None, ptr(y) if p["y"] else None, p["y_ld"], p["N"], p["batch"],
                              p["t_ref"], p["wnorm"], ptr(f) if p["f_ptr"] else None, p["M"], ptr(mean),
                              *[ptr(o) if p[k] else None for o, k in zip(outs, ("common", "rows", "totals"))], 0)
    else:
        ins = [np.ones(64) for _ in range(3)]
        rc = lib.sp_lomb_finish(*[ptr(a) if p[k] else None for a, k in zip(ins, ("common", "rows", "totals"))], p["N"], p["batch"], p["t_ref"],
                                ptr(f) if p["f_ptr"] else None, p["M"], ptr(mean), p["fm"], p["nz"], ptr(P) if p["P"] else None, 0)
    return rc, (lib.sp_last_error() or b"").decode(), [P] + outs


SHARED = [(dict(N=0), "N must"), (dict(N=1 << 31), "N must"), (dict(M=0), "M must"), (dict(M=(1 << 24) + 1), "M must"),
          (dict(batch=-1), "batch"), (dict(batch=65536), "batch"), (dict(f=(0.1, float("nan"), 0.3)), "f must"),
          (dict(f=(float("inf"), 0.2, 0.3)), "f must"), (dict(t_ref=float("nan")), "t_ref"), (dict(t_ref=float("inf")), "t_ref"),
          (dict(mean=(0.0, float("nan"))), "mean"), (dict(f_ptr=False), "f is")]
REFUSALS = ([("sp_lomb", o, w) for o, w in SHARED + [(dict(y_ld=99), "y_ld"), (dict(nz=3), "normalize"), (dict(nz=-1), "normalize"),
                                                     (dict(t=False), "t is"), (dict(y=False), "y is"), (dict(P=False), "P is")]]
            + [("sp_lomb_sums", o, w) for o, w in SHARED + [(dict(y_ld=99), "y_ld"), (dict(t=False), "t is"), (dict(y=False), "y is"),
                                                          (dict(wnorm=float("nan")), "wnorm"), (dict(common=False), "common is"),
                                                          (dict(rows=False), "rows is"), (dict(totals=False), "totals is")]]
            + [("sp_lomb_finish", o, w) for o, w in SHARED + [(dict(nz=3), "normalize"), (dict(common=False), "common is"),
                                                            (dict(rows=False), "rows is"), (dict(totals=False), "totals is"),
                                                            (dict(P=False), "P is")]])


@pytest.mark.parametrize("entry,over,word", REFUSALS, ids=["%s-%s-%d" % (e, w.split()[0], i) for i, (e, _, w) in enumerate(REFUSALS)])
def test_c_refusals(entry, over, word):
    rc, msg, outs = _call(_c_entry(), entry, **over)
    assert rc < 0 and msg.startswith(entry + ": ") and word in msg, (rc, msg)
    assert all(np.all(o == o.dtype.type(SENT)) for o in outs)


def test_nothing_to_do():
    lib = _c_entry()
    for entry in ("sp_lomb", "sp_lomb_finish"):
        rc, _, outs = _call(lib, entry, batch=0)
        assert rc == 0 and all(np.all(o == o.dtype.type(SENT)) for o in outs)
        rc, _, outs = _call(lib, entry, batch=0, y=False)           # without rows y is not looked at
        assert rc == 0 or entry == "sp_lomb_finish"


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_LOMB_FREQS", raising=False)
    monkeypatch.delenv("SP_LOMB_SPLIT", raising=False)
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    plan = lambda N, M, b: (lib.sp_lomb_plan(N, M, b, _ffi.ptr(out)), tuple(int(v) for v in out))[1]
    # before the library is initialised the plan counts 256 CUs: about 4 x 256 workgroups over (tile, group, run), runs of >= 1024 samples
    assert plan(1000, 300, 1) == (1, 300, 1, 1, 2)
    assert plan(1 << 16, 64, 1) == (1, 64, 1, 64, 64)                       # one tile: 64 runs of 1024 samples
    assert plan(1 << 17, 1 << 17, 8) == (8, 1 << 17, 1, 2, 1024)
    assert plan(777, 257, 3) == (4, 257, 1, 1, 2) and plan(500, 130, 17) == (8, 130, 1, 1, 3) and plan(5, 1, 0) == (0, 1, 1, 1, 1)
    # 2^24 frequencies, 8 rows: a tile's partials are 256 x 20 float64 = 40 KiB, 6553 tiles in 256 MiB
    assert plan(1 << 20, 1 << 24, 8) == (8, 6553 * 256, 11, 1, 65536)
    # 65535 rows are 8192 groups: one tile of all of them does not fit, 6553 groups go into a launch
    assert plan(4096, 256, 65535) == (8, 256, 1, 1, 8192)
    monkeypatch.setenv("SP_LOMB_FREQS", str(R.FREQS_HOOK))
    assert plan(600, 300, 2) == (4, 128, 3, 1, 3)
    monkeypatch.setenv("SP_LOMB_SPLIT", str(R.SPLIT_HOOK))
    assert plan(1500, 100, 3) == (4, 100, 1, 5, 5) and plan(3, 100, 1)[3] == 1         # never more runs than samples allow
    monkeypatch.setenv("SP_LOMB_FREQS", "0")
    monkeypatch.setenv("SP_LOMB_SPLIT", "0")
    assert plan(600, 300, 2) == (4, 300, 1, 1, 2)
    assert E.lomb_plan(1 << 16, 64) == dict(rows_per_group=1, freqs_per_pass=64, passes=1, split=64, workgroups=64) == LS.ls_plan(1 << 16, 64)
    assert lib.sp_lomb_plan(100, 10, 1, None) < 0
    for bad in ((0, 10, 1), (1 << 31, 10, 1), (100, 0, 1), (100, (1 << 24) + 1, 1), (100, 10, -1), (100, 10, 65536)):
        assert lib.sp_lomb_plan(*bad, _ffi.ptr(out)) < 0
        with pytest.raises(E.LombRefused):
            E.lomb_plan(*bad)


def _both(exc):
    return isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    t, y, f = np.arange(50.0), np.ones(50, dtype=np.float32), [0.1, 0.2]
    tn, yn = t.copy(), y.copy()
    tn[3], yn[4] = np.nan, np.inf
    bad = [lambda: E.lomb(t, y, []), lambda: E.lomb(t, y[:49], f), lambda: E.lomb(t.reshape(5, 10), y, f), lambda: E.lomb(t, y, [[0.1]]),
           lambda: E.lomb(t, y, [0.1, np.nan]), lambda: E.lomb(tn, y, f), lambda: E.lomb(t, yn, f), lambda: E.lomb(t, y, f, weights=np.ones(49)),
           lambda: E.lomb(t, y, f, weights=-np.ones(50)), lambda: E.lomb(t, y, f, weights=np.zeros(50)),
           lambda: E.lomb(t, y, f, weights=np.full(50, np.nan)), lambda: E.lomb(t, y, f, normalize="psd"), lambda: E.lomb(t, y, f, normalize=3),
           lambda: E.lomb(t, y, f, t_ref=np.inf), lambda: E.lomb(t, y, f, mean_value=np.nan), lambda: E.lomb(t, y, f, mean_value=[0.0, 1.0]),
           lambda: E.lomb(t, None, f), lambda: E.lomb(np.zeros(0), np.zeros(0, dtype=np.float32), f),
           lambda: E.lomb(t, np.ones((65536, 50), dtype=np.float32), f), lambda: E.lomb_sums(t, y, f, wnorm=0.0),
           lambda: E.lomb_sums(t, y, f, wnorm=np.inf), lambda: E.lomb_sums(tn, None, f), lambda: E.lomb_finish((1, 2, 3), f),
           lambda: E.lomb_finish(E.LombSums(np.ones((3, 4)), np.ones((3, 2)), np.ones(3), np.zeros(1), 0.0, 50), f),
           lambda: LS.ls_periodogram(t, y, f, weights=-np.ones(50)), lambda: LS.ls_window(tn, f), lambda: E.lomb_plan(0, 1)]
    for fn in bad:
        with pytest.raises(E.LombRefused) as exc:
            fn()
        assert _both(exc)
    assert LS.LombRefused is E.LombRefused
    a = E.LombSums(np.ones((2, 4)), None, np.ones(1), np.zeros(0), 1.0, 5)
    s = a + a
    assert s.N == 10 and s.rows is None and np.all(s.common == 2)
    with pytest.raises(E.LombRefused):
        a + E.LombSums(np.ones((2, 4)), None, np.ones(1), np.zeros(0), 2.0, 5)


def test_lombscargle_raises_scipys_errors(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    t, y, f = np.arange(20.0), np.ones(20), np.array([0.5, 1.0])
    cases = [((t, y[:19], f), {}), ((t.reshape(4, 5), y.reshape(4, 5), f), {}), ((np.zeros(0), np.zeros(0), f), {}), ((t, y, np.zeros(0)), {}),
             ((t, y, f.reshape(1, 2)), {}), ((t, y, f), dict(weights=np.ones(19))), ((t, y, f), dict(weights=-np.ones(20))),
             ((t, y, f), dict(weights=np.zeros(20))), ((t, y, f), dict(normalize="psd"))]
    for args, kw in cases:
        with pytest.raises(ValueError) as ours:
            pyfft_amd.lombscargle(*args, **kw)
        with pytest.raises(ValueError) as theirs:
            ss.lombscargle(*args, **kw)
        assert str(ours.value) == str(theirs.value)
        assert not isinstance(ours.value, E.LombRefused)


def test_exported_declared_and_bound():
    for name in ("lombscargle", "ls_periodogram", "ls_window", "ls_grid", "ls_level", "ls_plan"):
        assert getattr(pyfft_amd, name) is getattr(LS, name)
    for name in ("lomb", "lomb_sums", "lomb_finish", "lomb_plan", "lomb_check", "LOMB_SUB", "LombRefused"):
        assert hasattr(E, name)
    assert issubclass(E.LombRefused, ValueError) and issubclass(E.LombRefused, NotImplementedError)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_uneven.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.UNEVEN_SIGNATURES) == {"sp_lomb", "sp_lomb_sums", "sp_lomb_finish", "sp_lomb_plan"}
    others = (set(_ffi.SIGNATURES) | set(_ffi.EXT_SIGNATURES) | set(_ffi.TFR_SIGNATURES) | set(_ffi.QUAD_SIGNATURES)
              | set(_ffi.CYCLO_SIGNATURES))
    assert not set(_ffi.UNEVEN_SIGNATURES) & others
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_lomb", 14), ("sp_lomb_sums", 15), ("sp_lomb_finish", 13), ("sp_lomb_plan", 4)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.UNEVEN_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.UNEVEN_SIGNATURES[name][1]
    for other in ("spectral.h", "spectral_ext.h", "spectral_tfr.h", "spectral_quad.h", "spectral_cyclo.h"):
        assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other)))
    assert "spectral_uneven.h" in open(os.path.join(ROOT, "Makefile")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "SP_LOMB_FREQS" in launch and "SP_LOMB_SPLIT" in launch
