"""The type-2 NUFFT, the fit and regridding without a GPU: the measured method and float32 figures the GPU test's allowances rest on
(tests/nufft2_ref.py), the adjoint identity of the two float64 algorithms, the conjugate-gradient restatement against the float64 solve,
the plan figures, the refusals of the C entries and of their Python front ends before the library is loaded, regrid's default period
and mode count, and the declared set of include/spectral_nufft2.h.  pyfft_amd/csrc/nufft_plan.h gained no arithmetic with type 2
(the interpolation kernel's workgroup count is a sum in sp_nufft2_plan, held here), so there is no further sanitizer-built program."""
import ctypes
import os
import re

import numpy as np
import pytest

import nufft2_ref as R2
import nufft_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, nufft as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_measured_deviations():
    """METHOD2_DEV and F32_2_DEV: nufft2_def and nufft2_def32 against the direct sums over the GPU test's cases"""
    wm, wf = (0.0, None), (0.0, None)
    for name, sign in R2.CASES:
        t, F, t_ref = R2.signals(name)
        f0, df = R2.grid_of(name)
        ref = R2.reference(name, sign)
        assert F.shape == (R2.SHAPES[name]["rows"], R2.SHAPES[name]["M"]) and F.dtype == np.complex64 and t is R.signals(name)[0]
        a = R2.deviation(R2.nufft2_def(t, F, f0, df, sign, t_ref), ref, F)
        b = R2.deviation(R2.nufft2_def32(t, F, f0, df, sign, t_ref), ref, F)
        print("  %-10s %+d method %.3e float32 %.3e" % (name, sign, a, b))
        wm, wf = max(wm, (a, name)), max(wf, (b, name))
    print("method %.3e at %s, recorded %.3e; float32 %.3e at %s, recorded %.3e; allowance %.3e" % (wm + (R2.METHOD2_DEV,) + wf + (R2.F32_2_DEV, R2.ALLOWANCE2)))
    assert 0.5 * R2.METHOD2_DEV <= wm[0] <= R2.METHOD2_DEV <= 4.0e-8
    assert 0.5 * R2.F32_2_DEV <= wf[0] <= R2.F32_2_DEV
    assert R2.METHOD2_DEV <= R2.F32_2_DEV
    assert R2.ALLOWANCE2 == R.MARGIN * R2.F32_2_DEV and R.MARGIN == 4.0 and R2.ALLOWANCE2 <= R.PARITY == 2e-4
    F7 = R2.signals("rows-17")[1]
    assert not F7[7].any() and abs(F7[3].mean().real) > 900 and abs(F7[11].mean().imag) > 900


def test_the_recorded_device_shares():
    """what tests/test_gpu_nufft2.py used of its allowances on an MI355X"""
    assert 0 < R2.DEVICE_SHARE2 <= 1 and 0 < R2.FIT_DEVICE_SHARE <= 1


@pytest.mark.parametrize("name", ("tails", "seams", "m-odd"))
def test_adjoint_of_the_float64_algorithms(name):
    """<G, nufft_def(c; -)> = <nufft2_def(G; +), c> in float64.  The sums are exact adjoints; the two algorithms place a sample at
    p and at 1 - p (the signs differ), so they are mirror images, not transposes, of each other, and each side carries its own
    method's error: METHOD_DEV of sum|c| per bin and METHOD2_DEV of sum|G| per sample"""
    t, c, t_ref = R.signals(name)
    G_ = R2.signals(name)[1]
    f0, df = R.grid_of(name)
    M = R.SHAPES[name]["M"]
    c, G_ = c[0].astype(np.complex128), G_[0].astype(np.complex128)
    a = np.sum(np.conj(G_) * R.nufft_def(t, c, f0, df, M, -1, t_ref)[0])
    b = np.sum(np.conj(R2.nufft2_def(t, G_, f0, df, 1, t_ref)[0]) * c)
    assert abs(a - b) <= (R.METHOD_DEV + R2.METHOD2_DEV) * np.sum(np.abs(c)) * np.sum(np.abs(G_))
    # and nufft2_def of nufft1's output is A A^H c to the two methods' errors
    F = R.nufft_def(t, c, f0, df, M, -1, t_ref)[0]
    back = R2.nufft2_def(t, F, f0, df, 1, t_ref)[0]
    ref = R2.direct2(t, R.direct(t, c, f0, df, M, -1, t_ref)[0], f0, df, 1, t_ref)[0]
    assert np.max(np.abs(back - ref)) <= (R.METHOD_DEV * M + R2.METHOD2_DEV * M) * np.sum(np.abs(c))


def test_the_fit_restated():
    """FIT_F32_DEV: the conjugate-gradient fit with complex64 transforms against the float64 solve over the two fit cases; the float64
    iteration's counts"""
    f0, df, M = R2.fit_grid()
    assert (f0, df, M) == (-0.4, 0.01, 81)
    worst = 0.0
    for name in R2.FIT_CASES:
        t, y, F_true = R2.fit_signals(name)
        assert y.dtype == np.complex64 and np.all(np.diff(t) > 0)
        if name == "gapped":
            assert t.size < R2.FIT_N and not np.any((t > 50) & (t < 53))
        ref = R2.fit_def(t, y, f0, df, M)[0]
        assert np.linalg.norm(ref - F_true) <= 1e-6 * np.linalg.norm(F_true)           # y = A F_true rounded to complex64
        F64, it64, ok64 = R2.fit_cg(t, y, f0, df, M, f32=False)
        F32, it32, ok32 = R2.fit_cg(t, y, f0, df, M, f32=True)
        d64, d32 = R2.fit_deviation(F64, ref), R2.fit_deviation(F32, ref)
        A = R2.design(t, f0, df, M)
        print("  %-7s N %d cond %.3g: float64 %d iterations, off %.3e; complex64 %d iterations, off %.3e" %
              (name, t.size, np.linalg.cond(A.conj().T @ A), it64, d64, it32, d32))
        assert ok64.all() and ok32.all() and it64 == R2.FIT_ITERATIONS[name][0] and it32 <= R2.FIT_ITERATIONS[name][1]
        worst = max(worst, d32)
        assert np.array_equal(R2.fit_def32(t, y, f0, df, M), F32)
    print("complex64 fit off by %.3e at the most, recorded %.3e" % (worst, R2.FIT_F32_DEV))
    assert 0.5 * R2.FIT_F32_DEV <= worst <= R2.FIT_F32_DEV and R2.FIT_ALLOWANCE == R.MARGIN * R2.FIT_F32_DEV
    assert R2.FIT_ITERATIONS == {"clean": (5, 8), "gapped": (12, 16)}


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.NUFFT2_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.NUFFT2_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


def plan_ref(M, rows, rows_force=0):
    """nufft_ref.plan_of with the interpolation kernel's own workgroup count: row groups of 4"""
    nf, w, tiles, tile, rpp, passes, _ = R.plan_of(M, rows, rows_force=rows_force)
    return nf, w, tiles, tile, rpp, passes, sum(tiles * -(-min(rpp, rows - r0) // 4) for r0 in range(0, rows, rpp)), 4


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_NUFFT_ROWS", raising=False)
    lib = _c_entry()
    out = np.zeros(8, dtype=np.int64)
    plan = lambda N, M, b: (lib.sp_nufft2_plan(N, M, b, _ffi.ptr(out)), tuple(int(v) for v in out))[1]
    shapes = [(777, 257, 3), (1000, 3000, 1), (1000, 5000, 1), (500, 130, 17), (1 << 20, 1 << 20, 9), (1, 1, 1), (5, 1 << 24, 65535), (5, 7, 0)]
    for N, M, b in shapes:
        assert plan(N, M, b) == plan_ref(M, b), (N, M, b)
    assert plan(1000, 3000, 1) == (8192, 8, 8, 1024, 1, 1, 8, 4) and plan(1 << 20, 1 << 20, 9) == (1 << 21, 8, 2048, 1024, 9, 1, 3 * 2048, 4)
    assert plan(5, 1 << 24, 3) == (1 << 25, 8, 32768, 1024, 1, 3, 3 * 32768, 4)             # 256 MiB a row: one row per pass
    monkeypatch.setenv("SP_NUFFT_ROWS", str(R.ROWS_HOOK))
    assert plan(500, 130, 17) == plan_ref(130, 17, R.ROWS_HOOK) == (1024, 8, 1, 1024, 2, 9, 9, 4)
    monkeypatch.setenv("SP_NUFFT_ROWS", "0")
    assert plan(500, 130, 17) == (1024, 8, 1, 1024, 17, 1, 5, 4)
    d = E.nufft2_plan(1000, 3000, 5)
    assert d == NU.nufft_plan(1000, 3000, 5, type=2) == NU.nufft2_plan(1000, 3000, 5) == pyfft_amd.nufft2_plan(1000, 3000, 5)
    assert tuple(d[k] for k in ("nf", "width", "tiles", "tile", "rows_per_pass", "passes", "workgroups", "row_group")) == plan_ref(3000, 5)
    assert NU.nufft_plan(1000, 3000, 5) == NU.nufft_plan(1000, 3000, 5, type=1) == E.nufft_plan(1000, 3000, 5)      # as it was
    assert lib.sp_nufft2_plan(100, 10, 1, None) < 0
    for bad in ((0, 10, 1), (1 << 31, 10, 1), (100, 0, 1), (100, (1 << 24) + 1, 1), (100, 10, -1), (100, 10, 65536)):
        assert lib.sp_nufft2_plan(*bad, _ffi.ptr(out)) < 0
        with pytest.raises(E.NufftRefused):
            E.nufft2_plan(*bad)
    with pytest.raises(E.NufftRefused):
        NU.nufft_plan(100, 10, 1, type=3)
    # the staged rows of a group stay within the 64 KiB a launch gets unasked
    assert d["row_group"] * (d["tile"] + d["width"] - 1) * 8 <= 64 * 1024


GOOD = dict(t=True, F=True, fld=3, N=100, batch=2, t_ref=0.5, f0=0.1, df=0.01, M=3, sign=1, out=True, old=100)
SENT = -12345.0
NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(N=0), "N must"), (dict(N=1 << 31), "N must"), (dict(M=0), "M must"), (dict(M=(1 << 24) + 1, fld=1 << 25), "M must"),
            (dict(batch=-1), "batch"), (dict(batch=65536), "batch"), (dict(fld=2), "F_ld"), (dict(old=99), "out_ld"),
            (dict(t_ref=NAN), "t_ref"), (dict(t_ref=INF), "t_ref"), (dict(f0=NAN), "f0"), (dict(f0=-INF), "f0"),
            (dict(df=NAN), "df must be finite"), (dict(df=INF), "df must be finite"), (dict(df=0.0), "df must not be zero"),
            (dict(f0=1e308, df=1e308), "f0 + M df"), (dict(sign=0), "sign"), (dict(sign=2), "sign"), (dict(t=False), "t is"),
            (dict(F=False), "F is"), (dict(out=False), "out is")]


def _call(lib, **over):
    p = dict(GOOD, **over)
    t, F = np.arange(400, dtype=np.float64), np.ones(800, dtype=np.complex64)
    out = np.full(400, SENT, dtype=np.complex64)
    ptr = _ffi.ptr
    rc = lib.sp_nufft2(ptr(t) if p["t"] else None, ptr(F) if p["F"] else None, p["fld"], p["N"], p["batch"], p["t_ref"], p["f0"], p["df"], p["M"],
                       p["sign"], ptr(out) if p["out"] else None, p["old"], 0)
    return rc, (lib.sp_last_error() or b"").decode(), out


@pytest.mark.parametrize("over,word", REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(REFUSALS)])
def test_c_refusals(over, word):
    rc, msg, out = _call(_c_entry(), **over)
    assert rc == -1 and msg.startswith("sp_nufft2: ") and word in msg, (rc, msg)
    assert np.all(out == np.complex64(SENT))


def test_nothing_to_do():
    rc, _, out = _call(_c_entry(), batch=0)
    assert rc == 0 and np.all(out == np.complex64(SENT))


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    t, F, y = np.arange(50.0), np.ones(5, dtype=np.complex64), np.ones(50, dtype=np.float32)
    tn, Fn, yn = t.copy(), F.copy(), y.copy()
    tn[3], Fn[4], yn[7] = np.nan, np.inf, np.nan
    t_new = np.linspace(1.0, 48.0, 16)
    bad = [lambda: E.nufft2(t.reshape(5, 10), F, 0.1, 0.1), lambda: E.nufft2(t, np.zeros((2, 0), dtype=np.complex64), 0.1, 0.1),
           lambda: E.nufft2(t, np.ones((1 << 24) + 1, dtype=np.complex64), 0.1, 0.1), lambda: E.nufft2(t, F, 0.1, 0.0),
           lambda: E.nufft2(t, F, np.nan, 0.1), lambda: E.nufft2(t, F, 0.1, np.inf), lambda: E.nufft2(t, F, 0.1, 0.1, sign=0),
           lambda: E.nufft2(t, F, 0.1, 0.1, sign=2), lambda: E.nufft2(t, F, 0.1, 0.1, t_ref=np.inf), lambda: E.nufft2(tn, F, 0.1, 0.1),
           lambda: E.nufft2(t, Fn, 0.1, 0.1), lambda: E.nufft2(np.zeros(0), F, 0.1, 0.1),
           lambda: E.nufft2(t, np.ones((65536, 2), dtype=np.complex64), 0.1, 0.1), lambda: NU.nufft2_modes(tn, F),
           lambda: E.nufft2_plan(0, 1), lambda: NU.nufft_plan(10, 10, 1, type=0),
           lambda: NU.nufft_fit(t, y, 0.1, 0.1, 0), lambda: NU.nufft_fit(t, y, 0.1, 0.1, (1 << 23) + 1), lambda: NU.nufft_fit(t, y, 0.1, 0.0, 5),
           lambda: NU.nufft_fit(t, y, 0.1, 0.1, 5, ridge=-1.0), lambda: NU.nufft_fit(t, y, 0.1, 0.1, 5, rtol=0.0),
           lambda: NU.nufft_fit(tn, y, 0.1, 0.1, 5), lambda: NU.nufft_fit(t, yn, 0.1, 0.1, 5), lambda: NU.nufft_fit(t, y[:49], 0.1, 0.1, 5),
           lambda: NU.nufft_fit(t, y, 0.1, 0.1, 5, weights=-np.ones(50)), lambda: NU.nufft_fit(t, y, 0.1, 0.1, 5, weights=np.ones(49)),
           lambda: NU.regrid(t, y, t_new, 0.6), lambda: NU.regrid(t, y, np.append(t_new, 49.5), 0.2),
           lambda: NU.regrid(t, y, np.append(-0.5, t_new), 0.2), lambda: NU.regrid(t, y, t_new, 0.2, period=-1.0),
           lambda: NU.regrid(t, y, t_new, np.nan), lambda: NU.regrid(t[:1], y[:1], t[:1], 0.2), lambda: NU.regrid(t, y, t_new, 0.2, rtol=-1.0)]
    for i, fn in enumerate(bad):
        with pytest.raises(E.NufftRefused) as exc:
            fn()
        assert isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError), i
    with pytest.raises(E.NufftRefused, match="more unknowns than samples"):
        NU.regrid(t, y, t_new, 0.6)                         # period 50: K = 30, M = 61 > 50
    with pytest.raises(E.NufftRefused, match="says nothing outside"):
        NU.regrid(t, y, np.array([49.0001]), 0.2)
    assert NU.NufftRefused is E.NufftRefused and NU.FIT_MAX_M == 1 << 23


def test_regrid_default_period_and_modes():
    """the default period closes the circle: span N / (N - 1), so that uniform samples give the harmonics of their own transform"""
    period, K, M, f0, df = NU.regrid_grid(0.0, 99.75, 400, 0.4)
    assert (period, K, M, f0, df) == (100.0, 40, 81, -0.4, 0.01)
    assert NU.regrid_grid(3.0, 102.75, 400, 0.405)[1:3] == (40, 81)               # floor
    assert NU.regrid_grid(0.0, 99.75, 400, 0.0)[1:] == (0, 1, 0.0, 0.01)          # the mean alone
    assert NU.regrid_grid(0.0, 99.75, 400, 0.4, period=50.0) == (50.0, 20, 41, -0.4, 0.02)
    assert NU.regrid_grid(0.0, 49.0, 50, 0.49)[:3] == (50.0, 24, 49)
    with pytest.raises(E.NufftRefused, match="more unknowns than samples"):
        NU.regrid_grid(0.0, 49.0, 50, 0.5)                  # K = 25, M = 51 > N = 50
    for bad in (lambda: NU.regrid_grid(1.0, 1.0, 5, 0.1), lambda: NU.regrid_grid(0.0, 1.0, 1, 0.1), lambda: NU.regrid_grid(0.0, 1.0, 5, -0.1),
                lambda: NU.regrid_grid(0.0, 1.0, 5, 0.1, period=0.0), lambda: NU.regrid_grid(0.0, 1.0, 5, 0.1, period=np.inf)):
        with pytest.raises(E.NufftRefused):
            bad()


def test_exported_declared_and_bound():
    for name in ("nufft2", "nufft2_modes", "nufft2_plan", "nufft_fit", "regrid", "NufftFit"):
        assert getattr(pyfft_amd, name) is getattr(NU, name)
    for name in ("nufft2", "nufft2_plan"):
        assert hasattr(E, name)
    assert NU.NufftFit._fields == ("F", "iterations", "converged", "residual")
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_nufft2.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.NUFFT2_SIGNATURES) == {"sp_nufft2", "sp_nufft2_plan"}
    assert len(_ffi.TABLES) == 6 and _ffi.NUFFT2_SIGNATURES in _ffi.MORE_TABLES and all(t is not _ffi.NUFFT2_SIGNATURES for t in _ffi.TABLES)
    for table in _ffi.TABLES + tuple(t for t in _ffi.MORE_TABLES if t is not _ffi.NUFFT2_SIGNATURES):
        assert not set(_ffi.NUFFT2_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_nufft2", 13), ("sp_nufft2_plan", 4)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.NUFFT2_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.NUFFT2_SIGNATURES[name][1]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "spectral_nufft2.h":
            assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other))), other
    assert "spectral_nufft2.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert '#include "../../include/spectral_nufft2.h"' in open(os.path.join(ROOT, "pyfft_amd", "csrc", "spectral.hip")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "NUFFT2_RG 4" in launch and "launch_nufft2_interp" in launch and "launch_nufft2_place" in launch
    ext = open(os.path.join(ROOT, "include", "spectral_ext.h")).read()
    assert "which = 6" in ext and "sp_nufft2" in ext and "nufft2" in E.last_passes.__doc__
    kernel = open(os.path.join(ROOT, "pyfft_amd", "csrc", "k_nufft2.hip")).read()
    assert "atomic" not in kernel.split("#include")[1].lower() and "hipMemset" not in kernel            # no atomics, no memset
