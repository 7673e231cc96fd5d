"""The type-1 NUFFT and the fast Lomb-Scargle sums without a GPU: the measured method and float32 figures the GPU test's allowances rest
on (tests/nufft_ref.py), integer sums that no order of the samples changes, the plan figures, the refusals of the C entries and of
their Python front ends, the uniform-grid rule of method='fast', the unchanged direct path, the declared set of
include/spectral_nufft.h, and the host arithmetic of pyfft_amd/csrc/nufft_plan.h under AddressSanitizer as its own program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lomb_ref as L
import nufft_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, lomb as LS, nufft as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_measured_deviations():
    """METHOD_DEV and F32_DEV: nufft_def and nufft_def32 against the direct sums over the GPU test's cases"""
    wm, wf = (0.0, None), (0.0, None)
    for name, sign in R.CASES:
        t, c, t_ref = R.signals(name)
        f0, df = R.grid_of(name)
        M, ref = R.SHAPES[name]["M"], R.reference(name, sign)
        a = R.deviation(R.nufft_def(t, c, f0, df, M, sign, t_ref), ref, c)
        b = R.deviation(R.nufft_def32(t, c, f0, df, M, sign, t_ref), ref, c)
        print("  %-10s %+d method %.3e float32 %.3e" % (name, sign, a, b))
        wm, wf = max(wm, (a, name)), max(wf, (b, name))
    print("method %.3e at %s, recorded %.3e; float32 %.3e at %s, recorded %.3e; allowance %.3e" % (wm + (R.METHOD_DEV,) + wf + (R.F32_DEV, R.ALLOWANCE)))
    assert 0.5 * R.METHOD_DEV <= wm[0] <= R.METHOD_DEV
    assert 0.5 * R.F32_DEV <= wf[0] <= R.F32_DEV
    assert R.METHOD_DEV <= R.F32_DEV                     # the kernel is wide enough: the method's error is under the float32 rounding
    assert R.ALLOWANCE == R.MARGIN * R.F32_DEV and R.MARGIN == 4.0 and R.ALLOWANCE <= R.PARITY == 2e-4
    assert (R.W, R.TILE) == (E.NUFFT_W, E.NUFFT_TILE)


def test_measured_deviations_of_the_periodogram_forms():
    """the same two figures through lomb_ref.finish, against lomb_ref.lomb_def, over every form of the periodogram cases"""
    wm, wf = (0.0, None), (0.0, None)
    for name in R.LS_SHAPES:
        t, y32, w, f, (f0, df) = R.ls_signals(name)
        for wt in (False, True):
            sums = [R.lomb_sums_grid_def(t, y32, f0, df, f.size, w if wt else None, float(t[0]), f32=f32) for f32 in (False, True)]
            for fm in (False, True):
                for nz in R.LS_FORMS_OF[name]:
                    ref = R.ls_reference(name, (wt, fm, nz))
                    a, b = (L.deviation(L.finish(s[0], s[1], s[2], s[3], f, t.size, float(t[0]), fm, nz), ref) for s in sums)
                    wm, wf = max(wm, (a, (name, wt, fm, nz))), max(wf, (b, (name, wt, fm, nz)))
    print("periodogram forms: method %.3e at %s, recorded %.3e; float32 %.3e at %s, recorded %.3e" % (wm + (R.LS_METHOD_DEV,) + wf + (R.LS_F32_DEV,)))
    assert 0.5 * R.LS_METHOD_DEV <= wm[0] <= R.LS_METHOD_DEV
    assert 0.5 * R.LS_F32_DEV <= wf[0] <= R.LS_F32_DEV
    assert R.LS_METHOD_DEV <= R.LS_F32_DEV
    assert R.LS_ALLOWANCE == R.MARGIN * R.LS_F32_DEV <= R.PARITY
    assert all(f[0] == 0.01 for f in (R.ls_signals(n)[3] for n in R.LS_SHAPES))         # from 1 / span on: lomb_ref says why


@pytest.mark.parametrize("name", ("tails", "seams", "pile", "unsorted"))
def test_a_permutation_gives_identical_integers(name):
    t, c, t_ref = R.signals(name)
    f0, df = R.grid_of(name)
    M = R.SHAPES[name]["M"]
    order = np.random.default_rng(3).permutation(t.size)
    a, sa, _, _ = R.spread32(t, c, f0, df, M, 1, t_ref)
    b, sb, _, _ = R.spread32(t[order], c[:, order], f0, df, M, 1, t_ref)
    assert np.array_equal(sa, sb) and np.array_equal(a, b)
    assert np.max(np.abs(a)) < 2 ** 62
    if name == "pile":                                    # eight cells take it all; 500 random strengths add up to some 2^-8 of the bound
        assert np.count_nonzero(a[0, :, 0]) <= R.W and np.max(np.abs(a)) > 2 ** 50


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.NUFFT_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.NUFFT_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_NUFFT_ROWS", raising=False)
    lib = _c_entry()
    out = np.zeros(8, dtype=np.int64)
    plan = lambda N, M, b: (lib.sp_nufft1_plan(N, M, b, _ffi.ptr(out)), tuple(int(v) for v in out[:7]))[1]
    shapes = [(777, 257, 3), (1000, 3000, 1), (1000, 5000, 1), (500, 130, 17), (1 << 20, 1 << 20, 9), (1, 1, 1), (5, 1 << 24, 65535), (5, 7, 0)]
    for N, M, b in shapes:
        assert plan(N, M, b) == R.plan_of(M, b), (N, M, b)
    assert plan(1000, 3000, 1) == (8192, 8, 8, 1024, 1, 1, 8) and plan(1 << 20, 1 << 20, 9) == (1 << 21, 8, 2048, 1024, 9, 1, 6144)
    assert plan(5, 1 << 24, 3) == (1 << 25, 8, 32768, 1024, 1, 3, 3 * 32768)              # 256 MiB a row: one row per pass
    monkeypatch.setenv("SP_NUFFT_ROWS", str(R.ROWS_HOOK))
    assert plan(500, 130, 17) == R.plan_of(130, 17, rows_force=R.ROWS_HOOK) == (1024, 8, 1, 1024, 2, 9, 9)
    assert plan(500, 130, 1)[4:6] == (1, 1)
    monkeypatch.setenv("SP_NUFFT_ROWS", "0")
    assert plan(500, 130, 17) == (1024, 8, 1, 1024, 17, 1, 6)
    d = E.nufft_plan(1000, 3000, 3)
    assert d == NU.nufft_plan(1000, 3000, 3) == pyfft_amd.nufft_plan(1000, 3000, 3)
    assert (d["nf"], d["width"], d["tiles"], d["tile"], d["rows_per_pass"], d["passes"], d["workgroups"]) == R.plan_of(3000, 3)
    assert d["fast_min_pairs"] == int(out[7]) > 0
    assert lib.sp_nufft1_plan(100, 10, 1, None) < 0
    for bad in ((0, 10, 1), (1 << 31, 10, 1), (100, 0, 1), (100, (1 << 24) + 1, 1), (100, 10, -1), (100, 10, 65536)):
        assert lib.sp_nufft1_plan(*bad, _ffi.ptr(out)) < 0
        with pytest.raises(E.NufftRefused):
            E.nufft_plan(*bad)
    assert LS.ls_plan(1 << 16, 64) == E.lomb_plan(1 << 16, 64)                             # as it was
    big, small = LS.ls_plan(1 << 20, 1 << 20, 8, method="auto"), LS.ls_plan(100, 10, 1, method="auto")
    assert big["path"] == "fast" and small["path"] == "direct" and big["fast"] == E.nufft_plan(1 << 20, 1 << 20, 9)
    assert LS.ls_plan(100, 10, 1, method="fast")["path"] == "fast" and LS.ls_plan(1 << 20, 1 << 20, 8, method="direct")["path"] == "direct"
    with pytest.raises(E.LombRefused):
        LS.ls_plan(100, 10, 1, method="quick")


GOOD = dict(t=True, c=True, ld=100, N=100, batch=2, t_ref=0.5, f0=0.1, df=0.01, M=3, sign=1, out=True, w=True, y=True, wnorm=0.0,
            mean=(0.0, 0.0), common=True, rows=True, totals=True)
SENT = -12345.0


def _call(lib, entry, **over):
    p = dict(GOOD, **over)
    t, w = np.arange(400, dtype=np.float64), np.ones(400)
    c = np.ones(800, dtype=np.complex64)
    y = np.ones(800, dtype=np.float32)
    mean = np.array(list(p["mean"]) * 4, dtype=np.float64)
    ptr = _ffi.ptr
    if entry == "sp_nufft1":
        outs = [np.full(64, SENT, dtype=np.complex64)]
        rc = lib.sp_nufft1(ptr(t) if p["t"] else None, ptr(c) if p["c"] else None, p["ld"], p["N"], p["batch"], p["t_ref"], p["f0"], p["df"],
                           p["M"], p["sign"], ptr(outs[0]) if p["out"] else None, 0)
    else:
        outs = [np.full(64, SENT, dtype=np.float64) for _ in range(3)]
        rc = lib.sp_lomb_sums_grid(ptr(t) if p["t"] else None, ptr(w) if p["w"] else None, ptr(y) if p["y"] else None, p["ld"], p["N"],
                                   p["batch"], p["t_ref"], p["wnorm"], p["f0"], p["df"], p["M"], ptr(mean),
                                   *[ptr(o) if p[k] else None for o, k in zip(outs, ("common", "rows", "totals"))], 0)
    return rc, (lib.sp_last_error() or b"").decode(), outs


NAN, INF = float("nan"), float("inf")
SHARED = [(dict(N=0), "N must"), (dict(N=1 << 31), "N must"), (dict(M=0), "M must"), (dict(M=(1 << 24) + 1), "M must"),
          (dict(batch=-1), "batch"), (dict(batch=65536), "batch"), (dict(ld=99), "_ld"), (dict(t_ref=NAN), "t_ref"), (dict(t_ref=INF), "t_ref"),
          (dict(f0=NAN), "f0"), (dict(f0=-INF), "f0"), (dict(df=NAN), "df must be finite"), (dict(df=INF), "df must be finite"),
          (dict(df=0.0), "df must not be zero"), (dict(f0=1e308, df=1e308), "f0 + M df"), (dict(t=False), "t is")]
REFUSALS = ([("sp_nufft1", o, w) for o, w in SHARED + [(dict(sign=0), "sign"), (dict(sign=2), "sign"), (dict(c=False), "c is"),
                                                       (dict(out=False), "out is")]]
            + [("sp_lomb_sums_grid", o, w) for o, w in SHARED + [(dict(y=False), "y is"), (dict(wnorm=NAN), "wnorm"), (dict(mean=(0.0, NAN)), "mean"),
                                                               (dict(common=False), "common is"), (dict(rows=False), "rows is"),
                                                               (dict(totals=False), "totals is")]])


@pytest.mark.parametrize("entry,over,word", REFUSALS, ids=["%s-%s-%d" % (e, w.split()[0], i) for i, (e, _, w) in enumerate(REFUSALS)])
def test_c_refusals(entry, over, word):
    rc, msg, outs = _call(_c_entry(), entry, **over)
    assert rc == -1 and msg.startswith(entry + ": ") and word in msg, (rc, msg)
    assert all(np.all(o == o.dtype.type(SENT)) for o in outs)


def test_nothing_to_do():
    rc, _, outs = _call(_c_entry(), "sp_nufft1", batch=0)
    assert rc == 0 and np.all(outs[0] == np.complex64(SENT))


def _both(exc):
    return isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    t, c, y = np.arange(50.0), np.ones(50, dtype=np.complex64), np.ones(50, dtype=np.float32)
    tn, cn = t.copy(), c.copy()
    tn[3], cn[4] = np.nan, np.inf
    bad = [lambda: E.nufft1(t, c[:49], 0.1, 0.1, 5), lambda: E.nufft1(t.reshape(5, 10), c, 0.1, 0.1, 5), lambda: E.nufft1(t, c, 0.1, 0.1, 0),
           lambda: E.nufft1(t, c, 0.1, 0.1, (1 << 24) + 1), lambda: E.nufft1(t, c, 0.1, 0.0, 5), lambda: E.nufft1(t, c, np.nan, 0.1, 5),
           lambda: E.nufft1(t, c, 0.1, np.inf, 5), lambda: E.nufft1(t, c, 0.1, 0.1, 5, sign=0), lambda: E.nufft1(t, c, 0.1, 0.1, 5, sign=2),
           lambda: E.nufft1(t, c, 0.1, 0.1, 5, t_ref=np.inf), lambda: E.nufft1(tn, c, 0.1, 0.1, 5), lambda: E.nufft1(t, cn, 0.1, 0.1, 5),
           lambda: E.nufft1(np.zeros(0), np.zeros(0, dtype=np.complex64), 0.1, 0.1, 5),
           lambda: E.nufft1(t, np.ones((65536, 50), dtype=np.complex64), 0.1, 0.1, 5), lambda: NU.nufft1_modes(t, c, 0),
           lambda: E.nufft_plan(0, 1)]
    for fn in bad:
        with pytest.raises(E.NufftRefused) as exc:
            fn()
        assert _both(exc)
    f = 0.1 + 0.05 * np.arange(20)
    lbad = [lambda: E.lomb_sums_grid(t, y, 0.1, 0.0, 5), lambda: E.lomb_sums_grid(t, y, 0.1, 0.1, 0), lambda: E.lomb_sums_grid(t, y, np.nan, 0.1, 5),
            lambda: E.lomb_sums_grid(tn, y, 0.1, 0.1, 5), lambda: E.lomb_sums_grid(t, y, 0.1, 0.1, 5, wnorm=0.0),
            lambda: E.lomb_sums_grid(t, y, 0.1, 0.1, 5, weights=-np.ones(50)), lambda: E.lomb_sums_grid(t, y[:49], 0.1, 0.1, 5),
            lambda: LS.ls_periodogram(t, y, f ** 2, method="fast"), lambda: LS.ls_periodogram(t, y, f, method="quick"),
            lambda: LS.ls_periodogram(t, None, f, method="fast"), lambda: LS.ls_window(t, f ** 2, method="fast"),
            lambda: LS.ls_periodogram(t, y, [0.3, 0.3, 0.3], method="fast")]
    for fn in lbad:
        with pytest.raises(E.LombRefused) as exc:
            fn()
        assert _both(exc)
    assert NU.NufftRefused is E.NufftRefused and E.NUFFT_PASSES == 6


def test_uniform_grid_rule():
    t = np.linspace(3.0, 103.0, 500)                         # span 100
    f0, df, M = 0.01, 0.013, 300
    f = f0 + df * np.arange(M)
    g = LS.uniform_grid(t, f)
    assert g is not None and g[0] == f[0] and g[2] == M and abs(g[1] - df) < 1e-15
    assert LS.uniform_grid(t, np.linspace(0.01, 4.0, 257)) is not None
    bent = f.copy()
    bent[150] += 0.5e-11                                     # 0.5e-9 turns over the span: still a grid
    assert LS.uniform_grid(t, bent) is not None
    bent[150] += 2e-11                                       # 2.5e-9 turns: not any more
    assert LS.uniform_grid(t, bent) is None
    assert LS.uniform_grid(t, f[::-1]) is not None and LS.uniform_grid(t, f[::-1])[1] < 0           # a falling grid is one
    assert LS.uniform_grid(t, [0.3]) == (0.3, 1.0, 1)
    assert LS.uniform_grid(t, [0.3, 0.3]) is None and LS.uniform_grid(t, f ** 2) is None and LS.uniform_grid(t, []) is None
    assert LS.uniform_grid(t, [0.1, np.nan, 0.3]) is None
    assert LS.UNIFORM_TURNS == R.UNIFORM_TURNS == 1e-9


def test_the_direct_method_is_the_call_it_was(monkeypatch):
    seen = []
    monkeypatch.setattr(E, "lomb", lambda *a, **k: seen.append(("lomb", a, k)) or "P")
    monkeypatch.setattr(E, "lomb_sums", lambda *a, **k: seen.append(("lomb_sums", a, k)) or E.LombSums(np.ones((2, 4)), None, np.ones(1), np.zeros(0), 0.0, 5))
    monkeypatch.setattr(E, "lomb_sums_grid", lambda *a, **k: seen.append(("grid", a, k)))
    t, y, f, w = np.arange(5.0), np.ones(5, dtype=np.float32), np.array([0.1, 0.2]), np.ones(5)
    for kw in ({}, dict(method="direct")):
        assert LS.ls_periodogram(t, y, f, weights=w, floating_mean=False, normalize="power", t_ref=1.0, **kw) == "P"
        name, a, k = seen.pop()
        assert name == "lomb" and a[0] is t and a[1] is y and a[2] is f
        assert k == dict(weights=w, floating_mean=False, normalize="power", t_ref=1.0)
        LS.ls_window(t, f, weights=w, **kw)
        name, a, k = seen.pop()
        assert name == "lomb_sums" and a[0] is t and a[1] is None and a[2] is f and k == dict(weights=w)
    assert not seen
    LS.ls_periodogram(t, y, f, method="auto")                # 10 pairs: far below the crossover
    assert seen.pop()[0] == "lomb"


def test_exported_declared_and_bound():
    for name in ("nufft1", "nufft1_modes", "nufft_plan"):
        assert getattr(pyfft_amd, name) is getattr(NU, name)
    for name in ("nufft1", "lomb_sums_grid", "nufft_plan", "nufft_check", "NufftRefused", "NUFFT_PASSES"):
        assert hasattr(E, name)
    assert issubclass(E.NufftRefused, ValueError) and issubclass(E.NufftRefused, NotImplementedError)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_nufft.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.NUFFT_SIGNATURES) == {"sp_nufft1", "sp_lomb_sums_grid", "sp_nufft1_plan"}
    assert len(_ffi.TABLES) == 6 and _ffi.NUFFT_SIGNATURES in _ffi.MORE_TABLES and all(t is not _ffi.NUFFT_SIGNATURES for t in _ffi.TABLES)
    for table in _ffi.TABLES + tuple(t for t in _ffi.MORE_TABLES if t is not _ffi.NUFFT_SIGNATURES):
        assert not set(_ffi.NUFFT_SIGNATURES) & set(table)
    assert not set(_ffi.NUFFT_SIGNATURES) & set(_ffi.UNEVEN_SIGNATURES)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_nufft1", 12), ("sp_lomb_sums_grid", 16), ("sp_nufft1_plan", 4)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.NUFFT_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.NUFFT_SIGNATURES[name][1]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "spectral_nufft.h":
            assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other))), other
    assert "spectral_nufft.h" in open(os.path.join(ROOT, "Makefile")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "SP_NUFFT_ROWS" in launch and "NUFFT_GRID_BYTES" in launch and "profiles/nufft_bench.txt" in launch
    assert "which = 6" in open(os.path.join(ROOT, "include", "spectral_ext.h")).read()
    assert _ffi.load_library().sp_last_passes(6) == 0


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """nufft_plan.h is host-only arithmetic: built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run here as its own
    process -- the shift bound at 2^31 - 1 samples in one cell, cells and tile lists at the tile seams and the periodic end of the
    grid, the far product of a position, the kernel's transform against Simpson's rule"""
    exe = str(tmp_path / "nufft_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "pyfft_amd", "csrc"), os.path.join(ROOT, "tests", "nufft_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nufft plan ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
