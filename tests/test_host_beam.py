"""The array scan without a GPU: the float64 definitions of tests/beam_ref.py against independent forms, the recorded CPU figures, the C
ABI's declarations, bindings and refusals, the plan arithmetic (restated here, and under sanitizers in tests/beam_plan_test.cpp), the
Python front ends' refusals and the host arithmetic of pyfft_amd.beamform."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import beam_ref as R
import subspace_ref as S
import pyfft_amd
from pyfft_amd import _ffi, beamform as BF, engine as E
from pyfft_amd.windows import get_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN = np.asarray(get_window("hann", R.NPERSEG), dtype=np.float64)


# ---- the definitions against independent forms ----------------------------------------------------------------------------------------
def _matrix(m, s=0):
    w, V = R.eig_of(m)
    return (V[s] * w[s][None, :]) @ np.conj(V[s].T), w[s], V[s]


@pytest.mark.parametrize("m", R.DEF_M)
def test_capon_and_bartlett_against_the_matrix_forms(m):
    """1 / Re(a^H (G + delta I)^-1 a) and Re(a^H G a) / m^2"""
    worst_c = worst_b = 0.0
    for s in range(3):
        G, w, V = _matrix(m, s)
        for nk, ndim, far in R.GEOMS[:5]:
            pos, kv = R.geometry(m, nk, ndim, far)
            A = R.steer_def(pos, kv, R.SCALES[s])
            for loading in R.LOADINGS:
                got, st = R.beam_def(V, w, pos, kv, "capon", 0, loading, R.SCALES[s])
                Gi = np.linalg.inv(G + R.delta_def(w, loading) * np.eye(m))
                want = 1.0 / np.einsum("qi,ij,qj->q", np.conj(A), Gi, A).real
                assert st == 0
                worst_c = max(worst_c, float(np.max(np.abs(got - want) / want)))
            got, st = R.beam_def(V, w, pos, kv, "bartlett", 0, 0.0, R.SCALES[s])
            want = np.einsum("qi,ij,qj->q", np.conj(A), G, A).real / m ** 2
            worst_b = max(worst_b, float(np.max(np.abs(got - want)) / np.max(want)))
    print("m %d: capon against the inverse %.1e, bartlett against a^H G a %.1e" % (m, worst_c, worst_b))
    assert worst_c <= 1e-11 and worst_b <= 1e-13       # the inverse of a matrix of condition 1e3 .. 1e4; a sum of m^2 terms


@pytest.mark.parametrize("method", ("music", "ev"))
def test_music_on_unit_spacing_is_the_pseudospectrum(method):
    for m in R.DEF_M:
        w, V = R.eig_of(m)
        for p in sorted({0, min(2, m - 1), m - 1}):
            nb, start, step = 129, -0.3, 1.0 / 200
            want, st0 = S.pseudo_def(V[0], w[0], p, nb, start, step, method)
            got, st = R.beam_def(V[0], w[0], np.arange(m, dtype=np.float64), start + np.arange(nb) * step, method, p)
            assert st == st0 == 0 and np.max(np.abs(got - want) / want) <= 1e-12, (m, p)


def test_weights_flags_and_zero_sums():
    w, V = R.eig_of(23)
    w2 = w[0].copy()
    w2[-1], w2[-3] = 0.0, -2.0
    pos, kv = R.geometry(23, 40, 2, False)
    for method, loading, want in (("capon", 0.0, 1), ("ev", 0.0, 1), ("music", 0.0, 0), ("bartlett", 0.0, 0), ("capon", 1e-3, 1)):
        P, st = R.beam_def(V[0], w2, pos, kv, method, 2, loading)
        assert st == want and np.all(np.isfinite(P)), method
    for method in R.METHODS:
        P, st = R.beam_def(V[0], np.zeros(23), pos, kv, method, 2)
        assert np.all(np.isfinite(P)) and (method == "music" or not P.any())
    assert R.delta_def(np.array([3.0, 2.0, 1.0]), 0.5) == 1.0 and R.delta_def(np.array([1.0, -2.0]), 0.5) == 0.0


def test_the_phase_rule():
    pos, kv = R.geometry(5, 7, 3, True)
    fr = R.phase_def(pos, kv, 0.37)
    for q in range(7):
        for i in range(5):
            t = pos[i, 0] * kv[q, 0]
            t = t + pos[i, 1] * kv[q, 1]
            t = t + pos[i, 2] * kv[q, 2]
            ph = 0.37 * t
            assert fr[q, i] == ph - np.floor(ph)
    assert np.all((fr >= 0) & (fr <= 1)) and np.array_equal(R.phase_def(pos, kv), R.phase_def(pos, kv, 1.0))
    a = R.steer_def(np.arange(4.0), np.array([0.25]))
    assert np.allclose(a[0], [1, 1j, -1, -1j], atol=1e-15)                # +2 pi i nu i: sp_pseudospectrum's steering vector


def test_the_bound_is_small_and_has_no_measured_term():
    for m in R.DEF_M:
        w, V = R.eig_of(m)
        pos, kv = R.geometry(m, 65, 3, True)
        for method, p, loading in R.variants(m):
            P, _ = R.beam_def(V[0], w[0], pos, kv, method, p, loading)
            b = R.beam_bound(V[0], w[0], pos, kv, method, p, loading)
            ok = P != 0
            assert np.all(b[ok] > 0) and np.max(b[ok] / np.abs(P[ok])) < 1e-6, (m, method, p)


# ---- end to end on the reference alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.E2E))
def test_the_cases_hold_on_the_reference(case):
    G, w, V = R.e2e_matrix(case, WIN)
    print("%s: eigenvalue gap w[1] / w[2] = %.0f" % (case, w[1] / w[2]))
    assert w[1] / w[2] >= R.MIN_GAP
    near = R.nearest(case)
    for method in R.METHODS:
        pk = R.peak_bins(R.e2e_reference(case, method, WIN), 2)
        if case == "ring" or method != "bartlett":
            assert all(min(abs(int(i) - n) for i in pk) <= (0 if case == "ring" else 1) for n in near), (method, pk, near)
        else:                                                            # half a Rayleigh width apart: the conventional beam does not split them
            every = R.peak_bins(R.e2e_reference(case, method, WIN), len(R.LINE_GRID))
            assert min(abs(int(i) - near[1]) for i in every) > 1, (every[:4], near)


def test_the_recorded_perturbation_figures():
    for (case, method), rec in R.E2E_PERT.items():
        now = R.perturbation_change(case, method, WIN)
        print("%s %s: relative change under a perturbation of %.0e ||G||: %.3g (recorded %.3g, allowance %.3g)"
              % (case, method, R.CSDM_PARITY, now, rec, R.e2e_allowance(case, method)))
        assert rec / 2 <= now <= rec * 2


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.ARRAY_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.ARRAY_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


def test_exported_declared_and_bound():
    for name in ("array_spectrum", "mode_spectrum", "beam_scan", "slowness_scan", "array_pattern", "beam_peaks", "beam_plan", "BeamRefused"):
        assert getattr(pyfft_amd, name) is getattr(BF, name)
    for name in ("BeamRefused", "beam_check", "beamscan", "beam_plan"):
        assert hasattr(E, name)
    assert issubclass(E.BeamRefused, ValueError) and issubclass(E.BeamRefused, NotImplementedError) and BF.BeamRefused is E.BeamRefused
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_array.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.ARRAY_SIGNATURES) == {"sp_beamscan", "sp_beamscan_plan"}
    # the three older tuples are as they were
    assert len(_ffi.TABLES) == 6 and len(_ffi.MORE_TABLES) == 6 and _ffi.MORE_TABLES[-1] is _ffi.AR_SIGNATURES
    assert _ffi.LATER_TABLES == (_ffi.DWT_SIGNATURES,) and _ffi.ARRAY_TABLES == (_ffi.ARRAY_SIGNATURES,)
    for table in _ffi.TABLES + _ffi.MORE_TABLES + _ffi.LATER_TABLES:
        assert not set(_ffi.ARRAY_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_beamscan", 18), ("sp_beamscan_plan", 7)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.ARRAY_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.ARRAY_SIGNATURES[name][1]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "spectral_array.h":
            assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other))), other
    assert "spectral_array.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert '#include "../../include/spectral_array.h"' in open(os.path.join(ROOT, "pyfft_amd", "csrc", "spectral.hip")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "launch_beam" in launch and "SP_BEAM_GRID" in launch and '#include "beam_plan.h"' in launch
    kernel = open(os.path.join(ROOT, "pyfft_amd", "csrc", "k_beam.hip")).read()
    code = kernel.split("#include")[1].lower()
    assert "atomic" not in code and "hipmemset" not in code and "asm" not in code and "void k_beam(" in kernel
    assert "__dmul_rn" in kernel and "__dadd_rn" in kernel and "sincospi" in kernel


def plan_ref(m, nk, nmodels, method, p, hook=0):
    """beam_plan.h restated: steering vectors of a tile, tiles, vectors of a stage, LDS bytes, workgroups, items of a workgroup, stages, 0"""
    tiles = -(-nk // 64)
    nn = m - (p if method >= 2 else 0)
    items = nmodels * tiles
    grid = min(items, 1 << 16)
    if hook > 0:
        grid = min(grid, hook)
    return 64, tiles, 32, m * (64 + 32) * 16 + 8 * 64 * 8 + 64 * 8, grid, -(-items // grid) if grid else 0, -(-nn // 32), 0


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_BEAM_GRID", raising=False)
    lib = _c_entry()
    out = np.zeros(8, dtype=np.int64)
    plan = lambda *a: (lib.sp_beamscan_plan(*a, _ffi.ptr(out)), tuple(int(v) for v in out))
    shapes = [(2, 1, 1, 1, 0, 0), (23, 2, 63, 3, 1, 0), (64, 3, 64, 3, 2, 2), (64, 1, 65, 3, 3, 63), (64, 1, 1024, 2049, 2, 2), (16, 1, 256, 513, 1, 0),
              (8, 1, 4096, 129, 3, 7), (64, 1, (1 << 31) - 1, 1 << 14, 0, 0), (33, 1, 300, 0, 2, 0), (64, 2, 1024, 1 << 20, 2, 31)]
    for m, ndim, nk, nm, me, p in shapes:
        rc, got = plan(m, ndim, nk, nm, me, p)
        assert rc == 0 and got == plan_ref(m, nk, nm, me, p), (m, ndim, nk, nm, me, p, got)
    assert plan(64, 1, 1024, 2049, 2, 2)[1] == (64, 16, 32, 102912, 32784, 1, 2, 0)
    assert plan(64, 2, 1024, 1 << 20, 2, 31)[1][4:7] == (65536, 256, 2)
    monkeypatch.setenv("SP_BEAM_GRID", "1")
    assert plan(23, 2, 300, 3, 1, 0)[1] == plan_ref(23, 300, 3, 1, 0, hook=1) and plan(23, 2, 300, 3, 1, 0)[1][4:6] == (1, 15)
    monkeypatch.delenv("SP_BEAM_GRID")
    d = E.beam_plan(64, 1024, 2049, "music", 2)
    assert d == BF.beam_plan(64, 1024, 2049, "music", 2) == pyfft_amd.beam_plan(64, 1024, 2049, "music", 2)
    assert tuple(d[k] for k in E.BEAM_PLAN_NAMES) == plan_ref(64, 1024, 2049, 2, 2) and d["lds_bytes"] <= 160 * 1024
    assert lib.sp_beamscan_plan(8, 1, 10, 1, 0, 0, None) < 0
    for bad in ((1, 1, 10, 1, 0, 0), (65, 1, 10, 1, 0, 0), (8, 0, 10, 1, 0, 0), (8, 4, 10, 1, 0, 0), (8, 1, 0, 1, 0, 0), (8, 1, 1 << 31, 1, 0, 0),
                (8, 1, 10, -1, 0, 0), (8, 1, 10, 1, 4, 0), (8, 1, 10, 1, -1, 0), (8, 1, 10, 1, 2, 8), (8, 1, 10, 1, 3, -1), (8, 1, 100, 1 << 40, 0, 0)):
        assert lib.sp_beamscan_plan(*bad, _ffi.ptr(out)) < 0, bad
    for bad in ((1, 10), (65, 10), (8, 0), (8, 10, -1), (8, 10, 1, "mvdr"), (8, 10, 1, "music", 8), (8, 10, 1, "ev", -1), (8, 10, 1, "capon", 0, 4)):
        with pytest.raises(E.BeamRefused):
            E.beam_plan(*bad)


GOOD = dict(V=True, vld=6, w=True, m=6, nm=2, pos=True, ndim=2, kv=True, nk=20, scale=True, method=2, p=2, loading=0.0, out64=0, P=True, pld=20, st=True)
SENT = -12345.0
NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(m=1), "m must"), (dict(m=65, vld=65), "m must"), (dict(vld=5), "V_ld"), (dict(ndim=0), "ndim"), (dict(ndim=4), "ndim"), (dict(nk=0), "nk must"),
            (dict(nk=1 << 31, pld=1 << 31), "nk must"), (dict(pld=19), "P_ld"), (dict(method=4), "method"), (dict(method=-1), "method"), (dict(p=-1), "p must"),
            (dict(p=6), "p must"), (dict(method=3, p=6), "p must"), (dict(loading=-1e-3), "loading"), (dict(loading=NAN), "loading"), (dict(loading=INF), "loading"),
            (dict(bad="pos"), "pos must be finite"), (dict(bad="kv"), "kv must be finite"), (dict(bad="scale"), "scale must be finite"),
            (dict(bad="posinf"), "pos must be finite"), (dict(V=False), "V is"), (dict(w=False), "w is"), (dict(pos=False), "pos is"), (dict(kv=False), "kv is"),
            (dict(P=False), "P is"), (dict(st=False), "status is"), (dict(nm=-1), "nmodels"), (dict(nm=(1 << 40) + 1), "nmodels")]


def _call(lib, p):
    V, w, P, st = np.ones(2 * 36 * 2), np.ones(12), np.full(64, SENT, dtype=np.float32), np.full(2, -77, dtype=np.int32)
    pos, kv, scale = np.ones(6 * 3), np.ones(20 * 3), np.ones(2)
    bad = p.get("bad")
    if bad == "pos":
        pos[6 * p["ndim"] - 1] = NAN
    if bad == "posinf":
        pos[0] = INF
    if bad == "kv":
        kv[20 * p["ndim"] - 1] = NAN
    if bad == "scale":
        scale[1] = INF
    ptr = _ffi.ptr
    rc = lib.sp_beamscan(ptr(V) if p["V"] else None, p["vld"], ptr(w) if p["w"] else None, p["m"], p["nm"], ptr(pos) if p["pos"] else None, p["ndim"],
                         ptr(kv) if p["kv"] else None, p["nk"], ptr(scale) if p["scale"] else None, p["method"], p["p"], p["loading"], p["out64"],
                         ptr(P) if p["P"] else None, p["pld"], ptr(st) if p["st"] else None, 0)
    return rc, (lib.sp_last_error() or b"").decode(), bool(np.all(P == np.float32(SENT)) and np.all(st == -77))


@pytest.mark.parametrize("over,word", REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(REFUSALS)])
def test_c_refusals(over, word):
    rc, msg, untouched = _call(_c_entry(), dict(GOOD, **over))
    assert rc == -1 and msg.startswith("sp_beamscan: ") and word in msg and untouched, (rc, msg)


def test_p_counts_for_music_and_ev_only_and_nothing_to_do_returns_zero():
    lib = _c_entry()
    for method in (0, 1):                                               # the device is not there: what is not refused gets as far as sp_init
        rc, msg, untouched = _call(lib, dict(GOOD, method=method, p=99, nm=0))
        assert rc == 0 and untouched
    rc, msg, untouched = _call(lib, dict(GOOD, nm=0))
    assert rc == 0 and untouched
    rc, msg, untouched = _call(lib, dict(GOOD, nm=0, scale=False))
    assert rc == 0 and untouched


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    V, w = np.ones((3, 6, 6), dtype=np.complex128), np.ones((3, 6))
    pos, kv = np.arange(6.0), np.linspace(-0.5, 0.5, 11)
    x, G = np.ones((6, 600), dtype=np.float32), np.ones((3, 6, 6), dtype=np.complex128)
    bad = [lambda: E.beamscan(V, w[:2], pos, kv), lambda: E.beamscan(V, w, pos[:5], kv), lambda: E.beamscan(V, w, pos, kv, "mvdr"),
           lambda: E.beamscan(V, w, pos, kv, "music", 6), lambda: E.beamscan(V, w, pos, kv, "ev", -1), lambda: E.beamscan(V, w, pos, kv, "capon", 0, -1.0),
           lambda: E.beamscan(V, w, pos, kv, "capon", 0, np.nan), lambda: E.beamscan(V, w, pos, kv * np.nan), lambda: E.beamscan(V, w, pos + np.inf, kv),
           lambda: E.beamscan(V, w, pos, kv, scale=[1.0, np.nan, 1.0]), lambda: E.beamscan(V, w, pos, np.ones((11, 2))), lambda: E.beamscan(V, w, pos, kv[:0]),
           lambda: E.beamscan(V, w, np.ones((6, 4)), np.ones((11, 4))), lambda: E.beamscan(V * np.nan, w, pos, kv), lambda: E.beamscan(V[:, :, :5], w, pos, kv),
           lambda: E.beamscan(np.ones((3, 65, 65)), np.ones((3, 65)), np.arange(65.0), kv), lambda: E.beamscan(np.ones((1, 1)), np.ones(1), np.ones(1), kv),
           lambda: BF.array_spectrum(x, pos, kv, method="mvdr"), lambda: BF.array_spectrum(x, pos, kv, method="music"), lambda: BF.array_spectrum(x, pos, kv, method="ev", nsources=6),
           lambda: BF.array_spectrum(x, pos[:5], kv), lambda: BF.array_spectrum(x[0], pos, kv), lambda: BF.array_spectrum(x, pos, kv, fs=0.0),
           lambda: BF.array_spectrum(x, pos, kv, nperseg=601), lambda: BF.array_spectrum(x, pos, kv, noverlap=256), lambda: BF.array_spectrum(x, pos, kv, loading=-1.0),
           lambda: BF.array_spectrum(x, pos, kv, band=(0.7, 0.9)), lambda: BF.array_spectrum(x, pos, kv, window=np.zeros(256)),
           lambda: BF.array_spectrum(np.ones((65, 600), dtype=np.float32), np.arange(65.0), kv), lambda: BF.array_spectrum(x[:1], pos[:1], kv),
           lambda: BF.mode_spectrum(x, pos, [0.5, 1.0]), lambda: BF.mode_spectrum(x, np.ones((6, 2)), [1, 2]), lambda: BF.mode_spectrum(x, pos, [1, 2], method="music"),
           lambda: BF.beam_scan(G[0, 0], pos, kv), lambda: BF.beam_scan(G, pos, kv, method="ev"), lambda: BF.beam_scan(G, pos, np.ones((11, 2))),
           lambda: BF.slowness_scan(G, np.ones(2), pos, kv), lambda: BF.slowness_scan(G, [1.0, np.nan, 2.0], pos, kv), lambda: BF.slowness_scan(G, np.ones(3), pos, kv * np.nan),
           lambda: BF.array_pattern(pos, np.ones((11, 2))), lambda: BF.array_pattern(pos, kv, np.nan), lambda: BF.beam_peaks(np.ones((3, 11)), kv[:10], 2),
           lambda: BF.beam_peaks(np.ones((3, 11)), kv, 0), lambda: BF.beam_plan(65, 10), lambda: BF.beam_plan(8, 10, method="music", nsources=8)]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError) as exc:
            fn()
        assert isinstance(exc.value, NotImplementedError) and isinstance(exc.value, E.BeamRefused), i


# ---- the host arithmetic of the module --------------------------------------------------------------------------------------------------
def test_array_pattern():
    pos = R.sensors("line")
    k = 2 * np.pi * R.LINE_GRID
    W = BF.array_pattern(pos, k, k0=k[700])
    a = lambda kk: np.exp(-1j * kk * pos)
    want = np.array([abs(np.vdot(a(kk), a(k[700]))) ** 2 for kk in k]) / len(pos) ** 2
    assert np.max(np.abs(W - want)) <= 1e-13 and abs(W[700] - 1.0) <= 1e-15 and np.argmax(W) == 700 and np.all(W <= 1 + 1e-15)
    # the Bartlett spectrum of one noiseless wave is its power times the pattern
    G = np.outer(a(k[700]), np.conj(a(k[700]))) * 3.0
    w, V = R.eigh_desc(G)
    assert np.max(np.abs(R.beam_def(V, w, pos, -k / (2 * np.pi), "bartlett")[0] - 3.0 * W)) <= 1e-12
    P2 = BF.array_pattern(np.stack([pos, 0.5 * pos], axis=1), np.stack([k, 0 * k], axis=1), k0=(k[700], 0.0))
    assert np.max(np.abs(P2 - W)) <= 1e-13
    # an even ring of 8 has grating lobes 8 modes apart
    ring = 2 * np.pi * np.arange(8) / 8
    assert np.allclose(BF.array_pattern(ring, np.array([-6.0, 2.0, 10.0, 3.0]), 2.0), [1, 1, 1, 0], atol=1e-13)


def test_beam_peaks():
    k = np.linspace(-1.0, 1.0, 201)
    y = 3.0 - 40.0 * (k - 0.2037) ** 2
    y2 = np.maximum(y, 2.0 - 40.0 * (k + 0.5012) ** 2)
    kp, pp = BF.beam_peaks(np.stack([y, y2]), k, 2)
    assert kp.shape == pp.shape == (2, 2)
    assert abs(kp[0, 0] - 0.2037) <= 1e-12 and abs(pp[0, 0] - 3.0) <= 1e-12 and np.isnan(kp[0, 1]) and np.isnan(pp[0, 1])     # a parabola is found exactly
    assert abs(kp[1, 0] - 0.2037) <= 1e-12 and abs(kp[1, 1] + 0.5012) <= 1e-12 and abs(pp[1, 1] - 2.0) <= 1e-12
    kp, pp = BF.beam_peaks(np.array([5.0, 1.0, 2.0, 1.0, 0.0, 4.0]), np.arange(6.0), 3)                                          # the ends count, unrefined
    assert list(kp) == [0.0, 5.0, 2.0] and list(pp) == [5.0, 4.0, 2.0]
    assert BF.beam_peaks(np.zeros((2, 3, 6)), np.arange(6.0), 2)[0].shape == (2, 3, 2)


def test_the_sign_convention_on_a_noiseless_delay():
    """two sensors, the one at larger r hears the wave LATER: k > 0 at f > 0, as wavenumber.skf has it"""
    fs, f0, r, tau = 100.0, 5.0, np.array([0.0, 0.4]), 0.013            # the wave takes tau to travel 0.4: k = 2 pi f0 tau / 0.4
    t = np.arange(4096) / fs
    x = np.stack([np.cos(2 * np.pi * f0 * (t - 0.0)), np.cos(2 * np.pi * f0 * (t - tau))])
    k_true = 2 * np.pi * f0 * tau / 0.4
    G = R.csd_def(x, np.asarray(get_window("hann", 256), dtype=np.float64), fs)
    b = int(round(f0 * 256 / fs))
    w, V = R.eigh_desc(G[b])
    k = np.linspace(-2 * np.pi, 2 * np.pi, 2001)                         # within the two sensors' ambiguity of 2 pi / 0.4
    P = R.beam_def(V, w, r, -k / (2 * np.pi), "bartlett")[0]
    assert abs(k[np.argmax(P)] - k_true) <= 1.5 * (k[1] - k[0]) and k_true > 0
    # the module forms kv = -k / 2 pi and nothing else
    pos, kv, p = BF._judge("t", 2, r, k, "music", 1, 0.0)
    assert np.array_equal(kv[:, 0], -k / (2 * np.pi)) and np.array_equal(pos[:, 0], r) and p == 1


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """beam_plan.h is host-only arithmetic: built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run here as its own
    process -- the tiles, stages and items walked as k_beam walks them, the LDS regions, the refusals"""
    exe = str(tmp_path / "beam_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "pyfft_amd", "csrc"), os.path.join(ROOT, "tests", "beam_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "beam plan ok" in r.stdout
