"""Subspace spectra and covariance fits without a GPU: the float64 restatements of tests/subspace_ref.py against independent forms
(the explicit data matrix, numpy.linalg.lstsq, the projector form of MUSIC), the measured figures the GPU test's allowances rest
on, the declared set of include/spectral_sub.h, the refusals of the C entries and of their Python front ends before the device is
touched, the plan figures, the host arithmetic of pyfft_amd.subspace, and sub_plan.h under sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import burg_ref as B
import subspace_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, parametric as PM, subspace as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seg(name, r=0, g=0):
    c = R.shape_of(name)
    return B.segment(R.signals(name)[r], c["n"], c["first"], g, c["hop"]), c


# ---- the definitions against independent forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", (False, True))
@pytest.mark.parametrize("name", ("c2", "c8", "c64", "c333c", "seam", "frames"))
def test_covmat_def_is_the_data_matrix_product(name, fb):
    s, c = _seg(name)
    X = R.data_matrix(s, c["m"], fb)
    N = c["n"] - c["m"] + 1
    C = R.covmat_def(s, c["m"], fb)
    ref = np.conj(X.T) @ X / N
    assert X.shape == ((2 if fb else 1) * N, c["m"])
    assert np.max(np.abs(C - ref)) <= 1e-13 * np.max(np.abs(ref))
    assert np.array_equal(C, np.conj(C.T)) or np.max(np.abs(C - np.conj(C.T))) <= 1e-15 * np.max(np.abs(C))
    if fb:                                                              # persymmetric: J conj(C) J = C
        assert np.max(np.abs(C - np.conj(C[::-1, ::-1]))) <= 1e-15 * np.max(np.abs(C))


@pytest.mark.parametrize("name", list(R.COV_CASES))
def test_the_recursion_restates_the_definition_within_the_bound(name):
    """covmat_rec is the kernels' arithmetic; it stays within the GPU test's derived bound with room, is exactly Hermitian, and its
    worst deviation is the recorded figure"""
    s, c = _seg(name)
    for fb in (False, True):
        a, b = R.covmat_rec(s, c["m"], fb), R.covmat_def(s, c["m"], fb)
        assert np.array_equal(a, np.conj(a.T)) and not a.diagonal().imag.any()
        assert np.max(np.abs(a - b)) <= 0.01 * R.covmat_bound(s, c["m"])


def test_the_recorded_recursion_figure():
    worst = 0.0
    for name in R.COV_CASES:
        s, c = _seg(name)
        pw = np.sum(np.abs(s) ** 2) / (c["n"] - c["m"] + 1)
        for fb in (False, True):
            worst = max(worst, float(np.max(np.abs(R.covmat_rec(s, c["m"], fb) - R.covmat_def(s, c["m"], fb))) / pw))
    print("recursion against the direct sums: %.3e of the mean power, recorded %.3e" % (worst, R.COV_REC_DEV))
    assert 0.5 * R.COV_REC_DEV <= worst <= R.COV_REC_DEV <= 2.3e-15


@pytest.mark.parametrize("fb", (False, True))
@pytest.mark.parametrize("name", ("c64", "c333c", "frames"))
def test_ls_def_against_lstsq(name, fb):
    s, c = _seg(name)
    p = c["m"] - 1
    a, e, st = R.ls_def(s, p, fb)
    a2, e2 = R.ls_lstsq(s, p, fb)
    assert st == 0 and a[0] == 1 and a.dtype == a2.dtype == (np.complex128 if c["cplx"] else np.float64)
    assert np.max(np.abs(a - a2)) <= 1e-11 * np.sum(np.abs(a2)) and abs(e - e2) <= 1e-11 * e2


def test_ls_of_a_noiseless_tone_stops_at_a_pivot():
    s = np.cos(2 * np.pi * 0.123 * np.arange(100))
    a, e, st = R.ls_def(s, 8, True)
    assert 1 <= st <= 8 and e == 0.0 and np.array_equal(a, np.eye(1, 9)[0])
    a, e, st = R.ls_def(np.zeros(40), 5, False)
    assert st == 1 and e == 0.0


@pytest.mark.parametrize("name", list(R.E2E_CASES))
def test_music_against_the_projector_form(name):
    cplx, p, _ = R.E2E_CASES[name]
    C, w, V, P = R.e2e_reference(name)
    nb, start, step = R.e2e_axis(cplx)
    ref = R.music_projector(C, p, start + np.arange(nb) * step)
    assert np.max(np.abs(P - ref) / ref) <= 1e-6                       # the projector form cancels where P is large: 1 - |V_s^H e|^2 / m
    # the conjugate steering convention puts no peak at the tones
    Pc = R.pseudo_def(np.conj(V), w, p, nb, start, step, "music")[0] if cplx else None
    pk = R.peaks(P, 2) / R.E2E_GRID
    assert np.max(np.abs(pk - np.array(R.TONES))) <= 1.0 / R.E2E_GRID
    if cplx:
        assert np.max(np.abs(R.peaks(Pc, 2) / R.E2E_GRID - np.array(R.TONES))) > 0.1
    assert w[p - 1] / w[p] >= R.MIN_GAP


def test_ev_weights_and_flags():
    C, w, V, _ = R.e2e_reference("cplx20")
    P, st = R.pseudo_def(V, w, 2, 64, 0.0, 1.0 / 64, "ev")
    assert st == 0 and np.all(np.isfinite(P)) and np.all(P > 0)
    w2 = w.copy()
    w2[-1], w2[-2] = 0.0, -1.0
    P2, st2 = R.pseudo_def(V, w2, 2, 64, 0.0, 1.0 / 64, "ev")
    assert st2 == 1 and np.all(np.isfinite(P2)) and np.all(P2 >= P)       # two terms fewer in the sum
    assert R.pseudo_def(V, w2, 2, 64, 0.0, 1.0 / 64, "music")[1] == 0
    w3 = np.zeros_like(w)
    P3, st3 = R.pseudo_def(V, w3, 2, 8, 0.0, 0.125, "ev")
    assert st3 == 1 and not P3.any()


# ---- the measured constants --------------------------------------------------------------------------------------------------------
def test_the_recorded_ls_figures():
    worst = np.zeros(3)
    for name in R.LS_CASES:
        for fb in (False, True):
            worst = np.maximum(worst, R.ls_deviations(R.ls_reference(name, fb, "chol"), R.ls_reference(name, fb, "lstsq")))
    print("Cholesky from the kernels' matrix against lstsq: P %.3e a %.3e e %.3e, recorded %s" % (tuple(worst) + (R.LS_CHOL_DEV,)))
    for got, rec in zip(worst, R.LS_CHOL_DEV):
        assert 0.5 * rec <= got <= rec
    assert R.LS_ALLOWANCE == tuple(R.MARGIN * d for d in R.LS_CHOL_DEV) and R.MARGIN == 4.0
    assert max(R.LS_CASES.values()) == 63


def test_the_recorded_perturbation_figure():
    worst = max(R.perturbation_change(name, weighting=wt) for name in R.E2E_CASES for wt in ("music", "ev"))
    print("reference P under a perturbation of C of eigh's tolerance: %.3e, recorded %.3e" % (worst, R.E2E_PERT))
    assert 0.5 * R.E2E_PERT <= worst <= R.E2E_PERT and R.E2E_ALLOWANCE == R.MARGIN * R.E2E_PERT
    for name in R.E2E_CASES:
        cplx, p, _ = R.E2E_CASES[name]
        w = R.e2e_reference(name)[1]
        assert w[p - 1] / w[p] >= R.MIN_GAP == 50.0


def test_the_recorded_device_shares():
    """what tests/test_gpu_subspace.py used of its allowances on an MI355X"""
    for share in (R.COV_DEVICE_SHARE, R.LS_DEVICE_SHARE, R.PSEUDO_DEVICE_SHARE, R.E2E_DEVICE_SHARE):
        assert 0 < share <= 1


# ---- the host arithmetic of pyfft_amd.subspace -------------------------------------------------------------------------------------
def test_esprit_and_the_order_criteria():
    for name in R.E2E_CASES:
        cplx, p, _ = R.E2E_CASES[name]
        C, w, V, _ = R.e2e_reference(name)
        f = SS.esprit(V, p)
        assert f.shape == (p,) and np.max(np.abs(f[-2:] - np.array(R.TONES))) <= 1.0 / R.E2E_GRID
        assert np.allclose(SS.esprit(V, p, fs=8.0), 8.0 * f)
        assert SS.subspace_order(w, R.E2E_N - R.E2E_M + 1, "mdl") >= p      # forward-backward snapshots are not independent: never fewer
    for cplx in (False, True):
        for m in (8, 24):
            w = R.eigh_desc(R.covmat_def(R.white(512, cplx).astype(np.complex128), m, True))[0]
            assert SS.subspace_order(w, 512 - m + 1, "mdl") == 0 and SS.subspace_order(w, 512 - m + 1, "aic") == 0
    ws = np.stack([np.array([9.0, 5.0, 1.0, 1.0, 1.0, 1.0]), np.ones(6)])
    assert np.array_equal(SS.subspace_order(ws, 100), [2, 0])
    for bad in (lambda: SS.subspace_order(ws, 100, "fpe"), lambda: SS.subspace_order(np.ones(1), 10), lambda: SS.esprit(np.eye(4), 4),
                lambda: SS.esprit(np.eye(4), 0)):
        with pytest.raises(E.SubRefused):
            bad()


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.SUB_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.SUB_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


def test_exported_declared_and_bound():
    for name in ("arcov", "armcov", "pcov", "pmcov"):
        assert getattr(pyfft_amd, name) is getattr(PM, name)
    for name in ("corrmtx_cov", "pmusic", "peig", "subspace_spectrogram", "subspace_order", "esprit", "subspace_plan", "SubRefused"):
        assert getattr(pyfft_amd, name) is getattr(SS, name)
    for name in ("SubRefused", "sub_check", "covmat", "ar_ls", "pseudospectrum", "sub_plan"):
        assert hasattr(E, name)
    assert issubclass(E.SubRefused, ValueError) and issubclass(E.SubRefused, NotImplementedError) and SS.SubRefused is E.SubRefused
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_sub.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.SUB_SIGNATURES) == {"sp_covmat", "sp_ar_ls", "sp_pseudospectrum", "sp_sub_plan"}
    assert len(_ffi.TABLES) == 6 and _ffi.SUB_SIGNATURES in _ffi.MORE_TABLES and all(t is not _ffi.SUB_SIGNATURES for t in _ffi.TABLES)
    assert len(_ffi.MORE_TABLES) == 6
    for table in _ffi.TABLES + tuple(t for t in _ffi.MORE_TABLES if t is not _ffi.SUB_SIGNATURES):
        assert not set(_ffi.SUB_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_covmat", 17), ("sp_ar_ls", 19), ("sp_pseudospectrum", 15), ("sp_sub_plan", 7)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.SUB_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.SUB_SIGNATURES[name][1]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "spectral_sub.h":
            assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other))), other
    assert "spectral_sub.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert '#include "../../include/spectral_sub.h"' in open(os.path.join(ROOT, "pyfft_amd", "csrc", "spectral.hip")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "launch_cov_row" in launch and "launch_cov_fill" in launch and "launch_ls_chol" in launch and "launch_pseudo" in launch
    ext = open(os.path.join(ROOT, "include", "spectral_ext.h")).read()
    assert "which = 8" in ext and "sp_covmat" in ext and "which=8" in E.last_passes.__doc__
    assert _ffi.load_library().sp_last_passes(8) == 0 and E.SUB_PASSES == 8
    kernel = open(os.path.join(ROOT, "pyfft_amd", "csrc", "k_subspace.hip")).read()
    assert "atomic" not in kernel.split("#include")[1].lower() and "hipMemset" not in kernel
    for k in ("k_cov_row", "k_cov_fill", "k_ls_chol", "k_pseudo"):
        assert "void %s(" % k in kernel


def plan_ref(what, cplx, n, m, segs, hook=0):
    """sub_plan.h restated: chunk, tiles, shares, LDS bytes, workgroups, passes, bytes of a segment, segments of a pass"""
    el = 16 if cplx else 8
    chunk = max(2048, -(-(-(-n // 1024)) // 2048) * 2048)
    tiles = -(-n // chunk)
    seg = tiles * m * el + (m * m * 16 if what == 1 else 0)
    fit = min(1 << 20, max(1, (256 << 20) // seg))
    if hook > 0:
        fit = min(fit, hook)
    spp = min(max(segs, 1), fit)
    return chunk, tiles, 256 // m, (63 + 2048 + 256) * el, segs * tiles, -(-segs // spp), seg, spp


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_AR_SEGS", raising=False)
    lib = _c_entry()
    out = np.zeros(8, dtype=np.int64)
    plan = lambda wh, dt, n, m, b, f: (lib.sp_sub_plan(wh, dt, n, m, b, f, _ffi.ptr(out)), tuple(int(v) for v in out))[1]
    shapes = [(0, 0, 2, 2, 1, 1), (0, 0, 8, 8, 1, 1), (0, 1, 333, 24, 1, 1), (0, 0, 2 * 2048 + 63, 64, 1, 1), (0, 1, 100003, 32, 1, 1), (0, 0, 200, 7, 3, 5),
              (1, 1, 64, 4, 1, 11), (1, 0, 4096, 64, 1, 1), (0, 1, (1 << 31) - 1, 64, 100, 1), (1, 1, 256, 64, 1 << 10, 1 << 8), (0, 0, 64, 4, 0, 5)]
    for wh, dt, n, m, b, f in shapes:
        assert plan(wh, dt, n, m, b, f) == plan_ref(wh, dt, n, m, b * f), (wh, dt, n, m, b, f)
    assert plan(0, 1, 100003, 32, 1, 1) == (2048, 49, 8, 2367 * 16, 49, 1, 49 * 32 * 16, 1)
    assert plan(1, 1, 256, 64, 1 << 10, 1 << 8)[5] == 66                  # 2^18 fits of 66560 bytes each through 256 MiB, 4032 a pass
    monkeypatch.setenv("SP_AR_SEGS", str(R.SEGS_HOOK))
    assert plan(1, 1, 64, 4, 1, 11) == plan_ref(1, 1, 64, 4, 11, hook=R.SEGS_HOOK) and plan(1, 1, 64, 4, 1, 11)[5] == 2
    monkeypatch.delenv("SP_AR_SEGS")
    d = E.sub_plan("covmat", 333, 24, 2, 3, cplx=True)
    assert d == SS.subspace_plan(333, 24, 2, 3, True) == pyfft_amd.subspace_plan(333, 24, 2, 3, True, what=0)
    assert tuple(d[k] for k in ("chunk", "tiles", "shares", "lds_bytes", "workgroups", "passes", "seg_bytes", "segs_per_pass")) == plan_ref(0, True, 333, 24, 6)
    assert d["lds_bytes"] <= 64 * 1024
    assert lib.sp_sub_plan(0, 0, 64, 4, 1, 1, None) < 0
    for bad in ((2, 0, 64, 4, 1, 1), (0, 2, 64, 4, 1, 1), (0, 0, 64, 1, 1, 1), (0, 0, 64, 65, 1, 1), (0, 0, 7, 8, 1, 1), (1, 0, 125, 64, 1, 1),
                (0, 0, 1 << 31, 4, 1, 1), (0, 0, 64, 4, -1, 1), (0, 0, 64, 4, 1, -1)):
        assert lib.sp_sub_plan(*bad, _ffi.ptr(out)) < 0, bad
    for bad in (("covmat", 64, 1), ("covmat", 64, 65), ("covmat", 7, 8), ("ls", 125, 64), (3, 64, 4), ("covmat", 64, 4, -1)):
        with pytest.raises(E.SubRefused):
            E.sub_plan(*bad)


REC_GOOD = dict(x=True, dtype=0, xld=400, nsig=400, batch=2, n=100, hop=50, first=10, nframes=3, m=6, fb=1, detrend=3, mre=0.0, mim=0.0, out=True)
SENT = -12345.0
NAN, INF = float("nan"), float("inf")
REC_REFUSALS = [(dict(dtype=2), "dtype"), (dict(fb=2), "fb"), (dict(n=1), "n must"), (dict(hop=0), "hop"), (dict(first=-1), "first"),
                (dict(nframes=-1), "nframes"), (dict(batch=-1), "batch"), (dict(nframes=7), "reach outside"), (dict(first=301), "reach outside"),
                (dict(nsig=0), "nsig"), (dict(xld=399), "x_ld"), (dict(detrend=1), "detrend"), (dict(detrend=0, mre=NAN), "mean"),
                (dict(detrend=0, mim=INF), "mean"), (dict(x=False), "x is")]
COV_REFUSALS = REC_REFUSALS + [(dict(m=1), "m must"), (dict(m=65, n=200, hop=1, nframes=1), "m must"), (dict(m=9, n=8), "exceed n"), (dict(cld=35), "C_ld"),
                               (dict(out=False), "C is")]
LS_REFUSALS = REC_REFUSALS + [(dict(m=1), "order must"), (dict(m=65, n=200, hop=1, nframes=1), "order must"), (dict(m=52), "n / 2"), (dict(old=5), "out_ld"),
                              (dict(out=False), "a is"), (dict(e=False), "e is"), (dict(st=False), "status is")]


def _rec_args(p):
    x = np.ones(800, dtype=np.float32)
    return x, (_ffi.ptr(x) if p["x"] else None, p["dtype"], p["xld"], p["nsig"], p["batch"], p["n"], p["hop"], p["first"], p["nframes"])


@pytest.mark.parametrize("over,word", COV_REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(COV_REFUSALS)])
def test_c_refusals_of_covmat(over, word):
    lib = _c_entry()
    p = dict(dict(REC_GOOD, cld=36), **over)
    x, rec = _rec_args(p)
    C = np.full(6 * 36 * 2 * 4, SENT)
    rc = lib.sp_covmat(*rec, p["m"], p["fb"], p["detrend"], p["mre"], p["mim"], _ffi.ptr(C) if p["out"] else None, p["cld"], 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc == -1 and msg.startswith("sp_covmat: ") and word in msg and np.all(C == SENT), (rc, msg)


@pytest.mark.parametrize("over,word", LS_REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(LS_REFUSALS)])
def test_c_refusals_of_ar_ls(over, word):
    lib = _c_entry()
    p = dict(dict(REC_GOOD, old=6, e=True, st=True), **over)
    x, rec = _rec_args(p)
    a, e, st = np.full(6 * 64, SENT), np.full(6, SENT), np.full(6, -77, dtype=np.int32)
    rc = lib.sp_ar_ls(*rec, p["m"] - 1, p["fb"], p["detrend"], p["mre"], p["mim"], _ffi.ptr(a) if p["out"] else None, _ffi.ptr(e) if p["e"] else None,
                      _ffi.ptr(st) if p["st"] else None, p["old"], 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc == -1 and msg.startswith("sp_ar_ls: ") and word in msg and np.all(a == SENT) and np.all(e == SENT) and np.all(st == -77), (rc, msg)


def test_nothing_to_do_returns_zero():
    lib = _c_entry()
    for over in (dict(batch=0), dict(nframes=0)):
        p = dict(REC_GOOD, **over)
        x, rec = _rec_args(p)
        C, a, e, st = np.full(6 * 36 * 2, SENT), np.full(64, SENT), np.full(6, SENT), np.full(6, -77, dtype=np.int32)
        assert lib.sp_covmat(*rec, 6, 1, 3, 0.0, 0.0, _ffi.ptr(C), 36, 0) == 0 and np.all(C == SENT)
        assert lib.sp_ar_ls(*rec, 5, 1, 3, 0.0, 0.0, _ffi.ptr(a), _ffi.ptr(e), _ffi.ptr(st), 6, 0) == 0 and np.all(a == SENT) and np.all(st == -77)
    V, w, P, st = np.ones(2 * 36 * 2), np.ones(12), np.full(40, SENT, dtype=np.float32), np.full(2, -77, dtype=np.int32)
    assert lib.sp_pseudospectrum(_ffi.ptr(V), 6, _ffi.ptr(w), 6, 2, 0, 0, 20, 0.0, 0.01, 0, _ffi.ptr(P), 20, _ffi.ptr(st), 0) == 0
    assert np.all(P == np.float32(SENT)) and np.all(st == -77)


PS_GOOD = dict(V=True, vld=6, w=True, m=6, p=2, nm=2, wt=0, nb=20, start=0.0, step=0.01, out64=0, P=True, pld=20, st=True)
PS_REFUSALS = [(dict(m=1), "m ="), (dict(m=65, vld=65), "m ="), (dict(p=-1), "p ="), (dict(p=6), "p ="), (dict(vld=5), "V_ld"), (dict(wt=2), "weighting"),
               (dict(nb=0), "nbins"), (dict(nb=1 << 31, pld=1 << 31), "nbins"), (dict(pld=19), "P_ld"), (dict(nm=-1), "nmodels"),
               (dict(nm=1 << 30, nb=1000, pld=1000), "nmodels"), (dict(start=NAN), "finite"), (dict(step=INF), "finite"), (dict(V=False), "V is"),
               (dict(w=False), "w is"), (dict(P=False), "P is"), (dict(st=False), "status is")]


@pytest.mark.parametrize("over,word", PS_REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(PS_REFUSALS)])
def test_c_refusals_of_the_pseudospectrum(over, word):
    lib = _c_entry()
    p = dict(PS_GOOD, **over)
    V, w, P, st = np.ones(2 * 36 * 2), np.ones(12), np.full(64, SENT, dtype=np.float32), np.full(2, -77, dtype=np.int32)
    ptr = _ffi.ptr
    rc = lib.sp_pseudospectrum(ptr(V) if p["V"] else None, p["vld"], ptr(w) if p["w"] else None, p["m"], p["p"], p["nm"], p["wt"], p["nb"], p["start"],
                               p["step"], p["out64"], ptr(P) if p["P"] else None, p["pld"], ptr(st) if p["st"] else None, 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc == -1 and msg.startswith("sp_pseudospectrum: ") and word in msg and np.all(P == np.float32(SENT)) and np.all(st == -77), (rc, msg)


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    x = np.ones(400, dtype=np.float32)
    xn = x.copy()
    xn[17] = np.nan
    V, w = np.ones((3, 6, 6), dtype=np.complex128), np.ones((3, 6))
    bad = [lambda: E.covmat(x, 100, 50, 0, 3, 1), lambda: E.covmat(x, 100, 50, 0, 3, 65), lambda: E.covmat(x, 8, 50, 0, 3, 9),
           lambda: E.covmat(x, 100, 50, 0, 8, 6), lambda: E.covmat(x, 100, 0, 0, 3, 6), lambda: E.covmat(x, 100, 50, -1, 3, 6),
           lambda: E.covmat(x, 100, 50, 0, -1, 6), lambda: E.covmat(xn, 100, 50, 0, 3, 6), lambda: E.covmat(x, 100, 50, 0, 3, 6, mean_value=np.nan),
           lambda: E.covmat(x, 100, 50, 0, 3, 6, mean_value=1j), lambda: E.covmat(x, 100, 50, 0, 3, 6, detrend="linear"),
           lambda: E.covmat(x, 100, 50, 0, 3, 6, detrend=False, mean_value=0.5), lambda: E.covmat(np.float32(1.0), 100, 50, 0, 3, 6),
           lambda: E.ar_ls(x, 100, 50, 0, 3, 0), lambda: E.ar_ls(x, 100, 50, 0, 3, 51), lambda: E.ar_ls(x, 400, 1, 0, 1, 64), lambda: E.ar_ls(xn, 100, 50, 0, 3, 5),
           lambda: E.pseudospectrum(V, w[:2], 2, 10, 0.0, 0.1), lambda: E.pseudospectrum(V, w, 6, 10, 0.0, 0.1), lambda: E.pseudospectrum(V, w, -1, 10, 0.0, 0.1),
           lambda: E.pseudospectrum(V, w, 2, 0, 0.0, 0.1), lambda: E.pseudospectrum(V, w, 2, 10, np.nan, 0.1), lambda: E.pseudospectrum(V, w, 2, 10, 0.0, np.inf),
           lambda: E.pseudospectrum(V, w, 2, 10, 0.0, 0.1, weighting="minnorm"), lambda: E.pseudospectrum(V[:, :, :5], w, 2, 10, 0.0, 0.1),
           lambda: E.pseudospectrum(V * np.nan, w, 2, 10, 0.0, 0.1), lambda: E.pseudospectrum(np.ones((3, 65, 65)), np.ones((3, 65)), 2, 10, 0.0, 0.1),
           lambda: PM.arcov(x, 201), lambda: PM.armcov(x[:1], 1), lambda: PM.pcov(x, 5, nfft=0), lambda: PM.pmcov(x, 5, fs=0.0),
           lambda: PM.ar_spectrogram(x, 64, 200, method="cov"), lambda: PM.ar_spectrogram(x, 5, 100, method="modified"),
           lambda: SS.corrmtx_cov(x, 6, method="autocorrelation"), lambda: SS.corrmtx_cov(x, 65), lambda: SS.pmusic(x, 6, m=6), lambda: SS.pmusic(x, -1),
           lambda: SS.peig(x, 2, m=8, nfft=0), lambda: SS.peig(x, 2, m=8, fs=-1.0), lambda: SS.pmusic(x, 2, m=8, band=(0.3, 0.2), nbins=8),
           lambda: SS.pmusic(x, 2, method="fb"), lambda: SS.subspace_spectrogram(x, 2, 401), lambda: SS.subspace_spectrogram(x, 2, 100, noverlap=100),
           lambda: SS.subspace_spectrogram(x, 2, 100, weighting="minnorm"), lambda: SS.subspace_spectrogram(x, 8, 100, m=8), lambda: E.sub_plan("covmat", 7, 8)]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError) as exc:
            fn()
        assert isinstance(exc.value, NotImplementedError) and isinstance(exc.value, (E.SubRefused, E.ArRefused)), i


def test_axes():
    f, nb, start, step = SS._axis("t", 8, 4.0, False, None, None)
    assert np.array_equal(f, np.arange(5) * 0.5) and (nb, start, step) == (5, 0.0, 0.125)
    f, nb, start, step = SS._axis("t", 8, 4.0, True, None, None)
    assert np.array_equal(f, np.fft.fftfreq(8, 0.25)) and nb == 8
    f, nb, start, step = SS._axis("t", 8, 10.0, False, (0.0, 5.0), 11)
    assert np.allclose(f, np.arange(11) * 0.5) and (nb, start) == (11, 0.0) and abs(step - 0.05) < 1e-17
    assert SS._default_m(128, 4) == 42 and SS._default_m(1000, 4) == 64 and SS._default_m(4, 2) == 3 and SS._default_m(2, 0) == 2


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """sub_plan.h is host-only arithmetic: built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run here as its own
    process -- the tiles and shares of every length walked as k_cov_row walks them, the scratch of a pass, the passes, the refusals"""
    exe = str(tmp_path / "sub_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "pyfft_amd", "csrc"), os.path.join(ROOT, "tests", "sub_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sub plan ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
