"""The discrete wavelet transforms without a GPU: the two forms of the reference of tests/dwt_ref.py against each other, perfect
reconstruction in float64, the values pywt documents, the Daubechies banks the package computes, the MODWT's energy split and
inversion, the packet orderings, the float32 figures the GPU test's allowances rest on, the declared set of include/spectral_dwt.h,
the refusals of every C entry and every Python front before the device is touched, the plan figures, and dwt_plan.h under sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dwt_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, _dwt_mod as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVELETS = {2: "db1", 4: "db2", 8: "db4", 20: "db10"}
NS = (1, 2, 3, 5, 8, 17, 37, 64)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("L", sorted(WAVELETS))
def test_the_two_forms_of_the_reference_agree(L, mode):
    dl, dh, rl, rh = D.wavelet_filters(WAVELETS[L])
    for n in NS:
        for cplx in (False, True):
            x = R.signal(n, 1, cplx, seed=L)[0].astype(np.complex128 if cplx else np.float64)
            a, d, _, _ = R.dwt_level(x, dl, dh, mode)
            a2, d2 = R.dwt_level_conv(x, dl, dh, mode)
            scale = np.max(np.abs(x))
            assert a.shape == a2.shape == (R.coeff_len(n, L, mode),)
            assert max(np.max(np.abs(a - a2)), np.max(np.abs(d - d2))) <= 1e-12 * scale
            back, _ = R.idwt_level(a, d, n, rl, rh, mode)
            assert np.max(np.abs(back - R.idwt_level_conv(a, d, n, rl, rh, mode))) <= 1e-12 * scale


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("L", sorted(WAVELETS))
def test_perfect_reconstruction_in_float64(L, mode, monkeypatch):
    monkeypatch.setattr(R, "EXACT_FILTERS", True)
    dl, dh, rl, rh = D.wavelet_filters(WAVELETS[L])
    for n in NS:
        x = R.signal(n, 2, True, seed=1).astype(np.complex128)
        for levels in sorted({1, min(3, E.dwt_max_levels(n, L, mode))}):
            c, _ = R.wavedec(x, dl, dh, mode, levels)
            assert [p.shape[-1] for p in c] == [ln for ln, _ in E.dwt_layout(n, L, mode, levels)[1]]
            back, _ = R.waverec(c, n, rl, rh, mode)
            assert np.max(np.abs(back - x)) <= 1e-13 * np.max(np.abs(x)), (n, levels)


def test_the_values_pywt_documents(monkeypatch):
    monkeypatch.setattr(R, "EXACT_FILTERS", True)
    dl, dh, rl, rh = D.wavelet_filters("db1")
    a, d, _, _ = R.dwt_level(np.array([1.0, 2, 3, 4]), dl, dh, "symmetric")
    assert np.allclose(a, [2.12132034, 4.94974747], atol=5e-9, rtol=0) and np.allclose(d, [-0.70710678, -0.70710678], atol=5e-9, rtol=0)
    c, _ = R.wavedec(np.arange(1.0, 9.0), dl, dh, "symmetric", 2)
    assert np.allclose(c[0], [5, 13], atol=1e-6) and np.allclose(c[1], [-2, -2], atol=1e-6) and np.allclose(c[2], [-0.70710678] * 4, atol=5e-9, rtol=0)
    assert D.dwt_max_level(1000, 10) == 6 and D.dwt_max_level(8, 2) == 3 and D.dwt_max_level(5, 8) == 0
    assert D.dwt_coeff_len(1000, 8, "symmetric") == 503 and D.dwt_coeff_len(1001, 8, "periodization") == 501
    assert [np.sign(f[0]) for f in (dl, dh, rl, rh)] == [1, -1, 1, 1]                  # pywt's Haar bank, sign for sign
    assert pyfft_amd.dwt_max_level is D.dwt_max_level and pyfft_amd.wavelet_filters is D.wavelet_filters


def test_the_daubechies_banks():
    s3 = np.sqrt(3.0)
    assert np.max(np.abs(D.daubechies(2) - np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0)))) <= 1e-15
    assert np.array_equal(D.wavelet_filters("haar")[2], D.wavelet_filters("db1")[2])
    for N in range(1, 11):
        dl, dh, rl, rh = D.wavelet_filters("db%d" % N)
        L = 2 * N
        assert rl.size == L and abs(rl.sum() - np.sqrt(2.0)) <= 1e-14
        for m in range(N):                                                            # orthonormal to its even shifts
            assert abs(np.dot(rl[:L - 2 * m], rl[2 * m:]) - (m == 0)) <= 1e-13, (N, m)
            assert abs(np.dot(rl[:L - 2 * m], rh[2 * m:])) <= 1e-13 and abs(np.dot(rh[:L - 2 * m], rl[2 * m:])) <= 1e-13
        t = np.arange(L, dtype=np.float64)
        for p in range(N):                                                            # N vanishing moments of the wavelet
            assert abs(np.sum(rh * t ** p)) <= 1e-12 * np.sum(np.abs(rh) * t ** p + (p == 0)), (N, p)
        assert np.array_equal(dl, rl[::-1]) and np.array_equal(dh, rh[::-1]) and np.array_equal(rh, rl[::-1] * (-1.0) ** np.arange(L))
        roots = np.roots(rl)                                                          # N at -1 (a multiple root: found to eps^(1/N)), the rest inside
        inner = roots[np.abs(roots + 1) > 0.2]
        assert inner.size == N - 1 and np.all(np.abs(inner) < 1)                      # minimum phase
    ours = D.wavelet_filters(tuple(R.bank_of(8)))

    class W:
        filter_bank = R.bank_of(8)
    assert all(np.array_equal(a, b) for a, b in zip(ours, D.wavelet_filters(W())))
    for bad in ("sym4", "db0", "db11", "coif1", 5, (dl, dh, rl), (dl, dh, rl, rh[:-1]), (dl[:3],) * 4, (np.full(4, np.nan),) * 4):
        with pytest.raises(E.DwtRefused):
            D.wavelet_filters(bad)


def test_modwt_energy_and_inversion(monkeypatch):
    monkeypatch.setattr(R, "EXACT_FILTERS", True)
    for L in sorted(WAVELETS):
        _, _, rl, rh = D.wavelet_filters(WAVELETS[L])
        for n, levels in ((5, 4), (37, 3), (64, 6), (333, 5)):
            x = R.signal(n, 2, True, seed=8).astype(np.complex128)
            W, _ = R.modwt(x, rl, rh, levels)
            e = np.sum(np.abs(x) ** 2)
            assert W.shape == (levels + 1, 2, n) and abs(np.sum(np.abs(W) ** 2) - e) <= 1e-12 * e
            assert np.max(np.abs(R.imodwt(W, rl, rh)[0] - x)) <= 1e-12 * np.max(np.abs(x))
            assert np.max(np.abs(R.modwt_mra(W, rl, rh).sum(axis=0) - x)) <= 1e-12 * np.max(np.abs(x))
    # level 1 of the Haar MODWT by hand
    W, _ = R.modwt(np.array([1.0, 2, 4, 8]), *D.wavelet_filters("haar")[2:], 1)
    assert np.allclose(W[1], [4.5, 1.5, 3, 6]) and np.allclose(W[0], [-3.5, 0.5, 1, 2])


def test_packet_orderings(monkeypatch):
    monkeypatch.setattr(R, "EXACT_FILTERS", True)
    dl, dh, rl, rh = D.wavelet_filters("db4")
    n, level = 256, 4
    m = n >> level
    t = np.arange(n)
    c, _ = R.wpdec(R.signal(n, 1, seed=3).astype(np.float64), dl, dh, level)
    assert c.shape == (1, 1 << level, m) and np.max(np.abs(R.wprec(c, rl, rh)[0] - R.signal(n, 1, seed=3))) <= 1e-12
    a, d, _, _ = R.dwt_level(R.signal(n, 1, seed=3).astype(np.float64), dl, dh, "periodization")
    aa, ad, _, _ = R.dwt_level(a, dl, dh, "periodization")
    da, dd, _, _ = R.dwt_level(d, dl, dh, "periodization")
    c2, _ = R.wpdec(R.signal(n, 1, seed=3).astype(np.float64), dl, dh, 2)
    assert all(np.max(np.abs(c2[:, p] - w)) <= 1e-13 for p, w in enumerate((aa, ad, da, dd)))      # node p has the children 2p (low), 2p + 1 (high)
    # a tone in band f of the 2^level bands lands at node gray(f) in natural order, at f in frequency order
    g = R.gray(level)
    assert sorted(g) == list(range(1 << level)) and list(R.gray(2)) == [0, 1, 3, 2] and np.array_equal(D._gray(level), g)
    for f in range(1 << level):
        tone = np.cos(np.pi * (f + 0.5) / (1 << level) * t)
        e = np.sum(R.wpdec(tone, dl, dh, level)[0] ** 2, axis=-1)
        assert int(np.argmax(e)) == g[f], (f, e)


def test_the_recorded_float32_figures():
    """the figures the GPU test's allowances are 4 x of: the float32 restatement against float64 on the octave record"""
    _, _, rl, rh = D.wavelet_filters("db4")
    var, mra = R.float32_figures(rl, rh)
    print("float32 restatement: variance %.3e relative (recorded %.3e), mra sum %.3e (recorded %.3e)" % (var, R.F32_VARIANCE_REL, mra, R.F32_MRA_SUM))
    assert abs(var - R.F32_VARIANCE_REL) <= 0.02 * R.F32_VARIANCE_REL and abs(mra - R.F32_MRA_SUM) <= 0.02 * R.F32_MRA_SUM
    x = R.octave_record().astype(np.float64)
    nu2, edof = R.modwt_variance(x, rl, rh, R.OCTAVE_LEVEL)
    assert int(np.argmax(nu2)) == 3 and nu2[0] > 10 * nu2[1] and abs(nu2[0] - 0.5) < 0.05 and abs(nu2[3] - 2.0) < 0.3     # sin^2 -> 1/2, (2 sin)^2 -> 2
    assert np.array_equal(edof, [max((4096 - (2 ** j - 1) * 7) / 2.0 ** j, 1.0) for j in range(1, 7)])
    e32, b = R.wavedec(x[None, :1000], *D.wavelet_filters("db4")[:2], "symmetric", 4, B=0.0, single=True)
    e64, _ = R.wavedec(x[None, :1000], *D.wavelet_filters("db4")[:2], "symmetric", 4)
    assert all(np.all(np.abs(p - q) <= bb + R.TINY) for p, q, bb in zip(e32, e64, b))          # the restatement keeps the bound itself


# ---- the C entries ------------------------------------------------------------------------------------------------------------------
NAMES = ("sp_dwt", "sp_dwt_level", "sp_idwt", "sp_idwt_level", "sp_modwt", "sp_imodwt", "sp_dwt_plan")


def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.DWT_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.DWT_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


def test_exported_declared_and_bound():
    for name in ("wavelet_filters", "dwt_max_level", "dwt_coeff_len", "dwt", "idwt", "wavedec", "waverec", "modwt", "imodwt", "modwt_mra", "modwt_variance",
                 "wpdec", "wprec", "dwt_plan", "DwtRefused"):
        assert getattr(pyfft_amd, name) is getattr(D, name), name
    for name in ("dwt", "dwt_level", "idwt", "idwt_level", "modwt", "imodwt", "dwt_plan", "DwtRefused"):
        assert hasattr(E, name)
    assert issubclass(E.DwtRefused, ValueError) and issubclass(E.DwtRefused, NotImplementedError) and D.DwtRefused is E.DwtRefused
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_dwt.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.DWT_SIGNATURES) == set(NAMES)
    assert len(_ffi.TABLES) == 6 and len(_ffi.MORE_TABLES) == 6 and _ffi.MORE_TABLES[-1] is _ffi.AR_SIGNATURES
    assert all(t is not _ffi.DWT_SIGNATURES for t in _ffi.TABLES + _ffi.MORE_TABLES) and _ffi.LATER_TABLES == (_ffi.DWT_SIGNATURES,)
    for table in _ffi.TABLES + _ffi.MORE_TABLES:
        assert not set(_ffi.DWT_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in zip(NAMES, (14, 15, 14, 15, 13, 13, 9)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.DWT_SIGNATURES[name][1]) == want, name
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.DWT_SIGNATURES[name][1]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "spectral_dwt.h":
            assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other))), other
    assert "spectral_dwt.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert '#include "../../include/spectral_dwt.h"' in open(os.path.join(ROOT, "pyfft_amd", "csrc", "spectral.hip")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    for k in ("dwt_row", "idwt_row", "modwt_row", "imodwt_row", "dwt_tile", "idwt_tile", "modwt_tile", "imodwt_tile"):
        assert "launch_%s(" % k in launch
    ext = open(os.path.join(ROOT, "include", "spectral_ext.h")).read()
    assert "which = 9" in ext and "sp_dwt" in ext and "which=9" in E.last_passes.__doc__
    assert _ffi.load_library().sp_last_passes(9) == 0 and E.DWT_PASSES == 9
    kernel = open(os.path.join(ROOT, "pyfft_amd", "csrc", "k_dwt.hip")).read()
    assert "atomic" not in kernel.split("#include")[1].lower() and "hipMemset" not in kernel and "asm" not in kernel.split("#include")[1]
    for k in ("k_dwt_row", "k_idwt_row", "k_modwt_row", "k_imodwt_row", "k_dwt_tile", "k_idwt_tile", "k_modwt_tile", "k_imodwt_tile"):
        assert "void %s(" % k in kernel
    assert kernel.count("fmaf(") == 3                                       # one place multiplies: dwt_fma, which dwt_ana and dwt_syn call


def plan_ref(what, cplx, n, L, mode, levels, rows, form=0, hook=0):
    """dwt_plan.h restated -> (the ten figures, the entries)"""
    el, mo = (8 if cplx else 4), what >= 2
    lens = [n]
    for _ in range(levels):
        lens.append(n if mo else E.dwt_coeff_len(lens[-1], L, mode))
    if mo:
        entries = [(n, e * rows * n) for e in range(levels + 1)]
        top = 30
    else:
        entries, top = E.dwt_layout(n, L, mode, levels)[1], E.dwt_max_levels(n, L, mode)
    rpw = 4 if n <= 1024 else 1
    lds = 512 + 2 * rpw * (max(n, L - 1) + 2 * (L - 1)) * el
    if form != 2 and lds <= 160 * 1024:
        return (1, 1024, lds, -(-rows // rpw), min(rows, 1), min(rows, 1), 0, max(rows, 1), top, rpw), entries
    buf, tiles, most = [0, 0], 0, 1
    for j in range(1, levels + 1):
        t = -(-(lens[j - 1] if what == 1 else lens[j]) // 1024)
        tiles, most = tiles + t, max(most, t)
        if j < levels:
            buf[j & 1] = max(buf[j & 1], lens[j])
    row_bytes = sum(buf) * el
    fit = max(1, (512 << 20) // row_bytes) if row_bytes else (1 << 31) - 1
    fit = min(fit, ((1 << 31) - 1) // most)
    if hook > 0:
        fit = min(fit, hook)
    rpp = min(max(rows, 1), fit)
    passes = -(-rows // rpp)
    lds = {0: (2 * 1024 + L - 2) * el, 1: 2 * (512 + L // 2 + 1) * el}.get(what, 0)
    return (2, 1024, lds, rows * tiles, passes * levels, passes, rpp * row_bytes if rows else 0, rpp, top, rpw), entries


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_DWT_ROWS", raising=False)
    lib = _c_entry()
    out = np.zeros(80, dtype=np.int64)

    def plan(what, cplx, n, L, mode, levels, rows, form=0):
        assert lib.sp_dwt_plan(what, int(cplx), n, L, mode, levels, rows, form, _ffi.ptr(out)) == 0, (what, cplx, n, L, mode, levels, rows, form)
        return tuple(int(v) for v in out[:10]), [(int(out[10 + 2 * e]), int(out[11 + 2 * e])) for e in range(levels + 1)]
    shapes = [(0, 0, 1, 2, 0, 1, 1), (0, 1, 1000, 8, 2, 7, 3), (1, 0, 1024, 8, 5, 10, 1 << 14), (0, 0, 1024, 8, 2, 7, 1 << 14), (0, 0, 1025, 20, 3, 5, 9),
              (0, 0, 20402, 8, 2, 3, 2), (0, 0, 20403, 8, 2, 3, 2), (1, 1, 10194, 8, 4, 3, 2), (1, 1, 10195, 8, 1, 3, 2), (0, 0, 1 << 26, 8, 2, 8, 1),
              (0, 1, (1 << 31) - 1, 64, 5, 31, 3), (2, 0, 1 << 22, 8, 0, 10, 1), (3, 1, 4099, 20, 0, 6, 2), (2, 0, 5, 20, 0, 4, 0), (0, 0, 37, 8, 3, 3, 257)]
    for s in shapes:
        for form in (0, 2):
            assert plan(*s, form) == plan_ref(s[0], bool(s[1]), *s[2:], form), (s, form)
    assert plan(0, 0, 1024, 8, 2, 7, 1 << 14)[0][:6] == (1, 1024, 512 + 2 * 4 * 1038 * 4, 4096, 1, 1)          # the many-short-rows shape: one launch, 33 KiB a workgroup
    assert plan(0, 0, 1 << 26, 8, 2, 8, 1)[0][:2] == (2, 1024) and plan(0, 0, 1 << 26, 8, 2, 8, 1)[0][4] == 8
    assert plan(0, 0, 20402, 8, 2, 3, 2)[0][0] == 1 and plan(0, 0, 20403, 8, 2, 3, 2)[0][0] == 2 and lib.sp_dwt_plan(0, 0, 20403, 8, 2, 3, 2, 1, _ffi.ptr(out)) < 0
    monkeypatch.setenv("SP_DWT_ROWS", "2")
    assert plan(0, 0, 37, 8, 3, 3, 257, 2) == plan_ref(0, False, 37, 8, 3, 3, 257, 2, hook=2) and plan(0, 0, 37, 8, 3, 3, 257, 2)[0][5] == 129
    monkeypatch.delenv("SP_DWT_ROWS")
    d = E.dwt_plan("dwt", 1000, 8, "symmetric", 7, 3, True)
    assert d == D.dwt_plan("dwt", 1000, "db4", "symmetric", 7, 3, True) == pyfft_amd.dwt_plan("dwt", 1000, "db4", level=7, rows=3, cplx=True)
    ref = plan_ref(0, True, 1000, 8, 2, 7, 3)
    assert tuple(d[k] for k in E.DWT_PLAN_NAMES) == ref[0] and d["entries"] == ref[1]
    assert lib.sp_dwt_plan(0, 0, 64, 8, 2, 1, 1, 0, None) < 0
    for bad in ((4, 0, 64, 8, 2, 1, 1, 0), (0, 2, 64, 8, 2, 1, 1, 0), (0, 0, 0, 8, 2, 1, 1, 0), (0, 0, 64, 7, 2, 1, 1, 0), (0, 0, 64, 66, 2, 1, 1, 0), (0, 0, 64, 8, 6, 1, 1, 0),
                (0, 0, 64, 8, 2, 0, 1, 0), (0, 0, 64, 2, 2, 7, 1, 0), (0, 0, 64, 8, 2, 1, -1, 0), (0, 0, 64, 8, 2, 1, 1, 3), (2, 0, 64, 8, 0, 31, 1, 0), (0, 0, 1 << 31, 8, 2, 1, 1, 0)):
        assert lib.sp_dwt_plan(*bad, _ffi.ptr(out)) < 0, bad
    for bad in (("cwt", 64, 8), ("dwt", 64, 7), ("dwt", 64, 8, "smooth"), ("dwt", 64, 8, "symmetric", 0), ("dwt", 64, 2, "zero", 7), ("modwt", 64, 8, None, 31),
                ("dwt", 64, 8, "zero", 1, -1), ("dwt", 30000, 8, "zero", 1, 1, False, "row"), ("dwt", 64, 8, "zero", 1, 1, False, "wave")):
        with pytest.raises(E.DwtRefused):
            E.dwt_plan(*bad)


SENT = -12345.0
NAN, INF = float("nan"), float("inf")
GOOD = dict(x=True, dtype=0, ild=64, n=64, batch=2, lo=True, hi=True, L=8, mode=2, levels=2, out=True, old=None, form=0, taps=None)
COMMON = [(dict(dtype=2), "dtype"), (dict(L=7), "even"), (dict(L=0), "even"), (dict(L=66), "2 .. 64"), (dict(lo=False), "filters are required"),
          (dict(hi=False), "filters are required"), (dict(taps=NAN), "finite"), (dict(taps=INF), "finite"), (dict(n=0), "n must"), (dict(n=1 << 31, ild=1 << 31), "n must"),
          (dict(batch=-1), "batch"), (dict(form=3), "form"), (dict(form=-1), "form"), (dict(n=30000, ild=30000, old=40000, form=1), "row form does not fit"),
          (dict(ild=63), "_ld"), (dict(old=0), "_ld"), (dict(x=False), "is required"), (dict(out=False), "is required")]
PYRAMID = COMMON + [(dict(mode=6), "mode"), (dict(mode=-1), "mode"), (dict(levels=0), "levels"), (dict(levels=33), "levels"), (dict(L=2, levels=7), "one coefficient")]
MODWT = COMMON + [(dict(levels=0), "levels"), (dict(levels=31), "levels"), (dict(L=64, levels=27), "2^31")]
ENTRIES = [("sp_dwt", PYRAMID), ("sp_idwt", PYRAMID), ("sp_dwt_level", [c for c in PYRAMID if "levels" not in c[0]]),
           ("sp_idwt_level", [c for c in PYRAMID if "levels" not in c[0]]), ("sp_modwt", MODWT), ("sp_imodwt", MODWT)]
CASES = [(name, over, word) for name, lst in ENTRIES for over, word in lst]


@pytest.mark.parametrize("name,over,word", CASES, ids=["%s-%s-%d" % (n, w.split()[0], i) for i, (n, _, w) in enumerate(CASES)])
def test_c_refusals(name, over, word):
    """every entry refuses before the device is touched (this machine has none: a call that reached it would fail otherwise) and leaves
    its outputs alone"""
    lib = _c_entry()
    p = dict(GOOD, **over)
    L = max(2, min(p["L"], 64))
    lo, hi = np.full(L, 0.5), np.full(L, -0.5)
    if p["taps"] is not None:
        hi[L - 1] = p["taps"]
    buf_in, buf_out = np.ones(1 << 16, dtype=np.float32), np.full(1 << 16, SENT, dtype=np.float32)
    second = buf_out[1 << 15:]
    lo_p, hi_p = (_ffi.ptr(lo) if p["lo"] else None), (_ffi.ptr(hi) if p["hi"] else None)
    xin, out = (_ffi.ptr(buf_in) if p["x"] else None), (_ffi.ptr(buf_out) if p["out"] else None)
    n, b, ild = p["n"], p["batch"], p["ild"]
    lev = 1 if "level" in name else p["levels"]
    mo = "modwt" in name
    need_out = 200 if p["old"] is None else p["old"]             # at least the 64 samples, 70 coefficients of a level or 77 of the pyramid
    if name == "sp_dwt":
        rc = lib.sp_dwt(xin, p["dtype"], ild, n, b, lo_p, hi_p, p["L"], p["mode"], lev, out, need_out, p["form"], 0)
    elif name == "sp_idwt":
        rc = lib.sp_idwt(xin, p["dtype"], max(ild, 200) if ild >= 64 else ild - 40, n, b, lo_p, hi_p, p["L"], p["mode"], lev, out, need_out, p["form"], 0)
    elif name == "sp_dwt_level":
        rc = lib.sp_dwt_level(xin, p["dtype"], ild, n, b, lo_p, hi_p, p["L"], p["mode"], out, need_out, _ffi.ptr(second) if p["out"] else None, need_out, p["form"], 0)
    elif name == "sp_idwt_level":
        rc = lib.sp_idwt_level(xin, max(ild, 200) if ild >= 64 else ild - 40, xin, max(ild, 200) if ild >= 64 else ild - 40, p["dtype"], n, b, lo_p, hi_p, p["L"], p["mode"], out,
                               need_out, p["form"], 0)
    elif name == "sp_modwt":
        rc = lib.sp_modwt(xin, p["dtype"], ild, n, b, lo_p, hi_p, p["L"], lev, out, need_out, p["form"], 0)
    else:
        rc = lib.sp_imodwt(xin, p["dtype"], ild, n, b, lo_p, hi_p, p["L"], lev, out, need_out, p["form"], 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc == -1 and msg.startswith(name + ": ") and word in msg and np.all(buf_out == np.float32(SENT)), (rc, msg)
    assert not mo or "mode" not in over


def test_nothing_to_do_and_overlapping_host_outputs():
    lib = _c_entry()
    lo, hi = np.full(8, 0.5), np.full(8, -0.5)
    x, out = np.ones(4096, dtype=np.float32), np.full(4096, SENT, dtype=np.float32)
    P = _ffi.ptr
    assert lib.sp_dwt(P(x), 0, 64, 64, 0, P(lo), P(hi), 8, 2, 2, P(out), 200, 0, 0) == 0
    assert lib.sp_idwt(P(x), 0, 200, 64, 0, P(lo), P(hi), 8, 2, 2, P(out), 64, 0, 0) == 0
    assert lib.sp_dwt_level(P(x), 0, 64, 64, 0, P(lo), P(hi), 8, 2, P(out), 35, P(out[2048:]), 35, 0, 0) == 0
    assert lib.sp_idwt_level(P(x), 35, P(x), 35, 0, 64, 0, P(lo), P(hi), 8, 2, P(out), 64, 0, 0) == 0
    assert lib.sp_modwt(P(x), 0, 64, 64, 0, P(lo), P(hi), 8, 3, P(out), 64, 0, 0) == 0
    assert lib.sp_imodwt(P(x), 0, 64, 64, 0, P(lo), P(hi), 8, 3, P(out), 64, 0, 0) == 0
    assert np.all(out == np.float32(SENT))
    rc = lib.sp_dwt_level(P(x), 0, 64, 64, 2, P(lo), P(hi), 8, 2, P(out), 70, P(out[35:]), 70, 0, 0)        # interleaved host rows: only on the device
    assert rc == -1 and b"must not overlap" in lib.sp_last_error() and np.all(out == np.float32(SENT))


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    x = np.ones((2, 64), dtype=np.float32)
    dl, dh, rl, rh = D.wavelet_filters("db4")
    W = np.ones((4, 2, 64), dtype=np.float32)
    bad = [lambda: E.dwt(x, dl[:7], dh[:7]), lambda: E.dwt(x, dl, dh[:6]), lambda: E.dwt(x, np.ones(66), np.ones(66)), lambda: E.dwt(x, dl * np.nan, dh),
           lambda: E.dwt(x, dl, dh, "smooth"), lambda: E.dwt(x, dl, dh, "antisymmetric"), lambda: E.dwt(x, dl, dh, "antireflect"), lambda: E.dwt(x, dl, dh, "mirror"),
           lambda: E.dwt(x, dl, dh, 6), lambda: E.dwt(x, dl, dh, levels=0), lambda: E.dwt(x, dl, dh, levels=33), lambda: E.dwt(x, *D.wavelet_filters("haar")[:2], levels=7),
           lambda: E.dwt(x, dl, dh, form="wave"), lambda: E.dwt(x[:, :0], dl, dh), lambda: E.dwt_level(x, dl, dh, "smooth"),
           lambda: E.dwt_level(x, dl[:5], dh[:5]), lambda: E.idwt(x, 64, rl, rh), lambda: E.idwt(np.ones((2, 70), np.float32), 64, rl, rh, levels=2),
           lambda: E.idwt(x, 0, rl, rh), lambda: E.idwt_level(x[:, :35], x[:, :34], 64, rl, rh), lambda: E.idwt_level(x[:, :35], x[:, :35], 66, rl, rh),
           lambda: E.idwt_level(x, None, 64, rl, rh), lambda: E.modwt(x, rl, rh, 0), lambda: E.modwt(x, rl, rh, 31), lambda: E.modwt(x, np.ones(64), np.ones(64), 27),
           lambda: E.modwt(x, rl, rh[:4], 2), lambda: E.imodwt(W[:1], rl, rh), lambda: E.imodwt(W[0, 0], rl, rh), lambda: E.imodwt(W, rl[:3], rh[:3]),
           lambda: D.wavedec(x, "sym4"), lambda: D.wavedec(x, "db4", "smooth"), lambda: D.wavedec(x, "db4", level=40), lambda: D.wavedec(x, "db4", axis=2),
           lambda: D.waverec([x[:, :35]], "db4"), lambda: D.waverec([x[:, :20], x[:, :20], x[:, :35]], "db4"), lambda: D.waverec([x[:, :35], x[:, :35]], "db4", n=62),
           lambda: D.dwt(x, "db12"), lambda: D.idwt(x[:, :35], x[:, :35], "db4", n=70), lambda: D.modwt(x, "db4", 40), lambda: D.modwt_mra(W[:1], "db4"),
           lambda: D.modwt_variance(x, "db4", 4), lambda: D.modwt_variance(x, "db4", 0), lambda: D.wpdec(x, "db4", 7), lambda: D.wpdec(x, "db4", 0),
           lambda: D.wpdec(x[:, :60], "db4", 3), lambda: D.wpdec(x, "db4", 2, order="paley"), lambda: D.wprec(np.ones((2, 3, 8), np.float32), "db4"), lambda: D.wprec(x[0], "db4"),
           lambda: D.wprec(W[0], "db4", order="gray"), lambda: D.dwt_max_level(0, 8), lambda: D.dwt_coeff_len(64, 8, "smooth"), lambda: D.dwt_plan("dwt", 64, "db4", "smooth")]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError) as exc:
            fn()
        assert isinstance(exc.value, NotImplementedError) and isinstance(exc.value, E.DwtRefused), i


def test_layouts_and_levels():
    assert E.dwt_layout(8, 2, "symmetric", 2) == ([8, 4, 2], [(2, 0), (2, 2), (4, 4)], 8)
    assert E.dwt_layout(1000, 8, "symmetric", 3)[0] == [1000, 503, 255, 131] and E.dwt_layout(1001, 8, "periodization", 3)[0] == [1001, 501, 251, 126]
    assert E.dwt_max_levels(1, 2, "symmetric") == 1 and E.dwt_max_levels(1024, 2, "zero") == 10 and E.dwt_max_levels(1000, 8, "periodization") == 10
    assert E.dwt_max_levels(1000, 20, "symmetric") == 32 and E.dwt_max_levels((1 << 31) - 1, 64, "periodization") == 31
    for L in sorted(WAVELETS):
        for mode in R.MODES:
            for n in NS:
                top = E.dwt_max_levels(n, L, mode)
                assert E.dwt_layout(n, L, mode, top)[0] == R.level_lens(n, L, mode, top)


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """dwt_plan.h is host-only arithmetic: built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run here as its own
    process -- the index maps, every level's length and offset, the tiles of both directions walked as the kernels walk them, the
    halo arithmetic at the largest row, the row form's limit, the passes, the refusals"""
    exe = str(tmp_path / "dwt_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "pyfft_amd", "csrc"), os.path.join(ROOT, "tests", "dwt_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dwt plan ok" in r.stdout
