"""The wavelet bispectrum without a GPU: the float64 reference of tests/wbic_ref.py on two records with quadratic phase coupling (what
the reference must show before the device is asked to), the float32 loss of the transform against the parity bound, the plan arithmetic
of sp_wbic_plan, the refusals of the C entry and of the Python front ends, the frequency grid, the reductions, and the declared set of
include/spectral_wbic.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import wbic_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, wavelet as W, wbicoherence as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QPC_KW = dict(dt=1.0, df=R.QPC_DF, fmin=R.QPC_KLO * R.QPC_DF, fmax=R.QPC_KHI * R.QPC_DF)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_grid_of_the_coupling_records():
    k_lo, k_hi, f, sc = WB.wbic_freqs(R.QPC_N, **QPC_KW)
    assert (k_lo, k_hi, sc.size) == (R.QPC_KLO, R.QPC_KHI, 70)
    np.testing.assert_allclose(sc, R.qpc_scales(), rtol=1e-14)
    np.testing.assert_allclose(f, np.arange(3, 73) / 400.0, rtol=1e-14)
    plan = W.cwt_plan(R.QPC_N, 1.0, wavelet=W.Morlet(6.0), scales=sc)
    assert (plan["M"], plan["L"], plan["hop"]) == (R.QPC_M, R.QPC_L, 2830) and plan["fused"].all()


def test_reference_finds_the_coupled_pair_and_not_the_control():
    B, b2, A, P = R.qpc_reference(False)
    assert b2.shape == (1, 70, 70)
    R.assert_qpc_whole(b2[0])
    ok = ~np.isnan(b2[0])
    i, j = np.nonzero(ok)
    assert np.all(i + j + R.QPC_KLO <= 69) and ok.sum() == sum(70 - R.QPC_KLO - r for r in range(70 - R.QPC_KLO))
    assert np.all(b2[0][ok] >= 0) and np.all(b2[0][ok] <= 1 + 1e-12) and np.all(np.abs(B[0][ok]) <= A[0][ok] * (1 + 1e-12))
    np.testing.assert_allclose(b2[0][ok], b2[0].T[ok], rtol=1e-9)                  # the auto form is symmetric


def test_reference_sees_the_coupling_switch_on():
    _, b2, _, _ = R.qpc_reference(True)
    assert b2.shape == (4, 70, 70)
    R.assert_qpc_switched(b2)
    sb, tot = WB.summed_bicoherence(b2), WB.total_bicoherence(b2)
    m = R.QPC_COUPLED[2] - R.QPC_KLO
    assert sb.shape == (4, 70) and np.all(np.isnan(sb[:, :R.QPC_KLO])) and np.all(np.isfinite(sb[:, R.QPC_KLO:]))
    assert sb[2, m] > 2 * sb[0, m] and sb[3, m] > 2 * sb[1, m]
    # written out once more: the mean over the valid pairs with the sum row m, and over all valid pairs
    pairs = [b2[3, i, m - R.QPC_KLO - i] for i in range(m - R.QPC_KLO + 1)]
    assert np.isclose(sb[3, m], np.mean(pairs)) and np.isclose(tot[3], np.nanmean(b2[3]))
    with pytest.raises(E.WbicRefused):
        WB.summed_bicoherence(np.zeros((3, 4)))


def test_float32_loss_stays_within_a_quarter_of_the_parity_bound():
    """the float32 restatement of the transform (overlap-save at complex64) feeding the float64 sums, against the float64 reference on
    the first record: measured here 0.0038 of the |dB| bound and 8.9e-8 for |db2|"""
    Bo, b2o, A, Po = R.qpc_reference(False)
    B, b2, _, P = R.wbic_ref32(R.qpc_record(0), R.qpc_scales(), R.QPC_KLO, 0, R.QPC_N, R.QPC_N, 1, R.QPC_L, R.QPC_M)
    ok = ~np.isnan(Bo)
    np.testing.assert_array_equal(np.isnan(B), ~ok)
    dB = float(np.max(np.abs(B[ok] - Bo[ok]) / R.parity_bound(A)[ok]))
    db2 = float(np.max(np.abs(b2[ok] - b2o[ok])))
    print("float32 restatement: max |dB| / bound = %.4g, max |db2| = %.3g" % (dB, db2))
    assert dB <= 0.25 and db2 <= 5e-5
    np.testing.assert_allclose(P, Po, rtol=1e-5)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.WBIC_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.WBIC_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


def _plan(lib, nsig, S, k_lo, L, M, n0, block, step, nblocks, nrec=1, sym=1):
    out = np.full(8, -7, dtype=np.int64)
    rc = lib.sp_wbic_plan(nsig, S, k_lo, L, M, n0, block, step, nblocks, nrec, sym, _ffi.ptr(out))
    return rc, dict(zip(("cells", "cell_len", "groups", "passes", "workgroups", "scratch", "chunk", "tiles"), (int(v) for v in out)))


def test_plan_arithmetic(monkeypatch):
    monkeypatch.delenv("SP_WBIC_CHUNK", raising=False)
    lib = _c_entry()
    # one block over 24 000 samples: one cell, 12 groups of at most 2048; S = 70 auto: the tiles (0, 0) and (1, 0)
    rc, p = _plan(lib, 24000, 70, 3, 4096, 633, 0, 24000, 24000, 1)
    assert rc == 0 and (p["cells"], p["cell_len"], p["groups"], p["passes"], p["tiles"], p["workgroups"]) == (1, 24000, 12, 1, 2, 24)
    assert p["chunk"] == (128 << 20) // (8 * 70)
    # the transforms [S][span + 2 M clipped], 48 KiB of partials and S float64 per (tile, group), 96 KiB and S float64 per (tile, cell)
    assert p["scratch"] == 8 * 70 * 24000 + 12 * (2 * 49152 + 8 * 70) + 1 * (2 * 98304 + 8 * 70)
    # the cross form computes every tile with a valid pair: (0, 0), (0, 1), (1, 0); three records share the budget
    rc, p = _plan(lib, 24000, 70, 3, 4096, 633, 0, 24000, 24000, 1, 3, 0)
    assert rc == 0 and p["tiles"] == 3 and p["chunk"] == (128 << 20) // (8 * 70 * 3)
    # disjoint blocks with gaps: a cell is a block; 1500 samples are one group
    rc, p = _plan(lib, 24000, 70, 3, 4096, 633, 183, 1500, 2000, 5)
    assert rc == 0 and (p["cells"], p["cell_len"], p["groups"], p["passes"]) == (5, 1500, 5, 1)
    # overlapping blocks: a cell is `step` samples, nblocks - 1 + block / step of them; 5000-sample cells are 3 groups
    rc, p = _plan(lib, 24000, 70, 3, 4096, 633, 0, 2000, 500, 5)
    assert rc == 0 and (p["cells"], p["cell_len"], p["groups"]) == (8, 500, 8)
    rc, p = _plan(lib, 100000, 70, 3, 4096, 633, 0, 10000, 5000, 4)
    assert rc == 0 and (p["cells"], p["cell_len"], p["groups"]) == (5, 5000, 15)
    # the hook caps the samples a pass spans: whole groups, at least one
    monkeypatch.setenv("SP_WBIC_CHUNK", "3000")
    rc, p = _plan(lib, 24000, 70, 3, 4096, 633, 183, 1500, 1500, 5, 3, 0)
    assert rc == 0 and (p["groups"], p["passes"], p["chunk"]) == (5, 3, 3000)
    rc, p = _plan(lib, 24000, 70, 3, 4096, 633, 0, 24000, 24000, 1)
    assert rc == 0 and (p["groups"], p["passes"]) == (12, 12)                   # a group of 2048 is never cut
    monkeypatch.setenv("SP_WBIC_CHUNK", "4096")
    assert _plan(lib, 24000, 70, 3, 4096, 633, 0, 24000, 24000, 1)[1]["passes"] == 6
    monkeypatch.setenv("SP_WBIC_CHUNK", "0")
    assert _plan(lib, 24000, 70, 3, 4096, 633, 0, 24000, 24000, 1)[1]["passes"] == 1
    # the front ends give the same figures
    assert E.wbic_plan(24000, 70, 3, 4096, 633, 0, 2000, 500, 5)["cells"] == 8
    d = WB.wbic_plan(R.QPC_N, block=6000, **QPC_KW)
    assert (d["S"], d["k_lo"], d["M"], d["L"], d["nblocks"], d["cells"], d["groups"], d["tiles"]) == (70, 3, 633, 4096, 4, 4, 12, 2)
    d = WB.wbic_plan(8527, trim=True, block=1500, nrec=3, sym=False, **QPC_KW)
    assert (d["n0"], d["n1"], d["nblocks"]) == (R.qpc_trim(), 8527 - R.qpc_trim(), 5) and R.qpc_trim() == 183
    assert lib.sp_wbic_plan(24000, 70, 3, 4096, 633, 0, 24000, 24000, 1, 1, 1, None) < 0


GOOD = dict(x=True, y=False, z=False, xd=0, yd=0, zd=0, nsig=6000, sc=None, sc_ptr=True, S=20, k_lo=2, fam=0, p0=6.0, L=1024, M=200, n0=0,
            block=1000, step=1000, nblocks=5, B=True, b2=True, P=True)
SENT = -12345.0


def _call(lib, **over):
    p = dict(GOOD, **over)
    recs = [np.ones(8000, dtype=np.float32) for _ in range(3)]
    sc = np.array(p["sc"] if p["sc"] is not None else np.linspace(40.0, 4.0, 520), dtype=np.float64)
    outs = [np.full(4096, SENT, dtype=np.float64) for _ in range(3)]
    passes = ctypes.c_int(-5)
    ptr = _ffi.ptr
    rc = lib.sp_wbic(*[ptr(r) if p[k] else None for r, k in zip(recs, "xyz")], p["xd"], p["yd"], p["zd"], p["nsig"],
                     ptr(sc) if p["sc_ptr"] else None, p["S"], p["k_lo"], p["fam"], p["p0"], p["L"], p["M"], p["n0"], p["block"], p["step"],
                     p["nblocks"], *[ptr(o) if p[k] else None for o, k in zip(outs, ("B", "b2", "P"))], ctypes.byref(passes), 0)
    return rc, (lib.sp_last_error() or b"").decode(), outs, passes.value


REFUSALS = [(dict(S=1), "nscales"), (dict(S=513), "nscales"), (dict(k_lo=0), "k_lo"), (dict(k_lo=20), "k_lo"),
            (dict(sc=[float("nan")] * 20), "scales[0]"), (dict(sc=[4.0] * 19 + [float("inf")]), "scales[19]"), (dict(sc=[4.0, -1.0] * 10), "scales[1]"),
            (dict(sc=[0.0] * 20), "scales[0]"), (dict(L=8192, M=3073), "3072"), (dict(L=1000), "power of two"), (dict(L=128, M=10), "power of two"),
            (dict(L=16384, M=3000), "power of two"), (dict(M=512), "M must"), (dict(M=-1), "M must"), (dict(M=400), "hop"),
            (dict(block=1000, step=300), "step >= block"), (dict(block=1000, step=999), "step >= block"), (dict(block=0), "at least 1"),
            (dict(step=0), "at least 1"), (dict(nblocks=0), "nblocks"), (dict(nblocks=7), "outside the record"), (dict(n0=-1), "outside the record"),
            (dict(n0=1001), "outside the record"), (dict(block=6001, step=6001, nblocks=1), "outside the record"),
            (dict(step=1 << 62, nblocks=3), "outside the record"), (dict(S=512, k_lo=2, nsig=8000, block=1, step=1, nblocks=171), "1 GiB"),
            (dict(S=512, block=6000, step=1, nblocks=1), "cell sums"), (dict(xd=2), "dtype"), (dict(xd=-1), "dtype"), (dict(y=True, yd=1), "differ"),
            (dict(z=True, zd=1), "differ"), (dict(x=False), "required"), (dict(sc_ptr=False), "required"), (dict(B=False), "required"),
            (dict(b2=False), "required"), (dict(P=False), "required"), (dict(fam=2), "family"), (dict(p0=0.0), "parameter"),
            (dict(fam=1, p0=0.5), "parameter"), (dict(nsig=0), "nsig")]


@pytest.mark.parametrize("over,word", REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(REFUSALS)])
def test_c_refusals(over, word):
    rc, msg, outs, passes = _call(_c_entry(), **over)
    assert rc < 0 and msg.startswith("sp_wbic: ") and word in msg, (rc, msg)
    assert all(np.all(o == SENT) for o in outs) and passes == -5
    p = dict(GOOD, **over)
    if not set(over) & {"sc", "xd", "yd", "zd", "x", "y", "z", "sc_ptr", "B", "b2", "P", "fam", "p0"}:       # what the plan judges as well
        out = np.zeros(8, dtype=np.int64)
        lib = _c_entry()
        assert lib.sp_wbic_plan(p["nsig"], p["S"], p["k_lo"], p["L"], p["M"], p["n0"], p["block"], p["step"], p["nblocks"], 1, 1,
                                _ffi.ptr(out)) < 0


def _both(exc):
    return isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    x = np.ones(6000, dtype=np.float32)
    sc = np.linspace(40.0, 4.0, 20)
    ok = dict(scales=sc, k_lo=2, family="morlet", param=6.0, L=1024, M=200, n0=0, block=1000, step=1000, nblocks=5)
    call = lambda v=x, **over: (lambda: E.wbic(v, **dict(ok, **over)))
    bad = [call(scales=sc[:1]), call(scales=np.ones(513)), call(scales=sc.reshape(4, 5)), call(k_lo=0), call(k_lo=20),
           call(scales=np.where(np.arange(20) == 3, np.nan, sc)), call(scales=-sc), call(L=1000), call(L=128, M=10), call(L=16384, M=3000),
           call(L=8192, M=3073), call(M=512), call(M=400), call(M=-1), call(family="dog"), call(family=None), call(param=0.0),
           call(family="paul", param=0.5), call(block=1000, step=300), call(block=0), call(step=0), call(nblocks=0), call(nblocks=7), call(n0=-1),
           call(n0=1001), call(scales=np.linspace(40.0, 4.0, 512), block=1, step=1, nblocks=171), call(scales=np.linspace(40.0, 4.0, 512), block=6000, step=1, nblocks=1),
           call(np.ones((2, 6000), dtype=np.float32)), call(y=np.ones(5999, dtype=np.float32)), call(y=np.ones(6000, dtype=np.complex64)),
           call(z=np.ones(6000, dtype=np.complex64)), call(np.float32(1.0)),
           lambda: E.wbic_plan(6000, 20, 0, 1024, 200, 0, 1000, 1000, 5), lambda: E.wbic_plan(6000, 1, 1, 1024, 200, 0, 1000, 1000, 5),
           lambda: E.wbic_plan(6000, 20, 2, 1024, 200, 0, 1000, 300, 5), lambda: E.wbic_plan(6000, 20, 2, 1024, 200, 0, 1000, 1000, 5, nrec=4),
           lambda: WB.wavelet_bispectrum(x), lambda: WB.wavelet_bispectrum(x, df=-1.0), lambda: WB.wavelet_bispectrum(x, df=0.01, wavelet="dog"),
           lambda: WB.wavelet_bispectrum(x, df=0.01, fmin=0.4, fmax=0.5),           # scales below the smallest that fuses
           lambda: WB.wavelet_bispectrum(x, df=0.01, fmax=0.2, block=1000, step=300),
           lambda: WB.wavelet_bispectrum(x, df=0.01, fmax=0.2, step=300), lambda: WB.wavelet_bispectrum(x, df=0.01, fmax=0.2, block=7000),
           lambda: WB.wavelet_bispectrum(x, df=0.01, fmax=0.2, trim=True, span=(0, 100)),
           lambda: WB.wavelet_bispectrum(x, df=0.01, fmax=0.2, span=(100, 100)), lambda: WB.wavelet_bispectrum(x, df=0.01, fmax=0.2, span=(0, 6001)),
           lambda: WB.wavelet_bispectrum(np.ones((2, 6000), dtype=np.float32), df=0.01, fmax=0.2),
           lambda: WB.wbic_plan(6000, df=0.01, fmax=0.2, block=1000, step=300), lambda: WB.wbic_freqs(0, 1.0, 0.01),
           lambda: WB.wbic_freqs(6000, 1.0, 0.01, fmin=0.3, fmax=0.2), lambda: WB.total_bicoherence(np.zeros(5))]
    for fn in bad:
        with pytest.raises(E.WbicRefused) as exc:
            fn()
        assert _both(exc)
    assert WB.WbicRefused is E.WbicRefused


def test_wbic_freqs_returns_only_fusing_scales():
    for wv, lowest in ((W.Morlet(6.0), 3.72), (W.Paul(4.0), 8.4)):
        k_lo, k_hi, f, sc = WB.wbic_freqs(5000, 1.0, 1 / 100, fmin=2 / 100, fmax=40 / 100, wavelet=wv)
        assert k_lo == 2 and f.size == sc.size == k_hi - k_lo + 1 and np.all(np.diff(f) > 0) and np.all(np.diff(sc) < 0)
        np.testing.assert_allclose(sc, 1.0 / (wv.flambda() * f), rtol=1e-14)
        assert all(W.margin(wv, s) <= W.FUSED_MAX_MARGIN for s in sc) and sc.min() >= lowest == W.smallest_fused_scale(wv)
        assert W.margin(wv, 1.0 / (wv.flambda() * (k_hi + 1) / 100)) > W.FUSED_MAX_MARGIN     # the next row does not fuse
    assert WB.wbic_freqs(5000, 1.0, 1 / 100, fmin=2 / 100, fmax=40 / 100)[1] == 26
    # dt scales the grid: the same rows at dt = 0.5 with twice the frequencies
    a, b = WB.wbic_freqs(5000, 1.0, 1 / 100, fmax=0.2), WB.wbic_freqs(5000, 0.5, 2 / 100, fmax=0.4)
    assert a[:2] == b[:2] == (1, 20) and np.allclose(2 * a[2], b[2]) and np.allclose(a[3], 2 * b[3])
    # long scales do not fuse either: the run starts where the margin fits
    k_lo, k_hi, f, sc = WB.wbic_freqs(1 << 20, 1.0, 1 / 4000, fmax=0.01)
    assert k_lo > 1 and W.margin(W.Morlet(6.0), sc[0]) <= 3072 < W.margin(W.Morlet(6.0), 1.0 / (W.Morlet(6.0).flambda() * (k_lo - 1) / 4000))


def test_exported_declared_and_bound():
    for name in ("wbic_freqs", "wavelet_bispectrum", "wavelet_bicoherence", "summed_bicoherence", "total_bicoherence", "wbic_plan"):
        assert getattr(pyfft_amd, name) is getattr(WB, name)
    for name in ("wbic", "wbic_plan", "wbic_check", "WbicRefused"):
        assert hasattr(E, name)
    assert issubclass(E.WbicRefused, ValueError) and issubclass(E.WbicRefused, NotImplementedError)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_wbic.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.WBIC_SIGNATURES) == {"sp_wbic", "sp_wbic_plan"}
    assert len(_ffi.TABLES) == 6 and all(t is not _ffi.WBIC_SIGNATURES for t in _ffi.TABLES)
    for table in _ffi.TABLES:
        assert not set(_ffi.WBIC_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_wbic", 23), ("sp_wbic_plan", 12)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.WBIC_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.WBIC_SIGNATURES[name][1]
    for other in ("spectral.h", "spectral_ext.h", "spectral_tfr.h", "spectral_quad.h", "spectral_cyclo.h", "spectral_uneven.h"):
        assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other)))
    assert "spectral_wbic.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert "SP_WBIC_CHUNK" in open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
