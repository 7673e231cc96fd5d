"""The smoothed pseudo Wigner-Ville distribution without a GPU: the numpy restatements of tests/wvd_ref.py against a plain triple loop
and against what the distribution is for (a chirp's ridge, cross-term suppression, the frequency marginal), the refusals of sp_wvd,
sp_wvd_plan and their Python front ends, the declared set of include/spectral_quad.h, and the measured float32 figure the GPU test's
allowance rests on."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
import wvd_ref as R
from pyfft_amd import _ffi, engine as E, wigner as WG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


TINY = dict(hop=3, first=-3, ntimes=15, nfft=32)


def _tiny():
    return _noise(40, 1), R.hamming(15), R.hamming(5) / np.sum(R.hamming(5))


def test_reference_against_triple_loop():
    z, h, g = _tiny()
    y = _noise(40, 2)
    for other in (None, y):
        a, b = R.wvd_ref(z, h, g, y=other, scale=0.7, **TINY), R.wvd_loops(z, h, g, y=other, scale=0.7, **TINY)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))


def test_auto_is_real_and_cross_is_hermitian_in_its_arguments():
    z, h, g = _tiny()
    W = R.wvd_ref(z, h, g, **TINY)
    assert np.max(np.abs(W.imag)) <= 1e-12 * np.max(np.abs(W))
    y = _noise(40, 2)
    assert np.max(np.abs(R.wvd_ref(z, h, g, y=y, **TINY) - np.conj(R.wvd_ref(y, h, g, y=z, **TINY)))) <= 1e-12 * np.max(np.abs(W))


def marginal(z, h, g, hop, first, ntimes, nfft, scale):
    """nfft scale h[0] sum_mu g[mu] |z[n_j + mu]|^2"""
    Lg = len(g) // 2
    zp = np.concatenate((np.zeros(Lg + abs(first) + 1), np.abs(np.asarray(z, dtype=np.complex128)) ** 2,
                         np.zeros(Lg + first + ntimes * hop + 1)))
    off = Lg + abs(first) + 1
    return np.array([nfft * scale * h[len(h) // 2] * np.sum(g * zp[off + first + j * hop - Lg:off + first + j * hop + Lg + 1])
                     for j in range(ntimes)])


def test_frequency_marginal():
    z, h, g = _tiny()
    W = R.wvd_ref(z, h, g, scale=1.0 / 32, **TINY).real
    want = marginal(z, h, g, 3, -3, 15, 32, 1.0 / 32)
    assert np.max(np.abs(W.sum(axis=1) - want)) <= 1e-12 * np.max(want)


def test_chirp_ridge_follows_the_instantaneous_frequency():
    n = np.arange(600)
    f_inst = 0.05 + 0.30 * n / 600.0
    z = ss.hilbert(np.cos(2 * np.pi * (0.05 * n + 0.15 * n ** 2 / 600.0)))
    nfft, hop = 256, 7
    h, g = R.hamming(127), R.hamming(9) / np.sum(R.hamming(9))
    ntimes = (600 - 1) // hop + 1
    W = R.wvd_ref(z, h, g, hop, 0, ntimes, nfft).real
    cols = [j for j in range(ntimes) if 80 <= j * hop < 520]
    dev = np.array([abs(int(np.argmax(W[j])) - 2 * nfft * f_inst[j * hop]) for j in cols])
    print("chirp: largest ridge deviation %.2f bins over %d columns" % (dev.max(), len(cols)))
    assert len(cols) >= 60 and dev.max() <= 1.0


def test_time_smoothing_suppresses_the_cross_term():
    n = np.arange(800)
    z = np.exp(2j * np.pi * 0.10 * n) + np.exp(2j * np.pi * 0.20 * n)
    nfft, h = 256, R.hamming(127)
    ratio = {}
    for name, g in (("pseudo", np.ones(1)), ("smoothed", R.hamming(21) / np.sum(R.hamming(21)))):
        W = R.wvd_ref(z, h, g, 1, 350, 100, nfft).real
        ridge = np.mean(W[:, int(round(2 * nfft * 0.10))])
        ratio[name] = np.max(np.abs(W[:, int(round(2 * nfft * 0.15))])) / ridge
    print("cross-term over ridge: pseudo %.2f, smoothed %.3f" % (ratio["pseudo"], ratio["smoothed"]))
    assert ratio["pseudo"] > 1.5 and ratio["smoothed"] < 0.05


def test_float32_restatement_deviation():
    """the figure the GPU allowance rests on: wvd_ref32 against wvd_ref over the GPU test's shapes, per column, relative to the column's
    largest |W|"""
    worst = 0.0
    for name, s in R.SHAPES.items():
        x, y = R.signals(name)
        h, g = (w.astype(np.float32) for w in R.windows_of(s))
        for cross in (False, True):
            ref = R.reference(name, cross)
            for r in range(s["rows"]):
                w32 = R.wvd_ref32(x[r], h, g, s["hop"], s["first"], s["ntimes"], s["nfft"], y[r] if cross else None)
                e = R.column_error(w32 if cross else w32.real, ref[r])
                assert np.all(np.isfinite(e)), name             # a column of zeros stays a column of zeros
                worst = max(worst, float(e.max()))
    print("float32 restatement: %.3e of a column's largest cell; recorded %.3e; allowance %.3e" % (worst, R.F32_DEV, R.ALLOWANCE))
    assert 0.5 * R.F32_DEV <= worst <= R.F32_DEV
    assert R.ALLOWANCE == 4 * R.F32_DEV and R.ALLOWANCE <= R.PARITY


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.QUAD_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.QUAD_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


GOOD = dict(x=True, y=False, x_ld=500, nsig=500, batch=2, h=True, nh=63, g=True, ng=9, nfft=256, hop=10, first=-5, ntimes=7, b0=0, nb=256,
            scale=1.0, W=True)
SENT = np.float32(-12345.0)


def _call(lib, **over):
    p = dict(GOOD, **over)
    x = np.ones(1000, dtype=np.complex64)
    y = np.ones(1000, dtype=np.complex64)
    h, g = np.ones(max(p["nh"], 1), dtype=np.float32), np.ones(max(p["ng"], 1), dtype=np.float32)
    W = np.full(4096, SENT, dtype=np.float32)
    rc = lib.sp_wvd(_ffi.ptr(x) if p["x"] else None, _ffi.ptr(y) if p["y"] else None, p["x_ld"], p["nsig"], p["batch"],
                    _ffi.ptr(h) if p["h"] else None, p["nh"], _ffi.ptr(g) if p["g"] else None, p["ng"], p["nfft"], p["hop"], p["first"],
                    p["ntimes"], p["b0"], p["nb"], p["scale"], _ffi.ptr(W) if p["W"] else None, 0)
    return rc, (lib.sp_last_error() or b"").decode(), W


REFUSALS = [
    (dict(nfft=16), "nfft"), (dict(nfft=16384), "nfft"), (dict(nfft=250), "nfft"),
    (dict(nh=64), "nh"), (dict(nh=0), "nh"), (dict(nh=257), "nh"), (dict(nfft=32, nb=32, nh=33), "nh"),
    (dict(ng=8), "ng"), (dict(ng=0), "ng"), (dict(ng=257), "ng"),
    (dict(hop=0), "hop"), (dict(ntimes=-1), "ntimes"), (dict(batch=-1), "batch"), (dict(batch=65536), "batch"),
    (dict(nsig=0), "nsig"), (dict(x_ld=499), "x_ld"), (dict(nb=0), "nb"), (dict(nb=257), "nb"), (dict(b0=-1), "b0"), (dict(b0=256), "b0"),
    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"),
    (dict(x=False), "x is"), (dict(h=False), "h is"), (dict(g=False), "g is"), (dict(W=False), "W is"),
    (dict(hop=100000, ntimes=2), "LDS"),     # auto: a pair of columns is staged in one piece (cross always fits with one column per run)
]


@pytest.mark.parametrize("over,word", REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(REFUSALS)])
def test_c_refusals(over, word):
    rc, msg, W = _call(_c_entry(), **over)
    assert rc < 0 and msg.startswith("sp_wvd: ") and word in msg, (rc, msg)
    assert np.all(W == SENT)


def test_nothing_to_do():
    lib = _c_entry()
    for over in (dict(batch=0), dict(ntimes=0)):
        rc, _, W = _call(lib, **over)
        assert rc == 0 and np.all(W == SENT)


def lds_formula(cross, nfft, nh, ng, hop, cpr, ntimes):
    """max(1, 4096 / nfft) images of nfft + 16 complex; the staged samples of c columns, c = cpr (auto: rounded up to even) or ntimes"""
    c = min(cpr if cross else cpr + cpr % 2, ntimes)
    return max(1, 4096 // nfft) * (nfft + 16) * 8 + 8 * ((c - 1) * hop + 2 * (nh // 2 + ng // 2) + 1)


PLAN_SHAPES = [(256, 127, 9, 7, 41, 1), (32, 31, 1, 1, 37, 1), (256, 63, 255, 300, 6, 1), (2048, 2047, 33, 64, 9, 3), (8192, 8191, 5, 1000, 5, 1),
               (1024, 255, 33, 1, 1 << 20, 1), (256, 63, 1, 16, 65536, 4)]


@pytest.mark.parametrize("nfft,nh,ng,hop,ntimes,batch", PLAN_SHAPES)
@pytest.mark.parametrize("cross", (0, 1))
def test_plan(cross, nfft, nh, ng, hop, ntimes, batch, monkeypatch):
    monkeypatch.delenv("SP_WVD_CPR", raising=False)
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    assert lib.sp_wvd_plan(cross, nfft, nh, ng, hop, ntimes, batch, nfft, _ffi.ptr(out)) == 0
    cpr, wgs, lds, xf, fits = (int(v) for v in out)
    assert 1 <= cpr <= ntimes and wgs == -(-ntimes // cpr) * batch
    assert lds == lds_formula(cross, nfft, nh, ng, hop, cpr, ntimes) == E.wvd_lds_bytes(cross, nfft, nh, ng, hop, cpr, ntimes)
    assert xf == (cpr if cross else (cpr + 1) // 2)
    assert fits == 1 and lds <= 160 * 1024          # every shape of the GPU tests fits, auto and cross
    assert cross or cpr % 2 == 0 or cpr == ntimes   # auto: whole pairs by default
    d = E.wvd_plan(nfft, nh, ng, hop, ntimes, rows=batch, cross=bool(cross))
    assert d == dict(cpr=cpr, workgroups=wgs, lds_bytes=lds, transforms=xf, fits=True)


def test_plan_refusals_and_what_does_not_fit():
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    assert lib.sp_wvd_plan(0, 256, 63, 9, 10, 7, 1, 256, None) < 0
    for bad in ((0, 100, 63, 9, 10, 7, 1, 100), (0, 256, 64, 9, 10, 7, 1, 256), (0, 256, 63, 257, 10, 7, 1, 256), (0, 256, 63, 9, 0, 7, 1, 256),
                (0, 256, 63, 9, 10, -1, 1, 256), (0, 256, 63, 9, 10, 7, 65536, 256), (0, 256, 63, 9, 10, 7, 1, 257)):
        assert lib.sp_wvd_plan(*bad, _ffi.ptr(out)) < 0
    assert lib.sp_wvd_plan(0, 256, 63, 9, 100000, 2, 1, 256, _ffi.ptr(out)) == 0
    assert out[0] == 1 and out[4] == 0 and out[2] == lds_formula(0, 256, 63, 9, 100000, 1, 2) > 160 * 1024     # one column, its pair staged


def test_environment_override(monkeypatch):
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    for forced, auto_cols in ((1, 2), (3, 4), (6, 6)):
        monkeypatch.setenv("SP_WVD_CPR", str(forced))
        for cross in (0, 1):
            assert lib.sp_wvd_plan(cross, 256, 127, 9, 7, 41, 1, 256, _ffi.ptr(out)) == 0
            assert out[0] == forced and out[1] == -(-41 // forced) and out[3] == (forced if cross else (forced + 1) // 2)
            assert out[2] == lds_formula(cross, 256, 127, 9, 7, forced, 41)
            assert out[2] == 16 * 272 * 8 + 8 * (((forced if cross else auto_cols) - 1) * 7 + 135)
    monkeypatch.setenv("SP_WVD_CPR", "1000")                     # never more than the row has
    assert lib.sp_wvd_plan(0, 256, 127, 9, 7, 41, 1, 256, _ffi.ptr(out)) == 0 and out[0] == 41 and out[1] == 1
    monkeypatch.setenv("SP_WVD_CPR", "40")                       # a forced number that does not fit is refused, not cut down
    assert lib.sp_wvd_plan(0, 256, 127, 9, 1000, 41, 1, 256, _ffi.ptr(out)) == 0 and out[0] == 40 and out[4] == 0
    rc, msg, W = _call(lib, hop=1000, ntimes=41)
    assert rc < 0 and msg.startswith("sp_wvd: ") and "LDS" in msg and np.all(W == SENT)
    with pytest.raises(E.WvdRefused, match="LDS"):
        E.wvd(np.ones(100, dtype=np.complex64), np.ones(63), np.ones(9), 1000, 0, 41, 256)
    monkeypatch.delenv("SP_WVD_CPR")
    assert lib.sp_wvd_plan(0, 256, 127, 9, 7, 41, 1, 256, _ffi.ptr(out)) == 0 and out[0] == 32 and out[1] == 2      # a whole round of 16 pairs


def _both(exc):
    return isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)


def test_engine_refusals_carry_both_types():
    x = np.ones(100, dtype=np.complex64)
    h, g = np.ones(63), np.ones(9)
    bad = [lambda: E.wvd(x, h, g, 1, 0, 10, 100), lambda: E.wvd(x, h, g, 1, 0, 10, 16384), lambda: E.wvd(x, np.ones(64), g, 1, 0, 10, 256),
           lambda: E.wvd(x, np.ones(257), g, 1, 0, 10, 256), lambda: E.wvd(x, h, np.ones(8), 1, 0, 10, 256),
           lambda: E.wvd(x, h, np.ones(257), 1, 0, 10, 256), lambda: E.wvd(x, h, g, 0, 0, 10, 256), lambda: E.wvd(x, h, g, 1, 0, -1, 256),
           lambda: E.wvd(x, h, g, 1, 0, 10, 256, nb=0), lambda: E.wvd(x, h, g, 1, 0, 10, 256, nb=257), lambda: E.wvd(x, h, g, 1, 0, 10, 256, b0=256),
           lambda: E.wvd(x, h, g, 1, 0, 10, 256, scale=float("nan")), lambda: E.wvd(x.real.copy(), h, g, 1, 0, 10, 256),
           lambda: E.wvd(x, None, g, 1, 0, 10, 256), lambda: E.wvd(x, h, g, 1, 0, 10, 256, y=x[:50]),
           lambda: E.wvd(x, h, g, 100000, 0, 2, 256), lambda: E.wvd_plan(256, 64, 9, 1, 10), lambda: E.wvd_plan(100, 63, 9, 1, 10)]
    for f in bad:
        with pytest.raises(E.WvdRefused) as exc:
            f()
        assert _both(exc)


def test_public_refusals_carry_both_types():
    x = np.ones(300)
    bad = [lambda: WG.spwvd(x, nfft=100), lambda: WG.spwvd(x, hop=0), lambda: WG.spwvd(x, window=("hamming", 64)),
           lambda: WG.spwvd(x, twindow=("hamming", 257)), lambda: WG.spwvd(x, analytic=False), lambda: WG.spwvd(x + 0j, analytic=True),
           lambda: WG.spwvd(x, boundary="even"), lambda: WG.spwvd(x, band=(0.3, 0.2)), lambda: WG.pwvd(x, window=np.ones(300)),
           lambda: WG.xwvd(x, None), lambda: WG.xwvd(x, x[:100]), lambda: WG.wvd(np.ones(9000)), lambda: WG.wvd(x, nfft=256),
           lambda: WG.wvd_plan(300, nfft=100)]
    for f in bad:
        with pytest.raises(WG.WvdRefused) as exc:
            f()
        assert _both(exc)
    with pytest.raises(WG.WvdRefused, match="pwvd"):
        WG.wvd(np.ones(8191))
    assert WG.WvdRefused is E.WvdRefused


def test_public_plan_and_axes_of_the_setup():
    d = WG.wvd_plan(1000, nfft=256, hop=7)
    assert d["nframes"] == 143 and d["first"] == 0 and d["b0"] == 0 and d["nb"] == 256 and d["fits"]
    d = WG.wvd_plan(1000, nfft=256, hop=7, band=(-0.05, 0.1), cplx=True)
    assert d["b0"] == 256 - 25 and d["nb"] == 25 + 51 + 1
    h, g = WG._windows("t", None, None, 256)
    assert h.size == 65 and g.size == 25 and h[32] == 1.0 and abs(np.sum(g) - 1) < 1e-15
    h, g = WG._windows("t", ("kaiser", 8.0, 31), np.array([1.0, 2.0, 1.0]), 256)
    assert h.size == 31 and np.array_equal(g, [1.0, 2.0, 1.0])


def test_exported_declared_and_bound():
    for name in ("spwvd", "pwvd", "wvd", "xwvd", "wvd_plan"):
        assert getattr(pyfft_amd, name) is getattr(WG, name)
    assert issubclass(E.WvdRefused, ValueError) and issubclass(E.WvdRefused, NotImplementedError)
    assert callable(E.wvd) and callable(E.wvd_plan)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_quad.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.QUAD_SIGNATURES) == {"sp_wvd", "sp_wvd_plan"}
    assert not set(_ffi.QUAD_SIGNATURES) & (set(_ffi.SIGNATURES) | set(_ffi.EXT_SIGNATURES) | set(_ffi.TFR_SIGNATURES))
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_wvd", 18), ("sp_wvd_plan", 9)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.QUAD_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.QUAD_SIGNATURES[name][1]
    for other in ("spectral.h", "spectral_ext.h", "spectral_tfr.h"):
        assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other)))
    assert "spectral_quad.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert "SP_WVD_CPR" in open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
