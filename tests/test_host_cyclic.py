"""Spectral correlation without a GPU: the numpy restatement of tests/cyclic_ref.py against scipy's Welch CSD of the shifted records and
against what the estimator is for (the coherence of amplitude-modulated noise, the significance level on white noise), its identities
(the mirrored form, additivity under `first`, a shift of the origin), the refusals of sp_cyclic, sp_cyclic_plan and their Python front
ends, the plan figures, the declared set of include/spectral_cyclo.h, and the measured float32 figure the GPU test's allowance rests on."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
import cyclic_ref as R
from pyfft_amd import _ffi, cyclic as CY, engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rowmax(a):
    return np.max(np.abs(a), axis=-1, keepdims=True)


def test_reference_is_scipy_csd_of_the_shifted_records():
    rng = np.random.default_rng(3)
    n, hop, nsig = 64, 16, 1000
    nframes = (nsig - n) // hop + 1
    w = R.hann(n)
    t = np.arange(nsig)
    worst = 0.0
    for cplx in (False, True):
        x = rng.standard_normal(nsig) + (1j * rng.standard_normal(nsig) if cplx else 0)
        y = rng.standard_normal(nsig) + (1j * rng.standard_normal(nsig) if cplx else 0)
        for nu in (0.0, 1 / 64, R.NU_AM, -0.3, 1.0):
            nq = R.nuh_units(nu) / 2.0 ** 64 * 2                   # the rounded nu: the shifts below use the same number
            S, Pp, Pm = R.cyclic_def(x, w, hop, nframes, [nu], y=y, scale=1.0 / nframes)
            _, ref = ss.csd(x * np.exp(1j * np.pi * nq * t), y * np.exp(-1j * np.pi * nq * t), window=w, noverlap=n - hop, detrend=False,
                            return_onesided=False, scaling="spectrum")
            ref = ref * np.sum(w) ** 2
            worst = max(worst, float(np.max(np.abs(S[0] - ref) / _rowmax(ref))))
            _, pp = ss.welch(y * np.exp(-1j * np.pi * nq * t), window=w, noverlap=n - hop, detrend=False, return_onesided=False, scaling="spectrum")
            worst = max(worst, float(np.max(np.abs(Pp[0] - pp * np.sum(w) ** 2) / _rowmax(pp * np.sum(w) ** 2))))
    print("reference against scipy.signal.csd: %.2e of the row maximum" % worst)
    assert worst <= 1e-12


def test_mirrored_identity():
    rng = np.random.default_rng(4)
    n, hop, nframes = 64, 16, 20
    w = R.hann(n)
    for x, conj in ((rng.standard_normal(400), False), (rng.standard_normal(400) + 1j * rng.standard_normal(400), True)):
        m = np.mean(x)
        S, Pp, Pm = R.cyclic_def(x, w, hop, nframes, [R.NU_AM, -0.3], conj=conj, first=12345, mx=m)
        idx = 12345 + np.arange(nframes)[:, None] * hop + np.arange(n)[None, :]
        fr = x[np.arange(nframes)[:, None] * hop + np.arange(n)[None, :]] - m
        for a, nu in enumerate((R.NU_AM, -0.3)):
            Zp = np.fft.fft(w * fr * np.conj(R.e(R.turn(R.nuh_units(nu), idx))), axis=-1)
            mir = Zp[:, (n - np.arange(n)) % n]
            assert np.max(np.abs(S[a] - np.sum(Zp * mir, axis=0))) <= 1e-13 * np.max(np.abs(S[a]))
            assert np.max(np.abs(Pm[a] - Pp[a][(n - np.arange(n)) % n])) <= 1e-13 * np.max(Pp[a])


def test_additive_under_first_across_a_cut_at_a_frame_start():
    rng = np.random.default_rng(5)
    n, hop, nframes, cut = 64, 16, 30, 17
    x = rng.standard_normal((nframes - 1) * hop + n) + 1j * rng.standard_normal((nframes - 1) * hop + n)
    w, nu, first = R.hann(n), [0.0, R.NU_AM, -0.41, 1.0], (1 << 40) + 3
    whole = R.cyclic_def(x, w, hop, nframes, nu, first=first, mx=0.1 - 0.2j)
    a = R.cyclic_def(x[:(cut - 1) * hop + n], w, hop, cut, nu, first=first, mx=0.1 - 0.2j)
    b = R.cyclic_def(x[cut * hop:], w, hop, nframes - cut, nu, first=first + cut * hop, mx=0.1 - 0.2j)
    wrong = R.cyclic_def(x[cut * hop:], w, hop, nframes - cut, nu, first=first, mx=0.1 - 0.2j)
    for i in range(3):
        assert np.max(np.abs(a[i] + b[i] - whole[i]) / _rowmax(whole[i])) <= 1e-12
    assert np.max(np.abs(a[0] + wrong[0] - whole[0]) / _rowmax(whole[0])) > 1e-2       # the local index would not add up


def test_origin_shift_rotates_S_by_python_integer_phases():
    rng = np.random.default_rng(6)
    n, hop, nframes = 64, 16, 12
    x = rng.standard_normal((nframes - 1) * hop + n)
    w, nus, d = R.hann(n), [R.NU_AM, -0.3, 1 / 64, 0.999], (1 << 40) + 3
    S0, P0, _ = R.cyclic_def(x, w, hop, nframes, nus, first=0)
    S1, P1, _ = R.cyclic_def(x, w, hop, nframes, nus, first=d)
    for a, nu in enumerate(nus):
        frac = ((2 * R.nuh_units(nu) * d) % (1 << 64)) / float(1 << 64)              # Python integers: exact
        rot = np.exp(-2j * np.pi * frac)
        assert np.max(np.abs(S1[a] - rot * S0[a])) <= 1e-9 * np.max(np.abs(S0[a]))
        assert np.max(np.abs(P1[a] - P0[a])) <= 1e-12 * np.max(P0[a])
    assert R.nuh_units(1.0) == R.nuh_units(-1.0) == 1 << 63 and R.nuh_units(0.5) == 1 << 62 and R.nuh_units(-0.5) == 3 << 62


def test_float32_restatement_deviation():
    """the figure the GPU allowance rests on: cyclic_def32 against cyclic_def over the GPU test's shapes and forms"""
    worst = 0.0
    for name, form in R.CASES:
        dev = R.deviation(R.reference32(name, form), R.reference(name, form))
        print("  %-26s %-6s %.3e" % (name, form, dev))
        worst = max(worst, dev)
    print("float32 restatement: %.3e; recorded %.3e; allowance %.3e" % (worst, R.F32_DEV, R.ALLOWANCE))
    assert 0.5 * R.F32_DEV <= worst <= R.F32_DEV
    assert R.ALLOWANCE == R.MARGIN * R.F32_DEV and R.MARGIN == 4.0 and R.ALLOWANCE <= R.PARITY == 2e-4


def test_coherence_of_amplitude_modulated_noise():
    S, Pp, Pm = R.level_reference(1)
    g = np.abs(R.coherence(S[0], Pp[0], Pm[0]))
    print("mean |gamma| at the modulation rate: %.4f (theory %.4f)" % (g.mean(), R.GAMMA_AM))
    assert abs(R.GAMMA_AM - 0.606) < 5e-4 and abs(g.mean() - 0.606) <= 0.03


def test_cyclic_level_on_white_noise():
    w = R.hann(R.LEVEL_N)
    ke = CY.effective_segments(R.LEVEL_FRAMES, w, R.LEVEL_HOP)
    assert R.LEVEL_FRAMES == 509 and abs(ke - 264.7) <= 0.1, ke
    lvl = CY.cyclic_level(R.LEVEL_FRAMES, w, R.LEVEL_HOP, 0.05)
    assert lvl == pytest.approx(1 - 0.05 ** (1 / (ke - 1)), rel=1e-12)
    S, Pp, Pm = R.level_reference(0)
    g2 = np.abs(R.coherence(S, Pp, Pm)) ** 2
    share, naive = float(np.mean(g2 > lvl)), float(np.mean(g2 > pyfft_amd.coherence_level(R.LEVEL_FRAMES, 0.05)))
    print("K_eff %.2f, level %.5f, share above it %.4f (uncorrected level: %.4f)" % (ke, lvl, share, naive))
    assert 0.03 <= share <= 0.08
    assert naive > 0.15                                   # what the correction is for
    assert CY.cyclic_level(1, w, R.LEVEL_HOP) == 1.0 and CY.effective_segments(7, w, R.LEVEL_N) == 7.0
    with pytest.raises(CY.CyclicRefused):
        CY.cyclic_level(10, w, 64, p=1.0)


def test_alpha_grid_and_profile():
    a = CY.alpha_grid(1000, 2000.0, 10.0)
    assert a[0] == 0 and np.allclose(np.diff(a), 2.0) and a[-1] == 10.0 and a.size == 6
    assert CY.alpha_grid(1000, 2000.0, 10.0, oversample=2).size == 11
    g = np.array([[[1j, 0.5, 0.0, 1.0]], [[0.0, 0.0, 2.0, 0.0]]])
    assert np.allclose(CY.cyclic_profile(g), [[(1 + 0.25 + 1) / 4], [1.0]])
    assert np.allclose(CY.cyclic_profile(g, band=(1, 3)), [[0.125], [2.0]])


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.CYCLO_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.CYCLO_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


GOOD = dict(x=True, y=False, x_dtype=0, y_dtype=0, x_ld=500, nsig=500, batch=2, w=True, n=64, hop=16, nframes=20, first=-5, nu=(0.0, 0.1),
            nu_ptr=True, A=2, conj=0, mean=(0.0, 0.0), b0=0, nb=64, scale=1.0, S=True, Pp=True, Pm=True)
SENT = np.float32(-12345.0)


def _call(lib, **over):
    p = dict(GOOD, **over)
    x = np.ones(2000, dtype=np.float32)
    y = np.ones(2000, dtype=np.float32)
    w = np.ones(8192, dtype=np.float32)
    nu = np.array(list(p["nu"]) + [0.0] * 8, dtype=np.float64)
    mean = np.array(list(p["mean"]) * 4, dtype=np.float64)
    outs = [np.full(8192, SENT, dtype=np.float32) for _ in range(3)]
    rc = lib.sp_cyclic(_ffi.ptr(x) if p["x"] else None, _ffi.ptr(y) if p["y"] else None, p["x_dtype"], p["y_dtype"], p["x_ld"], p["nsig"],
                       p["batch"], _ffi.ptr(w) if p["w"] else None, p["n"], p["hop"], p["nframes"], p["first"],
                       _ffi.ptr(nu) if p["nu_ptr"] else None, p["A"], p["conj"], _ffi.ptr(mean), _ffi.ptr(mean),
                       p["b0"], p["nb"], p["scale"], *[_ffi.ptr(o) if p[k] else None for o, k in zip(outs, ("S", "Pp", "Pm"))], 0)
    return rc, (lib.sp_last_error() or b"").decode(), outs


REFUSALS = [
    (dict(n=16), "n must"), (dict(n=16384), "n must"), (dict(n=100), "n must"), (dict(hop=0), "hop"), (dict(nframes=-1), "nframes"),
    (dict(nframes=29), "frames"), (dict(n=1024, nb=64), "frames"), (dict(hop=1 << 40, nframes=2), "frames"),
    (dict(A=0), "A must"), (dict(A=65536), "A must"), (dict(batch=-1), "batch"), (dict(batch=65536), "batch"),
    (dict(nu=(0.0, float("nan"))), "nu[1]"), (dict(nu=(float("inf"), 0.0)), "nu[0]"), (dict(nu=(0.0, 1.0000001)), "nu[1]"),
    (dict(nu=(-1.5, 0.0)), "nu[0]"), (dict(x_dtype=2), "x_dtype"), (dict(y=True, y_dtype=1), "y_dtype"),
    (dict(nb=0), "band"), (dict(nb=65), "band"), (dict(b0=-1), "band"), (dict(b0=64), "band"),
    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"), (dict(mean=(float("nan"), 0.0)), "mean"),
    (dict(nsig=0), "nsig"), (dict(x_ld=499), "x_ld"), (dict(first=(1 << 62) + 1), "first"),
    (dict(x=False), "x is"), (dict(w=False), "w is"), (dict(nu_ptr=False), "nu is"), (dict(S=False, Pp=False, Pm=False), "no output"),
]


@pytest.mark.parametrize("over,word", REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(REFUSALS)])
def test_c_refusals(over, word):
    rc, msg, outs = _call(_c_entry(), **over)
    assert rc < 0 and msg.startswith("sp_cyclic: ") and word in msg, (rc, msg)
    assert all(np.all(o == SENT) for o in outs)


def test_nothing_to_do():
    lib = _c_entry()
    for over in (dict(batch=0), dict(nframes=0)):
        rc, _, outs = _call(lib, **over)
        assert rc == 0 and all(np.all(o == SENT) for o in outs)


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_plan_of_every_shape(name, monkeypatch):
    monkeypatch.delenv("SP_CYCLIC_CHUNK", raising=False)
    monkeypatch.delenv("SP_CYCLIC_FPG", raising=False)
    s = R.SHAPES[name]
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    for form in s["forms"]:
        cross, conj = R.form_args(form)
        mirror = not cross and (not s["cplx"] or conj)
        A = len(s["nu"])
        assert lib.sp_cyclic_plan(1 if s["cplx"] else 0, int(cross), int(conj), s["n"], s["hop"], s["nframes"], A, s["rows"], _ffi.ptr(out)) == 0
        fpg, wgs, apass, passes, xf = (int(v) for v in out)
        # before the library is initialised the plan counts 256 CUs: about 4 x 256 workgroups over (alpha, rows, blocks)
        want_blocks = -(-4 * 256 // (A * s["rows"]))
        groups_per_block = 256 // max(s["n"] // 16, 1) if s["n"] < 4096 else 1
        assert fpg == max(1, -(-s["nframes"] // (want_blocks * groups_per_block)))
        blocks = -(-(-(-s["nframes"] // fpg)) // groups_per_block)
        assert wgs == blocks * A * s["rows"] and apass == A and passes == 1 and xf == (1 if mirror else 2)
        d = E.cyclic_plan(s["n"], s["hop"], s["nframes"], A, rows=s["rows"], cplx=s["cplx"], cross=cross, conj=conj)
        assert d == dict(fpg=fpg, workgroups=wgs, alpha_per_pass=apass, passes=passes, transforms=xf)
    if name == "n64-many-alpha":
        monkeypatch.setenv("SP_CYCLIC_CHUNK", str(R.MANY_ALPHA_CHUNK))
        assert lib.sp_cyclic_plan(0, 0, 0, s["n"], s["hop"], s["nframes"], 300, 1, _ffi.ptr(out)) == 0
        assert out[2] == 128 and out[3] == 3
        monkeypatch.setenv("SP_CYCLIC_CHUNK", "0")
        assert lib.sp_cyclic_plan(0, 0, 0, s["n"], s["hop"], s["nframes"], 300, 1, _ffi.ptr(out)) == 0 and out[3] == 1


def test_frames_per_group_hook_and_the_shape_that_needs_none(monkeypatch):
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    monkeypatch.delenv("SP_CYCLIC_FPG", raising=False)
    s = R.SHAPES["n4096-runs-of-three"]
    assert lib.sp_cyclic_plan(0, 0, 0, s["n"], s["hop"], s["nframes"], len(s["nu"]), 1, _ffi.ptr(out)) == 0
    assert out[0] == 3 and out[1] == 2 * 600                    # two groups: three frames, then two and a clamped one
    for name, fpg in R.FPG.items():
        s = R.SHAPES[name]
        assert fpg > 1 and s["nframes"] % fpg and s["nframes"] > fpg, name          # a loop, and a last group that is not full
        monkeypatch.setenv("SP_CYCLIC_FPG", str(fpg))
        assert lib.sp_cyclic_plan(int(s["cplx"]), 0, 0, s["n"], s["hop"], s["nframes"], len(s["nu"]), s["rows"], _ffi.ptr(out)) == 0
        groups_per_block = 256 // max(s["n"] // 16, 1) if s["n"] < 4096 else 1
        assert out[0] == fpg and out[1] == -(-(-(-s["nframes"] // fpg)) // groups_per_block) * len(s["nu"]) * s["rows"]
    monkeypatch.setenv("SP_CYCLIC_FPG", "0")
    assert lib.sp_cyclic_plan(0, 0, 0, 32, 8, 37, 5, 1, _ffi.ptr(out)) == 0 and out[0] == 1


def test_no_frames_give_zeros_without_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    S, Pp, Pm = E.cyclic(np.ones((2, 100), dtype=np.float32), np.ones(64), 16, 0, [0.1, 0.2], nb=5, Pm=False)
    assert S.shape == (2, 2, 5) and S.dtype == np.complex64 and Pp.dtype == np.float32 and Pm is None
    assert not S.any() and not Pp.any()


def test_plan_refusals_and_the_partials_budget():
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    assert lib.sp_cyclic_plan(0, 0, 0, 256, 64, 100, 4, 1, None) < 0
    for bad in ((2, 0, 0, 256, 64, 100, 4, 1), (0, 0, 0, 100, 64, 100, 4, 1), (0, 0, 0, 256, 0, 100, 4, 1), (0, 0, 0, 256, 64, -1, 4, 1),
                (0, 0, 0, 256, 64, 100, 0, 1), (0, 0, 0, 256, 64, 100, 65536, 1), (0, 0, 0, 256, 64, 100, 4, 65536)):
        assert lib.sp_cyclic_plan(*bad, _ffi.ptr(out)) < 0
    # 65535 cycle frequencies at 8192 points: one group each, 3 planes of 8192 floats = 96 KiB a cell, 2730 cells in 256 MiB
    assert lib.sp_cyclic_plan(0, 0, 0, 8192, 64, 1000, 65535, 1, _ffi.ptr(out)) == 0
    assert out[0] == 1000 and out[2] == 2730 and out[3] == -(-65535 // 2730) and out[4] == 1
    # the plain form of a complex row at 8192 points keeps its window table in memory: 4 planes + 2 = 192 KiB a cell
    assert lib.sp_cyclic_plan(1, 0, 0, 8192, 64, 1000, 65535, 1, _ffi.ptr(out)) == 0 and out[2] == 1365 and out[4] == 2


def _both(exc):
    return isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    x, w = np.ones(1000, dtype=np.float32), np.ones(64)
    bad = [lambda: E.cyclic(x, np.ones(100), 16, 10, [0.1]), lambda: E.cyclic(x, np.ones(16), 16, 10, [0.1]),
           lambda: E.cyclic(x, w, 0, 10, [0.1]), lambda: E.cyclic(x, w, 16, -1, [0.1]), lambda: E.cyclic(x, w, 16, 60, [0.1]),
           lambda: E.cyclic(x, w, 16, 10, []), lambda: E.cyclic(x, w, 16, 10, [1.5]), lambda: E.cyclic(x, w, 16, 10, [float("nan")]),
           lambda: E.cyclic(x, w, 16, 10, [0.1], nb=65), lambda: E.cyclic(x, w, 16, 10, [0.1], b0=64),
           lambda: E.cyclic(x, w, 16, 10, [0.1], scale=float("inf")), lambda: E.cyclic(x, w, 16, 10, [0.1], S=False, Pp=False, Pm=False),
           lambda: E.cyclic(x, w, 16, 10, [0.1], y=x.astype(np.complex64)), lambda: E.cyclic(x, w, 16, 10, [0.1], y=x[:500]),
           lambda: E.cyclic(x, w, 16, 10, [0.1], first=1 << 63), lambda: E.cyclic(x, np.full(64, np.nan), 16, 10, [0.1]),
           lambda: E.cyclic_plan(100, 16, 10, 4), lambda: E.cyclic_plan(64, 16, 10, 0),
           lambda: CY.scd(x, [0.1], nperseg=100), lambda: CY.scd(x, [0.1], nperseg=16384), lambda: CY.scd(x, [0.1], noverlap=256),
           lambda: CY.scd(x, [0.1], detrend="linear"), lambda: CY.scd(x, [0.1], scaling="psd"), lambda: CY.scd(x, [3.0], fs=2.0),
           lambda: CY.scd(x[:100], [0.1]), lambda: CY.scd(x, [0.1], fs=0.0), lambda: CY.scd(x, [0.1], window=np.ones(10)),
           lambda: CY.cyclic_coherence(x, []), lambda: CY.cyclic_spectra(x, [0.1], nperseg=48), lambda: CY.cyclic_plan(100, [0.1]),
           lambda: CY.alpha_grid(0, 1.0, 1.0)]
    for f in bad:
        with pytest.raises(E.CyclicRefused) as exc:
            f()
        assert _both(exc)
    assert CY.CyclicRefused is E.CyclicRefused


def test_public_plan():
    d = CY.cyclic_plan(1 << 15, np.arange(8) * 0.01, nperseg=256)
    assert d["nframes"] == 509 and d["hop"] == 64 and d["transforms"] == 1 and d["passes"] == 1
    assert CY.cyclic_plan(1 << 15, [0.1], nperseg=256, cplx=True)["transforms"] == 2
    assert CY.cyclic_plan(1 << 15, [0.1], nperseg=256, cplx=True, conjugate=True)["transforms"] == 1


def test_exported_declared_and_bound():
    for name in ("scd", "cyclic_coherence", "cyclic_spectra", "cyclic_profile", "alpha_grid", "cyclic_level", "cyclic_plan"):
        assert getattr(pyfft_amd, name) is getattr(CY, name)
    assert issubclass(E.CyclicRefused, ValueError) and issubclass(E.CyclicRefused, NotImplementedError)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_cyclo.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.CYCLO_SIGNATURES) == {"sp_cyclic", "sp_cyclic_plan"}
    others = set(_ffi.SIGNATURES) | set(_ffi.EXT_SIGNATURES) | set(_ffi.TFR_SIGNATURES) | set(_ffi.QUAD_SIGNATURES)
    assert not set(_ffi.CYCLO_SIGNATURES) & others
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_cyclic", 24), ("sp_cyclic_plan", 9)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.CYCLO_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.CYCLO_SIGNATURES[name][1]
    for other in ("spectral.h", "spectral_ext.h", "spectral_tfr.h", "spectral_quad.h"):
        assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other)))
    assert "spectral_cyclo.h" in open(os.path.join(ROOT, "Makefile")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "SP_CYCLIC_CHUNK" in launch and "SP_CYCLIC_FPG" in launch
