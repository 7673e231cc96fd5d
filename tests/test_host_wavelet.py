"""Host side of the continuous wavelet transform (pyfft_amd.wavelet, engine.cwt, sp_cwt): the float64 reference of tests/cwt_ref.py
against a direct time-domain convolution and against itself on a longer grid, the margin rule, the float64 restatement of the
overlap-save plan, the plan arithmetic, every refusal of the C entry before the device is touched and of the Python side before the
library loads, the exports, and the host quantities (Fourier period, cone of influence, C_delta, the reconstruction weights).
No GPU needed.  tests/test_gpu_wavelet.py takes the reference from here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import pyfft_amd
from pyfft_amd import _ffi, engine as E, wavelet as WV
from test_host_multitaper import no_library        # noqa: F401  (a fixture)
import cwt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M6, P4 = WV.Morlet(6.0), WV.Paul(4)


@pytest.mark.parametrize("family,param", [("morlet", 6.0), ("paul", 4.0)])
def test_reference_is_a_linear_convolution(family, param):
    """cwt_ref against the direct O(N K) sum W[s, n] = sum_m g_s[m] x[n - m], g_s from a grid long enough that it does not wrap."""
    n, grid = 300, 1 << 15
    x = R.make_signal(n, True, 1).astype(np.complex128)
    scales = np.array([4.0, 5.5, 9.0, 17.0]) if family == "morlet" else np.array([8.5, 12.0, 20.0])
    W = R.cwt_ref(x, scales, family, param, n_full=grid)
    for j, s in enumerate(scales):
        g = R.kernel_time(family, param, s, grid)
        direct = np.array([sum(g[(i - m) % grid] * x[m] for m in range(n)) for i in range(n)])
        err = np.max(np.abs(direct - W[j])) / np.sqrt(np.mean(np.abs(W[j]) ** 2))
        assert err <= 1e-10, (s, err)


def test_reference_against_itself_on_twice_the_grid():
    """1e-9 of the row rms, as the rms of the difference.  Its largest entry (printed) sits at the first sample of the record and is of
    the order of the step the Heaviside cut leaves in a Morlet filter at w = 0, exp(-w0^2 / 2) = 1.5e-8 of its peak: g_s has 1 / n
    tails of that size, and the two grids fold them differently (1.2e-9 with make_signal's two slowest lines in the record)."""
    n = 3000
    x = R.make_signal(n, False, 2, slow=False)          # (the folded tails weigh the record's sum: without the lines slower than the record)
    scales = 4.0 * 2 ** (np.arange(24) / 4.0)
    assert all(WV.margin(M6, s) <= WV.FUSED_MAX_MARGIN for s in scales)
    a, b = R.cwt_ref(x, scales), R.cwt_ref(x, scales, n_full=2 * R.next_pow2(2 * n))
    rms = np.sqrt(np.mean(np.abs(b) ** 2, axis=-1))
    err = float(np.max(np.sqrt(np.mean(np.abs(a - b) ** 2, axis=-1)) / rms))
    print("cwt_ref against twice the grid: rms %.3g, largest entry %.3g of the row rms" % (err, R.row_err(a, b)))
    assert err <= 1e-9 and R.row_err(a, b) <= 1e-9


def test_margin_rule():
    s = np.concatenate([[3.7, 3.8, 4.0], 4.0 * 2 ** (np.arange(1, 30) / 4.0)])
    m = np.array([WV.margin(M6, v) for v in s])
    assert np.all(np.diff(m) >= 0), m
    big = s >= 8                                            # (whole samples: 19 at 3.7 is 5.1 s', the ratio settles with the scale)
    assert np.all(m[big] >= 4.5 * s[big]) and np.all(m[big] <= 5.5 * s[big]), m / s
    assert np.all(m <= 5.5 * s + 1) and np.all(m >= 4.5 * s)
    for v in (2.0, 3.0, 3.5):
        assert WV.margin(M6, v) > WV.FUSED_MAX_MARGIN
    assert WV.margin(M6, 3.5) == R.margin_ref("morlet", 6.0, 3.5) and WV.margin(M6, 50.0) == R.margin_ref("morlet", 6.0, 50.0)
    assert WV.margin(P4, 20.0) == R.margin_ref("paul", 4.0, 20.0)
    # Paul-4 against Morlet-6 at equal Fourier period
    for period in (20.0, 60.0, 150.0):
        assert WV.margin(P4, period / P4.flambda()) > WV.margin(M6, period / M6.flambda())
    plan = WV.cwt_plan(10000, scales=[2.0, 3.5, 3.7, 10.0, 600.0, 700.0])
    assert list(plan["path"]) == ["composed", "composed", "fused", "fused", "fused", "composed"]
    assert 3.5 < WV.smallest_fused_scale(M6) <= 3.8
    assert WV.cwt_scales(1000, 0.5, wavelet=M6)[0] == WV.smallest_fused_scale(M6) * 0.5


def test_overlap_save_restatement():
    """The plan in float64 against cwt_ref: what is lost is what lies beyond the margins."""
    n, tail = 20000, 1e-6
    scales = 4.0 * 2 ** (np.arange(40) / 8.0)
    plan = WV.cwt_plan(n, scales=scales, tail=tail)
    assert (plan["L"], plan["M"], plan["hop"], plan["frames"]) == (4096, 576, 2944, 7) and plan["fused"].all()
    x = R.make_signal(n, False, 3)
    err = R.row_err(R.overlap_save(x, scales, "morlet", 6.0, plan["L"], plan["M"]), R.cwt_ref(x, scales))
    print("float64 overlap-save against cwt_ref: %.3g (tail %g)" % (err, tail))
    assert err <= 4 * tail


# (nsig, nscales, rows, L, M, outputs) -> (hop, frames)
PLANS = [
    ((100, 5, 1, 256, 61, 1), (134, 1)),                 # N < hop
    ((134 * 3, 5, 1, 256, 61, 1), (134, 3)),             # N = k hop exactly
    ((134 * 3 + 1, 5, 1, 256, 61, 1), (134, 4)),         # a one-sample remainder
    ((5477, 30, 1, 8192, 2736, 1), (2720, 3)),
    ((5477, 30, 2, 8192, 2736, 6), (2720, 3)),
    ((1 << 20, 88, 1, 8192, 3072, 1), (2048, 512)),
    ((1 << 20, 88, 1, 8192, 3072, 12), (2048, 512)),
    ((1 << 20, 24, 1, 1024, 243, 3), (538, 1950)),
    ((777, 7, 3, 512, 0, 15), (512, 2)),
]


@pytest.mark.parametrize("shape,want", PLANS, ids=[str(p[0]) for p in PLANS])
def test_plan_arithmetic(shape, want):
    nsig, S, rows, L, M, outputs = shape
    p = E.cwt_plan(nsig, S, L, M, rows=rows, W=bool(outputs & 1), gws=bool(outputs & 2), recon=bool(outputs & 4),
                   bandpow=bool(outputs & 8))
    hop, frames = want
    assert (p["hop"], p["frames"]) == (hop, frames) and hop == L - 2 * M and frames == -(-nsig // hop)
    assert (frames - 1) * hop < nsig <= frames * hop
    fpw = max(1, 4096 // L)
    bx = -(-frames // fpw)
    if outputs & 12:
        assert p["chunk"] == S                               # recon and bandpow need every scale of a frame in one workgroup
    assert 1 <= p["chunk"] <= S
    nchunks = -(-S // p["chunk"])
    assert p["workgroups"] == bx * nchunks * rows
    if not outputs & 12 and bx * rows < 1024 and S > 1:
        assert nchunks > 1                                   # short records: the scales fill the CUs
    if nsig == 1 << 20 and not outputs & 12:
        assert p["workgroups"] >= 256
    assert p["scratch"] == (4 * rows * S * frames if outputs & 2 else 0)


def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("sp_cwt", "sp_cwt_plan", "sp_icwt"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


GOOD = dict(dtype=0, nsig=1000, x_ld=1000, batch=2, nscales=4, family=0, p0=6.0, p1=0.0, L=256, M=61)
C_REFUSALS = [
    (dict(L=300), "L must"), (dict(L=128), "L must"), (dict(L=16384), "L must"), (dict(L=0), "L must"),
    (dict(M=128), "M must"), (dict(M=-1), "M must"), (dict(M=200), "M must"), (dict(M=97), "M leaves hop"),
    (dict(nscales=0), "nscales"), (dict(nscales=-2), "nscales"),
    (dict(scales=[4.0, 0.0, 5.0, 6.0]), "scales[1]"), (dict(scales=[4.0, 5.0, -1.0, 6.0]), "scales[2]"),
    (dict(scales=[4.0, 5.0, 6.0, float("nan")]), "scales[3]"), (dict(scales=[float("inf"), 5.0, 6.0, 7.0]), "scales[0]"),
    (dict(scales=None), "scales is required"),
    (dict(nsig=0), "nsig"), (dict(batch=-1), "batch"), (dict(batch=70000), "batch"), (dict(x_ld=999), "x_ld"),
    (dict(dtype=5), "dtype"), (dict(family=2), "family"), (dict(p0=0.0), "parameter"), (dict(p0=float("nan")), "parameter"),
    (dict(family=1, p0=0.5), "parameter"), (dict(p1=1.0), "parameter"),
    (dict(outputs=()), "an output is required"), (dict(wrec=None), "wrec"), (dict(wband=None), "wband"),
    (dict(wrec=[1.0, float("nan"), 1.0, 1.0]), "weights"), (dict(x=None), "x is required"),
]


@pytest.mark.parametrize("kw,name", C_REFUSALS, ids=["%s-%d" % (n.split()[0], i) for i, (_, n) in enumerate(C_REFUSALS)])
def test_c_entry_refuses_before_the_device(kw, name):
    """< 0, the message names sp_cwt and the argument, the outputs are untouched."""
    lib = _c_entry()
    a = dict(GOOD)
    a.update({k: v for k, v in kw.items() if k in GOOD})
    x = np.ones((2, 1000), dtype=np.float32)
    scales = kw.get("scales", [4.0, 5.0, 6.0, 7.0])
    sc = None if scales is None else np.array(scales, dtype=np.float64)
    wrec = kw.get("wrec", [1.0, 1.0, 1.0, 1.0])
    wband = kw.get("wband", [1.0, 1.0, 1.0, 1.0])
    wr = None if wrec is None else np.array(wrec, dtype=np.float32)
    wb = None if wband is None else np.array(wband, dtype=np.float32)
    bufs = dict(W=np.full((2, 4, 1000), 7.0 + 7.0j, np.complex64), gws=np.full((2, 4), 7.0), recon=np.full((2, 1000), 7.0 + 7.0j, np.complex64),
                bandpow=np.full((2, 1000), 7.0, np.float32))
    outs = kw.get("outputs", ("W", "gws", "recon", "bandpow"))
    ptrs = {k: (_ffi.ptr(v) if k in outs else None) for k, v in bufs.items()}
    xp = None if ("x" in kw and kw["x"] is None) else _ffi.ptr(x)
    rc = lib.sp_cwt(xp, a["dtype"], a["nsig"], a["x_ld"], a["batch"], _ffi.ptr(sc), a["nscales"], a["family"], a["p0"], a["p1"], a["L"],
                    a["M"], _ffi.ptr(wr), _ffi.ptr(wb), ptrs["W"], ptrs["gws"], ptrs["recon"], ptrs["bandpow"], 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc < 0, msg
    assert msg.startswith("sp_cwt: " + name), msg
    assert np.all(bufs["W"] == 7.0 + 7.0j) and np.all(bufs["gws"] == 7.0) and np.all(bufs["recon"] == 7.0 + 7.0j)
    assert np.all(bufs["bandpow"] == 7.0)


def test_c_plan_and_icwt_refuse():
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    assert lib.sp_cwt_plan(1000, 4, 1, 256, 61, 1, out.ctypes.data) == 0 and (out[0], out[1]) == (134, 8)
    for bad in ((1000, 4, 1, 300, 61, 1), (1000, 4, 1, 256, 128, 1), (1000, 4, 1, 256, 97, 1), (1000, 0, 1, 256, 61, 1),
                (0, 4, 1, 256, 61, 1), (1000, 4, -1, 256, 61, 1), (1000, 4, 1, 256, 61, 0), (1000, 4, 1, 256, 61, 16),
                (1000, 4, 1, 16384, 61, 1)):
        assert lib.sp_cwt_plan(*bad, out.ctypes.data) < 0, bad
    assert lib.sp_cwt_plan(1000, 4, 1, 256, 61, 1, None) < 0
    W = np.zeros((4, 100), dtype=np.complex64)
    y = np.full(100, 7.0 + 7.0j, np.complex64)
    w = np.ones(4, dtype=np.float32)
    for args, text in (((_ffi.ptr(W), 100, 0, 1, _ffi.ptr(w), _ffi.ptr(y), 0), "nscales"), ((_ffi.ptr(W), 0, 4, 1, _ffi.ptr(w), _ffi.ptr(y), 0), "nsig"),
                       ((_ffi.ptr(W), 100, 4, -1, _ffi.ptr(w), _ffi.ptr(y), 0), "batch"), ((_ffi.ptr(W), 100, 4, 1, None, _ffi.ptr(y), 0), "w is"),
                       ((None, 100, 4, 1, _ffi.ptr(w), _ffi.ptr(y), 0), "W and out"),
                       ((_ffi.ptr(W), 100, 4, 1, _ffi.ptr(np.array([1, np.inf, 1, 1], np.float32)), _ffi.ptr(y), 0), "weights")):
        assert lib.sp_icwt(*args) < 0
        assert (lib.sp_last_error() or b"").decode().startswith("sp_icwt: " + text)
    assert np.all(y == 7.0 + 7.0j)


def test_engine_refusals_carry_both_types(no_library):
    x = np.zeros(1000, dtype=np.float32)
    sc = [4.0, 5.0]
    for args, kw, text in (((x, sc, "morlet", 6.0, 300, 61), {}, "power of two"), ((x, sc, "morlet", 6.0, 128, 10), {}, "power of two"),
                           ((x, sc, "morlet", 6.0, 16384, 61), {}, "power of two"), ((x, sc, "morlet", 6.0, 256, 128), {}, "M = 128"),
                           ((x, sc, "morlet", 6.0, 256, 97), {}, "below L / 4"), ((x, [], "morlet", 6.0, 256, 61), {}, "at least one scale"),
                           ((x, [4.0, -1.0], "morlet", 6.0, 256, 61), {}, "positive and finite"),
                           ((x, [4.0, np.nan], "morlet", 6.0, 256, 61), {}, "positive and finite"),
                           ((x, sc, "dog", 2.0, 256, 61), {}, "not built"), ((x, sc, "paul", 0.5, 256, 61), {}, "parameter"),
                           ((x, sc, "morlet", 6.0, 256, 61), dict(W=False), "an output is required"),
                           ((x, sc, "morlet", 6.0, 256, 61), dict(recon=[1.0]), "one finite weight per scale"),
                           ((x, sc, "morlet", 6.0, 256, 61), dict(bandpow=[1.0, np.inf]), "one finite weight per scale"),
                           ((np.zeros((0, 5), np.float32), sc, "morlet", 6.0, 256, 61), {}, "rows")):
        with pytest.raises(NotImplementedError) as ei:
            E.cwt(*args, **kw)
        assert isinstance(ei.value, ValueError) and isinstance(ei.value, E.CwtRefused) and text in str(ei.value), str(ei.value)
    for args, text in (((np.zeros((2, 10), np.complex64), [1.0]), "one finite weight"), ((np.zeros(10, np.complex64), [1.0]), "[..., S, N]"),
                       ((np.zeros((2, 10), np.complex64), None), "weights are required")):
        with pytest.raises(NotImplementedError) as ei:
            E.icwt_sum(*args)
        assert isinstance(ei.value, ValueError) and text in str(ei.value)


def test_public_refusals_carry_both_types(no_library):
    x = np.zeros(1000)
    for call, text in ((lambda: WV.cwt(x, wavelet="dog"), "not built"), (lambda: WV.cwt(x, scales=[-1.0]), "positive"),
                       (lambda: WV.cwt_filter(x, scales=[4.0, 8.0], band=(100.0, 200.0)), "no scale lies in the band"),
                       (lambda: WV.cwt_power(x, scales=[4.0, 8.0], band=(0.1, 0.2)), "no scale lies in the band"),
                       (lambda: WV.Morlet(0.0), "w0"), (lambda: WV.Paul(0.5), "m ="),
                       (lambda: WV.cwt_plan((1 << 25) + 1, scales=[2.0, 8.0]), "resample_poly"),
                       (lambda: WV.cwt_plan(0, scales=[8.0]), "at least one sample")):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert isinstance(ei.value, ValueError) and isinstance(ei.value, WV.CwtRefused) and text in str(ei.value), str(ei.value)
    # the long record is taken as long as every scale fuses
    assert WV.cwt_plan((1 << 25) + 1, scales=[8.0, 16.0])["n_full"] is None


def test_exported():
    for name in ("Morlet", "Paul", "cwt_scales", "cwt", "icwt", "cwt_power", "cwt_filter", "cwt_plan"):
        assert getattr(pyfft_amd, name) is getattr(WV, name)
    assert callable(E.cwt) and callable(E.icwt_sum) and callable(E.cwt_plan)
    assert issubclass(E.CwtRefused, ValueError) and issubclass(E.CwtRefused, NotImplementedError)
    assert WV.CwtRefused is E.CwtRefused
    for w in (M6, P4):
        for attr in ("psi_ft", "flambda", "coi", "psi0"):
            assert callable(getattr(w, attr))


def test_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("sp_cwt", 19), ("sp_cwt_plan", 7), ("sp_icwt", 7)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt, "%s is not declared in include/spectral.h" % name
        nargs = len([a for a in mt.group(1).split(",") if a.strip()])
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs == want
        assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_closed_forms():
    assert M6.flambda() == pytest.approx(4 * math.pi / (6 + math.sqrt(38.0)), rel=1e-15)
    assert P4.flambda() == pytest.approx(4 * math.pi / 9, rel=1e-15)
    assert M6.coi() == pytest.approx(math.sqrt(2), rel=1e-15) and P4.coi() == pytest.approx(1 / math.sqrt(2), rel=1e-15)
    assert M6.psi0() == pytest.approx(math.pi ** -0.25, rel=1e-15)
    assert P4.psi0() == pytest.approx(2 ** 4 * math.factorial(4) / math.sqrt(math.pi * math.factorial(8)), rel=1e-13)
    assert P4.psi0() == pytest.approx(1.079, abs=5e-4)                       # T&C table 2
    u = np.linspace(-1, 30, 500)
    np.testing.assert_allclose(M6.psi_ft(u), R.psi_ft("morlet", 6.0, u), rtol=1e-13, atol=0)
    np.testing.assert_allclose(P4.psi_ft(u), R.psi_ft("paul", 4.0, u), rtol=1e-12, atol=0)
    np.testing.assert_allclose(WV.filter_rows(M6, [5.0, 40.0], 512), R.filters("morlet", 6.0, [5.0, 40.0], 512), rtol=1e-13, atol=0)
    # the wavelets have unit energy: sum |H|^2 / L = L ... (T&C eq. 6), away from the Nyquist cut
    for w, s in ((M6, 20.0), (P4, 20.0)):
        assert np.sum(WV.filter_rows(w, [s], 4096)[0] ** 2) == pytest.approx(4096.0, rel=1e-6)
    sc = WV.cwt_scales(1024, 0.5, dj=0.25, s0=2.0, J=12)
    np.testing.assert_allclose(sc, 2.0 * 2 ** (np.arange(13) * 0.25), rtol=1e-15)


def test_cdelta_is_torrence_and_compo():
    """C_delta for Morlet-6, dj = 1/16, scales 2 .. N/4: wavelet.cdelta and the factor read off cwt_ref's transform of a line in the
    middle of the band both reproduce T&C's 0.776 to 1 % (and Paul-4 their 1.132).  Eq. 13 read literally, a unit sample through
    cwt_ref, is printed beside them: 0.7026 on this scale set, which starts too far above Nyquist to cover a unit sample's spectrum."""
    n, dj = 4096, 1.0 / 16
    scales = 2.0 * 2 ** (np.arange(int(math.log2(n / 4 / 2.0) / dj) + 1) * dj)
    assert scales[0] == 2.0 and scales[-1] == n / 4
    ref = R.cdelta_ref("morlet", 6.0, scales, dj, math.pi ** -0.25)
    literal = R.cdelta_ref("morlet", 6.0, scales, dj, math.pi ** -0.25, probe="delta")
    got = WV.cdelta(M6, scales, 1.0, dj)
    print("C_delta: %.4f from a line through cwt_ref, %.4f from wavelet.cdelta, %.4f from a unit sample, T&C 0.776" % (ref, got, literal))
    assert ref == pytest.approx(0.776, rel=0.01)
    assert got == pytest.approx(0.776, rel=0.01)
    assert got == pytest.approx(ref, rel=1e-3)
    assert WV.cdelta(M6, 0.5 * scales, 0.5, dj) == pytest.approx(got, rel=1e-12)          # no dependence on dt
    sp = 8.0 * 2 ** (np.arange(8 * 16 + 1) / 16.0)
    assert WV.cdelta(P4, sp, 1.0, dj) == pytest.approx(1.132, rel=0.01)
    assert WV.cdelta(P4, sp, 1.0, dj) == pytest.approx(R.cdelta_ref("paul", 4.0, sp, dj, P4.psi0()), rel=1e-3)


def test_reconstruction_weights():
    """sum_j w_j Re W_j of a band-limited record, W from cwt_ref: wavelet.recon_weights against T&C eq. 11 restated here with C_delta
    from a unit sample through cwt_ref.  The bound is twice the residual the restatement leaves."""
    n, dt, dj = 4096, 0.25, 1.0 / 8
    scales = WV.cwt_scales(n, dt, dj, s0=4.0 * dt, J=int(math.log2(600 / 4.0) / dj), wavelet=M6)
    x = R.band_limited(n, (14.0, 37.0, 95.0, 240.0)).astype(np.float64)
    W = R.cwt_ref(x, scales / dt)
    cd = R.cdelta_ref("morlet", 6.0, scales / dt, dj, M6.psi0())           # (a line through cwt_ref; C_delta does not depend on dt)
    restated = dj * math.sqrt(dt) / (cd * M6.psi0()) * np.sum(W.real / np.sqrt(scales)[:, None], axis=0)
    mine = np.sum(WV.recon_weights(M6, scales, dt, dj)[:, None] * W.real, axis=0)
    rms = np.sqrt(np.mean(x ** 2))
    r_ref, r_mine = np.sqrt(np.mean((restated - x) ** 2)) / rms, np.sqrt(np.mean((mine - x) ** 2)) / rms
    print("reconstruction residual over rms: %.3g restated, %.3g from recon_weights" % (r_ref, r_mine))
    assert r_ref < 0.05
    assert r_mine <= 2 * r_ref
