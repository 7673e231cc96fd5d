"""Host side of the cross-wavelet transform and the wavelet coherence (pyfft_amd.wavelet.xwt / wct, engine.wct_time / wct_scale,
sp_wct_time / sp_wct_scale / sp_wct_plan): the float64 reference of tests/wct_ref.py against a direct time-domain double sum and against
its own invariants, the scale window against scipy, the Gaussian's margin, the plan arithmetic, the float64 restatement of the
overlap-save plan, every refusal of the C entries before the device is touched and of the Python side before the library loads, and
the second ABI table.  No GPU needed.  tests/test_gpu_wct.py takes the reference from here."""
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
import wct_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M6 = WV.Morlet(6.0)


def test_reference_is_a_double_sum():
    """wct_ref against direct O(N K) sums in the time domain: W by np.convolve with g_s, the smoothing by np.convolve with the Gaussian
    written down in the time domain, exp(-m^2 / (2 s'^2)) / (s' sqrt(2 pi)) -- its transform on the integers is the periodised
    exp(-(s' w)^2 / 2), which differs from the reference's cut at |w| = pi by exp(-(pi s')^2 / 2) < 1e-30 for s' >= 4."""
    n, grid = 300, 1 << 13
    x, y = Q.make_pair(n, True, 1)
    x, y = x.astype(np.complex128), y.astype(np.complex128)
    scales = np.array([4.0, 5.5, 9.0, 17.0])
    ref = Q.wct_ref(x, y, scales, 6.0, dj=0.25, n_full=grid)      # (g_s of the same grid: its 1 / n tails fold with the grid, 1e-9)
    T = np.zeros((len(scales), n, 4))
    for j, s in enumerate(scales):
        g = R.kernel_time("morlet", 6.0, s, grid)
        gk = np.concatenate([g[grid // 2:], g[:grid // 2]])                       # lags -grid / 2 .. grid / 2 - 1
        Wx = np.convolve(x, gk)[grid // 2:grid // 2 + n]
        Wy = np.convolve(y, gk)[grid // 2:grid // 2 + n]
        m = np.arange(-int(10 * s) - 1, int(10 * s) + 2)
        ga = np.exp(-0.5 * (m / s) ** 2) / (s * math.sqrt(2 * math.pi))
        for k, p in enumerate((np.abs(Wx) ** 2 / s, np.abs(Wy) ** 2 / s, (Wx * np.conj(Wy)).real / s, (Wx * np.conj(Wy)).imag / s)):
            T[j, :, k] = np.convolve(p, ga)[len(m) // 2:len(m) // 2 + n]
    err = Q.row_err(T, ref["T"])
    print("reference against the double sum: %.3g of the row rms" % err)
    assert err <= 1e-10
    win = Q.scale_window(0.25)
    K = len(win)
    D = np.zeros_like(T)
    for s in range(len(scales)):
        for t in range(K):
            r = s + (K - 1) // 2 - t
            if 0 <= r < len(scales):
                D[s] += win[t] * T[r]
    assert np.max(np.abs(D[..., 0] - ref["A"])) <= 1e-12 * np.max(ref["A"])
    assert np.max(np.abs(D[..., 2] + 1j * D[..., 3] - ref["C"])) <= 1e-12 * np.max(np.abs(ref["C"]))
    np.testing.assert_allclose(Q.xwt_ref(x, y, scales), R.cwt_ref(x, scales) * np.conj(R.cwt_ref(y, scales)), rtol=0, atol=0)


@pytest.mark.parametrize("n,S,cplx", [(700, 11, False), (3000, 24, False), (3000, 24, True)])
def test_reference_invariants(n, S, cplx):
    x, y = Q.make_pair(n, cplx, 1)
    scales = 4.0 * 2 ** (np.arange(S) / 4.0)
    ref = Q.wct_ref(x, y, scales, 6.0, dj=0.25)
    Q.assert_conditioned(ref)
    assert ref["R2"].min() >= 0 and ref["R2"].max() <= 1 + 1e-12                  # Cauchy-Schwarz under a positive smoothing
    assert ref["R2"].min() < 0.01 and ref["R2"].max() > 0.95
    same = Q.wct_ref(x, x, scales, 6.0, dj=0.25)
    assert np.max(np.abs(same["R2"] - 1)) <= 1e-12 and np.max(np.abs(same["phase"])) <= 1e-12


def test_reference_sees_a_delay_and_no_coherence_in_noise():
    n, d, f = 4000, 5, 0.037
    rng = np.random.default_rng(11)
    t = np.arange(n)
    x = np.cos(2 * math.pi * f * t) + 0.3 * rng.standard_normal(n)
    y = np.concatenate([np.zeros(d), x[:-d]])                                     # y[n] = x[n - d]
    scales = 4.0 * 2 ** (np.arange(17) / 4.0)
    ref = Q.wct_ref(x, y, scales, 6.0, dj=0.25)
    j = int(np.argmin(np.abs(1.0 / (M6.flambda() * scales) - f)))               # the line's scale
    mid = slice(1000, 3000)
    assert ref["R2"][j, mid].min() > 0.99
    assert np.max(np.abs(ref["phase"][j, mid] - 2 * math.pi * f * d)) < 0.02     # x leads: Wx conj(Wy) turns by + w d
    a, b = 0.5 * rng.standard_normal(n), 0.5 * rng.standard_normal(n)
    noise = Q.wct_ref(a, b, scales, 6.0, dj=0.25)
    shared = Q.wct_ref(a + np.cos(2 * math.pi * f * t), b + np.cos(2 * math.pi * f * t + 0.4), scales, 6.0, dj=0.25)
    print("mean R2: independent noises %.3f, with a shared line %.3f at its scale" % (noise["R2"][j].mean(), shared["R2"][j].mean()))
    assert noise["R2"][j].mean() < 0.5 < 0.9 < shared["R2"][j].mean()


@pytest.mark.parametrize("dj,K", [(1 / 4, 7), (1 / 8, 12), (1 / 12, 16)])
def test_scale_window(dj, K):
    import scipy.signal as ss
    win = WV.scale_window(dj)
    assert len(win) == K == int(round(2 * 0.6 / dj)) + 2 and abs(win.sum() - 1) < 1e-15 and win[0] == win[-1] == 0.5 * win[1]
    np.testing.assert_array_equal(win, Q.scale_window(dj))
    rng = np.random.default_rng(3)
    T = rng.standard_normal((23, 5))
    want = ss.convolve2d(T, win[:, None], "same")
    # the kernel's rule: row s - K // 2 + j takes win[K - 1 - j], rows outside are zero
    got = np.zeros_like(T)
    for s in range(23):
        for j in range(K):
            r = s - K // 2 + j
            if 0 <= r < 23:
                got[s] += win[K - 1 - j] * T[r]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(Q.smooth_scale_f32(T, win), want, rtol=0, atol=1e-5)
    ones = ss.convolve2d(np.ones((23, 1)), win[:, None], "same")[:, 0]           # the common factor that cancels in the ratio
    assert np.all(ones[K:-K] == pytest.approx(1.0)) and ones[0] < 0.6


def test_smooth_margin():
    s = 4.0 * 2 ** (np.arange(30) / 4.0)
    m = np.array([WV.smooth_margin(v) for v in s])
    assert np.all(np.diff(m) > 0) and np.all(m >= 4.5 * s) and np.all(m <= 5.5 * s), m / s
    assert WV.smooth_margin(10.0) == Q.smooth_margin_ref(10.0) and WV.smooth_margin(133.0, 1e-5) == Q.smooth_margin_ref(133.0, 1e-5)
    assert WV.smooth_margin(50.0, 1e-4) < WV.smooth_margin(50.0, 1e-6) < WV.smooth_margin(50.0, 1e-8)
    # 2 Q(M / s) = tail: 4.89 standard deviations at 1e-6
    assert abs(WV.smooth_margin(300.0) / 300.0 - 4.8916) < 0.01


def test_plan_arithmetic():
    sc = np.concatenate([[2.0], 4.0 * 2 ** (np.arange(76) / 12.0), [330.0, 700.0]])
    plan = WV.wct_plan(9000, scales=sc)
    mw, mg = plan["margins_w"], plan["margins_g"]
    assert list(plan["path"][:2]) == ["composed", "fused"] and list(plan["path"][-3:]) == ["fused", "composed", "composed"]
    own = (mw + mg <= 3072)
    assert np.array_equal(plan["fused"], own)                                     # the split at 3072 samples of Mw + Mg
    assert sc[plan["fused"]].max() > 300 and (mw + mg)[plan["fused"]].max() <= 3072 < (mw + mg)[-2]
    assert plan["Mw"] == mw[own].max() and plan["Mg"] == mg[own].max() and plan["M"] == plan["Mw"] + plan["Mg"]
    assert plan["L"] == 8192 and plan["hop"] == 8192 - 2 * plan["M"] and plan["frames"] == -(-9000 // plan["hop"])
    assert plan["n_full"] == 32768 and plan["n_smooth"] == R.next_pow2(9000 + mg[-1]) and plan["bytes_T"] == 16 * len(sc) * 9000
    for top, L in ((6.4, 256), (12.0, 512), (25.0, 1024), (50.0, 2048), (100.0, 4096), (200.0, 8192)):
        p = WV.wct_plan(1000, scales=np.linspace(3.8, top, 5))
        assert p["L"] == L and p["fused"].all() and 4 * p["M"] <= L < 8 * p["M"] and p["n_full"] is None, (top, p["L"], p["M"])
        assert p["hop"] == L - 2 * (p["Mw"] + p["Mg"])
    # a far-reaching wavelet beside a far-reaching Gaussian: the scale with the longest wavelet leaves the fused set
    near = 3.6
    assert 1000 < WV.margin(M6, near) <= 3072
    p = WV.wct_plan(1000, scales=[near, 8.0, 300.0])
    assert list(p["path"]) == ["composed", "fused", "fused"] and p["M"] <= 3072


PLANS = [((100, 5, 1, 256, 40, 21), (134, 1)), ((134 * 3 + 1, 5, 1, 256, 40, 21), (134, 4)), ((5477, 30, 2, 8192, 1400, 1336), (2720, 3)),
         ((1 << 20, 88, 1, 8192, 1536, 1536), (2048, 512)), ((777, 7, 3, 512, 0, 0), (512, 2)), ((9000, 3, 1, 2048, 300, 200), (1048, 9))]


@pytest.mark.parametrize("shape,want", PLANS, ids=[str(p[0]) for p in PLANS])
def test_engine_plan(shape, want):
    nsig, S, rows, L, Mw, Mg = shape
    p = E.wct_plan(nsig, S, L, Mw, Mg, rows=rows)
    hop, frames = want
    assert (p["hop"], p["frames"]) == (hop, frames) and hop == L - 2 * (Mw + Mg) and frames == -(-nsig // hop)
    fpw = max(1, 4096 // L)
    assert 1 <= p["chunk"] <= S and p["workgroups"] == -(-frames // fpw) * -(-S // p["chunk"]) * rows
    # the exchange images (16 rows of L / 16 + 1 complex) and, from 2048 points on, two half spectra per transform group
    assert p["lds_bytes"] == 8 * fpw * (L + 16 + (L if L >= 2048 else 0)) <= 160 * 1024
    if Mg == 0:
        assert E.wct_plan(nsig, S, L, Mw, 0, rows=rows, xwt=True) == p


def test_overlap_save_restatement():
    """The plan in float64 against wct_ref.  A transform loses at most 4 tail of its row rms beyond the wavelet's margin
    (tests/test_host_wavelet.py); a product of two transforms then 8 tail to first order; the Gaussian is a positive unit-gain
    average, which does not amplify that, and leaves its own tail x the largest product behind its margin: (8 + crest) tail of
    the row rms, crest = the products' peak over rms, taken from the reference.  For Wxy, which nothing averages, the 8 tail apply to
    the local magnitude: 8 crest tail of the row rms.
    As numbers, on this case (crest 9.9): T is held to 17.9 tail and loses 0.013 tail -- the smoothing averages the transforms'
    oscillating losses away; Wxy is held to 79 tail and loses 1.2 tail."""
    n, tail = 6000, 1e-6
    scales = 4.0 * 2 ** (np.arange(40) / 8.0)[:38]
    plan = WV.wct_plan(n, scales=scales, tail=tail)
    assert plan["fused"].all() and plan["L"] == 4096 and 4 * plan["M"] > 3600
    x, y = Q.make_pair(n, False, 3)
    ref = Q.wct_ref(x, y, scales, 6.0, dj=1 / 8)
    T = Q.overlap_save(x, y, scales, 6.0, plan["L"], plan["Mw"], plan["Mg"])
    err = Q.row_err(T, ref["T"])
    P = Q.products(R.cwt_ref(x, scales), R.cwt_ref(y, scales), scales)
    crest = float(np.max(np.max(np.abs(P), axis=1) / np.sqrt(np.mean(np.abs(P) ** 2, axis=1))))
    print("float64 overlap-save against wct_ref: %.3g of the row rms = %.3g tail (crest %.3g, bound %.3g tail)"
          % (err, err / tail, crest, 8 + crest))
    assert 0 < err <= (8 + crest) * tail
    Wxy = Q.overlap_save(x, y, scales, 6.0, plan["L"], plan["Mw"], 0, xwt=True)
    exy = Q.row_err(Wxy, Q.xwt_ref(x, y, scales))
    print("float64 overlap-save against xwt_ref: %.3g of the row rms = %.3g tail (bound %.3g tail)" % (exy, exy / tail, 8 * crest))
    assert 0 < exy <= 8 * tail * crest


def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.EXT_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.EXT_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


GOOD = dict(dtype=0, nsig=1000, x_ld=1000, y_ld=1000, batch=2, nscales=4, family=0, p0=6.0, L=256, Mw=40, Mg=21, out="T")
TIME_REFUSALS = [
    (dict(L=300), "L must"), (dict(L=128), "L must"), (dict(L=16384), "L must"), (dict(Mw=-1), "Mw and Mg"), (dict(Mg=-1), "Mw and Mg"),
    (dict(Mw=110), "Mw and Mg"), (dict(Mw=77), "Mw + Mg leaves hop"), (dict(out="Wxy"), "Mg must be 0"),
    (dict(nscales=0), "nscales"), (dict(nscales=70000), "nscales"),
    (dict(scales=[4.0, 0.0, 5.0, 6.0]), "scales[1]"), (dict(scales=[4.0, 5.0, 6.0, float("nan")]), "scales[3]"),
    (dict(scales=None), "scales is required"), (dict(nsig=0), "nsig"), (dict(batch=-1), "batch"), (dict(batch=70000), "batch"),
    (dict(x_ld=999), "x_ld"), (dict(y_ld=999), "y_ld"), (dict(dtype=5), "dtype"), (dict(family=2), "family 2"),
    (dict(family=1, p0=4.0), "family must be SP_CWT_MORLET with T"), (dict(p0=0.0), "parameter"), (dict(p0=float("nan")), "parameter"),
    (dict(out="Wxy", Mg=0, family=1, p0=0.5), "parameter"), (dict(out="both"), "exactly one output"), (dict(out="none"), "exactly one output"),
    (dict(x=None), "x and y are required"), (dict(y=None), "x and y are required"),
]


@pytest.mark.parametrize("kw,name", TIME_REFUSALS, ids=["%s-%d" % (n.split()[0], i) for i, (_, n) in enumerate(TIME_REFUSALS)])
def test_c_time_entry_refuses_before_the_device(kw, name):
    """< 0, the message names sp_wct_time and the argument, the outputs are untouched."""
    lib = _c_entry()
    a = dict(GOOD)
    a.update({k: v for k, v in kw.items() if k in GOOD})
    x, y = np.ones((2, 1000), dtype=np.float32), np.ones((2, 1000), dtype=np.float32)
    scales = kw.get("scales", [4.0, 5.0, 6.0, 7.0])
    sc = None if scales is None else np.array(scales, dtype=np.float64)
    T, Wxy = np.full((2, 4, 1000, 4), 7.0, np.float32), np.full((2, 4, 1000), 7.0 + 7.0j, np.complex64)
    xp = None if ("x" in kw and kw["x"] is None) else _ffi.ptr(x)
    yp = None if ("y" in kw and kw["y"] is None) else _ffi.ptr(y)
    rc = lib.sp_wct_time(xp, a["x_ld"], yp, a["y_ld"], a["dtype"], a["nsig"], a["batch"], _ffi.ptr(sc), a["nscales"], a["family"], a["p0"],
                         a["L"], a["Mw"], a["Mg"], _ffi.ptr(T) if a["out"] in ("T", "both") else None,
                         _ffi.ptr(Wxy) if a["out"] in ("Wxy", "both") else None, 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc < 0, msg
    assert msg.startswith("sp_wct_time: " + name), msg
    assert np.all(T == 7.0) and np.all(Wxy == 7.0 + 7.0j)


def test_c_scale_and_plan_refuse():
    lib = _c_entry()
    out = np.zeros(5, dtype=np.int64)
    assert lib.sp_wct_plan(1000, 4, 1, 256, 40, 21, 0, out.ctypes.data) == 0 and tuple(out[:2]) == (134, 8) and out[4] == 8 * 16 * 272
    assert lib.sp_wct_plan(1000, 4, 1, 256, 61, 0, 1, out.ctypes.data) == 0
    for bad in ((1000, 4, 1, 300, 40, 21, 0), (1000, 4, 1, 256, 100, 28, 0), (1000, 4, 1, 256, 77, 20, 0), (1000, 0, 1, 256, 40, 21, 0),
                (0, 4, 1, 256, 40, 21, 0), (1000, 4, -1, 256, 40, 21, 0), (1000, 4, 1, 256, 40, 21, 1), (1000, 4, 1, 256, -1, 21, 0)):
        assert lib.sp_wct_plan(*bad, out.ctypes.data) < 0, bad
    assert lib.sp_wct_plan(1000, 4, 1, 256, 40, 21, 0, None) < 0
    T = np.zeros((1, 4, 100, 4), dtype=np.float32)
    o = [np.full((1, 4, 100), 7.0, np.float32) for _ in range(4)] + [np.full((1, 4, 100), 7.0 + 7.0j, np.complex64)]
    w = np.ones(3, dtype=np.float32)
    P = _ffi.ptr
    for args, text in (((P(T), 100, 0, 1, P(w), 3, P(o[0]), P(o[1]), None, None, None, 0), "nscales"),
                       ((P(T), 0, 4, 1, P(w), 3, P(o[0]), P(o[1]), None, None, None, 0), "nsig"),
                       ((P(T), 100, 4, -1, P(w), 3, P(o[0]), P(o[1]), None, None, None, 0), "batch"),
                       ((P(T), 100, 4, 1, P(w), 0, P(o[0]), P(o[1]), None, None, None, 0), "ntaps"),
                       ((P(T), 100, 4, 1, P(w), 5000, P(o[0]), P(o[1]), None, None, None, 0), "ntaps"),
                       ((P(T), 100, 4, 1, None, 3, P(o[0]), P(o[1]), None, None, None, 0), "taps is required"),
                       ((P(T), 100, 4, 1, P(np.array([1, np.nan, 1], np.float32)), 3, P(o[0]), P(o[1]), None, None, None, 0), "taps must be finite"),
                       ((P(T), 100, 4, 1, P(w), 3, P(o[0]), P(o[1]), P(o[2]), None, None, 0), "A, B and C"),
                       ((P(T), 100, 4, 1, P(w), 3, P(o[0]), P(o[1]), P(o[2]), P(o[3]), None, 0), "A, B and C"),
                       ((P(T), 100, 4, 1, P(w), 3, P(o[0]), P(o[1]), None, None, P(o[4]), 0), "A, B and C"),
                       ((P(T.ctypes.data + 4), 100, 4, 1, P(w), 3, P(o[0]), P(o[1]), None, None, None, 1), "T must be 16-byte aligned"),
                       ((None, 100, 4, 1, P(w), 3, P(o[0]), P(o[1]), None, None, None, 0), "T, R2 and phase"),
                       ((P(T), 100, 4, 1, P(w), 3, None, P(o[1]), None, None, None, 0), "T, R2 and phase")):
        assert lib.sp_wct_scale(*args) < 0
        assert (lib.sp_last_error() or b"").decode().startswith("sp_wct_scale: " + text), lib.sp_last_error()
    assert all(np.all(v == 7.0) for v in o[:4]) and np.all(o[4] == 7.0 + 7.0j)


def test_engine_refusals_carry_both_types(no_library):
    x = np.zeros(1000, dtype=np.float32)
    sc = [4.0, 5.0]
    for args, kw, text in (((x, x, sc, "morlet", 6.0, 300, 40, 21), {}, "power of two"), ((x, x, sc, "morlet", 6.0, 256, 100, 28), {}, "Mw + Mg"),
                           ((x, x, sc, "morlet", 6.0, 256, 77, 20), {}, "below L / 4"), ((x, x, sc, "morlet", 6.0, 256, -1, 21), {}, "negative"),
                           ((x, x, [], "morlet", 6.0, 256, 40, 21), {}, "at least one scale"),
                           ((x, x, [4.0, np.nan], "morlet", 6.0, 256, 40, 21), {}, "positive and finite"),
                           ((x, x, sc, "paul", 4.0, 256, 40, 21), {}, "Morlet wavelets only"), ((x, x, sc, "dog", 2.0, 256, 40, 0), dict(xwt=True), "not built"),
                           ((x, x, sc, "paul", 4.0, 256, 40, 21), dict(xwt=True), "must be 0"),
                           ((x, x[:-1], sc, "morlet", 6.0, 256, 40, 21), {}, "share their shape"),
                           ((x, x.astype(np.complex64), sc, "morlet", 6.0, 256, 40, 21), {}, "share their shape"),
                           ((np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), sc, "morlet", 6.0, 256, 40, 21), {}, "rows")):
        with pytest.raises(NotImplementedError) as ei:
            E.wct_time(*args, **kw)
        assert isinstance(ei.value, ValueError) and isinstance(ei.value, E.WctRefused) and text in str(ei.value), str(ei.value)
    T = np.zeros((2, 3, 10, 4), np.float32)
    for args, text in (((T, []), "taps"), ((T, [1.0, np.inf]), "taps"), ((T[..., :3], [1.0]), "[..., S, N, 4]"), ((T[0, 0], [1.0]), "[..., S, N, 4]"),
                       ((np.zeros((0, 3, 10, 4), np.float32), [1.0]), "rows")):
        with pytest.raises(NotImplementedError) as ei:
            E.wct_scale(*args)
        assert isinstance(ei.value, ValueError) and isinstance(ei.value, E.WctRefused) and text in str(ei.value), str(ei.value)
    with pytest.raises(E.WctRefused, match="power of two"):
        E.wct_plan(1000, 4, 300, 40, 21)


def test_public_refusals_carry_both_types(no_library):
    x = np.zeros(1000)
    for call, text in ((lambda: WV.wct(x, x, wavelet=WV.Paul(4)), "Morlet wavelets only"), (lambda: WV.wct(x, x[:-1]), "equal shapes"),
                       (lambda: WV.xwt(x, x[:-1]), "equal shapes"), (lambda: WV.wct(x, x, scales=[-1.0]), "positive"),
                       (lambda: WV.wct(x, x, wavelet="dog"), "not built"), (lambda: WV.wct(x, x, dj=0.0, scales=[8.0]), "dj and dj0"),
                       (lambda: WV.wct_plan((1 << 25) + 1, scales=[8.0, 400.0]), "resample_poly"),
                       (lambda: WV.wct_plan(0, scales=[8.0]), "at least one sample"), (lambda: WV.smooth_margin(-1.0), "positive and finite")):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert isinstance(ei.value, ValueError) and text in str(ei.value), str(ei.value)
    with pytest.raises(E.WctRefused):
        WV.wct(x, x, wavelet=WV.Paul(4))
    assert WV.wct_plan((1 << 25) + 1, scales=[8.0, 16.0])["n_full"] is None


def test_exported_declared_and_bound():
    for name in ("xwt", "wct", "wct_plan"):
        assert getattr(pyfft_amd, name) is getattr(WV, name)
    assert issubclass(E.WctRefused, ValueError) and issubclass(E.WctRefused, NotImplementedError)
    assert callable(E.wct_time) and callable(E.wct_scale) and callable(E.wct_plan)
    hdr = open(os.path.join(ROOT, "include", "spectral_ext.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.EXT_SIGNATURES) == {"sp_wct_time", "sp_wct_scale", "sp_wct_plan", "sp_last_passes"}
    assert not set(_ffi.SIGNATURES) & set(_ffi.EXT_SIGNATURES)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_wct_time", 17), ("sp_wct_scale", 12), ("sp_wct_plan", 8), ("sp_last_passes", 1)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.EXT_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.EXT_SIGNATURES[name][1]
    first = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spectral.h")).read(), flags=re.S)
    assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", first))
    assert "spectral_ext.h" in open(os.path.join(ROOT, "Makefile")).read()
