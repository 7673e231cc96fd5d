"""Host side of the synchrosqueezed STFT and the reassignment fields (pyfft_amd.reassign, engine.ssq / ssq_bands / ssq_sum / ssq_plan,
sp_ssq / sp_ssq_bands / sp_ssq_sum / sp_ssq_plan): the float64 reference of tests/ssq_ref.py against the three facts that fix its
signs, the chirp line, the fixed-point sum against the plain one, the condition on the GPU table (how much of a frame the unsure
coefficients hold), the exact window derivatives, every refusal of the C entries before the device is touched and of the Python side
before the library loads, the plan, and the third ABI table.  No GPU needed.  tests/test_gpu_ssq.py takes the reference from here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import pyfft_amd
from pyfft_amd import _ffi, engine as E, reassign as RA
from test_host_multitaper import no_library        # noqa: F401  (a fixture)
import ssq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.case_id(c) for c in R.CASES]


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("hop,first", [(1, 0), (37, 0), (64, -128)])
def test_fact_tone(hop, first):
    """A complex tone on bin 40 under a periodic Hann window: khat = 40 in every used cell, T[g, 40] = n h[c] x[centre], all else 0
    (in the frames that lie inside the record: a frame cut by the record's end does not hold a tone)."""
    n, G = 256, 37
    x = np.exp(2j * math.pi * 40 * np.arange(G * hop + n) / n)
    w = R.hann_windows(n)
    c = R.cells(x, *w, hop, first, G, rel=1e-6)
    full = first + hop * np.arange(G) >= 0
    used = c["used"][full]
    assert full.sum() >= 35 and np.all(used.sum(axis=1) == 3) and np.all(used[:, 39:42])
    assert rel_err(c["khat"][full][used], np.full(int(used.sum()), 40.0)) <= 1e-12
    sq = R.squeeze(c)
    want = n * w[0][n // 2] * x[(first + hop * np.arange(G) + n // 2)[full]]
    assert rel_err(sq["T"][full, 40], want) <= 1e-12
    rest = sq["T"][full].copy()
    rest[:, 40] = 0
    assert np.all(rest == 0)


def test_fact_impulse():
    """A unit impulse at t0: that = t0 in every used cell of every frame that contains it."""
    n, hop, first, G, t0 = 256, 37, -128, 20, 301
    x = np.zeros(900)
    x[t0] = 1.0
    c = R.cells(x.astype(np.complex128), *R.hann_windows(n), hop, first, G, rel=1e-9)
    start = first + hop * np.arange(G)
    holds = (start < t0) & (t0 < start + n)                                          # (h[0] = 0: the frame starting on t0 sees nothing)
    assert holds.sum() >= 6 and np.all(c["used"][holds]) and not np.any(c["used"][~holds])
    that = (start + n // 2)[:, None] + c["gd"]
    assert rel_err(that[holds], np.full_like(that[holds], t0)) <= 1e-12


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_fact_centre_sum(cplx):
    """gamma = rel = 0: the sum of Xc over all n bins is n h[c] x[centre]; for real rows 2 Re of the half sum, 1/2 at DC and Nyquist."""
    n, hop, first, G = 256, 37, -128, 37
    rng = np.random.default_rng(2)
    x = rng.standard_normal(2000) + (1j * rng.standard_normal(2000) if cplx else 0)
    w = R.hann_windows(n)
    c = R.cells(x, *w, hop, first, G)
    centre = first + hop * np.arange(G) + n // 2
    want = n * w[0][n // 2] * x[centre]
    if cplx:
        got = c["Xc"].sum(axis=1)
    else:
        wk = np.ones(n // 2 + 1)
        wk[0] = wk[-1] = 0.5
        got = 2 * np.sum(wk * c["Xc"], axis=1).real
    assert rel_err(got, want) <= 1e-12
    # with the frame-start phase the main lobe sums to n h[0] = 0 instead
    assert np.max(np.abs(c["Xh"].sum(axis=1))) <= 1e-9 * np.max(np.abs(want)) or not cplx


def test_chirp_line():
    """A complex linear chirp under a Gaussian window of std n / 12: every used cell lies on the line fhat = f0 + alpha that.  The
    window's truncation at +-6 std leaves 4.6e-8 cycles per sample on this chirp at n = 256 (2.4e-4 at std n / 8); held to 1e-7."""
    n, hop, first, G = 256, 37, 0, 37
    f0, alpha = 0.05, 0.3 / 2000
    t = np.arange(2000.0)
    x = np.exp(2j * math.pi * (f0 * t + 0.5 * alpha * t * t))
    w = RA.reassignment_windows(("gaussian", n / 12.0), n)
    c = R.cells(x, *w, hop, first, G, rel=1e-3)
    that = (first + hop * np.arange(G) + n // 2)[:, None] + c["gd"]
    fhat = c["khat"] / n
    dev = np.abs(fhat - (f0 + alpha * that))[c["used"]]
    print("chirp line: %.3g cycles per sample over %d used cells" % (dev.max(), dev.size))
    assert dev.size > 37 * 5 and dev.max() <= 1e-7


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_table_condition_and_fixed_point(i):
    """The condition of the GPU table -- the unsure coefficients hold at most 2 % of the frame-summed |X_h| in every case -- and the
    fixed-point sum against the plain float64 sum at 1e-12 of the largest cell."""
    cs = R.CASES[i]
    x = R.make_signal(cs)
    c = R.cells(x, *R.hann_windows(cs["n"]), cs["hop"], cs["first"], R.NFRAMES, rel=R.REL)
    b0, nb = cs["band"] if cs["band"] else (0, None)
    plain, fixed = R.squeeze(c, b0, nb), R.squeeze(c, b0, nb, fixed=True)
    share = R.unsure_share(c, plain)
    eT, eP = rel_err(fixed["T"], plain["T"]), rel_err(fixed["P"], plain["P"])
    print("unsure share %.4f (%d coefficients); fixed against plain sums: T %.3g, P %.3g" % (share, int(plain["unsure"].sum()), eT, eP))
    assert share <= 0.02
    assert eT <= 1e-12 and eP <= 1e-12
    assert np.all(plain["reach"][np.abs(plain["T"]) > 0] > 0)


def test_recorded_constants():
    kappa, dt, _, _ = R.measure_constants()
    print("measured kappa %.4g, delta_t %.3g" % (kappa, dt))
    assert 0.98 * R.KAPPA_MEASURED <= kappa <= 1.005 * R.KAPPA_MEASURED and 0.98 * R.DELTA_T_MEASURED <= dt <= 1.005 * R.DELTA_T_MEASURED
    assert R.KAPPA == 4 * R.KAPPA_MEASURED and R.DELTA_T == 4 * R.DELTA_T_MEASURED


def test_float32_restatement_stays_inside_the_allowance():
    cs = R.CASES[3]
    x = R.make_signal(cs)
    w = R.hann_windows(cs["n"])
    a = R.cells(x, *w, cs["hop"], cs["first"], R.NFRAMES, rel=R.REL)
    b = R.cells(x, *w, cs["hop"], cs["first"], R.NFRAMES, rel=R.REL, prec=32)
    sa, sb = R.squeeze(a, *cs["band"]), R.squeeze(b, *cs["band"])
    big = np.max(np.abs(sa["T"]), axis=1, keepdims=True)
    assert np.all(np.abs(sb["T"] - sa["T"]) <= 2e-4 * np.abs(sa["T"]) + 1e-6 * big + sa["slackT"])
    assert rel_err(R.fft32(np.eye(64, dtype=np.complex64)[3]), np.fft.fft(np.eye(64)[3])) < 1e-6


@pytest.mark.parametrize("name", ["hann", "hamming", "blackman", "nuttall", "blackmanharris", "flattop"])
def test_windows_exact_derivative(name):
    n = 256
    h, dh, th = RA.reassignment_windows(name, n)
    np.testing.assert_array_equal(h, pyfft_amd.windows.__globals__["get_window"](name, n))
    spectral = np.fft.ifft(2j * math.pi * np.fft.fftfreq(n) * np.fft.fft(h)).real
    assert np.max(np.abs(dh - spectral)) <= 1e-13 and np.array_equal(th, (np.arange(n) - n / 2) * h)


def test_windows_other_tables():
    n = 128
    h, dh, th = RA.reassignment_windows(("gaussian", 9.0), n)
    j = np.arange(n) - n / 2
    np.testing.assert_allclose(h, np.exp(-j * j / 162.0), rtol=1e-14)
    np.testing.assert_allclose(dh, -j / 81.0 * h, rtol=1e-14, atol=1e-300)
    k = RA.reassignment_windows(("kaiser", 8.0), n)
    np.testing.assert_array_equal(k[1], 0.5 * (np.roll(k[0], -1) - np.roll(k[0], 1)))
    own = np.hanning(n)
    o = RA.reassignment_windows(own, n)
    np.testing.assert_array_equal(o[0], own)
    np.testing.assert_array_equal(o[1], 0.5 * (np.roll(own, -1) - np.roll(own, 1)))
    triple = (own, own * 2, own * 3)
    assert all(np.array_equal(a, b) for a, b in zip(RA.reassignment_windows(triple, n), triple))
    with pytest.raises(ValueError):
        RA.reassignment_windows(own[:-1], n)


def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in _ffi.TFR_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.TFR_SIGNATURES[name]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib


GOOD = dict(x_ld=1000, dtype=0, nsig=1000, batch=2, n=256, hop=10, first=-128, nframes=5, segmean=0, gamma=0.0, rel=1e-3, b0=0, nb=129,
            out="T", th=True, h=True, dh=True, x=True)
SSQ_REFUSALS = [
    (dict(n=300), "n must"), (dict(n=16), "n must"), (dict(n=16384), "n must"), (dict(hop=0), "hop"), (dict(nframes=-1), "nframes"),
    (dict(batch=-1), "batch"), (dict(batch=70000), "batch"), (dict(dtype=5), "dtype"), (dict(nsig=0), "nsig"), (dict(x_ld=999), "x_ld"),
    (dict(gamma=-1.0), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(rel=-1e-3), "rel"), (dict(rel=float("inf")), "rel"),
    (dict(out="none"), "an output is required"), (dict(out="IF", th=False), "th is required"), (dict(out="GD", th=False), "th is required"),
    (dict(nb=0), "nb = 0 bins"), (dict(nb=130), "nb = 130 bins"), (dict(b0=100, nb=30), "nb = 30 bins from b0 = 100"), (dict(b0=-1), "nb = 129 bins from b0 = -1"),
    (dict(dtype=1, n=8192, nb=8192), "the LDS of a workgroup"), (dict(n=8192, nb=4097, out="TP"), "the LDS of a workgroup"),
    (dict(h=False), "h and dh are required"), (dict(dh=False), "h and dh are required"), (dict(x=False), "x is required"),
]


@pytest.mark.parametrize("kw,name", SSQ_REFUSALS, ids=["%s-%d" % (n.split()[0], i) for i, (_, n) in enumerate(SSQ_REFUSALS)])
def test_c_entry_refuses_before_the_device(kw, name):
    """< 0, the message names sp_ssq and the argument, the outputs are untouched."""
    lib = _c_entry()
    a = dict(GOOD)
    a.update(kw)
    n = a["n"]
    x = np.ones((2, 1000), dtype=np.float32)
    tabs = [np.ones(n, dtype=np.float32) for _ in range(3)]
    outs = {k: np.full(64, 7.0, np.float32) for k in ("T", "P", "IF", "GD")}
    P = _ffi.ptr
    rc = lib.sp_ssq(P(x) if a["x"] else None, a["x_ld"], a["dtype"], a["nsig"], a["batch"], P(tabs[0]) if a["h"] else None,
                    P(tabs[1]) if a["dh"] else None, P(tabs[2]) if a["th"] else None, n, a["hop"], a["first"], a["nframes"], a["segmean"],
                    a["gamma"], a["rel"], a["b0"], a["nb"], *[P(outs[k]) if k in a["out"] else None for k in ("T", "P", "IF", "GD")], 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc < 0, msg
    assert msg.startswith("sp_ssq: " + name), msg
    assert all(np.all(v == 7.0) for v in outs.values())


def test_c_bands_sum_and_plan_refuse():
    lib = _c_entry()
    P = _ffi.ptr
    x, w = np.ones(1000, dtype=np.float32), np.ones(256, dtype=np.float32)
    e = np.array([[3.0, 9.0]])
    et = np.zeros((1, 5, 2), dtype=np.float32)
    out = np.full(64, 7.0 + 7.0j, np.complex64)
    good = [P(x), 1000, 0, 1000, 1, P(w), P(w), 256, 10, -128, 5, 0, 0.0, 1e-3, 1, P(e), None, 1.0, P(out), 0]
    for pos, val, text in ((7, 300, "n must"), (8, 0, "hop"), (10, -1, "nframes"), (4, 70000, "batch"), (2, 7, "dtype"), (1, 999, "x_ld"),
                           (12, -1.0, "gamma"), (13, float("nan"), "rel"), (14, 0, "nbands"), (14, 9, "nbands"),
                           (15, None, "exactly one of edges and edges_t"), (16, P(et), "exactly one of edges and edges_t"),
                           (15, P(np.array([[3.0, np.inf]])), "edges must be finite"), (17, float("nan"), "scale"),
                           (5, None, "h and dh are required"), (18, None, "out is required"), (0, None, "x is required")):
        args = list(good)
        args[pos] = val
        assert lib.sp_ssq_bands(*args) < 0, (pos, val)
        assert (lib.sp_last_error() or b"").decode().startswith("sp_ssq_bands: " + text), lib.sp_last_error()
    T = np.zeros((5, 129), dtype=np.complex64)
    good = [P(T), 5, 129, 1, 256, 0, 1, P(e), None, 1, 1.0, P(out), 0]
    for pos, val, text in ((4, 100, "n = 100"), (1, -1, "nframes"), (3, -1, "batch"), (2, 0, "nb = 0 bins"), (5, 256, "nb = 129 bins from b0 = 256"),
                           (6, 0, "nbands"), (7, None, "exactly one of"), (10, float("inf"), "scale"), (11, None, "out is required"),
                           (0, None, "T is required")):
        args = list(good)
        args[pos] = val
        assert lib.sp_ssq_sum(*args) < 0, (pos, val)
        assert (lib.sp_last_error() or b"").decode().startswith("sp_ssq_sum: " + text), lib.sp_last_error()
    assert np.all(out == 7.0 + 7.0j)
    # nothing to do: 0, nothing launched, nothing written
    th, outs = np.ones(256, dtype=np.float32), [np.full(64, 7.0, np.float32) for _ in range(4)]
    for batch, nframes in ((0, 5), (2, 0)):
        assert lib.sp_ssq(P(x), 500, 0, 500, batch, P(w), P(w), P(th), 256, 10, -128, nframes, 0, 0.0, 1e-3, 0, 129, *[P(o) for o in outs], 0) == 0
        assert lib.sp_ssq_sum(P(np.zeros((1, 129), np.complex64)), nframes, 129, batch, 256, 0, 1, P(e), None, 1, 1.0, P(out), 0) == 0
    assert all(np.all(o == 7.0) for o in outs)
    assert lib.sp_ssq_bands(*(good_b := [P(x), 1000, 0, 1000, 0, P(w), P(w), 256, 10, -128, 5, 0, 0.0, 1e-3, 1, P(e), None, 1.0, P(out), 0])) == 0
    good_b[4], good_b[10] = 1, 0
    assert lib.sp_ssq_bands(*good_b) == 0 and np.all(out == 7.0 + 7.0j)
    plan = np.zeros(5, dtype=np.int64)
    for bad in ((0, 300, 10, 1, 129, 1), (0, 256, -1, 1, 129, 1), (0, 256, 10, 70000, 129, 1), (0, 256, 10, 1, 130, 1), (0, 256, 10, 1, 129, 0),
                (0, 256, 10, 1, 129, 9)):
        assert lib.sp_ssq_plan(*bad, plan.ctypes.data) < 0, bad
    assert lib.sp_ssq_plan(0, 256, 10, 1, 129, 1, None) < 0


def test_plan():
    """Real rows fit up to 8192 points; complex rows at 8192 with the full band do not; the bytes are the images and the accumulators."""
    for n in (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
        fpw = max(1, 4096 // n)
        p = E.ssq_plan(n, 1000)
        assert p["fits"] and p["transforms"] == 1 and p["lds_bytes"] == fpw * ((n + 16) * 8 + 16 * (n // 2 + 1)) <= 160 * 1024
        assert p["fpr"] % fpw == 0 and p["workgroups"] == -(-1000 // p["fpr"])
        assert E.ssq_plan(n, 1000, T=False, P=True)["lds_bytes"] == fpw * ((n + 16) * 8 + 8 * (n // 2 + 1))
        assert E.ssq_plan(n, 1000, T=False, fields=True) == dict(p, transforms=2, lds_bytes=fpw * 2 * (n + 16) * 8)
        assert E.ssq_plan(n, 1000, bands=True) == dict(p, lds_bytes=fpw * (n + 16) * 8)
        q = E.ssq_plan(n, 1000, cplx=True, rows=3)
        assert q["transforms"] == 2 and q["lds_bytes"] == fpw * (2 * (n + 16) * 8 + 16 * n) and q["fits"] == (n <= 4096)
        assert q["workgroups"] == 3 * -(-1000 // q["fpr"])
    assert E.ssq_plan(8192, 10, cplx=True, nb=1000)["fits"] and E.ssq_plan(8192, 10, cplx=True, fields=True)["transforms"] == 3
    assert not E.ssq_plan(8192, 10, fields=True)["fits"] and E.ssq_plan(8192, 10, T=False, fields=True)["fits"]
    p = RA.ssq_plan(1 << 20, 256, band=(0.1, 0.2))
    assert (p["nframes"], p["hop"], p["first"], p["b0"], p["nb"]) == (1 << 20, 1, -128, 26, 26) and p["fits"]
    assert RA.ssq_plan(1000, 256, noverlap=192, boundary=None)["nframes"] == (1000 - 256) // 64 + 1
    os.environ["SP_SSQ_FPG"] = "5"
    try:
        assert E.ssq_plan(256, 37)["fpr"] == 5 and E.ssq_plan(256, 37)["workgroups"] == 8
    finally:
        del os.environ["SP_SSQ_FPG"]


def test_engine_refusals_carry_both_types(no_library):
    x = np.zeros(1000, dtype=np.float32)
    z = x.astype(np.complex64)
    h = np.ones(256)
    big = np.ones(8192)
    for call, text in ((lambda: E.ssq(x, np.ones(300), np.ones(300), 1, 0, 5), "power of two"), (lambda: E.ssq(x, np.ones(16), np.ones(16), 1, 0, 5), "power of two"),
                       (lambda: E.ssq(x, h, h, 0, 0, 5), "hop"), (lambda: E.ssq(x, h, h, 1, 0, -1), "nframes"),
                       (lambda: E.ssq(np.zeros((70000, 4), np.float32), h, h, 1, 0, 5), "rows"), (lambda: E.ssq(np.zeros(0, np.float32), h, h, 1, 0, 5), "at least one sample"),
                       (lambda: E.ssq(x, h, h, 1, 0, 5, gamma=-1.0), "gamma"), (lambda: E.ssq(x, h, h, 1, 0, 5, rel=float("nan")), "rel"),
                       (lambda: E.ssq(x, h, h, 1, 0, 5, T=False), "an output is required"), (lambda: E.ssq(x, h, h, 1, 0, 5, IF=True), "th is required"),
                       (lambda: E.ssq(x, h, h, 1, 0, 5, nb=0), "nb = 0"), (lambda: E.ssq(x, h, h, 1, 0, 5, b0=100, nb=30), "lie outside"),
                       (lambda: E.ssq(z, big, big, 1, 0, 5), "LDS of a workgroup"), (lambda: E.ssq(x, big, big, 1, 0, 5, P=True), "LDS of a workgroup"),
                       (lambda: E.ssq(x, h, h[:-1], 1, 0, 5), "dh must hold"), (lambda: E.ssq(x, h, None, 1, 0, 5), "h and dh are required"),
                       (lambda: E.ssq_bands(x, h, h, 1, 0, 5, np.zeros((9, 2))), "nbands"), (lambda: E.ssq_bands(x, h, h, 1, 0, 5, np.zeros((1, 4, 2))), "nframes = 5"),
                       (lambda: E.ssq_bands(x, h, h, 1, 0, 5, [(1.0, np.nan)]), "finite"), (lambda: E.ssq_bands(x, h, h, 1, 0, 5, [(1.0, 2.0)], scale=np.inf), "scale"),
                       (lambda: E.ssq_sum(np.zeros((5, 129), np.complex64), 100, [(1.0, 2.0)]), "power of two"),
                       (lambda: E.ssq_sum(np.zeros((5, 129), np.complex64), 256, [(1.0, 2.0)], b0=256), "lie outside"),
                       (lambda: E.ssq_sum(np.zeros(5, np.complex64), 256, [(1.0, 2.0)]), "[..., nframes, nb]"),
                       (lambda: E.ssq_plan(300, 10), "power of two"), (lambda: E.ssq_plan(256, 10, T=False), "an output is required"),
                       (lambda: E.ssq_plan(256, 10, nb=130), "lies outside")):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert isinstance(ei.value, ValueError) and isinstance(ei.value, E.SsqRefused) and text in str(ei.value), str(ei.value)


def test_public_refusals(no_library):
    x = np.zeros(1000)
    boxcar0 = np.ones(256)
    boxcar0[128] = 0.0
    Tx = np.zeros((129, 10), np.complex64)
    for call, text in ((lambda: RA.ssq_stft(x, nperseg=300), "power of two"), (lambda: RA.ssq_stft(x, nperseg=16384), "power of two"),
                       (lambda: RA.ssq_stft(x, hop=0), "hop"), (lambda: RA.ssq_stft(x, threshold=-1.0), "threshold"),
                       (lambda: RA.squeezed_spectrogram(x, band=(0.6, 0.7)), "holds no bins"), (lambda: RA.reassignment_fields(x, band=(0.3, 0.2)), "holds no bins"),
                       (lambda: RA.ssq_extract(x, [(0.1, 0.2)], window=boxcar0), "zero at its centre"),
                       (lambda: RA.issq_stft(Tx, window=boxcar0), "zero at its centre"),
                       (lambda: RA.ssq_extract(x, np.zeros((9, 2))), "nbands"), (lambda: RA.ssq_plan(1000, 100), "power of two")):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert isinstance(ei.value, ValueError) and text in str(ei.value), str(ei.value)
    with pytest.raises(ValueError, match="not both"):
        RA.ssq_stft(x, hop=2, noverlap=100)
    with pytest.raises(ValueError, match="boundary"):
        RA.ssq_stft(x, boundary="even")


def test_exported_declared_and_bound():
    for name in ("reassignment_windows", "ssq_stft", "issq_stft", "squeezed_spectrogram", "reassignment_fields", "ssq_extract", "ssq_plan"):
        assert getattr(pyfft_amd, name) is getattr(RA, name)
    assert issubclass(E.SsqRefused, ValueError) and issubclass(E.SsqRefused, NotImplementedError)
    assert all(callable(getattr(E, k)) for k in ("ssq", "ssq_bands", "ssq_sum", "ssq_plan"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spectral_tfr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.TFR_SIGNATURES) == {"sp_ssq", "sp_ssq_bands", "sp_ssq_sum", "sp_ssq_plan"}
    assert not set(_ffi.TFR_SIGNATURES) & (set(_ffi.SIGNATURES) | set(_ffi.EXT_SIGNATURES))
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_ssq", 22), ("sp_ssq_bands", 20), ("sp_ssq_sum", 13), ("sp_ssq_plan", 7)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.TFR_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.TFR_SIGNATURES[name][1]
    for other in ("spectral.h", "spectral_ext.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", text))
    assert "spectral_tfr.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert "SP_SSQ_FPG" in open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
