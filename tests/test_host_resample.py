"""The host side of the rational resampler: the float64 oracles upfirdn_ref / resample_poly_ref (which tests/test_gpu_resample.py holds
the device to) against scipy.signal.upfirdn / resample_poly, the bookkeeping of resample_plan and resample_rate, the refusals raised
before the library is loaded, and the two entry points of the C ABI.  No device work."""
import math
import re

import numpy as np
import pytest
import scipy.signal as ss

from pyfft_amd import _ffi, resample as RS
from test_host_multitaper import make_signal

# (up, down, ntaps): the caller's-taps shapes; the last three are the smallest records (n = 1, n = 3) and a filter shorter than `down`
SHAPES = [(3, 2, 31), (2, 3, 30), (7, 5, 141), (64, 63, 257), (5, 64, 1281), (160, 147, 41), (4, 1, 5), (1, 4, 9), (3, 7, 2)]
SHAPE_N = {(4, 1, 5): 1, (1, 4, 9): 3}
DEFAULTS = [(3, 2), (160, 147), (1, 64), (64, 1)]
PADTYPES = ["constant", "cval", "mean", "median", "minimum", "maximum", "line"]


def upfirdn_ref(h, x, up, down, m0=0, nout=None, dtype=np.float64):
    """The defining sum along the last axis, y[m] = sum_p h[phi + p up] x[i0 - p] with i0 = floor(m down / up), phi = (m down) mod up,
    x zero outside its row, for m = m0 .. m0 + nout - 1 (nout=None: up to the full length); the taps are accumulated in ascending
    order, in float64, or entirely in float32 with dtype=np.float32 (the restatement the device's bound is taken from)."""
    x = np.asarray(x)
    cdt = (np.complex64 if dtype == np.float32 else np.complex128) if np.iscomplexobj(x) else dtype
    n, T = x.shape[-1], len(h)
    if nout is None:
        nout = max(-(-((n - 1) * up + T) // down) - m0, 0)
    P = -(-T // up)
    hp = np.zeros(P * up, dtype=dtype)
    hp[:T] = np.asarray(h, dtype=dtype)
    hp = hp.reshape(P, up)
    rows = np.zeros((x.size // n, n + 1), dtype=cdt)                         # a zero behind every row: the sample outside
    rows[:, :n] = x.reshape(-1, n).astype(cdt)
    md = (m0 + np.arange(nout, dtype=np.int64)) * down
    i0, phi = md // up, md % up
    acc = np.zeros((rows.shape[0], nout), dtype=cdt)
    for p in range(P):
        i = i0 - p
        acc = acc + hp[p, phi] * rows[:, np.where((i >= 0) & (i < n), i, n)]
    assert acc.dtype == cdt
    return acc.reshape(x.shape[:-1] + (nout,))


def resample_poly_parts(x, up, down, window=("kaiser", 5.0), padtype="constant", cval=None, dtype=np.float64):
    """scipy's recipe on upfirdn_ref along the last axis: (core, add) with resample_poly = core + add, add the background put back
    (None when there is none).  'line' and a non-zero cval are scipy's boundary modes of upfirdn: here the row is extended by as many
    samples of its continuation as the filter reaches, and what a zero boundary would have given is split off as core."""
    x = np.asarray(x)
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down == 1:
        return x.copy(), None
    n = x.shape[-1]
    if isinstance(window, (list, np.ndarray)):
        h = np.array(window, dtype=np.float64)
    else:
        h = ss.firwin(2 * 10 * max(up, down) + 1, 1.0 / max(up, down), window=window)
    half = (h.size - 1) // 2
    h = h * up
    pre = down - half % down
    h = np.concatenate([np.zeros(pre), h])
    m0, nout = (half + pre) // down, -(-n * up // down)
    back = None
    if padtype in ("mean", "median", "minimum", "maximum"):
        back = {"mean": np.mean, "median": np.median, "minimum": np.amin, "maximum": np.amax}[padtype](x, axis=-1, keepdims=True)
        add = back
    elif padtype == "line" or (padtype == "constant" and cval not in (None, 0)):
        E = down * -(-(h.size // up + 2) // down)                           # a multiple of down beyond the filter's reach
        i = np.arange(-E, n + E)
        if padtype == "line":
            first = x[..., :1]
            slope = (x[..., -1:] - first) / (n - 1)
            ext = first + slope * i
        else:
            ext = np.broadcast_to(np.asarray(cval, dtype=np.float64) + 0.0 * i, x.shape[:-1] + (i.size,))
        add = upfirdn_ref(h, ext, up, down, m0 + E * up // down, nout)       # the endless continuation alone, float64
        back = ext[..., E:E + n]
    elif padtype != "constant":
        raise ValueError(padtype)
    core = upfirdn_ref(h, x if back is None else x - back, up, down, m0, nout, dtype)
    if back is None:
        return core, None
    return core, np.asarray(add)


def resample_poly_ref(x, up, down, axis=0, **kw):
    dtype = kw.get("dtype", np.float64)
    core, add = resample_poly_parts(np.moveaxis(np.asarray(x), axis, -1), up, down, **kw)
    y = core if add is None else (core + add).astype(core.dtype if dtype == np.float32 else np.result_type(core, add))
    return np.moveaxis(y, -1, axis)


def two_rows(n, cplx, seed, offset=0.0):
    return np.stack([make_signal(n, cplx, seed), make_signal(n, cplx, seed + 100)[::-1]]) + offset


def rel(got, ref):
    rms = float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    return float(np.max(np.abs(got - ref))) / (rms if rms > 0 else 1.0)


def pad_kw(padtype):
    return dict(padtype="constant", cval=1e3) if padtype == "cval" else dict(padtype=padtype)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("up,down,T", SHAPES, ids=["%d-%d-T%d" % s for s in SHAPES])
def test_oracles_match_scipy(up, down, T, cplx):
    """upfirdn_ref against scipy.signal.upfirdn (full length, and a window past the end that must be zero), resample_poly_ref against
    scipy.signal.resample_poly with the caller's taps."""
    n = SHAPE_N.get((up, down, T), 300)
    x = two_rows(n, cplx, 61)
    h = np.random.default_rng(T).standard_normal(T)
    want = ss.upfirdn(h, x, up, down)
    got = upfirdn_ref(h, x, up, down)
    assert got.shape == want.shape
    assert rel(got, want) <= 1e-12
    m0 = want.shape[-1] // 3
    win = upfirdn_ref(h, x, up, down, m0, want.shape[-1] - m0 + 9)
    assert rel(win[..., :-9], want[..., m0:]) <= 1e-12 and np.all(win[..., -9:] == 0)
    want = ss.resample_poly(x, up, down, axis=-1, window=h)
    got = resample_poly_ref(x, up, down, axis=-1, window=h)
    assert got.shape == want.shape == (2, -(-n * up // down))
    assert rel(got, want) <= 1e-12


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("up,down", DEFAULTS, ids=["%d-%d" % s for s in DEFAULTS])
def test_oracle_default_window(up, down, cplx):
    x = two_rows(500 if down == 1 else 4000, cplx, 62)
    want = ss.resample_poly(x, up, down, axis=-1)
    assert rel(resample_poly_ref(x, up, down, axis=-1), want) <= 1e-12
    assert rel(resample_poly_ref(x.T, 2 * up, 2 * down), want.T) <= 1e-12      # axis = 0 is the default, and the ratio is reduced


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("padtype", PADTYPES)
def test_oracle_padtypes(padtype, cplx):
    x = two_rows(400, cplx, 63, offset=1e3)
    for up, down in ((3, 2), (2, 5)):
        want = ss.resample_poly(x, up, down, axis=-1, **pad_kw(padtype))
        assert rel(resample_poly_ref(x, up, down, axis=-1, **pad_kw(padtype)), want) <= 1e-12


def test_oracle_copy_case():
    x = two_rows(50, False, 64)
    for fn in (resample_poly_ref, RS.resample_poly):
        y = fn(x, 7, 7, axis=-1)
        assert y is not x and y.dtype == x.dtype and np.array_equal(y, ss.resample_poly(x, 7, 7, axis=-1))
    plan = RS.resample_plan(50, 4, 4)
    assert plan["up"] == plan["down"] == 1 and plan["taps"] is None and plan["nout"] == 50


def test_plan_matches_scipy_lengths():
    """gcd reduction; m0 and nout give scipy's output length for n = 1 .. 50 over a grid of ratios: the outputs m0 .. m0 + nout - 1
    start where scipy's slice starts and the last one that carries signal lies inside the full length or the window ends in zeros."""
    for up, down in [(3, 2), (2, 3), (6, 4), (7, 5), (1, 4), (4, 1), (64, 63), (5, 64), (160, 147), (147, 160), (1, 256), (256, 1)]:
        g = math.gcd(up, down)
        for n in range(1, 51):
            plan = RS.resample_plan(n, up, down)
            assert (plan["up"], plan["down"]) == (up // g, down // g)
            assert plan["nout"] == ss.resample_poly(np.zeros(n), up, down).shape[0]
            T = plan["taps"].size
            half = (T - 1) // 2
            assert plan["pre"] == plan["down"] - half % plan["down"] and plan["m0"] == (half + plan["pre"]) // plan["down"]
            assert plan["tile"] == _ffi.load_library().sp_upfirdn_tile(plan["up"], plan["down"], T + plan["pre"], 0)
            assert plan["workgroups"] == -(-plan["nout"] // plan["tile"])
    plan = RS.resample_plan(1000, 320, 294, cplx=True)
    assert (plan["up"], plan["down"]) == (160, 147)
    np.testing.assert_array_equal(plan["taps"], 160 * ss.firwin(2 * 10 * 160 + 1, 1.0 / 160, window=("kaiser", 5.0)))
    np.testing.assert_array_equal(RS.resample_plan(10, 1, 4, window="hamming")["taps"], ss.firwin(81, 0.25, window="hamming"))
    h = np.arange(1.0, 8.0)
    np.testing.assert_array_equal(RS.resample_plan(10, 3, 1, window=h)["taps"], 3 * h)


def test_resample_rate_ratios(monkeypatch):
    calls = []
    monkeypatch.setattr(RS, "resample_poly", lambda x, up, down, **kw: calls.append((up, down, kw)) or "y")
    assert RS.resample_rate(None, 44100, 48000) == ("y", 48000.0)
    assert RS.resample_rate(None, 48000.0, 44100.0, axis=0, window="hamming") == ("y", 44100.0)
    assert RS.resample_rate(None, 1e6, 250e3)[1] == 250e3
    assert [c[:2] for c in calls] == [(160, 147), (147, 160), (1, 4)] and calls[1][2] == dict(axis=0, window="hamming")
    for fs_new in (math.sqrt(2.0), 1.0 / math.pi, 257.0, 1.0 / 257.0):
        with pytest.raises(RS.Unsupported):
            RS.resample_rate(None, 1.0, fs_new)
    with pytest.raises(RS.Unsupported):
        RS.resample_rate(None, 44100, 48000, max_factor=100)
    y, fs_out = RS.resample_rate(None, 1.0, math.sqrt(2.0), exact=False)
    up, down, _ = calls[-1]
    assert up <= 256 and down <= 256 and fs_out == up / down and abs(fs_out - math.sqrt(2.0)) < 1e-4
    assert RS.resample_rate(None, 44100, 48000, max_factor=100, exact=False)[1] == 44100 * calls[-1][0] / calls[-1][1]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            RS.resample_rate(None, bad, 1.0)


def test_python_refusals_come_before_the_library(monkeypatch):
    """Limits, complex taps, modes that are not built, an axis out of range: all raised without loading libspectral.so."""
    from pyfft_amd import engine

    def boom(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_ffi, "load_library", boom)
    monkeypatch.setattr(_ffi, "lib", boom)
    monkeypatch.setattr(engine, "lib", boom)
    x, h = np.zeros((2, 64)), np.ones(5)
    assert issubclass(RS.Unsupported, ValueError) and issubclass(RS.Unsupported, NotImplementedError)
    unsupported = [
        lambda: RS.upfirdn(h, x, 257, 1), lambda: RS.upfirdn(h, x, 1, 257), lambda: RS.upfirdn(np.ones(8192), x),
        lambda: RS.upfirdn(h * 1j, x), lambda: RS.upfirdn(h, x, mode="symmetric"), lambda: RS.upfirdn(h, x, mode="line"),
        lambda: RS.upfirdn(h, x, cval=1.0),
        lambda: RS.resample_poly(x, 257, 256), lambda: RS.resample_poly(x, 1, 257), lambda: RS.resample_poly(x, 514, 3),
        lambda: RS.resample_poly(x, 1, 2, window=np.ones(8191)), lambda: RS.resample_poly(x, 3, 2, window=h * 1j),
        lambda: RS.resample_poly(x, 3, 2, padtype="symmetric"), lambda: RS.resample_poly(x, 3, 2, padtype="edge"),
        lambda: RS.resample_poly(x, 3, 2, padtype="smooth"), lambda: RS.resample_plan(64, 1, 300),
    ]
    for call in unsupported:
        with pytest.raises(RS.Unsupported):
            call()
    plain = [
        lambda: RS.upfirdn(h, x, axis=2), lambda: RS.upfirdn(h, x, axis=-3), lambda: RS.upfirdn(h, x, 0, 1),
        lambda: RS.upfirdn(h, x, 1.5, 1), lambda: RS.upfirdn(np.ones((2, 2)), x), lambda: RS.upfirdn([], x),
        lambda: RS.upfirdn([1.0, float("nan")], x), lambda: RS.upfirdn(h, np.float64(1.0)),
        lambda: RS.resample_poly(x, 3, 2, axis=2), lambda: RS.resample_poly(x, 3, 0), lambda: RS.resample_poly(x, 3, 2.5),
        lambda: RS.resample_poly(x, 3, 2, padtype="mean", cval=1.0), lambda: RS.resample_poly(x, 3, 2, window=np.ones((3, 3))),
        lambda: RS.resample_poly(np.zeros((2, 0)), 3, 2, axis=1), lambda: RS.resample_plan(0, 3, 2),
    ]
    for call in plain:
        with pytest.raises(ValueError) as info:
            call()
        assert not isinstance(info.value, RS.Unsupported)
    import pyfft_amd
    for name in ("upfirdn", "resample_poly", "resample_rate", "resample_plan"):
        assert getattr(pyfft_amd, name) is getattr(RS, name)
    for name in ("upsample", "downsample", "downsample_efficient"):             # the reference's names keep raising
        with pytest.raises(NotImplementedError):
            getattr(pyfft_amd.filters, name)(x, 1.0, 2.0)


def test_c_abi_is_declared_bound_and_exported():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "spectral.h")).read(), flags=re.S)
    for name, nargs in (("sp_upfirdn", 13), ("sp_upfirdn_tile", 4)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(_ffi.SIGNATURES[name][1]) == nargs
        assert hasattr(_ffi.load_library(), name)


def test_tile_is_positive_inside_the_limits_and_zero_outside():
    """Every admitted shape has a tile that fits one workgroup; K is a multiple of up (whole phase classes) and of 4."""
    tile = _ffi.load_library().sp_upfirdn_tile
    for cplx in (0, 1):
        for ntaps in (1, 8191):
            for up in range(1, 257):
                for down in range(1, 257):
                    K = tile(up, down, ntaps, cplx)
                    assert 0 < K <= 4096 and K % (4 * up) == 0, (up, down, ntaps, cplx, K)
        for bad in ((0, 1, 5), (257, 1, 5), (1, 0, 5), (1, 257, 5), (3, 2, 0), (3, 2, 8192), (-1, 2, 5), (3, -2, 5)):
            assert tile(*bad, cplx) == 0, bad
    from pyfft_amd import engine
    assert engine.upfirdn_tile(1, 256, 5121, True) == tile(1, 256, 5121, 1)
    with pytest.raises(ValueError):
        engine.upfirdn_tile(1, 257, 5, False)
