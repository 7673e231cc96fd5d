"""The smoothed pseudo Wigner-Ville kernel (k_wvd.hip) on the device against the float64 restatement of tests/wvd_ref.py, under the
allowance that module derives: 4 x the measured deviation of the float32 restatement, of a column's largest cell, plus 1e-6 of the
call's largest cell.  The shapes (wvd_ref.SHAPES) are the smallest at which each mechanism first engages."""
import ctypes

import numpy as np
import pytest

import guard_ref as G
import wvd_ref as R
from pyfft_amd import _ffi, engine as E, hilbert as pyfft_hilbert, wigner as WG

pytestmark = pytest.mark.gpu
NAMES = list(R.SHAPES)


@pytest.fixture(scope="module")
def torch():
    import torch
    _ffi.init()
    return torch


def rows_of(name, which=0):
    """the samples [rows, nsig] of a shape; with a pitch, a strided view of a wider array"""
    s = R.SHAPES[name]
    a = R.signals(name)[which]
    if not s["pitch"]:
        return a
    wide = np.full((s["rows"], s["nsig"] + s["pitch"]), np.nan + 0j, dtype=np.complex64)
    wide[:, :s["nsig"]] = a
    return wide


def run(name, x, y=None, **kw):
    s = R.SHAPES[name]
    h, g = R.windows_of(s)
    return E.wvd(x, h, g, s["hop"], s["first"], s["ntimes"], s["nfft"], y=y, b0=s["b0"], nb=s["nb"], **kw)


def on_device(torch, name, which=0):
    """device rows; a shape with a pitch goes in as a row-strided view (x_ld > nsig)"""
    s = R.SHAPES[name]
    d = torch.as_tensor(np.array(rows_of(name, which)), device="cuda")       # (the shared arrays are read-only)
    return d[:, :s["nsig"]] if s["pitch"] else d


@pytest.mark.parametrize("cross", (False, True), ids=("auto", "cross"))
@pytest.mark.parametrize("name", NAMES)
def test_against_reference(torch, name, cross):
    s = R.SHAPES[name]
    x = on_device(torch, name)
    y = on_device(torch, name, 1) if cross else None
    assert not s["pitch"] or x.stride(0) == s["nsig"] + s["pitch"]
    W = run(name, x, y)
    assert W.dtype == (torch.complex64 if cross else torch.float32) and tuple(W.shape) == (s["rows"], s["ntimes"], s["nb"])
    got, ref = W.cpu().numpy(), R.band(R.reference(name, cross), s)
    R.assert_within(got, ref, "%s %s" % (name, "cross" if cross else "auto"))
    # columns whose time window misses the record are exactly zero
    n = s["first"] + s["hop"] * np.arange(s["ntimes"])
    out = (n + s["ng"] // 2 < 0) | (n - s["ng"] // 2 >= s["nsig"])
    assert np.all(got[:, out, :] == 0)
    assert np.all(np.max(np.abs(ref), axis=-1)[:, out] == 0) and np.all(np.max(np.abs(got), axis=-1)[:, ~out] > 0)
    if name in ("n32-full-lag", "n8192-right-of-record"):
        assert out.any()


@pytest.mark.parametrize("cross", (False, True), ids=("auto", "cross"))
@pytest.mark.parametrize("name", NAMES)
def test_bitwise_reproducible_under_any_partition(torch, name, cross, monkeypatch):
    s = R.SHAPES[name]
    x, y = on_device(torch, name), on_device(torch, name, 1) if cross else None
    monkeypatch.delenv("SP_WVD_CPR", raising=False)
    base = run(name, x, y).cpu().numpy()
    assert np.array_equal(base, run(name, x, y).cpu().numpy())
    default = E.wvd_plan(s["nfft"], s["nh"], s["ng"], s["hop"], s["ntimes"], rows=s["rows"], cross=cross, nb=s["nb"])["cpr"]
    for cpr in (1, 3, 2, 5):
        monkeypatch.setenv("SP_WVD_CPR", str(cpr))
        plan = E.wvd_plan(s["nfft"], s["nh"], s["ng"], s["hop"], s["ntimes"], rows=s["rows"], cross=cross, nb=s["nb"])
        assert plan["cpr"] == min(cpr, s["ntimes"])
        if not plan["fits"]:
            with pytest.raises(E.WvdRefused, match="LDS"):
                run(name, x, y)
            continue
        assert np.array_equal(base, run(name, x, y).cpu().numpy()), (name, cpr, default)
    monkeypatch.delenv("SP_WVD_CPR")


def test_symmetries(torch):
    name = "n256-band-wraps"
    x, y = on_device(torch, name), on_device(torch, name, 1)
    s = R.SHAPES[name]
    xy, yx, xx, auto = (run(name, a, b).cpu().numpy() for a, b in ((x, y), (y, x), (x, x), (x, None)))
    ref = R.band(R.reference(name, True), s)
    R.assert_within(np.conj(yx), ref, "conj xwvd(y, x)")
    R.assert_within(xy, ref, "xwvd(x, y)")
    ref_auto = R.band(R.reference(name, False), s)
    R.assert_within(xx.real, ref_auto, "Re xwvd(x, x)")
    R.assert_within(auto, ref_auto, "spwvd(x)")
    bound = R.ALLOWANCE * np.max(np.abs(ref_auto), axis=-1, keepdims=True) + R.ABS_TERM * np.max(np.abs(ref_auto))
    assert np.all(np.abs(xx.imag) <= bound)


def test_frequency_marginal(torch):
    """sum_k W[j][k] = nfft scale h[0] sum_mu g[mu] |z[n_j + mu]|^2 on the device output (full band)"""
    from test_host_wvd import marginal
    for name in ("n32-full-lag", "n256-long-g"):
        s = R.SHAPES[name]
        h, g = (w.astype(np.float32).astype(np.float64) for w in R.windows_of(s))
        x = R.signals(name)[0]
        W = run(name, on_device(torch, name), scale=1.0 / s["nfft"]).cpu().numpy().astype(np.float64)
        want = marginal(x[0], h, g, s["hop"], s["first"], s["ntimes"], s["nfft"], 1.0 / s["nfft"])
        # nfft cells, each within the allowance of the column's largest |W| (<= the marginal: W / scale is a transform of K, K[0] its sum)
        big = np.max(np.abs(R.reference(name, False)[0]), axis=-1) / s["nfft"]
        bound = s["nfft"] * (R.ALLOWANCE * big + R.ABS_TERM * big.max())
        err = np.abs(W[0].sum(axis=-1) - want)
        print("%s: marginal off by at most %.3g of its bound" % (name, float(np.max(err / bound))))
        assert np.all(err <= bound)


def test_numpy_arrays_and_device_tensors_give_the_same_bits(torch):
    for name in ("n32-full-lag", "n2048-batch-pitch"):
        s = R.SHAPES[name]
        for cross in (False, True):
            xh, yh = R.signals(name)[0], R.signals(name)[1] if cross else None
            host = run(name, xh, yh)
            assert isinstance(host, np.ndarray)
            dev = run(name, on_device(torch, name), on_device(torch, name, 1) if cross else None)
            assert isinstance(dev, torch.Tensor) and dev.is_cuda
            assert np.array_equal(host, dev.cpu().numpy())
            # through the C entry: host pointers, mem = 0
            lib = _ffi.load_library()
            h, g = (np.ascontiguousarray(w, dtype=np.float32) for w in R.windows_of(s))
            xc = np.ascontiguousarray(xh)
            yc = np.ascontiguousarray(yh) if cross else None
            W = np.empty((s["rows"], s["ntimes"], s["nb"]), dtype=np.complex64 if cross else np.float32)
            _ffi.check(lib.sp_wvd(_ffi.ptr(xc), _ffi.ptr(yc), s["nsig"], s["nsig"], s["rows"], _ffi.ptr(h), s["nh"], _ffi.ptr(g), s["ng"],
                                  s["nfft"], s["hop"], s["first"], s["ntimes"], s["b0"], s["nb"], 1.0, _ffi.ptr(W), 0))
            assert np.array_equal(W, host)


@pytest.mark.parametrize("cross", (False, True), ids=("auto", "cross"))
def test_offset_pointers_inside_poisoned_buffers(torch, cross):
    """device-resident x, y and W at every natural-alignment offset: the guards stay intact and every interior word is written"""
    name = "n256-band-wraps"
    s = R.SHAPES[name]
    lib = _ffi.load_library()
    h, g = (np.ascontiguousarray(w, dtype=np.float32) for w in R.windows_of(s))
    ref = R.band(R.reference(name, cross), s)
    x0, y0 = (torch.as_tensor(np.array(a[0]), device="cuda") for a in R.signals(name))
    nout = s["ntimes"] * s["nb"]
    first = None
    for lx, ly, lw in ((0, 0, 0), (1, 0, 1), (0, 1, 2), (1, 1, 3)):
        if cross and lw > 1:
            lw -= 2                                  # complex64 outputs: the offsets 0 and 1
        xb, xv = G.poisoned_input(x0, lx)
        yb, yv = G.poisoned_input(y0, ly)
        snaps = G.snapshot(xb), G.snapshot(yb)
        wb, waddr = G.sentinel_output(nout, torch.complex64 if cross else torch.float32, lw, device="cuda")
        E._bind_stream(xv)
        _ffi.check(lib.sp_wvd(_ffi.ptr(xv.data_ptr()), _ffi.ptr(yv.data_ptr()) if cross else None, s["nsig"], s["nsig"], 1, _ffi.ptr(h),
                              s["nh"], _ffi.ptr(g), s["ng"], s["nfft"], s["hop"], s["first"], s["ntimes"], s["b0"], s["nb"], 1.0,
                              ctypes.c_void_p(waddr), 1))
        torch.cuda.synchronize()
        assert G.guards_intact(wb, lw, nout) and G.all_written(wb, lw, nout)
        assert G.unchanged(xb, snaps[0]) and G.unchanged(yb, snaps[1])
        got = G.interior_of(wb, lw, nout).cpu().numpy().reshape(1, s["ntimes"], s["nb"])
        assert np.all(np.isfinite(got.view(np.float32)))
        R.assert_within(got, ref, "offsets %d %d %d" % (lx, ly, lw))
        first = got if first is None else first
        assert np.array_equal(first, got)


def test_public_functions(torch):
    rng = np.random.default_rng(5)
    nsig, fs, nfft, hop = 500, 200.0, 128, 3
    n = np.arange(nsig)
    xr = (np.cos(2 * np.pi * (0.05 * n + 0.1 * n ** 2 / nsig)) + 0.1 * rng.standard_normal(nsig)).astype(np.float32)
    xc = (np.exp(2j * np.pi * (-0.1 * n + 0.1 * n ** 2 / nsig)) + 0.1 * rng.standard_normal(nsig)).astype(np.complex64)
    ntimes = (nsig - 1) // hop + 1
    # a real record: made analytic, bins over 0 .. fs/2
    f, t, W = WG.spwvd(xr, fs=fs, nfft=nfft, hop=hop)
    assert W.shape == (nfft, ntimes) and W.dtype == np.float32
    assert np.allclose(f, np.arange(nfft) * fs / (2 * nfft)) and np.allclose(t, hop * np.arange(ntimes) / fs)
    za = WG.analytic(xr)
    assert za.dtype == np.complex64 and np.array_equal(za, pyfft_hilbert(xr))
    h, g = WG._windows("t", None, None, nfft)
    ref = R.wvd_ref(za, h.astype(np.float32), g.astype(np.float32), hop, 0, ntimes, nfft, scale=1.0 / nfft).real
    R.assert_within(W.T, ref, "spwvd of a real record")
    inner = slice(30, ntimes - 30)
    ridge = np.argmax(W[:, inner], axis=0) * fs / (2 * nfft)
    assert np.max(np.abs(ridge - fs * (0.05 + 0.2 * (hop * np.arange(ntimes)[inner]) / nsig))) <= 1.5 * fs / (2 * nfft)
    # the device tensor takes the same path and gives the same bits
    fd, td, Wd = WG.spwvd(torch.as_tensor(xr, device="cuda"), fs=fs, nfft=nfft, hop=hop)
    assert isinstance(Wd, torch.Tensor) and np.array_equal(Wd.cpu().numpy(), W) and np.array_equal(fd, f)
    # a complex record: used as it is, signed frequencies in transform order
    f, t, W = WG.spwvd(xc, fs=fs, nfft=nfft, hop=hop)
    k = np.arange(nfft)
    assert np.allclose(f, np.where(k >= nfft // 2, k - nfft, k) * fs / (2 * nfft)) and W.shape == (nfft, ntimes)
    R.assert_within(W.T, R.wvd_ref(xc, h.astype(np.float32), g.astype(np.float32), hop, 0, ntimes, nfft, scale=1.0 / nfft).real, "spwvd, complex")
    # a band of signed frequencies wraps past the last bin
    fb, _, Wb = WG.spwvd(xc, fs=fs, nfft=nfft, hop=hop, band=(-10.0, 15.0))
    sel = (f >= -10.0 - 1e-9) & (f <= 15.0 + 1e-9)
    assert fb[0] < 0 < fb[-1] and np.all(np.diff(fb) > 0) and Wb.shape == (int(sel.sum()), ntimes)
    assert np.array_equal(Wb, np.concatenate((W[nfft // 2:][sel[nfft // 2:]], W[:nfft // 2][sel[:nfft // 2]])))
    # pwvd = spwvd without smoothing; wvd = pwvd under a rectangular lag window over the whole record
    _, _, P = WG.pwvd(xc, fs=fs, nfft=nfft, hop=hop)
    R.assert_within(P.T, R.wvd_ref(xc, h.astype(np.float32), np.ones(1), hop, 0, ntimes, nfft, scale=1.0 / nfft).real, "pwvd")
    f, t, V = WG.wvd(xc[:100], fs=fs)
    assert V.shape == (128, 100) and f.shape == (128,) and t.shape == (100,)
    R.assert_within(V.T, R.wvd_ref(xc[:100], np.ones(101), np.ones(1), 1, 0, 100, 128, scale=1.0 / 128).real, "wvd")
    # the cross distribution
    yc = np.roll(xc, 2)
    _, _, X = WG.xwvd(xc, yc, fs=fs, nfft=nfft, hop=hop)
    assert X.dtype == np.complex64 and X.shape == (nfft, ntimes)
    R.assert_within(X.T, R.wvd_ref(xc, h.astype(np.float32), g.astype(np.float32), hop, 0, ntimes, nfft, y=yc, scale=1.0 / nfft), "xwvd")
    # leading axes
    _, _, W2 = WG.spwvd(np.stack((xc, yc)), fs=fs, nfft=nfft, hop=hop)
    assert W2.shape == (2, nfft, ntimes) and np.array_equal(W2[0], WG.spwvd(xc, fs=fs, nfft=nfft, hop=hop)[2])


def test_auto_with_a_lag_window_that_is_not_symmetric_is_the_real_part(torch):
    """include/spectral_quad.h: the auto distribution is the real part of the definition, i.e. the one under the even part of h"""
    name = "n256-band-wraps"
    s = R.SHAPES[name]
    h, g = R.windows_of(s)
    h = (h * np.linspace(0.5, 1.5, s["nh"])).astype(np.float32)
    x = R.signals(name)[0]
    W = E.wvd(on_device(torch, name), h, g, s["hop"], s["first"], s["ntimes"], s["nfft"]).cpu().numpy()
    ref = R.wvd_ref(x[0], h, g.astype(np.float32), s["hop"], s["first"], s["ntimes"], s["nfft"])
    assert np.max(np.abs(ref.imag)) > 1e-2 * np.max(np.abs(ref.real))          # the definition itself is complex here
    R.assert_within(W[0], ref.real, "asymmetric h")
