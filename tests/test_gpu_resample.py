"""The rational resampler on the MI355X: sp_upfirdn against upfirdn_ref of tests/test_host_resample.py (float64), resample_poly against
scipy.signal.resample_poly on the float64 input, and against the existing decimator.
Bounds, the convention of tests/test_gpu_baseband.py: the maximum error over the rms of the reference is at most 4 x what a float32 numpy
restatement of the same sum (samples and taps rounded to float32, taps accumulated in ascending order in float32) loses on the same
input; the factor covers another summation order.  The restatement itself must lose between 0 and 1e-4.  Where a padtype takes a
background off the rows, the rms is that of the reference without the background."""
import numpy as np
import pytest
import scipy.signal as ss

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E, resample as RS                                          # noqa: E402
from test_host_multitaper import make_signal                                                    # noqa: E402
from test_host_resample import upfirdn_ref, resample_poly_ref, resample_poly_parts, pad_kw, PADTYPES   # noqa: E402
from test_gpu_zoom import samples                                                               # noqa: E402
from test_gpu_baseband import ddc_f32, taps32                                                   # noqa: E402


def rows(n, cplx, seed, nrows=2):
    return np.stack([make_signal(n, cplx, seed + 7 * r) for r in range(nrows)])


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def strided(x):
    """The rows on the device with a row stride of n + 11."""
    import torch
    xs = _ffi.as_samples(x)
    base = torch.zeros((xs.shape[0], xs.shape[1] + 11), dtype=torch.complex64 if np.iscomplexobj(xs) else torch.float32, device="cuda")
    base[:, :xs.shape[1]] = torch.as_tensor(xs, device="cuda")
    view = base[:, :xs.shape[1]]
    assert view.stride(0) == xs.shape[1] + 11
    return view


def loss_of(ref, f32, what, rms=None):
    rms = float(np.sqrt(np.mean(np.abs(ref) ** 2))) if rms is None else rms
    loss = float(np.max(np.abs(f32.astype(ref.dtype) - ref))) / rms
    print("%s float32 restatement loses %.3g of the rms" % (what, loss))
    assert 0 < loss < 1e-4                                                   # a guard on the restatement itself, not the bound
    return rms, loss


def check_against(got, ref, f32, what, rms=None):
    rms, loss = loss_of(ref, f32, what, rms)
    got = host(got)
    assert got.shape == ref.shape and got.dtype == (np.complex64 if np.iscomplexobj(ref) else np.float32), what
    err = float(np.max(np.abs(got.astype(ref.dtype) - ref))) / rms
    print("%s max err / rms = %.3g (bound %.3g)" % (what, err, 4.0 * loss))
    assert err <= 4.0 * loss, what


def both_ways(x):
    """The numpy path and the device-resident, row-strided path."""
    return (("numpy", _ffi.as_samples(x)), ("device", strided(x)))


FACTORS = [2, 3, 7, 64, 256]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_identity_is_bit_exact(cplx):
    n = 2 * E.upfirdn_tile(1, 1, 1, cplx) + 905
    x = _ffi.as_samples(rows(n, cplx, 71))
    for name, xx in both_ways(x):
        got = host(E.upfirdn(xx, [1.0], 1, 1))
        assert got.dtype == x.dtype and got.shape == x.shape and got.tobytes() == x.tobytes(), name


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("L", FACTORS)
def test_zero_stuffing_and_hold_are_bit_exact(L, cplx):
    """up = L: h = [1] puts the input on every L-th output with exact zeros between, h = ones(L) holds every sample L times."""
    n = (2 * E.upfirdn_tile(L, 1, L, cplx) + 905) // L + 3
    x = _ffi.as_samples(rows(n, cplx, 72))
    stuffed = np.zeros((x.shape[0], (n - 1) * L + 1), dtype=x.dtype)
    stuffed[:, ::L] = x
    held = np.repeat(x, L, axis=-1)
    assert stuffed.shape[-1] > 2 * E.upfirdn_tile(L, 1, 1, cplx)
    for name, xx in both_ways(x):
        got = host(E.upfirdn(xx, [1.0], L, 1))
        assert got.dtype == x.dtype and got.shape == stuffed.shape and got.tobytes() == stuffed.tobytes(), name
        got = host(E.upfirdn(xx, np.ones(L), L, 1))
        assert got.shape == held.shape and got.tobytes() == held.tobytes(), name


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("q", FACTORS)
def test_decimation_is_bit_exact(q, cplx):
    n = (2 * E.upfirdn_tile(1, q, 1, cplx) + 9) * q + 5
    x = _ffi.as_samples(rows(n, cplx, 73))
    want = np.ascontiguousarray(x[:, ::q])
    for name, xx in both_ways(x):
        got = host(E.upfirdn(xx, [1.0], 1, q))
        assert got.dtype == x.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), name


SHAPES = [(2, 1, 5), (3, 2, 31), (2, 3, 30), (7, 5, 141), (64, 63, 257), (160, 147, 3201), (5, 64, 1281), (1, 256, 5121), (256, 1, 5121),
          (255, 256, 8191)]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("up,down,T", SHAPES, ids=["%d-%d-T%d" % s for s in SHAPES])
def test_parity(up, down, T, cplx):
    """Two rows over more than two tiles and an odd remainder, the full output; numpy, one row, and device-resident at a row stride of
    n + 11."""
    K = E.upfirdn_tile(up, down, T, cplx)
    n = -(-(2 * K + 37) * down // up)
    x = rows(n, cplx, 74)
    h = ss.firwin(T, 1.0 / max(up, down)) * up
    ref = upfirdn_ref(taps32(h), samples(x), up, down)
    f32 = upfirdn_ref(h, _ffi.as_samples(x), up, down, dtype=np.float32)
    assert ref.shape == (2, -(-((n - 1) * up + T) // down)) and ref.shape[-1] > 2 * K and ref.shape[-1] % K
    check_against(E.upfirdn(x, h, up, down), ref, f32, "numpy")
    check_against(E.upfirdn(x[1], h, up, down), ref[1], f32[1], "numpy, one row")
    out = E.upfirdn(strided(x), h, up, down)
    assert out.is_cuda
    check_against(out, ref, f32, "device, x_ld = n + 11")
    check_against(RS.upfirdn(h, x.T, up, down, axis=0), ref.T, f32.T, "resample.upfirdn(axis=0)")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_short_records_and_windows(cplx):
    """A record shorter than one filter span; a single sample; a window of outputs that starts inside one tile, crosses into the next
    and runs past the full length, where the outputs are exactly zero."""
    for up, down, T, n in ((3, 2, 31, 5), (5, 64, 1281, 40), (7, 5, 141, 1), (1, 4, 9, 1)):
        x = rows(n, cplx, 75)
        h = ss.firwin(T, 1.0 / max(up, down)) * up
        ref = upfirdn_ref(taps32(h), samples(x), up, down)
        f32 = upfirdn_ref(h, _ffi.as_samples(x), up, down, dtype=np.float32)
        check_against(E.upfirdn(x, h, up, down), ref, f32, "%d/%d T %d n %d numpy" % (up, down, T, n))
        check_against(E.upfirdn(strided(x), h, up, down), ref, f32, "%d/%d T %d n %d device" % (up, down, T, n))
    up, down, T = 3, 2, 31
    K = E.upfirdn_tile(up, down, T, cplx)
    n = -(-(2 * K + 500) * down // up)
    full = -(-((n - 1) * up + T) // down)
    m0, nout = K - 100, full - (K - 100) + 333
    assert nout > K and m0 + nout > full                 # the tiles of a call start at m0: this window takes two
    x = rows(n, cplx, 76)
    h = ss.firwin(T, 1.0 / up) * up
    ref = upfirdn_ref(taps32(h), samples(x), up, down, m0, nout)
    f32 = upfirdn_ref(h, _ffi.as_samples(x), up, down, m0, nout, dtype=np.float32)
    assert np.all(ref[:, -333:] == 0) and np.any(ref[:, -334] != 0)
    for name, xx in both_ways(x):
        got = host(E.upfirdn(xx, h, up, down, m0=m0, nout=nout))
        check_against(got, ref, f32, "window, " + name)
        assert np.all(got[:, -333:] == 0)
    assert E.upfirdn(x, h, up, down, m0=full + 5).shape == (2, 0)


@pytest.mark.parametrize("up,down,T", [(3, 2, 61), (1, 64, 1281), (160, 147, 3201)])
def test_two_runs_agree_bitwise(up, down, T):
    K = E.upfirdn_tile(up, down, T, True)
    x = strided(rows(-(-(2 * K + 37) * down // up), True, 77))
    h = ss.firwin(T, 1.0 / max(up, down)) * up
    a, b = E.upfirdn(x, h, up, down), E.upfirdn(x, h, up, down)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert host(E.upfirdn(host(x), h, up, down)).tobytes() == a.cpu().numpy().tobytes()


def check_poly(x, up, down, what, axis=-1, device=True, **kw):
    """resample_poly, numpy in (checked here) and device tensor in (returned), against scipy on the float64 input."""
    import torch
    want = ss.resample_poly(x, up, down, axis=axis, **kw)
    core, _ = resample_poly_parts(np.moveaxis(x, axis, -1), up, down, **kw)
    rms = float(np.sqrt(np.mean(np.abs(core) ** 2)))
    f32 = resample_poly_ref(x, up, down, axis=axis, dtype=np.float32, **kw)
    check_against(RS.resample_poly(x, up, down, axis=axis, **kw), want, f32, what + ", numpy", rms)
    out = RS.resample_poly(torch.as_tensor(_ffi.as_samples(x), device="cuda"), up, down, axis=axis, **kw) if device else None
    assert out is None or out.is_cuda
    return want, f32, rms, out


POLY = [(3, 2, 6000), (2, 3, 9000), (160, 147, 8000), (4, 1, 2100), (1, 4, 9000)]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("up,down,n", POLY, ids=["%d-%d" % s[:2] for s in POLY])
def test_resample_poly_default_window(up, down, n, cplx):
    x = rows(n, cplx, 78)
    want, f32, rms, out = check_poly(x, up, down, "%d/%d" % (up, down))
    assert want.shape[-1] > 2 * RS.resample_plan(n, up, down, cplx=cplx)["tile"]
    check_against(out, want, f32, "device", rms)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_resample_poly_taps_unreduced_and_axis(cplx):
    x = rows(3000, cplx, 79)
    h = ss.firwin(45, 0.3, window="hamming")
    want, f32, rms, out = check_poly(x, 3, 2, "taps array", window=h)
    check_against(out, want, f32, "taps array, device", rms)
    want, f32, rms, out = check_poly(x, 6, 4, "unreduced 6/4")
    check_against(out, want, f32, "unreduced 6/4, device", rms)
    assert np.array_equal(host(out), host(RS.resample_poly(x, 3, 2, axis=-1)))
    want, f32, rms, out = check_poly(np.ascontiguousarray(x.T), 2, 3, "axis 0", axis=0)
    assert want.shape == (2000, 2)
    check_against(out, want, f32, "axis 0, device", rms)
    y, fs_out = RS.resample_rate(x, 44100.0, 48000.0)
    assert fs_out == 48000.0 and y.shape == (2, 3266)
    f32 = resample_poly_ref(x, 160, 147, axis=-1, dtype=np.float32)
    check_against(y, ss.resample_poly(x, 160, 147, axis=-1), f32, "resample_rate")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("padtype", PADTYPES)
def test_resample_poly_padtypes(padtype, cplx):
    """An offset of 1e3: where the padtype takes it off the rows, the error is measured against what is left."""
    x = rows(3000, cplx, 80) + 1e3
    kw = pad_kw(padtype)
    want, f32, rms, _ = check_poly(x, 3, 2, padtype, device=False, **kw)
    assert (rms > 500) == (padtype == "constant")
    if not (cplx and padtype in ("median", "minimum", "maximum")):
        # the device tensor is float32 already: the offset has cost it bits before the background goes, so it is held to scipy on
        # the same float32 samples
        import torch
        xs = _ffi.as_samples(x)
        want = ss.resample_poly(samples(x), 3, 2, axis=-1, **kw)
        f32 = resample_poly_ref(xs, 3, 2, axis=-1, dtype=np.float32, **kw)
        check_against(RS.resample_poly(torch.as_tensor(xs, device="cuda"), 3, 2, axis=-1, **kw), want, f32, padtype + ", device", rms)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("q,T", [(4, 81), (64, 1281)])
def test_agrees_with_the_decimator(q, T, cplx):
    """resample_poly(x, 1, q, window=h) and engine.ddc(x, 0, q, h) compute the same sum with different kernels: they differ by at
    most the sum of their two bounds."""
    n = q * (2 * max(E.upfirdn_tile(1, q, T + q, cplx), E.ddc_tile(q)) + 77) + 3
    x = rows(n, cplx, 81)
    h = ss.firwin(T, 0.8 / q)
    ref = resample_poly_ref(samples(x), 1, q, axis=-1, window=taps32(h))
    np.testing.assert_allclose(ref, ss.resample_poly(samples(x), 1, q, axis=-1, window=taps32(h)), rtol=0, atol=1e-12 * np.abs(ref).max())
    rms, loss_a = loss_of(ref, resample_poly_ref(_ffi.as_samples(x), 1, q, axis=-1, window=h, dtype=np.float32), "upfirdn")
    f32 = ddc_f32(x, 0.0, q, h)
    _, loss_b = loss_of(ref, f32 if cplx else f32.real, "ddc")
    a = RS.resample_poly(x, 1, q, axis=-1, window=h)
    b = E.ddc(x, 0.0, q, h)
    b = b if cplx else b.real
    assert a.shape == b.shape == ref.shape and a.dtype == (np.complex64 if cplx else np.float32)
    diff = float(np.max(np.abs(a.astype(ref.dtype) - b.astype(ref.dtype)))) / rms
    print("q %d: resample_poly - ddc = %.3g of the rms (bound %.3g)" % (q, diff, 4 * loss_a + 4 * loss_b))
    assert diff <= 4 * loss_a + 4 * loss_b
    check_against(a, ref, resample_poly_ref(_ffi.as_samples(x), 1, q, axis=-1, window=h, dtype=np.float32), "resample_poly")


def test_refusals_through_the_raw_abi():
    """rc < 0, sp_last_error() names sp_upfirdn, and a poisoned output buffer is unchanged."""
    _ffi.init()
    lib, p = _ffi.lib(), _ffi.ptr
    x = np.ones(4096, dtype=np.float32)
    out = np.full(8192, 7.25, dtype=np.float32)
    h = np.ones(8192, dtype=np.float32)
    bad_h = h.copy()
    bad_h[17] = np.inf
    nan_h = h.copy()
    nan_h[3] = np.nan
    ok = dict(dtype=0, nsig=1024, ld=1024, batch=2, ntaps=31, up=3, down=2, m0=5, nout=1000, xp=x, hp=h, op=out)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_upfirdn(p(a["xp"]), a["dtype"], a["nsig"], a["ld"], a["batch"], p(a["hp"]), a["ntaps"], a["up"], a["down"],
                              a["m0"], a["nout"], p(a["op"]), 0)
    cases = [dict(dtype=2), dict(dtype=-1), dict(nsig=0), dict(nsig=-5), dict(ld=1023), dict(up=0), dict(up=257), dict(down=0),
             dict(down=257), dict(up=-3), dict(ntaps=0), dict(ntaps=8192), dict(ntaps=-1), dict(hp=bad_h), dict(hp=nan_h), dict(m0=-1),
             dict(nout=-1), dict(batch=-1), dict(m0=1 << 61), dict(nout=1 << 61), dict(m0=(1 << 61) - 500),
             dict(batch=1 << 40, nout=1 << 40), dict(batch=1 << 20, nout=1 << 24), dict(xp=None), dict(hp=None), dict(op=None)]
    for kw in cases:
        assert call(**kw) < 0, kw
        msg = lib.sp_last_error().decode()
        assert "sp_upfirdn" in msg, (kw, msg)
    assert np.all(out == 7.25)
    assert call(nout=0) == 0 and call(batch=0) == 0 and call(nout=0, op=None) == 0 and np.all(out == 7.25)
    assert call() == 0 and not np.any(out[:2000] == 7.25) and np.all(out[2000:] == 7.25)       # the same call with good arguments
    with pytest.raises(ValueError):
        E.upfirdn(x, h[:5], 257, 1)
    with pytest.raises(ValueError):
        E.upfirdn(x, h[:5] * 1j, 2, 1)
    with pytest.raises(ValueError):
        E.upfirdn(x, h[:5], 2, 1, m0=-1)
