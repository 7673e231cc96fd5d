"""GPU parity of the cascaded second-order sections (k_sos.hip through sp_sosfilt / sp_sosfiltfilt) against
scipy.signal in float64 on the float32-cast input.  Errors are measured per row against that row's max |y_ref|."""
import numpy as np
import pytest
import scipy.signal as ss

from conftest import load_golden

pytestmark = pytest.mark.gpu

TILE = 8192
NS = [1, 2, 8191, 8192, 8193, 3 * 8192 + 17, (1 << 20) + 3]


@pytest.fixture(scope="module")
def E():
    from pyfft_amd import engine, _ffi
    _ffi.init()
    return engine


@pytest.fixture(scope="module")
def F():
    from pyfft_amd import filters
    return filters


def rowerr(y, ref):
    y = np.asarray(y, dtype=np.float64).reshape(-1, np.shape(ref)[-1])
    ref = np.asarray(ref).reshape(y.shape)
    return float(np.max(np.max(np.abs(y - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-30)))


def designs(K):
    """K sections each: low-pass of order 2K at wn = 0.001 (K = 4: order 8), high-pass of order 2K at 0.1, band-pass
    of order K over the reference's default band [0.0005, 0.25] (K = 3: the reference's butter_bandpass)."""
    return {"lowpass": ss.butter(2 * K, 0.001, output="sos"),
            "highpass": ss.butter(2 * K, 0.1, btype="high", output="sos"),
            "bandpass": ss.butter(K, [0.0005, 0.25], btype="band", output="sos")}


@pytest.mark.parametrize("K", range(1, 9))
@pytest.mark.parametrize("kind", ["lowpass", "highpass", "bandpass"])
def test_sosfilt_grid(E, K, kind):
    sos = designs(K)[kind]
    assert sos.shape == (K, 6)
    rng = np.random.default_rng(100 * K + len(kind))
    for n in NS:
        for rows in (1, 3, 64):
            if n > (1 << 16) and rows == 64 and K not in (3, 8):
                continue                                          # (host time of the oracle)
            x = rng.standard_normal((rows, n)).astype(np.float32)
            y = E.sos_filter(sos, x)
            assert y.dtype == np.float32 and y.shape == x.shape
            err = rowerr(y, ss.sosfilt(sos, x.astype(np.float64), axis=-1))
            assert err <= 5e-7, (K, kind, n, rows, err)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_sosfilt_zi_pieces(E, K):
    sos = designs(K)["bandpass"]
    rng = np.random.default_rng(7 + K)
    n = 3 * TILE + 17
    x = rng.standard_normal((3, n)).astype(np.float32)
    x64 = x.astype(np.float64)
    zi = ss.sosfilt_zi(sos)[:, None, :] * x64[:, 0][None, :, None]       # (K, rows, 2)
    want, zf_want = ss.sosfilt(sos, x64, axis=-1, zi=zi)
    one, zf_one = E.sos_filter(sos, x, zi=zi)
    assert zf_one.shape == zi.shape
    assert rowerr(one, want) <= 1e-6
    cuts = [0, 5001, 17777, n]
    z = zi
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y, z = E.sos_filter(sos, np.ascontiguousarray(x[:, a:b]), zi=z)
        parts.append(y)
    assert rowerr(np.concatenate(parts, axis=1), want) <= 1e-6
    scale = np.abs(zf_want).max()
    assert np.abs(z - zf_want).max() <= 1e-6 * scale
    assert np.abs(zf_one - zf_want).max() <= 1e-6 * scale


@pytest.mark.parametrize("K", [2, 3, 8])
def test_sosfiltfilt_padtypes(E, F, K):
    sos = designs(K)["bandpass"]
    rng = np.random.default_rng(40 + K)
    for n, rows in ((3 * TILE + 17, 3), (2 * TILE, 2), (5000, 4)):
        x = rng.standard_normal((rows, n)).astype(np.float32)
        x64 = x.astype(np.float64)
        for padtype in ("odd", "even", "constant", None):
            y = F.sosfiltfilt(sos, x, padtype=padtype)
            err = rowerr(y, ss.sosfiltfilt(sos, x64, padtype=padtype))
            assert err <= 5e-7, (K, n, padtype, err)
        y = F.sosfiltfilt(sos, x, padlen=100)
        assert rowerr(y, ss.sosfiltfilt(sos, x64, padlen=100)) <= 5e-7
    padlen = F._sos_padlen(sos)
    x = rng.standard_normal((2, padlen + 1)).astype(np.float32)
    assert rowerr(F.sosfiltfilt(sos, x), ss.sosfiltfilt(sos, x.astype(np.float64))) <= 5e-7


def test_sosfiltfilt_lowpass_order8(E, F):
    sos = ss.butter(8, 0.001, output="sos")
    x = np.random.default_rng(5).standard_normal((2, 3 * TILE + 5)).astype(np.float32)
    assert rowerr(F.sosfiltfilt(sos, x), ss.sosfiltfilt(sos, x.astype(np.float64))) <= 5e-7


def test_tf_forms_well_conditioned(E, F):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 20000)).astype(np.float32)
    x64 = x.astype(np.float64)
    for b, a in (ss.butter(5, 0.02), ss.butter(5, 0.2), ss.butter(3, [0.0005, 0.25], btype="band"),
                 ss.butter(4, 0.3, btype="high"), ss.butter(2, [0.05, 0.1], btype="band")):
        assert rowerr(F.lfilter(b, a, x), ss.lfilter(b, a, x64)) <= 2e-6
        assert rowerr(F.filtfilt(b, a, x), ss.filtfilt(b, a, x64)) <= 2e-6
        assert rowerr(F.filtfilt(b, a, x.T, axis=0).T, ss.filtfilt(b, a, x64)) <= 2e-6


def test_reference_functions_against_fixture(E, F):
    import pyfft_amd
    g = load_golden("filters")
    x = g["bp_x"]
    assert rowerr(pyfft_amd.butter_bandpass(x.astype(np.float64)), g["bp_default"]) <= 2e-6
    fs, lf, hf, order = g["bp_other_args"]
    assert rowerr(F.butter_bandpass(x, fs=fs, lf=lf, hf=hf, order=int(order)), g["bp_other"]) <= 2e-6
    cutoff, fs, order = g["lpf_args"]
    y = pyfft_amd.butter_lowpass_filter(g["lpf_x"], cutoff, fs, order=int(order), axis=0)
    assert y.shape == g["lpf_y"].shape
    assert rowerr(y.T, g["lpf_y"].T) <= 2e-6
    z = F.complex_filtfilt(g["cf_b"], g["cf_a"], g["cf_x"])
    assert np.iscomplexobj(z)
    ref = g["cf_y"]
    assert np.abs(z - ref).max() <= 2e-6 * np.abs(ref).max()


def test_device_tensors_stay_on_device(E, F):
    import torch
    sos = designs(3)["bandpass"]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 3 * TILE + 17)).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    y = E.sos_filter(sos, xt)
    assert y.is_cuda and y.dtype == torch.float32
    np.testing.assert_array_equal(y.cpu().numpy(), E.sos_filter(sos, x))
    y = F.sosfiltfilt(sos, xt)
    assert y.is_cuda
    np.testing.assert_array_equal(y.cpu().numpy(), F.sosfiltfilt(sos, x))
    zi = ss.sosfilt_zi(sos)[:, None, :] * np.ones((1, 3, 1))
    y, zf = E.sos_filter(sos, xt, zi=torch.from_numpy(zi).cuda())
    assert y.is_cuda and zf.is_cuda
    y_np, zf_np = E.sos_filter(sos, x, zi=zi)
    np.testing.assert_array_equal(y.cpu().numpy(), y_np)
    np.testing.assert_array_equal(zf.cpu().numpy(), zf_np)
    z = (x[0] + 1j * x[1]).astype(np.complex64)
    zt = torch.from_numpy(z).cuda()
    w = F.sosfiltfilt(sos, zt)
    assert w.is_cuda and w.dtype == torch.complex64
    np.testing.assert_array_equal(w.cpu().numpy(), F.sosfiltfilt(sos, z))
    assert rowerr(np.stack([w.cpu().numpy().real, w.cpu().numpy().imag]),
                  np.stack([ss.sosfiltfilt(sos, x[0].astype(np.float64)), ss.sosfiltfilt(sos, x[1].astype(np.float64))])) <= 5e-7
    x64 = torch.from_numpy(x.astype(np.float64)).cuda()
    y = E.sos_filter(sos, x64)
    assert y.is_cuda and y.dtype == torch.float64


def chain_threads(K):
    """workgroup of k_sos_chain: a row's tiles are split over it, `per` consecutive tiles per thread"""
    return 1024 if K <= 3 else 512 if K <= 6 else 256


@pytest.mark.parametrize("K", range(1, 9))
def test_chain_several_tiles_per_thread(E, F, K):
    """Rows long enough that every chain thread carries several tiles (per = 5: not a multiple of the chain's batch of
    tile states, U = 8 at K <= 2 and 4 above), causal with zi / zf and zero-phase."""
    ct = chain_threads(K)
    nt = 4 * ct + 37                                      # per = ceil(nt / ct) = 5, the last threads partly past the row
    n = (nt - 1) * TILE + 101
    assert -(-n // TILE) == nt and -(-nt // ct) == 5
    sos = designs(K)["bandpass"]
    x = np.random.default_rng(500 + K).standard_normal((1, n)).astype(np.float32)
    x64 = x.astype(np.float64)
    zi = ss.sosfilt_zi(sos)[:, None, :] * 0.5
    y, zf = E.sos_filter(sos, x, zi=zi)
    want, zf_want = ss.sosfilt(sos, x64, axis=-1, zi=zi)
    assert rowerr(y, want) <= 5e-7
    assert np.abs(zf - zf_want).max() <= 1e-6 * np.abs(zf_want).max()
    del y, want
    assert rowerr(F.sosfiltfilt(sos, x), ss.sosfiltfilt(sos, x64)) <= 5e-7


def test_complex_input_real_zi(E):
    """A real zi with complex samples is the real parts' state (scipy's convention); the imaginary parts start from rest:
    numpy and device tensors alike."""
    import torch
    sos = designs(2)["highpass"]
    rng = np.random.default_rng(9)
    z = (rng.standard_normal((2, 3 * TILE + 7)) + 1j * rng.standard_normal((2, 3 * TILE + 7))).astype(np.complex64)
    zi = rng.standard_normal((2, 2, 2))
    want, zf_want = ss.sosfilt(sos, z.astype(np.complex128), axis=-1, zi=zi)
    y, zf = E.sos_filter(sos, z, zi=zi)
    assert np.abs(y - want).max() <= 5e-7 * np.abs(want).max()
    assert np.abs(zf - zf_want).max() <= 1e-6 * np.abs(zf_want).max()
    yt, zft = E.sos_filter(sos, torch.from_numpy(z).cuda(), zi=torch.from_numpy(zi).cuda())
    assert yt.is_cuda and yt.dtype == torch.complex64 and zft.is_cuda
    np.testing.assert_array_equal(yt.cpu().numpy(), y)
    np.testing.assert_array_equal(zft.cpu().numpy(), zf)


def test_refusals_on_device_path(E, F):
    import torch
    from pyfft_amd import _ffi
    xt = torch.zeros((2, 100), device="cuda")
    good = ss.butter(3, 0.1, output="sos")
    unstable = good.copy()
    unstable[0, 3:] = [1.0, -2.2, 1.21]
    with pytest.raises(ValueError):
        E.sos_filter(unstable, xt)
    with pytest.raises(ValueError):
        E.sos_filter(np.tile(good[:1], (9, 1)), xt)
    with pytest.raises(ValueError):
        E.sos_filtfilt(good, xt, "odd", 100)
    # the library itself, device pointers (mem = 1): -1 and the reason, nothing launched
    yt = torch.empty_like(xt)
    lib = _ffi.lib()
    s = np.ascontiguousarray(unstable)
    assert lib.sp_sosfilt(_ffi.ptr(s), 2, _ffi.ptr(xt.data_ptr()), 2, 100, None, _ffi.ptr(yt.data_ptr()), None, 1) == -1
    assert b"unstable" in lib.sp_last_error()
    s = np.ascontiguousarray(np.tile(good[:1], (9, 1)))
    assert lib.sp_sosfilt(_ffi.ptr(s), 9, _ffi.ptr(xt.data_ptr()), 2, 100, None, _ffi.ptr(yt.data_ptr()), None, 1) == -1
    s = np.ascontiguousarray(good)
    assert lib.sp_sosfiltfilt(_ffi.ptr(s), 2, _ffi.ptr(xt.data_ptr()), 2, 100, 1, 100, _ffi.ptr(yt.data_ptr()), 1) == -1
    assert b"padlen" in lib.sp_last_error()


def test_full_size_reference_bandpass(E, F):
    """2^28 float32 samples: zero-phase against whole-record sosfiltfilt, causal against chunked sosfilt with zi carried."""
    n = 1 << 28
    sos = ss.butter(3, [0.0005, 0.25], btype="band", output="sos")
    x = np.random.default_rng(28).standard_normal(n, dtype=np.float32)
    y = F.sosfiltfilt(sos, x)
    ref = ss.sosfiltfilt(sos, x.astype(np.float64))
    err = float(np.abs(y - ref).max() / np.abs(ref).max())
    del ref
    assert err <= 5e-7, err
    y = F.sosfilt(sos, x)
    z = np.zeros((3, 2))
    worst, peak = 0.0, 0.0
    step = 1 << 24
    for a in range(0, n, step):
        r, z = ss.sosfilt(sos, x[a:a + step].astype(np.float64), zi=z)
        worst = max(worst, float(np.abs(y[a:a + step] - r).max()))
        peak = max(peak, float(np.abs(r).max()))
    assert worst <= 5e-7 * peak, worst / peak
