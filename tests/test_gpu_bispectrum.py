"""Bispectrum / bicoherence on the GPU against the float64 oracle of tests/test_host_bispectrum.py."""
import ctypes

import numpy as np
import pytest

import pyfft_amd
from pyfft_amd import _ffi, engine as E
from test_host_bispectrum import make_signal, oracle_bispectrum, oracle_finish, oracle_spectra, oracle_sums

pytestmark = pytest.mark.gpu


def hann(nfft):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)


def frames_signal(nfft, hop, M, cplx, seed):
    return make_signal((M - 1) * hop + nfft + hop // 3, cplx, seed)


def assert_parity(B, b2, Bo, b2o, A):
    ok = ~np.isnan(Bo)
    np.testing.assert_array_equal(np.isnan(B), ~ok)
    np.testing.assert_array_equal(np.isnan(b2), ~ok)
    err = np.abs(B[ok] - Bo[ok])
    bound = 1e-4 * A[ok] + 1e-6 * np.nanmax(A)
    assert np.all(err <= bound), "max |dB| / bound = %.3g" % float(np.max(err / bound))
    np.testing.assert_allclose(b2[ok], b2o[ok], rtol=0, atol=2e-4)


# (kind, nfft, frames): real auto / real cross / complex auto, every nfft and frame count of the grid without the pairs whose
# float64 oracle would take minutes (nb^2 x frames)
CASES = [(k, n, m) for k in ("real", "cross", "cplx") for n, m in
         [(8, 1), (8, 2), (8, 3000), (64, 255), (64, 256), (64, 257), (64, 3000), (257, 2), (257, 256), (257, 257),
          (1000, 1), (1000, 255), (1024, 2), (1024, 257), (4096, 1), (4096, 2)]]


@pytest.mark.parametrize("detrend", [0, 1, 2])
@pytest.mark.parametrize("kind,nfft,M", CASES)
def test_parity_with_oracle(kind, nfft, M, detrend):
    if kind == "cplx" and nfft >= 1000 and M > 2:
        M = 20                                  # nb = nfft: keep the oracle's nb^2 M in reach
    cplx = kind == "cplx"
    hop = nfft - nfft // 3
    seed = nfft * 7 + M
    x = frames_signal(nfft, hop, M, cplx, seed)
    y = z = None
    if kind == "cross":
        y = frames_signal(nfft, hop, M, cplx, seed + 1)
        z = frames_signal(nfft, hop, M, cplx, seed + 2)
    win = hann(nfft)
    B, b2, P = E.bispectrum(x, win, hop, M, y=y, z=z, detrend=detrend)
    Bo, b2o, A, Po = oracle_bispectrum(x, win, hop, M, y, z, detrend)
    assert_parity(B, b2, Bo, b2o, A)
    np.testing.assert_allclose(P, Po, rtol=1e-5, atol=1e-7 * Po.max())


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("nfft", [64, 1000])
def test_exact_properties(cplx, nfft):
    hop = nfft // 2
    win = hann(nfft)
    x = frames_signal(nfft, hop, 300, cplx, 11)
    M = 1 + (x.size - nfft) // hop
    ok = pyfft_amd._bispectrum_mod.valid_region(nfft, cplx)
    # one frame: |B|^2 = D P exactly in real arithmetic, wherever the denominator is not 0
    B1, b21, _ = E.bispectrum(x, win, hop, 1)
    Bo, _, _, _ = oracle_bispectrum(x, win, hop, 1)
    live = ok & (np.abs(Bo) > 1e-12 * np.nanmax(np.abs(Bo)))
    assert live.sum() > 0.9 * ok.sum()
    np.testing.assert_allclose(b21[live], 1.0, rtol=0, atol=1e-5)
    # range, NaN exactly outside, symmetry, determinism
    B, b2, _ = E.bispectrum(x, win, hop, M)
    assert np.all(np.isnan(b2[~ok])) and np.all(np.isnan(B[~ok]))
    assert not np.any(np.isnan(b2[ok])) and not np.any(np.isnan(B[ok]))
    assert np.all(b2[ok] >= 0) and np.all(b2[ok] <= 1 + 1e-5)
    assert np.array_equal(B, B.T, equal_nan=True) and np.array_equal(b2, b2.T, equal_nan=True)
    B_again, b2_again, _ = E.bispectrum(x, win, hop, M)
    assert np.array_equal(B.view(np.float64), B_again.view(np.float64), equal_nan=True)
    assert np.array_equal(b2, b2_again, equal_nan=True)
    # the auto path (j <= i tiles, mirrored) against the cross path on three copies
    Bc, b2c, _ = E.bispectrum(x, win, hop, M, y=x, z=x)
    np.testing.assert_allclose(Bc[ok], B[ok], rtol=0, atol=1e-6 * np.max(np.abs(B[ok])))
    np.testing.assert_allclose(b2c[ok], b2[ok], rtol=0, atol=1e-5)


def test_public_wrappers():
    fs, nfft = 1000.0, 128
    x = make_signal(40 * nfft, False, 5)
    f1, f2, B, b2 = pyfft_amd.bispectrum(x, fs=fs, nfft=nfft)
    np.testing.assert_array_equal(f1, np.fft.rfftfreq(nfft, 1 / fs))
    np.testing.assert_array_equal(f2, f1)
    hop = nfft // 2
    M = 1 + (x.size - nfft) // hop
    win = pyfft_amd._bispectrum_mod.get_window("hanning", nfft)
    Bo, b2o, A, _ = oracle_bispectrum(x, win, hop, M, detrend=1)
    assert_parity(B, b2, Bo, b2o, A)
    g1, g2, c2 = pyfft_amd.bicoherence(x, fs=fs, nfft=nfft)
    assert np.array_equal(c2, b2, equal_nan=True)
    xc = make_signal(40 * nfft, True, 6)
    f1, _, B, _ = pyfft_amd.bispectrum(xc, fs=fs, nfft=nfft, noverlap=0, window=np.ones(nfft), detrend="linear")
    np.testing.assert_array_equal(f1, np.fft.fftshift(np.fft.fftfreq(nfft, 1 / fs)))
    Bo, _, A, _ = oracle_bispectrum(xc, np.ones(nfft), nfft, 40, detrend=2)
    ok = ~np.isnan(Bo)
    assert np.all(np.abs(B[ok] - Bo[ok]) <= 1e-4 * A[ok] + 1e-6 * np.nanmax(A))


def test_quadratic_phase_coupling():
    nfft, M = 256, 400
    rng = np.random.default_rng(3)
    t = np.arange(nfft)
    k1, k2, q1, q2 = 20, 33, 41, 57           # coupled triad (k1, k2, k1 + k2); independent triad (q1, q2, q1 + q2)
    segs = []
    for _ in range(M):
        a1, a2, b1, b2_, b3 = rng.uniform(0, 2 * np.pi, 5)
        s = (np.cos(2 * np.pi * k1 * t / nfft + a1) + np.cos(2 * np.pi * k2 * t / nfft + a2)
             + np.cos(2 * np.pi * (k1 + k2) * t / nfft + a1 + a2)
             + np.cos(2 * np.pi * q1 * t / nfft + b1) + np.cos(2 * np.pi * q2 * t / nfft + b2_)
             + np.cos(2 * np.pi * (q1 + q2) * t / nfft + b3) + 0.1 * rng.standard_normal(nfft))
        segs.append(s)
    x = np.concatenate(segs).astype(np.float32)
    f1, f2, b2 = pyfft_amd.bicoherence(x, fs=1.0, nfft=nfft, noverlap=0, window=np.ones(nfft), detrend="none")
    assert b2[k1, k2] > 0.9 and b2[k2, k1] > 0.9
    assert b2[q1, q2] < 0.1


def test_size_2_24_many_chunks(monkeypatch):
    monkeypatch.setenv("SP_BISPEC_MIB", "32")        # several spectra chunks (and many 256-frame chunks in each)
    nfft, hop = 512, 256
    n = 1 << 24
    x = make_signal(n, False, 9)
    win = hann(nfft)
    M = 1 + (n - nfft) // hop
    B, b2, P = E.bispectrum(x, win, hop, M)
    nb = nfft // 2 + 1
    ok = pyfft_amd._bispectrum_mod.valid_region(nfft, False)
    assert np.all(np.isnan(b2[~ok])) and not np.any(np.isnan(b2[ok]))
    assert np.all(b2[ok] >= 0) and np.all(b2[ok] <= 1 + 1e-5)
    assert np.array_equal(B, B.T, equal_nan=True)
    rows = np.arange(3, nb, nb // 8)[:8]
    sums = None
    for f0 in range(0, M, 8192):
        m = min(8192, M - f0)
        X = oracle_spectra(x, win, nfft, hop, m, 1, f0=f0)
        s = oracle_sums(X, X, X, 0, rows)
        sums = s if sums is None else tuple(a + b for a, b in zip(sums, s))
    Bo, b2o, A, Po = oracle_finish(*sums, M, 0, rows)
    ok_r = ~np.isnan(Bo)
    err = np.abs(B[rows][ok_r] - Bo[ok_r])
    bound = 1e-4 * A[ok_r] + 1e-6 * np.nanmax(A)
    assert np.all(err <= bound), "max |dB| / bound = %.3g" % float(np.max(err / bound))
    np.testing.assert_allclose(b2[rows][ok_r], b2o[ok_r], rtol=0, atol=2e-4)
    np.testing.assert_allclose(P, Po, rtol=1e-5)
    monkeypatch.delenv("SP_BISPEC_MIB")
    B1, b21, _ = E.bispectrum(x[: 1 << 20], win, hop, 1 + ((1 << 20) - nfft) // hop)
    monkeypatch.setenv("SP_BISPEC_MIB", "1")
    B2, b22, _ = E.bispectrum(x[: 1 << 20], win, hop, 1 + ((1 << 20) - nfft) // hop)
    np.testing.assert_allclose(B2[ok], B1[ok], rtol=0, atol=1e-9 * np.max(np.abs(B1[ok])))


@pytest.mark.parametrize("cplx,cross", [(False, False), (False, True), (True, False)])
def test_device_tensors_match_numpy(cplx, cross):
    torch = pytest.importorskip("torch")
    nfft, hop, M = 256, 128, 700
    x = frames_signal(nfft, hop, M, cplx, 21)
    y = frames_signal(nfft, hop, M, cplx, 22) if cross else None
    win = hann(nfft)
    Bn, b2n, Pn = E.bispectrum(x, win, hop, M, y=y, detrend=2)
    xt = torch.from_numpy(x).cuda()
    yt = torch.from_numpy(y).cuda() if cross else None
    Bt, b2t, Pt = E.bispectrum(xt, win, hop, M, y=yt, detrend=2)
    assert Bt.is_cuda and Bt.dtype == torch.complex128 and b2t.dtype == torch.float64
    torch.cuda.synchronize()
    assert np.array_equal(Bt.cpu().numpy().view(np.float64), Bn.view(np.float64), equal_nan=True)
    assert np.array_equal(b2t.cpu().numpy(), b2n, equal_nan=True)
    assert np.array_equal(Pt.cpu().numpy(), Pn)
    _, _, Bp, b2p = pyfft_amd.bispectrum(xt, yt, nfft=nfft, noverlap=nfft - hop, window=win, detrend="linear")
    assert np.array_equal(b2p.cpu().numpy(), b2n, equal_nan=True)


def test_c_entry_refuses_bad_arguments():
    lib = _ffi.load_library()
    _ffi.init()
    nfft, n = 64, 4096
    x = np.zeros(n, np.float32)
    win = np.ones(4096, np.float32)
    nb = 4096
    B = np.zeros((nb, nb), np.complex128)
    b2 = np.zeros((nb, nb), np.float64)
    p = _ffi.ptr

    def call(xx=x, dtype=0, nsig=n, nf=nfft, hop=32, M=10, detrend=1):
        return lib.sp_bispectrum(p(xx), None, None, dtype, nsig, p(win), nf, hop, M, detrend, 0.0, 0.0, p(B), p(b2), None, 0)

    assert call() == 0
    for kw in (dict(nf=4), dict(nf=7), dict(nf=4097), dict(nf=8192, nsig=1 << 14), dict(dtype=5), dict(M=1000),
               dict(hop=0), dict(M=0), dict(detrend=3)):
        lib.sp_bispectrum.restype = ctypes.c_int
        if "nsig" in kw:
            big = np.zeros(kw["nsig"], np.float32)
            rc = call(xx=big, **kw)
        else:
            rc = call(**kw)
        assert rc != 0, kw
        assert lib.sp_last_error().decode().startswith("sp_bispectrum"), kw
