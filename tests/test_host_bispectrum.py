"""Bispectrum / bicoherence: the float64 numpy oracle, the argument checks and the frequency axes (no GPU).

The oracle is shared with tests/test_gpu_bispectrum.py."""
import sys

import numpy as np
import pytest

import pyfft_amd
from pyfft_amd import _ffi

bis = sys.modules["pyfft_amd.bispectrum"]


# ---------------------------------------------------------------------------------------------------- oracle
def oracle_spectra(x, win, nfft, hop, nframes, detrend, f0=0):
    """float64 spectra [m, nb] of the frames f0 .. f0 + nframes - 1 of the float32 / complex64 record x, detrended over the WHOLE
    record (0 none, 1 mean, 2 least-squares line), window cast to float32 as the library does; real: bins 0 .. nfft/2;
    complex: fftshift-ed."""
    cplx = np.iscomplexobj(x)
    x64 = x.astype(np.complex128 if cplx else np.float64)
    n = x64.size
    lo, hi = f0 * hop, (f0 + nframes - 1) * hop + nfft
    seg = x64[lo:hi]
    if detrend == 1:
        seg = seg - x64.mean()
    elif detrend == 2:
        t = np.arange(n, dtype=np.float64)
        tb = 0.5 * (n - 1)
        sxx = np.sum((t - tb) ** 2)
        slope = np.sum((t - tb) * x64) / sxx
        seg = seg - (x64.mean() + slope * (np.arange(lo, hi, dtype=np.float64) - tb))
    w = np.asarray(win, dtype=np.float32).astype(np.float64)
    idx = np.arange(nframes)[:, None] * hop + np.arange(nfft)[None, :]
    F = np.fft.fft(seg[idx] * w, axis=1)
    if cplx:
        return np.fft.fftshift(F, axes=1)
    return F[:, : nfft // 2 + 1]


def oracle_sums(X, Y, Z, c0, rows=None):
    """Frame sums over [m, nb] spectra for the rows i in `rows` (default all): (Bsum, Asum, Dsum) [len(rows), nb] with NaN outside
    the valid region, and Psum [nb].  A = sum |X Y Z| (the parity test's scale)."""
    nb = X.shape[1]
    rows = np.arange(nb) if rows is None else np.asarray(rows)
    Bs = np.full((rows.size, nb), np.nan + 1j * np.nan)
    As = np.full((rows.size, nb), np.nan)
    for r, i in enumerate(rows):
        j0, j1 = max(0, c0 - i), min(nb, nb + c0 - i)
        if j1 <= j0:
            continue
        W = Y[:, j0:j1] * np.conj(Z[:, j0 + i - c0: j1 + i - c0])
        Bs[r, j0:j1] = X[:, i] @ W
        As[r, j0:j1] = np.abs(X[:, i]) @ np.abs(W)
    Ds = (np.abs(X[:, rows]) ** 2).T @ (np.abs(Y) ** 2)
    Ps = np.sum(np.abs(Z) ** 2, axis=0)
    return Bs, As, Ds, Ps


def oracle_finish(Bs, As, Ds, Ps, M, c0, rows=None):
    """(B, b2, A, P) from frame sums; b2 = 0 where D P = 0, NaN outside the region."""
    nb = Ps.size
    rows = np.arange(nb) if rows is None else np.asarray(rows)
    B, A, D, P = Bs / M, As / M, Ds / M, Ps / M
    s = rows[:, None] + np.arange(nb)[None, :] - c0
    ok = (s >= 0) & (s < nb)
    den = np.where(ok, D * P[np.clip(s, 0, nb - 1)], np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        b2 = np.where(den > 0, np.abs(B) ** 2 / np.where(den > 0, den, 1.0), 0.0)
    b2[~ok] = np.nan
    return B, b2, A, P


def oracle_bispectrum(x, win, hop, nframes, y=None, z=None, detrend=1):
    """(B, b2, A, P) of sp_bispectrum's definition, float64 throughout."""
    nfft = len(win)
    cplx = np.iscomplexobj(x)
    c0 = nfft // 2 if cplx else 0
    X = oracle_spectra(x, win, nfft, hop, nframes, detrend)
    Y = X if y is None else oracle_spectra(y, win, nfft, hop, nframes, detrend)
    Z = X if z is None else oracle_spectra(z, win, nfft, hop, nframes, detrend)
    return oracle_finish(*oracle_sums(X, Y, Z, c0), nframes, c0)


def brute_bispectrum(x, win, hop, nframes, y=None, z=None, detrend=1):
    """The definition as a triple loop (tiny inputs only)."""
    nfft = len(win)
    cplx = np.iscomplexobj(x)
    nb, c0 = (nfft, nfft // 2) if cplx else (nfft // 2 + 1, 0)
    sp = [oracle_spectra(v if v is not None else x, win, nfft, hop, nframes, detrend) for v in (x, y, z)]
    B = np.full((nb, nb), np.nan + 1j * np.nan)
    b2 = np.full((nb, nb), np.nan)
    for i in range(nb):
        for j in range(nb):
            s = i + j - c0
            if not 0 <= s < nb:
                continue
            b = d = p = 0.0
            for g in range(nframes):
                xy = sp[0][g, i] * sp[1][g, j]
                b = b + xy * np.conj(sp[2][g, s])
                d += abs(xy) ** 2
                p += abs(sp[2][g, s]) ** 2
            B[i, j] = b / nframes
            den = d * p / nframes ** 2
            b2[i, j] = abs(B[i, j]) ** 2 / den if den > 0 else 0.0
    return B, b2


def make_signal(n, cplx, seed):
    """White noise plus three lines within 40 dB of it, float32 / complex64, with an offset and a slope to detrend."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if cplx:
        v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    else:
        v = rng.standard_normal(n)
    for k, a in ((0.11, 30.0), (0.23, 10.0), (0.34, 3.0)):
        ph = rng.uniform(0, 2 * np.pi)
        v = v + (a * np.exp(1j * (2 * np.pi * k * t + ph)) if cplx else a * np.cos(2 * np.pi * k * t + ph))
    v = v + 0.7 + 2e-5 * t
    return v.astype(np.complex64 if cplx else np.float32)


# ---------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("nfft,detrend", [(8, 0), (9, 1), (12, 2)])
def test_oracle_matches_triple_loop(cplx, cross, nfft, detrend):
    hop = nfft // 2 + 1
    n = 5 * hop + nfft
    nframes = 1 + (n - nfft) // hop
    x = make_signal(n, cplx, 1)
    y = make_signal(n, cplx, 2) if cross else None
    z = make_signal(n, cplx, 3) if cross else None
    win = np.hanning(nfft + 1)[:-1] + 0.1
    B, b2, A, _ = oracle_bispectrum(x, win, hop, nframes, y, z, detrend)
    Bb, b2b = brute_bispectrum(x, win, hop, nframes, y, z, detrend)
    np.testing.assert_array_equal(np.isnan(B), np.isnan(Bb))
    ok = ~np.isnan(Bb)
    np.testing.assert_allclose(B[ok], Bb[ok], rtol=1e-12, atol=1e-12 * np.nanmax(A))
    np.testing.assert_allclose(b2[ok], b2b[ok], rtol=1e-10, atol=1e-12)
    assert np.all(b2[ok] <= 1 + 1e-12) and np.all(b2[ok] >= 0)


@pytest.mark.parametrize("nfft", [8, 9, 64, 65])
@pytest.mark.parametrize("cplx", [False, True])
def test_frequency_axes_and_region(nfft, cplx):
    fs = 250.0
    f = bis.freq_axis(nfft, fs, cplx)
    nb = nfft if cplx else nfft // 2 + 1
    assert f.size == nb
    if cplx:
        np.testing.assert_array_equal(f, np.fft.fftshift(np.fft.fftfreq(nfft, 1 / fs)))
        assert f[nfft // 2] == 0.0
    else:
        np.testing.assert_array_equal(f, np.fft.rfftfreq(nfft, 1 / fs))
    ok = bis.valid_region(nfft, cplx)
    df = fs / nfft
    # valid exactly where f1 + f2 is a frequency of the axis
    fsum = f[:, None] + f[None, :]
    on_axis = (fsum >= f[0] - df / 2) & (fsum <= f[-1] + df / 2)
    np.testing.assert_array_equal(ok, on_axis)
    np.testing.assert_array_equal(ok, ok.T)


def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "load_library", boom)
    monkeypatch.setattr(_ffi, "_lib", None)


@pytest.mark.parametrize("kw", [
    dict(x=np.zeros(4096, np.float32), y=np.zeros(4096, np.complex64)),          # mixed dtypes
    dict(x=np.zeros(4096, np.float32), y=np.zeros(4095, np.float32)),            # unequal lengths
    dict(x=np.zeros(4096, np.float32), z=np.zeros(4000, np.float32)),
    dict(x=np.zeros(100, np.float32)),                                           # nsig < nfft
    dict(x=np.zeros(4096, np.float32), noverlap=512),                            # noverlap >= nfft
    dict(x=np.zeros(4096, np.float32), noverlap=-1),
    dict(x=np.zeros(4096, np.float32), nfft=4),                                  # nfft out of range
    dict(x=np.zeros(1 << 14, np.float32), nfft=8192),
    dict(x=np.zeros(4096, np.float32), detrend="segmean"),
    dict(x=np.zeros(4096, np.float32), window=np.ones(100)),
    dict(x=np.zeros(4096, np.float32), fs=0.0),
    dict(x=np.zeros((2, 4096), np.float32)),
])
def test_bad_arguments_raise_before_the_library_loads(monkeypatch, kw):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        pyfft_amd.bispectrum(**kw)
    with pytest.raises(ValueError):
        pyfft_amd.bicoherence(**kw)


def test_exports_and_signature():
    assert pyfft_amd.bispectrum is bis.bispectrum and pyfft_amd.bicoherence is bis.bicoherence
    assert "sp_bispectrum" in _ffi.SIGNATURES
