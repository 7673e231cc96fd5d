"""Host side of the polyphase filter-bank channelizer: the float64 oracles pfb_ref (the defining sum) and pfb_fold_ref (the fold and one
M-point transform), their identities against scipy.signal (the every-P-th-bin STFT, Welch at P = 1), the constant-channel property of the
"time" phase reference, the prototype design, the host plan with every refusal that comes before the library loads, and the declaration
and binding of sp_pfb.  No GPU needed.  tests/test_gpu_channelizer.py imports pfb_ref from here."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
from pyfft_amd import channelizer as CH
from pyfft_amd.baseband import Unsupported
from test_host_multitaper import make_signal, no_library        # noqa: F401  (no_library: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(x, L, hop, first, nframes):
    """[..., nframes, L] float64 / complex128: frame m = x[first + m hop : first + m hop + L], zero outside the row."""
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    idx = first + np.arange(nframes)[:, None] * hop + np.arange(L)[None, :]
    inside = (idx >= 0) & (idx < x.shape[-1])
    return np.where(inside, x[..., np.clip(idx, 0, x.shape[-1] - 1)], 0.0)


def _rho(M, hop, nframes, phase_ref, r0):
    return (r0 + np.arange(nframes) * hop) % M if phase_ref else np.zeros(nframes, dtype=np.int64)


def pfb_ref(x, h, M, hop, first, nframes, phase_ref=0, r0=0):
    """The definition along the last axis, float64: X[..., m, k] = sum_{n<L} h[n] x[s + n] exp(-2 pi i k (n + rho_m) / M), s = first +
    m hop, x zero outside the row, rho_m = 0 (phase_ref 0) or (r0 + m hop) mod M (phase_ref 1); complex128 [..., nframes, M].
    The sum over n is taken without folding: exp(-2 pi i k n / M) = exp(-2 pi i (k P) n / L), so it is bin k P of the L-point
    float64 DFT of the weighted frame (pfb_literal below is the same sum written out, for small shapes); the rotation is a phase with
    the integer k rho_m reduced modulo M."""
    h = np.asarray(h, dtype=np.float64)
    L = h.size
    assert L % M == 0
    w = _frames(x, L, hop, first, nframes) * h
    X = np.fft.fft(w, axis=-1)[..., ::L // M]
    k = np.arange(M)
    rot = np.exp(-2j * np.pi * ((k[None, :] * _rho(M, hop, nframes, phase_ref, r0)[:, None]) % M) / M)
    return X * rot


def pfb_literal(x, h, M, hop, first, nframes, phase_ref=0, r0=0):
    """The same sum written out term by term (an [M, L] matrix of phases, integer exponents reduced modulo M): small shapes only."""
    h = np.asarray(h, dtype=np.float64)
    L = h.size
    w = _frames(x, L, hop, first, nframes) * h
    out = np.empty(w.shape[:-1] + (M,), dtype=np.complex128)
    k, n = np.arange(M)[:, None], np.arange(L)[None, :]
    for m, rho in enumerate(_rho(M, hop, nframes, phase_ref, r0)):
        E = np.exp(-2j * np.pi * ((k * (n + rho)) % M) / M)
        out[..., m, :] = np.einsum("kn,...n->...k", E, w[..., m, :])
    return out


def pfb_fold_ref(x, h, M, hop, first, nframes, phase_ref=0, r0=0):
    """The computed form, float64: u[i] = sum_{p<P} h[p M + j] x[s + p M + j], j = (i - rho_m) mod M, X[m, :] = FFT_M(u)."""
    h = np.asarray(h, dtype=np.float64)
    L = h.size
    P = L // M
    w = _frames(x, L, hop, first, nframes) * h
    v = w.reshape(w.shape[:-1] + (P, M)).sum(axis=-2)                     # v[j] = sum_p w[p M + j]
    i = np.arange(M)
    j = (i[None, :] - _rho(M, hop, nframes, phase_ref, r0)[:, None]) % M     # [nframes, M]
    u = np.take_along_axis(v, np.broadcast_to(j, v.shape), axis=-1)
    return np.fft.fft(u, axis=-1)


M0, P0, D0 = 32, 4, 24
L0 = M0 * P0


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("phase_ref", [0, 1])
def test_ref_equals_fold_and_literal(cplx, phase_ref):
    """M = 32, P = 4, D = 24, first = -L/2 (the ends zero-extended), r0 != 0, two rows."""
    x = make_signal(2 * 700, cplx, 61).reshape(2, 700)
    h = CH.pfb_prototype(M0, P0)
    args = (x, h, M0, D0, -L0 // 2, 30, phase_ref, 13)
    ref = pfb_ref(*args)
    assert ref.shape == (2, 30, M0)
    scale = np.max(np.abs(ref))
    for other in (pfb_fold_ref(*args), pfb_literal(*args)):
        assert np.max(np.abs(other - ref)) <= 1e-11 * scale


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_every_pth_bin_of_the_stft(cplx):
    """phase_ref 0, first = 0: X[m, k] is bin k P of the L-point STFT under the window h, scipy's scaling (1 / sum h) undone."""
    x = make_signal(900, cplx, 62)
    h = CH.pfb_prototype(M0, P0)
    _, _, Z = ss.stft(x, window=h, nperseg=L0, noverlap=L0 - D0, boundary=None, padded=False, return_onesided=False)
    nframes = (900 - L0) // D0 + 1
    assert Z.shape == (L0, nframes)
    ref = pfb_ref(x, h, M0, D0, 0, nframes)
    want = (Z * np.sum(h))[::P0].T
    assert np.max(np.abs(ref - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("hop", [3 * M0 // 4, M0 // 2 + 1])
def test_time_phase_makes_a_tone_constant(hop):
    """A tone at exactly k / M cycles per sample of absolute time, phase "time": channel k holds sum(h) in every interior frame,
    whatever the hop and wherever the chunk starts."""
    k, n0, nsig = 5, 1000003, 1200
    h = CH.pfb_prototype(M0, P0)
    x = np.exp(2j * np.pi * ((k * (n0 + np.arange(nsig))) % M0) / M0)
    p = CH.pfb_plan(nsig, True, M0, P0, hop, n0=n0)
    X = pfb_ref(x, h, M0, hop, p["first"], p["nframes"], 1, p["r0"])
    assert p["nframes"] > 20
    assert np.max(np.abs(X[:, k] - np.sum(h))) <= 1e-13
    # the frame reference does rotate at this hop: the property is the phase reference's, not the filter's
    Xf = pfb_ref(x, h, M0, hop, p["first"], p["nframes"], 0, 0)
    assert np.max(np.abs(Xf[:, k] - np.sum(h))) > 0.1


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_one_branch_hann_is_welch(cplx):
    """P = 1, h = hann(M), D = M / 2: the mean power of the frames is scipy.signal.welch(detrend=False)."""
    M, fs = 64, 250.0
    x = make_signal(5000, cplx, 63)
    h = ss.get_window("hann", M)
    nframes = (5000 - M) // (M // 2) + 1
    X = pfb_ref(x, h, M, M // 2, 0, nframes)
    pxx = np.mean(np.abs(X) ** 2, axis=0) / (fs * np.sum(h * h))
    f, want = ss.welch(x, fs=fs, window=h, nperseg=M, noverlap=M // 2, detrend=False, return_onesided=not cplx)
    if not cplx:
        pxx = pxx[:M // 2 + 1].copy()
        pxx[1:M // 2] *= 2.0
    np.testing.assert_allclose(pxx, want, rtol=1e-12, atol=1e-12 * want.max())
    assert np.array_equal(f, CH.pfb_plan(5000, cplx, M, h=h, hop=M // 2, fs=fs)["f"])


@pytest.mark.parametrize("M,taps,beta", [(32, 4, 8.0), (64, 8, 8.0), (256, 12, 10.0), (16, 6, 5.0)])
def test_prototype_response(M, taps, beta):
    """Unit DC gain, and from the stopband edge on the response is at or below the Kaiser design attenuation less 3 dB.  The edge follows
    from kaiserord's relations: A = beta / 0.1102 + 8.7 dB (A > 50) or the inverse of the 21 .. 50 dB branch, and a transition of
    width (A - 7.95) / (2.285 pi (N - 1)) of the Nyquist rate, centred on the cut-off 1 / M."""
    h = CH.pfb_prototype(M, taps, window=("kaiser", beta))
    N = taps * M
    assert h.dtype == np.float64 and h.shape == (N,)
    assert abs(np.sum(h) - 1.0) <= 1e-12
    assert np.array_equal(h, ss.firwin(N, 1.0 / M, window=("kaiser", beta)))
    A = beta / 0.1102 + 8.7
    if A <= 50:                                   # beta = 0.5842 (A - 21)^0.4 + 0.07886 (A - 21): solve for A
        lo, hi = 21.0, 50.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if 0.5842 * (mid - 21) ** 0.4 + 0.07886 * (mid - 21) < beta:
                lo = mid
            else:
                hi = mid
        A = 0.5 * (lo + hi)
    assert abs(ss.kaiser_beta(A) - beta) <= 1e-9
    width = (A - 7.95) / (2.285 * np.pi * (N - 1))
    edge = 1.0 / M + 0.5 * width                  # in units of the Nyquist rate
    w, H = ss.freqz(h, worN=64 * N)
    db = 20 * np.log10(np.maximum(np.abs(H), 1e-300))
    stop = w / np.pi >= edge
    assert stop.any() and edge < 1.0
    assert abs(db[0]) <= 1e-9
    assert np.max(db[stop]) <= -(A - 3.0), (np.max(db[stop]), A)


def test_prototype_and_plan_never_load_the_library(no_library):
    CH.pfb_prototype(64, 4)
    CH.pfb_plan(10000, True, 64)


def test_plan_geometry_and_axes():
    M, P, D, fs, n0 = 64, 4, 48, 1000.0, 12345
    L = M * P
    p = CH.pfb_plan(5000, True, M, P, D, fs=fs, n0=n0)
    assert (p["first"], p["nframes"], p["L"], p["P"], p["hop"], p["nb"]) == (0, (5000 - L) // D + 1, L, P, D, M)
    assert p["r0"] == n0 % M
    assert np.array_equal(p["h"], CH.pfb_prototype(M, P))
    assert np.array_equal(p["f"], np.fft.fftfreq(M, 1 / fs))
    np.testing.assert_allclose(p["t"], (n0 + np.arange(p["nframes"]) * D + (L - 1) / 2) / fs, rtol=0, atol=1e-12)
    c = CH.pfb_plan(5000, False, M, P, D, fs=fs, center=True, n0=n0)
    assert (c["first"], c["nframes"], c["nb"]) == (-(L // 2), -(-5000 // D), M // 2 + 1)
    assert c["r0"] == (n0 - L // 2) % M and 0 <= c["r0"] < M
    assert np.array_equal(c["f"], np.arange(M // 2 + 1) * fs / M)
    np.testing.assert_allclose(c["t"], (n0 - L // 2 + np.arange(c["nframes"]) * D + (L - 1) / 2) / fs, rtol=0, atol=1e-12)
    # the last centred frame still touches the record, the defaults: hop = M, taps = 8, one-sided for a real input
    assert c["first"] + (c["nframes"] - 1) * D < 5000
    d = CH.pfb_plan(1 << 14, False, M)
    assert (d["hop"], d["L"], d["onesided"]) == (M, 8 * M, True)
    assert CH.pfb_plan(L, True, M, P)["nframes"] == 1
    own = CH.pfb_plan(5000, True, M, h=np.hanning(3 * M), n0=-7)
    assert (own["P"], own["r0"]) == (3, (-7) % M)


def test_refusals_come_before_the_library(no_library):
    x = np.zeros(4096, dtype=np.float32)
    z = np.zeros(4096, dtype=np.complex64)
    for M in (48, 1, 0, 16384):
        with pytest.raises(Unsupported):
            CH.channelize(z, M)
    with pytest.raises(ValueError, match="multiple of M"):
        CH.channelize(z, 64, h=np.ones(100))
    with pytest.raises(ValueError, match="multiple of M"):
        CH.pfb_psd(z, 64, h=np.ones(0))
    with pytest.raises(Unsupported):
        CH.channelize(z, 16, taps=33)
    with pytest.raises(Unsupported):
        CH.pfb_psd(z, 16, h=np.ones(16 * 33))
    with pytest.raises(Unsupported):
        CH.channelize(x, 64, return_onesided=False)
    with pytest.raises(ValueError):
        CH.channelize(z, 64, return_onesided=True)
    with pytest.raises(ValueError, match="shorter than the filter"):
        CH.channelize(z[:500], 64)
    with pytest.raises(Unsupported):
        CH.channelize(z, 64, h=np.ones(128) * 1j)
    with pytest.raises(ValueError):
        CH.channelize(z, 64, h=np.full(128, np.nan))
    with pytest.raises(ValueError):
        CH.channelize(z, 64, hop=0)
    with pytest.raises(ValueError):
        CH.channelize(z, 64, phase="absolute")
    with pytest.raises(ValueError):
        CH.pfb_psd(z, 64, scaling="power")
    with pytest.raises(ValueError):
        CH.channelize(z, 64, axis=1)
    assert issubclass(Unsupported, ValueError) and issubclass(Unsupported, NotImplementedError)


def test_exported():
    for name in ("pfb_prototype", "pfb_plan", "channelize", "pfb_psd"):
        assert getattr(pyfft_amd, name) is getattr(CH, name)
    assert callable(pyfft_amd.engine.pfb)
    assert CH.Unsupported is Unsupported


def test_declared_and_bound():
    from pyfft_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    mt = re.search(r"int sp_pfb\(([^;]*)\);", hdr)
    assert mt, "sp_pfb is not declared in include/spectral.h"
    nargs = len([a for a in mt.group(1).split(",") if a.strip()])
    assert "sp_pfb" in _ffi.SIGNATURES and len(_ffi.SIGNATURES["sp_pfb"][1]) == nargs == 18
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "sp_pfb")
