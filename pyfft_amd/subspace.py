"""Subspace (noise-subspace) line spectra: MUSIC and the eigenvector method (Schmidt 1986; Johnson & DeGraaf 1982; Marple, Digital
Spectral Analysis; Stoica & Moses), MATLAB's pmusic / peig on the covariance-method data matrix, the order criteria of Wax & Kailath
and a least-squares ESPRIT finish.

A record of p complex exponentials in white noise has an m x m data covariance matrix whose m - p smallest eigenvectors are orthogonal
to the steering vectors e(nu)[i] = exp(2 pi i nu i) of the lines: 1 / sum_k g_k |v_k^H e(nu)|^2 peaks there, with a resolution that is
not tied to 1 / n.  A real sinusoid counts as two exponentials.  The matrix (engine.covmat), its eigendecomposition (engine.eigh) and
the pseudospectrum (engine.pseudospectrum) run on the device; what is here is axes and the small host arithmetic.  numpy in -> numpy
out; device tensors in -> device tensors (frequency and time axes are numpy arrays).  A pseudospectrum has no units: it is not a power
density, and its peak heights say nothing about the lines' powers."""
import math

import numpy as np

from . import engine as E
from .engine import SubRefused                                     # noqa: F401

try:
    import torch
except Exception:                                                  # pragma: no cover
    torch = None

_METHODS = {"modified": True, "covariance": False}


def _is_tensor(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _is_complex(x):
    return x.is_complex() if _is_tensor(x) else np.iscomplexobj(x)


def _fb(who, method):
    if method not in _METHODS:
        raise SubRefused("%s: method must be 'modified' or 'covariance', not %r" % (who, method))
    return _METHODS[method]


def _default_m(n, p):
    """the matrix order where none is given: a third of the segment, at least p + 1 and 2, at the most 64 and n"""
    return max(2, min(E.SUB_MAX_M, n, max(p + 1, n // 3)))


def corrmtx_cov(x, m, method="modified", detrend=False):
    """The m x m data covariance matrix of every row along the last axis: X'X of MATLAB's corrmtx(x, m - 1, method) for method =
    'covariance' (forward: C[i,j] = (1 / N) sum_t conj(x[t-i]) x[t-j], N = n - m + 1 snapshots) or 'modified' (forward-backward,
    (C + J conj(C) J) / 2) -> C[..., m, m] complex128, exactly Hermitian.  2 <= m <= 64."""
    who = "corrmtx_cov"
    fb = _fb(who, method)
    if not _is_tensor(x):
        x = np.asarray(x)
    if len(x.shape) < 1 or int(x.shape[-1]) < 2:
        raise SubRefused("%s: x needs a last axis of at least two samples" % who)
    return E.covmat(x, int(x.shape[-1]), 1, 0, 1, m, fb=fb, detrend=detrend)[..., 0, :, :]


def _axis(who, nfft, fs, cplx, band, nbins):
    """-> (f [bins] in Hz, bins, start, step in cycles per sample): 0 .. fs / 2 for a real record, fft order for a complex one, or
    nbins bins from f1 to f2 inclusive"""
    fs = float(fs)
    if not (math.isfinite(fs) and fs > 0):
        raise SubRefused("%s: fs must be positive" % who)
    if band is not None:
        f1, f2 = float(band[0]), float(band[1])
        nbins = int(nfft if nbins is None else nbins)
        if not (math.isfinite(f1) and math.isfinite(f2) and f2 > f1) or nbins < 2:
            raise SubRefused("%s: band = (f1, f2) needs f1 < f2, and at least 2 bins" % who)
        return f1 + (f2 - f1) * np.arange(nbins) / (nbins - 1), nbins, f1 / fs, (f2 - f1) / (fs * (nbins - 1))
    nfft = int(nfft)
    if nfft < 1:
        raise SubRefused("%s: nfft must be at least 1" % who)
    if not cplx:
        return np.arange(nfft // 2 + 1) * (fs / nfft), nfft // 2 + 1, 0.0, 1.0 / nfft
    return np.fft.fftfreq(nfft, 1.0 / fs), nfft, 0.0, 1.0 / nfft


def _pseudo(who, weighting, x, p, m, nfft, fs, method, band, nbins, detrend, out64):
    fb = _fb(who, method)
    if not _is_tensor(x):
        x = np.asarray(x)
    if len(x.shape) < 1 or int(x.shape[-1]) < 2:
        raise SubRefused("%s: x needs a last axis of at least two samples" % who)
    n, p = int(x.shape[-1]), int(p)
    m = _default_m(n, p) if m is None else int(m)
    if p < 0 or p > m - 1:
        raise SubRefused("%s: the signal dimension p = %d is outside 0 .. m - 1 = %d" % (who, p, m - 1))
    f, bins, start, step = _axis(who, nfft, fs, _is_complex(x), band, nbins)
    C = E.covmat(x, n, 1, 0, 1, m, fb=fb, detrend=detrend)[..., 0, :, :]
    w, V, _ = E.eigh(C)
    P, _ = E.pseudospectrum(V, w, p, bins, start, step, weighting, out64)
    return f, P


def pmusic(x, p, m=None, nfft=256, fs=1.0, method="modified", band=None, nbins=None, detrend=False, out64=False):
    """MATLAB's pmusic along the last axis on the covariance-method data matrix: -> f, P[..., bins], the MUSIC pseudospectrum with
    signal dimension p (the number of complex exponentials: two per real sinusoid) from the m x m matrix of `corrmtx_cov` (m
    defaults to a third of the record, at the most 64).  f: 0 .. fs / 2 on nfft // 2 + 1 bins for a real record, fft order for a
    complex one; band=(f1, f2), nbins=: bins from f1 to f2 inclusive.  float32, or float64 with out64."""
    return _pseudo("pmusic", "music", x, p, m, nfft, fs, method, band, nbins, detrend, out64)


def peig(x, p, m=None, nfft=256, fs=1.0, method="modified", band=None, nbins=None, detrend=False, out64=False):
    """MATLAB's peig: `pmusic` with every noise eigenvector weighted by 1 / its eigenvalue, which flattens the spurious peaks of an
    overestimated noise subspace."""
    return _pseudo("peig", "ev", x, p, m, nfft, fs, method, band, nbins, detrend, out64)


def subspace_spectrogram(x, p, nperseg, noverlap=None, m=None, weighting="music", nfft=None, fs=1.0, method="modified", band=None, nbins=None,
                         detrend=True, out64=False):
    """A time-resolved pseudospectrum: one matrix, eigendecomposition and pseudospectrum per segment of nperseg samples (noverlap
    defaults to nperseg // 2) less its own mean -> f, t, P[..., bins, segments] in scipy.signal.spectrogram's orientation."""
    who = "subspace_spectrogram"
    fb = _fb(who, method)
    if weighting not in E.SUB_WEIGHTINGS:
        raise SubRefused("%s: weighting must be 'music' or 'ev', not %r" % (who, weighting))
    if not _is_tensor(x):
        x = np.asarray(x)
    nperseg, p = int(nperseg), int(p)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if len(x.shape) < 1 or nperseg < 2 or int(x.shape[-1]) < nperseg or noverlap < 0 or noverlap >= nperseg:
        raise SubRefused("%s: nperseg must lie in 2 .. the rows' length and noverlap in 0 .. nperseg - 1" % who)
    m = _default_m(nperseg, p) if m is None else int(m)
    if p < 0 or p > m - 1:
        raise SubRefused("%s: the signal dimension p = %d is outside 0 .. m - 1 = %d" % (who, p, m - 1))
    hop = nperseg - noverlap
    nframes = (int(x.shape[-1]) - nperseg) // hop + 1
    f, bins, start, step = _axis(who, nperseg if nfft is None else nfft, fs, _is_complex(x), band, nbins)
    C = E.covmat(x, nperseg, hop, 0, nframes, m, fb=fb, detrend=detrend)
    w, V, _ = E.eigh(C)
    P, _ = E.pseudospectrum(V, w, p, bins, start, step, weighting, out64)
    t = (np.arange(nframes) * hop + nperseg / 2.0) / float(fs)
    return f, t, (P.transpose(-1, -2) if _is_tensor(P) else np.swapaxes(P, -1, -2))


def subspace_order(w, nsnap, criterion="mdl"):
    """The number of exponentials an information criterion of Wax & Kailath (1985) reads from the eigenvalues w[..., m] (descending,
    as `eigh` gives them) of a covariance matrix of nsnap snapshots: with L(k) = -nsnap (m - k) ln(geometric / arithmetic mean of the
    m - k smallest), 'mdl' minimises L(k) + k (2 m - k) ln(nsnap) / 2 and 'aic' L(k) + k (2 m - k) over k = 0 .. m - 1 (host arithmetic)
    -> an integer array of w's leading shape.  Eigenvalues at or below zero are taken as the smallest positive float64."""
    if criterion not in ("mdl", "aic"):
        raise SubRefused("subspace_order: criterion must be 'mdl' or 'aic', not %r" % (criterion,))
    if _is_tensor(w):
        w = w.detach().cpu().numpy()
    w = np.maximum(np.asarray(w, dtype=np.float64), np.finfo(np.float64).tiny)
    m, nsnap = int(w.shape[-1]), int(nsnap)
    if m < 2 or nsnap < 1:
        raise SubRefused("subspace_order: w needs a last axis of at least two eigenvalues and nsnap at least one snapshot")
    crit = np.empty(w.shape[:-1] + (m,))
    for k in range(m):
        tail = w[..., k:]
        L = -nsnap * (m - k) * (np.mean(np.log(tail), axis=-1) - np.log(np.mean(tail, axis=-1)))
        crit[..., k] = L + (0.5 * k * (2 * m - k) * math.log(nsnap) if criterion == "mdl" else k * (2 * m - k))
    return np.argmin(crit, axis=-1)


def esprit(V, p, fs=1.0):
    """LS-ESPRIT on the p signal eigenvectors V[..., m, :p] (the leading columns of `eigh`'s V): the rotation Psi with
    V_s[:-1] Psi = V_s[1:] in the least-squares sense has the eigenvalues e^{2 pi i nu} of the p lines -> f[..., p] in Hz, ascending in
    (-fs / 2, fs / 2].  A host finish (numpy.linalg.lstsq and eig on p columns): no grid, no search."""
    if _is_tensor(V):
        V = V.detach().cpu().numpy()
    V = np.asarray(V, dtype=np.complex128)
    p = int(p)
    if V.ndim < 2 or p < 1 or p > V.shape[-2] - 1 or p > V.shape[-1]:
        raise SubRefused("esprit: V must be [..., m, >= p] with 1 <= p <= m - 1")
    flat = V.reshape((-1,) + V.shape[-2:])
    out = np.empty((flat.shape[0], p))
    for i, Vi in enumerate(flat):
        Vs = Vi[:, :p]
        psi = np.linalg.lstsq(Vs[:-1], Vs[1:], rcond=None)[0]
        out[i] = np.sort(np.angle(np.linalg.eigvals(psi)) / (2 * np.pi))
    return out.reshape(V.shape[:-2] + (p,)) * float(fs)


def subspace_plan(n, m, rows=1, nframes=1, cplx=False, what="covmat"):
    """What the covariance matrices of this shape run as (engine.sub_plan; host only)."""
    return E.sub_plan(what, n, m, rows, nframes, cplx)
