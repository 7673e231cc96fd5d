"""Spectral proper orthogonal decomposition (SPOD; principal components in the frequency domain) of a probe array: the
eigendecomposition of the cross-spectral-density matrix at every frequency.

    G[k]       = engine.csd_matrix: Welch's estimate of E[X_i conj(X_j)] at bin k over the nch channels, as a density
                 (1 / (fs sum w^2)), interior bins doubled for a one-sided spectrum
    G[k] W phi = lam phi,   phi^H W phi = 1         W = diag(weights): quadrature weights or a metric, default 1
                 solved as the Hermitian problem  (W^1/2 G W^1/2) v = lam v,  phi = W^-1/2 v

lam[k, m] is the power the m-th coherent structure carries at frequency k (descending in m), phi[k, :, m] its shape across the array.
Both the matrix and its decomposition stay on the device: the matrix comes from k_csdm (sp_csd_matrix), the eigensolver is
k_eigh.hip (sp_eigh: parallel cyclic Jacobi in float64, one bin per workgroup), and for a device tensor x nothing but the frequency
axis is made on the host.  The array is limited to 64 channels by the eigensolver.  The CSD matrix is Hermitian only to about 1e-6
(float32 spectra): the solver reads its lower triangle, as numpy.linalg.eigh does."""
import ctypes as C
import math

import numpy as np

from .engine import _is_torch
from .windows import get_window

MAX_CHANNELS = 64


def _too_many(who, nch):
    from .engine import OrderTooLarge
    return OrderTooLarge("%s: %d channels; the eigensolver is built for at most %d (one matrix and its vectors live in the LDS of "
                         "one CU)" % (who, nch, MAX_CHANNELS))


def _weights(who, weights, nch):
    if weights is None:
        return None
    if _is_torch(weights):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights, dtype=np.float64).ravel()
    if w.shape != (nch,) or not np.all(np.isfinite(w)) or not np.all(w > 0):
        raise ValueError("%s: weights must be %d positive finite numbers" % (who, nch))
    return w


def csd_segments(who, Refused, nsig, fs, window, nperseg, noverlap, band=None):
    """What the record front ends that take a `band` (`array_spectrum`, `mimo_frf` and their kin) refuse about the segments, in one order
    and in one set of words, and what they then work with -> (win float64 [nperseg], hop, nframes, freq of the kept bins, b0, b1):
    segments of nperseg under `window` every nperseg - noverlap samples (noverlap defaults to nperseg // 2); band = (f1, f2) keeps the
    bins f1 <= f <= f2 of rfftfreq(nperseg, 1 / fs)."""
    nperseg, fs = int(nperseg), float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise Refused("%s: fs must be positive" % who)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if nperseg < 2 or not 0 <= noverlap < nperseg or nsig < nperseg:
        raise Refused("%s: need 2 <= nperseg <= nsig and 0 <= noverlap < nperseg" % who)
    if isinstance(window, (str, tuple)):
        win = np.asarray(get_window(window, nperseg), dtype=np.float64)
    else:
        win = np.asarray(window, dtype=np.float64)
    if win.shape != (nperseg,) or not np.all(np.isfinite(win)) or not np.sum(win * win) > 0:
        raise Refused("%s: window must be a name or nperseg = %d finite values with some weight" % (who, nperseg))
    freq = np.fft.rfftfreq(nperseg, 1.0 / fs)
    b0, b1 = 0, nperseg // 2 + 1
    if band is not None:
        f1, f2 = float(band[0]), float(band[1])
        inside = np.nonzero((freq >= f1) & (freq <= f2))[0] if math.isfinite(f1) and math.isfinite(f2) else ()
        if len(inside) == 0:
            raise Refused("%s: band = (f1, f2) holds no bin" % who)
        b0, b1 = int(inside[0]), int(inside[-1]) + 1
    hop = nperseg - noverlap
    return win, hop, 1 + (nsig - nperseg) // hop, freq[b0:b1], b0, b1


def one_sided_csd(x, win, hop, nframes, fs, detrend=True, b0=0, b1=None, doubling=True):
    """The CSD matrices G[b0:b1] of the real channels x[nch, nsig] under the one convention of `spod`, `array_spectrum` and `mimo_frf`:
    `engine.csd_matrix` scaled to a density, 1 / (fs sum w^2), with the interior bins doubled for a one-sided spectrum.  A device
    tensor in -> a device tensor, and the matrices never visit the host."""
    from . import engine
    nperseg = int(win.shape[0])
    nb = nperseg // 2 + 1
    b1 = nb if b1 is None else b1
    G = engine.csd_matrix(x, win, hop, nframes, detrend=bool(detrend), scale=1.0 / (fs * float(np.sum(win * win))))
    if not doubling:
        return G if (b0, b1) == (0, nb) else G[b0:b1]
    k = np.arange(nb)
    dbl = np.where((k >= 1) & (k <= (nperseg - 1) // 2), 2.0, 1.0)[b0:b1]
    if _is_torch(G):
        import torch
        dbl = torch.as_tensor(dbl, dtype=torch.float64, device=G.device)
    return (G if (b0, b1) == (0, nb) else G[b0:b1]) * dbl[:, None, None]


def spod_plan(nch, nmodes=None, nb=1):
    """What the eigensolver does with nb matrices of order nch and nmodes vectors each (sp_eigh_plan, host only):
    dict(NP = the padded order, lds_bytes of a workgroup, wg_per_cu, grid = workgroups launched)."""
    nch, nb = int(nch), int(nb)
    nmodes = nch if nmodes is None else int(nmodes)
    if nch > MAX_CHANNELS:
        raise _too_many("spod_plan", nch)
    if nch < 1 or not 0 <= nmodes <= nch or nb < 0:
        raise ValueError("spod_plan: need nch >= 1, 0 <= nmodes <= nch, nb >= 0")
    from . import _ffi
    out = (C.c_int64 * 4)()
    if _ffi.lib().sp_eigh_plan(nch, nmodes, nb, out) != 0:
        raise ValueError("spod_plan: sp_eigh_plan refused nch = %d, nmodes = %d, nb = %d" % (nch, nmodes, nb))
    return dict(NP=int(out[0]), lds_bytes=int(out[1]), wg_per_cu=int(out[2]), grid=int(out[3]))


def spod(x, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=True, nmodes=None, weights=None, onesided_doubling=True,
         return_csd=False):
    """(freq, lam, phi[, G]): the spectral POD of the real channels x[nch, nsig], nch <= 64, sampled at fs.
      freq [nb]              rfftfreq(nperseg, 1 / fs), nb = nperseg // 2 + 1
      lam  [nb, nmodes]      float64, descending: the eigenvalues of G[k] W (default nmodes = nch)
      phi  [nb, nch, nmodes] complex128 modes, phi^H W phi = 1, each turned so that the largest component of W^1/2 phi is real
                             and positive
      G    [nb, nch, nch]    (return_csd=True) the matrix that was decomposed, without the weights
    G is engine.csd_matrix's estimate (segments of nperseg under `window` -- a name, a (name, parameter) tuple or nperseg values --
    every nperseg - noverlap samples, noverlap defaulting to nperseg // 2) scaled to a density, 1 / (fs sum w^2), with the interior
    bins doubled if onesided_doubling.  detrend is csd_matrix's: True removes the mean of each channel's WHOLE record, False
    nothing; there is no per-segment detrend, because csd_matrix has none.  weights: nch positive numbers (quadrature weights, a
    metric).  numpy in -> numpy out; a device tensor in -> lam, phi, G on its device, and G never visits the host.
    Raises numpy.linalg.LinAlgError if a bin does not converge (a NaN in the record), and a ValueError that is also a
    NotImplementedError for more than 64 channels."""
    from . import engine
    if len(x.shape) != 2:
        raise ValueError("spod: x must be [nch, nsig]")
    nch, nsig = int(x.shape[0]), int(x.shape[1])
    if nch > MAX_CHANNELS:
        raise _too_many("spod", nch)
    if nch < 1:
        raise ValueError("spod: no channels")
    nperseg = int(nperseg)
    fs = float(fs)
    if not (fs > 0 and np.isfinite(fs)):
        raise ValueError("spod: fs must be positive")
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if nperseg < 2 or not 0 <= noverlap < nperseg:
        raise ValueError("spod: need nperseg >= 2 and 0 <= noverlap < nperseg")
    if nsig < nperseg:
        raise ValueError("spod: the record (%d samples) is shorter than a segment (%d)" % (nsig, nperseg))
    nmodes = nch if nmodes is None else int(nmodes)
    if not 1 <= nmodes <= nch:
        raise ValueError("spod: nmodes must lie in 1 .. nch = %d" % nch)
    if isinstance(window, (str, tuple)):
        win = np.asarray(get_window(window, nperseg), dtype=np.float64)
    else:
        win = np.asarray(window, dtype=np.float64)
    if win.shape != (nperseg,) or not np.all(np.isfinite(win)) or not np.sum(win * win) > 0:
        raise ValueError("spod: window must be a name or nperseg = %d finite values with some weight" % nperseg)
    wts = _weights("spod", weights, nch)
    hop = nperseg - noverlap
    nframes = 1 + (nsig - nperseg) // hop
    freq = np.fft.rfftfreq(nperseg, 1.0 / fs)
    G = one_sided_csd(x, win, hop, nframes, fs, detrend, doubling=onesided_doubling)
    dev = _is_torch(G)
    if dev:
        import torch
        host = lambda a: torch.as_tensor(a, dtype=torch.float64, device=G.device)      # noqa: E731
    else:
        host = lambda a: a                                                              # noqa: E731
    Gw = G
    if wts is not None:
        rw = host(np.sqrt(wts))
        Gw = G * rw[None, :, None] * rw[None, None, :]
    lam, v, _ = engine.eigh(Gw, nvec=nmodes, check=True)
    lam = lam[:, :nmodes]
    phi = v if wts is None else v / host(np.sqrt(wts))[None, :, None]
    return (freq, lam, phi, G) if return_csd else (freq, lam, phi)


def spod_energy(lam, trace=None):
    """The fraction of a bin's power each mode carries: lam[..., m] / trace, trace = sum_m lam (give it, e.g. the real trace of G W,
    when lam holds only the leading modes).  A bin without power gives 0."""
    if _is_torch(lam):
        import torch
        tr = lam.sum(dim=-1, keepdim=True) if trace is None else torch.as_tensor(trace, dtype=lam.dtype, device=lam.device)[..., None]
        return torch.where(tr > 0, lam / torch.where(tr > 0, tr, torch.ones_like(tr)), torch.zeros_like(lam))
    lam = np.asarray(lam, dtype=np.float64)
    tr = lam.sum(axis=-1, keepdims=True) if trace is None else np.asarray(trace, dtype=np.float64)[..., None]
    return np.divide(lam, tr, out=np.zeros(np.broadcast(lam, tr).shape), where=tr > 0)


def spod_reconstruct(lam, phi, weights=None):
    """sum_m lam[..., m] phi[..., :, m] phi[..., :, m]^H -> [..., nch, nch]: with all the modes the Hermitian part of the matrix that was
    decomposed, with the leading ones its best low-rank approximation in the W-norm.  The weights cancel (phi = W^-1/2 v carries
    them), so `weights` is only checked against phi's channels."""
    _weights("spod_reconstruct", weights, int(phi.shape[-2]))
    if _is_torch(phi):
        return (phi * lam[..., None, :].to(phi.dtype)) @ phi.conj().transpose(-1, -2)
    lam, phi = np.asarray(lam, dtype=np.float64), np.asarray(phi, dtype=np.complex128)
    return (phi * lam[..., None, :]) @ np.conj(np.swapaxes(phi, -1, -2))
