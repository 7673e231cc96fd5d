"""Parametric (autoregressive, maximum-entropy) spectra: Burg's method and Yule-Walker (Burg 1975; Marple, Digital Spectral Analysis;
Kay, Modern Spectral Estimation), MATLAB's arburg / aryule / pburg / pyulear and a time-resolved form.

An all-pole model x[i] = -sum_{j=1}^{p} a[j] x[i-j] + e[i] with var e = E has the spectrum E / (fs |A(e^{2 pi i f / fs})|^2): its resolution
is not tied to the record length, which is what a few hundred samples per estimate need.  The fits (engine.burg, engine.yule) and the
spectrum of a model (engine.ar_psd) run on the device; what is here is axes, units and the small arithmetic on the models.  numpy in ->
numpy out; device tensors in -> device tensors (frequency and time axes are numpy arrays)."""
import math

import numpy as np

from . import engine as E
from .engine import ArRefused, SubRefused                          # noqa: F401

try:
    import torch
except Exception:                                                  # pragma: no cover
    torch = None

_FITS = {"burg": E.burg, "yule": E.yule}
_LS = {"cov": False, "mcov": True}                                 # the least-squares fits (engine.ar_ls): forward, forward-backward


def _is_tensor(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _is_complex(x):
    return x.is_complex() if _is_tensor(x) else np.iscomplexobj(x)


def _fit(who, method, x, order, detrend, evar):
    if method not in _FITS:
        raise ArRefused("%s: method must be 'burg' or 'yule', not %r" % (who, method))
    if not _is_tensor(x):
        x = np.asarray(x)
    if len(x.shape) < 1 or int(x.shape[-1]) < 2:
        raise ArRefused("%s: x needs a last axis of at least two samples" % who)
    a, e, k = _FITS[method](x, int(x.shape[-1]), 1, 0, 1, order, detrend=detrend)
    a, e, k = a[..., 0, :], e[..., 0, :], k[..., 0, :]
    return a, (e if evar else e[..., -1]), k


def arburg(x, order, detrend=False, evar=False):
    """MATLAB's arburg along the last axis: -> a[..., order + 1] (a[..., 0] = 1), e[...] (the variance of the prediction error at `order`;
    evar=True: e[..., order + 1], by order, what `ar_order` takes), k[..., order] (the reflection coefficients).  float64 for real
    rows, complex128 for complex rows.  detrend=True removes every row's mean first (MATLAB does not).  Rows of up to 16384 samples."""
    return _fit("arburg", "burg", x, order, detrend, evar)


def aryule(x, order, detrend=False, evar=False):
    """MATLAB's aryule along the last axis (the biased autocorrelation estimate and Levinson-Durbin): the returns of `arburg`.  Rows of
    any length up to 2^31 - 1."""
    return _fit("aryule", "yule", x, order, detrend, evar)


def _ls_fit(who, fb, x, order, detrend, check=True):
    if not _is_tensor(x):
        x = np.asarray(x)
    if len(x.shape) < 1 or int(x.shape[-1]) < 2:
        raise SubRefused("%s: x needs a last axis of at least two samples" % who)
    a, e, _ = E.ar_ls(x, int(x.shape[-1]), 1, 0, 1, order, fb=fb, detrend=detrend, check=check)
    return a[..., 0, :], e[..., 0]


def arcov(x, order, detrend=False, check=True):
    """MATLAB's arcov along the last axis, the covariance (forward least-squares) fit: -> a[..., order + 1] (a[..., 0] = 1), e[...]
    (the mean square of the forward prediction error over the n - order predicted samples).  No window and no lattice: lines closer
    than 1 / n that `arburg` merges or splits come apart, and a noiseless sum of order / 2 real sinusoids is fitted exactly (then the
    normal matrix is singular: numpy.linalg.LinAlgError, or with check=False the model a = (1, 0 ..), e = 0).  order <= 63 and
    <= n / 2; the model need not be stable."""
    return _ls_fit("arcov", False, x, order, detrend, check)


def armcov(x, order, detrend=False, check=True):
    """MATLAB's armcov along the last axis, the modified covariance (forward-backward least-squares) fit: the returns of `arcov`; e is
    the mean of the forward and the backward error powers.  Free of Burg's line splitting and of its phase-dependent bias."""
    return _ls_fit("armcov", True, x, order, detrend, check)


def _axis(who, nfft, fs, onesided, band, m):
    """-> (f [m] in Hz, m, start, step in cycles per sample, the bins a one-sided spectrum doubles (a slice or a mask, or None))"""
    fs = float(fs)
    if not (math.isfinite(fs) and fs > 0):
        raise ArRefused("%s: fs must be positive" % who)
    if band is not None:
        f1, f2 = float(band[0]), float(band[1])
        m = int(nfft if m is None else m)
        if not (math.isfinite(f1) and math.isfinite(f2) and f2 > f1) or m < 2:
            raise ArRefused("%s: band = (f1, f2) needs f1 < f2, and m at least 2 bins" % who)
        f = f1 + (f2 - f1) * np.arange(m) / (m - 1)
        dbl = None
        if onesided:
            nu = np.abs(f / fs - np.round(f / fs))
            dbl = (nu > 0) & (nu < 0.5)
        return f, m, f1 / fs, (f2 - f1) / (fs * (m - 1)), dbl
    nfft = int(nfft)
    if nfft < 1:
        raise ArRefused("%s: nfft must be at least 1" % who)
    if onesided:
        m = nfft // 2 + 1
        return np.arange(m) * (fs / nfft), m, 0.0, 1.0 / nfft, slice(1, m - 1 if nfft % 2 == 0 else m)
    return np.fft.fftfreq(nfft, 1.0 / fs), nfft, 0.0, 1.0 / nfft, None


def ar_psd(a, e, nfft=256, fs=1.0, return_onesided=None, band=None, m=None, out64=False):
    """The power spectral density of all-pole models from anywhere: a[..., p + 1], e[...] -> f, Pxx[..., bins] in the units of
    scipy.signal.welch(scaling='density'): e / (fs |A|^2), doubled off DC and Nyquist for a one-sided spectrum (the default for real a).
    nfft: the bins of the full circle (fft order when two-sided); band=(f1, f2), m=: m bins from f1 to f2 inclusive instead."""
    cplx = _is_complex(a)
    onesided = (not cplx) if return_onesided is None else bool(return_onesided) and not cplx
    f, m, start, step, dbl = _axis("ar_psd", nfft, fs, onesided, band, m)
    P = E.ar_psd(a, e, m, start, step, 1.0 / float(fs), out64)
    if dbl is not None:
        if _is_tensor(P) and not isinstance(dbl, slice):
            dbl = torch.as_tensor(dbl, device=P.device)
        P[..., dbl] *= 2
    return f, P


def _pxx(who, method, x, order, nfft, fs, return_onesided, detrend, band, m, out64):
    _axis(who, nfft, fs, bool(return_onesided), band, m)               # the axis is judged before the device is touched
    a, e, _ = _fit(who, method, x, order, detrend, False)
    return ar_psd(a, e, nfft, fs, return_onesided, band, m, out64)


def pburg(x, order, nfft=256, fs=1.0, return_onesided=True, detrend=False, band=None, m=None, out64=False):
    """MATLAB's pburg along the last axis: -> f, Pxx: `ar_psd` of `arburg`."""
    return _pxx("pburg", "burg", x, order, nfft, fs, return_onesided, detrend, band, m, out64)


def pyulear(x, order, nfft=256, fs=1.0, return_onesided=True, detrend=False, band=None, m=None, out64=False):
    """MATLAB's pyulear along the last axis: -> f, Pxx: `ar_psd` of `aryule`.  The Yule-Walker model matches the biased lags, so the
    integral of the two-sided density over [0, fs) is the record's mean square."""
    return _pxx("pyulear", "yule", x, order, nfft, fs, return_onesided, detrend, band, m, out64)


def _pxx_ls(who, fb, x, order, nfft, fs, return_onesided, detrend, band, m, out64):
    _axis(who, nfft, fs, bool(return_onesided), band, m)
    a, e = _ls_fit(who, fb, x, order, detrend)
    return ar_psd(a, e, nfft, fs, return_onesided, band, m, out64)


def pcov(x, order, nfft=256, fs=1.0, return_onesided=True, detrend=False, band=None, m=None, out64=False):
    """MATLAB's pcov along the last axis: -> f, Pxx: `ar_psd` of `arcov`, in the units and the one-sided rule of `pburg`."""
    return _pxx_ls("pcov", False, x, order, nfft, fs, return_onesided, detrend, band, m, out64)


def pmcov(x, order, nfft=256, fs=1.0, return_onesided=True, detrend=False, band=None, m=None, out64=False):
    """MATLAB's pmcov along the last axis: -> f, Pxx: `ar_psd` of `armcov`."""
    return _pxx_ls("pmcov", True, x, order, nfft, fs, return_onesided, detrend, band, m, out64)


def ar_spectrogram(x, order, nperseg, noverlap=None, method="burg", fs=1.0, nfft=None, detrend=True, return_onesided=True, band=None,
                   m=None, out64=False):
    """A time-resolved autoregressive spectrum: one fit per segment of nperseg samples (noverlap defaults to nperseg // 2) -> f, t,
    Pxx[..., bins, segments] in scipy.signal.spectrogram's orientation and units; column g is `pburg` (`pyulear`) of segment g less
    its own mean (detrend=False: as it is).  t: the segments' centres.  nfft defaults to nperseg; band=(f1, f2), m= give a zoomed axis.
    method: 'burg', 'yule', or the least-squares fits 'cov' (`pcov`) and 'mcov' (`pmcov`), whose orders end at 63."""
    who = "ar_spectrogram"
    if method not in _FITS and method not in _LS:
        raise ArRefused("%s: method must be 'burg', 'yule', 'cov' or 'mcov', not %r" % (who, method))
    if not _is_tensor(x):
        x = np.asarray(x)
    nperseg = int(nperseg)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if len(x.shape) < 1 or nperseg < 2 or int(x.shape[-1]) < nperseg or noverlap < 0 or noverlap >= nperseg:
        raise ArRefused("%s: nperseg must lie in 2 .. the rows' length and noverlap in 0 .. nperseg - 1" % who)
    hop = nperseg - noverlap
    nframes = (int(x.shape[-1]) - nperseg) // hop + 1
    cplx = _is_complex(x)
    f, m, start, step, dbl = _axis(who, nperseg if nfft is None else nfft, fs, bool(return_onesided) and not cplx, band, m)
    if method in _LS:
        a, e1, _ = E.ar_ls(x, nperseg, hop, 0, nframes, order, fb=_LS[method], detrend=detrend)
    else:
        a, e, _ = _FITS[method](x, nperseg, hop, 0, nframes, order, detrend=detrend)
        e1 = e[..., -1]
    P = E.ar_psd(a, e1, m, start, step, 1.0 / float(fs), out64)
    if dbl is not None:
        if _is_tensor(P) and not isinstance(dbl, slice):
            dbl = torch.as_tensor(dbl, device=P.device)
        P[..., dbl] *= 2
    t = (np.arange(nframes) * hop + nperseg / 2.0) / float(fs)
    return f, t, (P.transpose(-1, -2) if _is_tensor(P) else np.swapaxes(P, -1, -2))


def ar_order(evar, n, criterion="aic"):
    """The order an information criterion picks from the prediction-error powers by order evar[..., p + 1] of a fit of n samples:
    'aic' n ln E_m + 2 m, 'aicc' the same with the small-sample term 2 m (m + 1) / (n - m - 1), 'mdl' n ln E_m + m ln n, 'fpe'
    E_m (n + m + 1) / (n - m - 1).  -> the minimising m per model (an integer array or tensor; 0 where the record is zero)."""
    n = int(n)
    p = int(evar.shape[-1]) - 1
    if p < 0 or n - p - 1 < 1:
        raise ArRefused("ar_order: evar needs a last axis of p + 1 <= n - 1 powers")
    mm = np.arange(p + 1, dtype=np.float64)
    if criterion in ("aic", "aicc", "mdl"):
        pen = {"aic": 2 * mm, "aicc": 2 * mm + 2 * mm * (mm + 1) / (n - mm - 1), "mdl": mm * math.log(n)}[criterion]
        if _is_tensor(evar):
            return torch.argmin(n * torch.log(evar.clamp_min(1e-300)) + torch.as_tensor(pen, device=evar.device), dim=-1)
        return np.argmin(n * np.log(np.maximum(np.asarray(evar, dtype=np.float64), 1e-300)) + pen, axis=-1)
    if criterion == "fpe":
        w = (n + mm + 1) / (n - mm - 1)
        if _is_tensor(evar):
            return torch.argmin(evar * torch.as_tensor(w, device=evar.device), dim=-1)
        return np.argmin(np.asarray(evar, dtype=np.float64) * w, axis=-1)
    raise ArRefused("ar_order: criterion must be 'aic', 'aicc', 'mdl' or 'fpe', not %r" % (criterion,))


def ar_stepup(k, order=None):
    """Reflection coefficients k[..., p] -> the polynomial a[..., order + 1] of the model of `order` <= p (default p) by the Levinson
    step-up a_m[j] = a_{m-1}[j] + k_m conj(a_{m-1}[m - j]): a lower order picked by `ar_order` costs no second fit."""
    p = int(k.shape[-1])
    order = p if order is None else int(order)
    if order < 0 or order > p:
        raise ArRefused("ar_stepup: order = %d is outside 0 .. %d" % (order, p))
    if _is_tensor(k):
        a = torch.zeros(tuple(k.shape[:-1]) + (order + 1,), dtype=k.dtype, device=k.device)
        conj = torch.conj
    else:
        k = np.asarray(k)
        a = np.zeros(k.shape[:-1] + (order + 1,), dtype=k.dtype)
        conj = np.conj
    a[..., 0] = 1
    for mth in range(1, order + 1):
        km = k[..., mth - 1:mth]
        if _is_tensor(k):
            rev = torch.flip(conj(a[..., 1:mth]), dims=(-1,)).clone()
        else:
            rev = conj(a[..., 1:mth])[..., ::-1].copy()
        a[..., 1:mth] += km * rev
        a[..., mth] = k[..., mth - 1]
    return a


def ar_poles(a, fs=1.0):
    """The poles of a model (host, numpy.roots): a[..., p + 1] -> (f, damping), each [..., p]: the frequencies angle(z) fs / (2 pi) in Hz
    and the decay rates -ln|z| fs in 1/s of the poles z, sorted by frequency.  Trailing zeros of a give poles at z = 0 (damping inf)."""
    if _is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    p = a.shape[-1] - 1
    flat = a.reshape(-1, p + 1)
    f = np.zeros((flat.shape[0], p))
    d = np.full((flat.shape[0], p), np.inf)
    for i, row in enumerate(flat):
        z = np.roots(np.trim_zeros(row, "b")) if np.any(row[1:]) else np.zeros(0)
        z = z[np.argsort(np.angle(z), kind="stable")]
        q = z.size
        f[i, p - q:] = np.angle(z) * float(fs) / (2 * np.pi)
        with np.errstate(divide="ignore"):
            d[i, p - q:] = -np.log(np.abs(z)) * float(fs)
    return f.reshape(a.shape[:-1] + (p,)), d.reshape(a.shape[:-1] + (p,))


def ar_plan(method, n, order, rows=1, nframes=1, cplx=False):
    """What a fit of this shape runs as (engine.ar_plan; host only)."""
    return E.ar_plan(method, n, order, rows, nframes, cplx)
