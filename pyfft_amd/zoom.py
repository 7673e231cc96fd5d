"""Chirp-z transform and zoom spectra: spectra on m bins of a band [f1, f2) at a spacing the caller chooses, instead of on the FFT grid.

    X[k] = sum_{j<n} x[j] exp(-2 pi i (start + k step) j),  k < m         start = f1 / fs, step = (f2 - f1) / (m fs) cycles per sample

czt / zoom_fft carry scipy.signal's signatures for contours ON the unit circle (|w| = |a| = 1); off-circle contours are refused: their
chirps leave the float32 range within a few hundred points.  zoom_stft / zoom_psd / zoom_csd / zoom_coherence are scipy.signal's stft
(boundary=None, padded=False) / welch / csd / coherence with the FFT of every segment replaced by the transform on the arc: the same
window normalisation and scaling, detrend over the WHOLE record (False / 'constant' / 'linear', as multitaper.py), and for real input with
return_onesided=True the bins with 0 < f < fs / 2 doubled -- a band that leaves [0, fs / 2] is then refused.  On an arc laid on FFT bins
(start = k0 / nperseg, step = 1 / nperseg) they return scipy's values on those bins.  The transform is Bluestein's: two L-point FFTs per
segment, L = next_pow2(nperseg + m - 1), fused in one kernel up to L = 8192 (k_czt.hip) and composed from the multi-pass FFT up to 2^26.
"""
import cmath
import math

import numpy as np

from .engine import _is_torch
from .windows import get_window

_DETRENDS = {False: 0, None: 0, "none": 0, "constant": 1, "mean": 1, "linear": 2}
MAX_LOG2 = 26                       # the longest multi-pass transform


class OffCircle(ValueError, NotImplementedError):
    """A contour off the unit circle: outside the limits, and a path that is not built."""


class TooLong(ValueError, NotImplementedError):
    """n + m - 1 beyond the longest multi-pass transform."""


def _check_len(who, n, m):
    if n < 1:
        raise ValueError("%s: the transform needs at least one input sample" % who)
    if m < 1:
        raise ValueError("%s: m must be at least 1" % who)
    if n + m - 1 > 1 << MAX_LOG2:
        raise TooLong("%s: n + m - 1 = %d is beyond the longest transform, 2^%d points" % (who, n + m - 1, MAX_LOG2))


def _arc_czt(x, m, start, step, axis, who):
    nd = x.dim() if _is_torch(x) else np.ndim(x)
    if nd < 1:
        raise ValueError("%s: x must have at least one axis" % who)
    if not -nd <= axis < nd:
        raise ValueError("%s: axis %d is out of range" % (who, axis))
    n = int(x.shape[axis]) if _is_torch(x) else int(np.shape(x)[axis])
    m = n if m is None else int(m)
    _check_len(who, n, m)
    if not (math.isfinite(start) and math.isfinite(step)):
        raise ValueError("%s: the contour must be finite" % who)
    from . import engine
    last = axis in (-1, nd - 1)
    if _is_torch(x):
        out = engine.czt(x if last else x.movedim(axis, -1), m, start, step)
        return out if last else out.movedim(-1, axis)
    out = engine.czt(np.asarray(x) if last else np.moveaxis(np.asarray(x), axis, -1), m, start, step)
    return out if last else np.moveaxis(out, -1, axis)


def czt(x, m=None, w=None, a=1 + 0j, *, axis=-1):
    """scipy.signal.czt for a contour on the unit circle: X[k] = sum_n x[n] z_k^-n at z_k = a w^-k, k < m (m=None: the length of the
    axis; w=None: exp(-2 pi i / m), the full circle).  complex64; numpy in -> numpy out, device tensor in -> device tensor out."""
    if not _is_torch(x):
        x = np.asarray(x)
    nd = len(x.shape)
    n = int(x.shape[axis]) if -nd <= axis < nd else 0
    mm = n if m is None else int(m)
    if mm < 1:
        raise ValueError("czt: m must be at least 1")
    w = cmath.exp(-2j * math.pi / mm) if w is None else complex(w)
    a = complex(a)
    if not (cmath.isfinite(w) and cmath.isfinite(a)):
        raise ValueError("czt: w and a must be finite")
    if abs(abs(w) - 1.0) > 1e-12 or abs(abs(a) - 1.0) > 1e-12:
        raise OffCircle("czt: only contours on the unit circle are supported (|w| = |a| = 1); got |w| = %r, |a| = %r" % (abs(w), abs(a)))
    return _arc_czt(x, mm, cmath.phase(a) / (2 * math.pi), -cmath.phase(w) / (2 * math.pi), axis, "czt")


def _band(who, fn, fs):
    f = np.asarray(fn, dtype=np.float64)
    if f.ndim == 0:
        f1, f2 = 0.0, float(f)
    elif f.shape == (2,):
        f1, f2 = float(f[0]), float(f[1])
    else:
        raise ValueError("%s: fn must be a scalar or a pair [f1, f2]" % who)
    if not (math.isfinite(f1) and math.isfinite(f2)):
        raise ValueError("%s: fn must be finite" % who)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    return f1, f2


def _arc(f1, f2, m, fs, endpoint):
    """(start, step, freq): cycles per sample, and the float64 frequency axis start fs + k step fs."""
    den = (m - 1) if endpoint and m > 1 else m
    step = (f2 - f1) / (den * fs)
    return f1 / fs, step, f1 + np.arange(m, dtype=np.float64) * ((f2 - f1) / den)


def zoom_fft(x, fn, m=None, *, fs=2, endpoint=False, axis=-1):
    """scipy.signal.zoom_fft: the DFT of x on m bins over [f1, f2) (fn a pair, or a scalar f2 with f1 = 0; endpoint=True includes
    f2).  complex64; numpy in -> numpy out, device tensor in -> device tensor out."""
    fs = float(fs)
    f1, f2 = _band("zoom_fft", fn, fs)
    if not _is_torch(x):
        x = np.asarray(x)
    nd = len(x.shape)
    n = int(x.shape[axis]) if -nd <= axis < nd else 0
    mm = n if m is None else int(m)
    if mm < 1:
        raise ValueError("zoom_fft: m must be at least 1")
    start, step, _ = _arc(f1, f2, mm, fs, endpoint)
    return _arc_czt(x, mm, start, step, axis, "zoom_fft")


def zoom_plan(nsig, cplx, fn, m, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=False, scaling="density",
              return_onesided=True, endpoint=False):
    """The validated host plan of a zoom spectrum (pure numpy, never loads the library): a dict with freq (float64 [m]), start and step
    (cycles per sample), window (float64 [nperseg]), nperseg, hop, nframes, detrend (device code), scale (scipy.signal.welch's: 1 / (fs
    sum w^2) for 'density', 1 / (sum w)^2 for 'spectrum'), amp (scipy.signal.stft's: 1 / sum w), onesided and fold (the factor of each bin
    of a PSD: 2 where 0 < f < fs / 2 for real input with return_onesided, else 1)."""
    who = "zoom"
    nsig, m, fs = int(nsig), int(m), float(fs)
    f1, f2 = _band(who, fn, fs)
    if isinstance(window, (str, tuple)):
        nperseg = int(nperseg)
        if nperseg < 1:
            raise ValueError("%s: nperseg must be at least 1" % who)
        win = np.asarray(get_window(window, nperseg), dtype=np.float64)
    else:
        win = np.asarray(window, dtype=np.float64)
        if win.ndim != 1 or win.size < 1:
            raise ValueError("%s: window must be a name or a one-dimensional array" % who)
        nperseg = win.size
    if not np.all(np.isfinite(win)):
        raise ValueError("%s: the window must be finite" % who)
    _check_len(who, nperseg, m)
    if nsig < nperseg:
        raise ValueError("%s: the record (%d samples) is shorter than nperseg (%d)" % (who, nsig, nperseg))
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap < 0 or noverlap >= nperseg:
        raise ValueError("%s: need 0 <= noverlap < nperseg" % who)
    try:
        code = _DETRENDS[detrend]
    except (KeyError, TypeError):
        raise ValueError("%s: detrend must be False, 'constant' or 'linear' (over the whole record)" % who) from None
    if scaling not in ("density", "spectrum"):
        raise ValueError("%s: scaling must be 'density' or 'spectrum'" % who)
    s1, s2 = float(np.sum(win)), float(np.sum(win * win))
    if not s2 > 0 or s1 == 0:
        raise ValueError("%s: the window sums to zero" % who)
    start, step, freq = _arc(f1, f2, m, fs, endpoint)
    onesided = bool(return_onesided) and not cplx
    fold = np.ones(m)
    if onesided:
        if freq.min() < 0 or freq.max() > fs / 2:
            raise ValueError("%s: a one-sided spectrum lives on [0, fs / 2]; the band [%g, %g] leaves it (return_onesided=False gives "
                             "the two-sided values)" % (who, freq.min(), freq.max()))
        fold[(freq > 0) & (freq < fs / 2)] = 2.0
    hop = nperseg - noverlap
    return dict(freq=freq, start=start, step=step, window=win, nperseg=nperseg, hop=hop, nframes=1 + (nsig - nperseg) // hop,
                detrend=code, scale=1.0 / (fs * s2) if scaling == "density" else 1.0 / (s1 * s1), amp=1.0 / s1, onesided=onesided,
                fold=fold, fs=fs, m=m, cplx=bool(cplx))


def _shape(v):
    if _is_torch(v):
        return v.dim(), v.numel(), v.is_complex()
    a = np.asarray(v)
    return a.ndim, a.size, np.iscomplexobj(a)


def _plan_for(x, y, fn, m, kw):
    sigs = [_shape(v) for v in (x, y) if v is not None]
    if any(ndim != 1 for ndim, _, _ in sigs):
        raise ValueError("zoom: signals must be one-dimensional")
    if len({c for _, _, c in sigs}) != 1:
        raise ValueError("zoom: x and y must both be real or both be complex")
    if len({n for _, n, _ in sigs}) != 1:
        raise ValueError("zoom: x and y must have equal lengths")
    return zoom_plan(sigs[0][1], sigs[0][2], fn, m, **kw)


def _spectra(x, y, fn, m, kw):
    p = _plan_for(x, y, fn, m, kw)
    from . import engine
    out = engine.zoom_welch(x, p["window"], p["hop"], p["nframes"], p["m"], p["start"], p["step"], y=y, detrend=p["detrend"],
                            scale=p["scale"])
    if p["onesided"]:
        fold = p["fold"]
        if _is_torch(out[0]):
            import torch
            fold = torch.as_tensor(fold, dtype=torch.float64, device=out[0].device)
        out = tuple(None if a is None else a * fold for a in out)
    return (p,) + tuple(out)


def zoom_stft(x, fn, m, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=False):
    """(f, t, Z): scipy.signal.stft(boundary=None, padded=False, scaling='spectrum') on the arc: Z[k, g] = X_g[k] / sum(w), complex64
    [m, nframes], t the segment centres."""
    p = _plan_for(x, None, fn, m, dict(fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend,
                                       return_onesided=False))
    from . import engine
    Z = engine.zoom_welch(x, p["window"], p["hop"], p["nframes"], p["m"], p["start"], p["step"], detrend=p["detrend"], scale=p["amp"],
                          frames=True)
    t = (np.arange(p["nframes"], dtype=np.float64) * p["hop"] + p["nperseg"] / 2.0) / p["fs"]
    return p["freq"], t, (Z.transpose(0, 1) if _is_torch(Z) else Z.T)


def _kw(fs, window, nperseg, noverlap, detrend, scaling, return_onesided):
    return dict(fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend, scaling=scaling,
                return_onesided=return_onesided)


def zoom_psd(x, fn, m, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=False, scaling="density", return_onesided=True):
    """(f, Pxx): scipy.signal.welch on the arc, float64 [m]."""
    p, pxx, _, _ = _spectra(x, None, fn, m, _kw(fs, window, nperseg, noverlap, detrend, scaling, return_onesided))
    return p["freq"], pxx


def zoom_csd(x, y, fn, m, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=False, scaling="density", return_onesided=True):
    """(f, Pxy): scipy.signal.csd on the arc (Pxy = mean conj(X) Y), complex128 [m]."""
    if y is None:
        raise ValueError("zoom_csd: y is required")
    p, _, _, pxy = _spectra(x, y, fn, m, _kw(fs, window, nperseg, noverlap, detrend, scaling, return_onesided))
    return p["freq"], pxy


def zoom_coherence(x, y, fn, m, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=False, scaling="density",
                   return_onesided=True):
    """(f, Cxy): the magnitude-squared coherence |Pxy|^2 / (Pxx Pyy) on the arc, 0 where the denominator is 0."""
    if y is None:
        raise ValueError("zoom_coherence: y is required")
    p, pxx, pyy, pxy = _spectra(x, y, fn, m, _kw(fs, window, nperseg, noverlap, detrend, scaling, return_onesided))
    den = pxx * pyy
    num = pxy.real ** 2 + pxy.imag ** 2
    if _is_torch(den):
        import torch
        return p["freq"], torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    return p["freq"], np.divide(num, den, out=np.zeros_like(den), where=den > 0)
