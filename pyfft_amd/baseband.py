"""Digital down-conversion and the spectra of a band: mix a record with a carrier, low-pass it and decimate by q -- one streaming pass
of k_ddc.hip per stage -- then run the library's STFT / Welch estimators on the complex baseband signal at the rate fs / q.

    v[n] = x[n] exp(-2 pi i fc (n0 + n) / fs);    y[k] = sum_j h[j] v[k q + (T - 1) / 2 - j],  k < ceil(n / q)

which is scipy.signal.resample_poly(v, 1, q, window=h) for the odd-length low-pass h.  ddc_plan designs h (Kaiser windows), as a cascade
of stages for q > 64; ddc runs it; band_stft / band_psd / band_csd / band_coherence are scipy.signal's stft(boundary=None, padded=False)
/ welch / csd / coherence with detrend=False on the result, two-sided, fftshift-ed, cut to the bins the filter leaves free of aliases
and put back on the frequency axis of the input: f = fc + fftshift(fftfreq(nperseg, q / fs))[kept].  For a narrow band this is the
cheap zoom: the transforms are q times shorter than those of zoom.zoom_psd at the same resolution.
"""
import math

import numpy as np

from .engine import _is_torch
from .windows import get_window

MAX_Q = 64                          # one launch decimates by at most this
MAX_TAPS = 4095                     # and takes at most this many taps
MAX_WG_FFT = 8192                   # the longest one-workgroup transform (sp_max_wg_fft)


class Unsupported(ValueError, NotImplementedError):
    """A decimation or a filter outside the limits of the kernel: a path that is not built."""


def _factor(q):
    """q as a product of factors <= MAX_Q, the largest first."""
    out, rest = [], q
    while rest > 1:
        f = max(d for d in range(1, MAX_Q + 1) if rest % d == 0)
        if f == 1:
            raise Unsupported("ddc: q = %d has a prime factor above %d: no cascade of stages <= %d reaches it" % (q, MAX_Q, MAX_Q))
        out.append(f)
        rest //= f
    return out or [1]


def ddc_plan(q, atten=90.0, width=0.2, taps=None):
    """The stages [(q_i, h_i)] of a down-conversion by q (pure numpy / scipy, never loads the library): q_i <= 64 with product q, h_i
    float64 low-pass taps of odd length <= 4095.  Kaiser designs with `atten` dB of stopband: every stage passes the band up to
    (1 - width) / (2 q) cycles per sample of the input; the last stops from 1 / (2 q), an earlier one, running at the rate 1 / Q and
    decimating by q_i, from 1 / (Q q_i) - 1 / (2 q): whatever it aliases lands outside the final passband.  taps=: one stage with the
    caller's own real odd-length taps (q <= 64)."""
    if isinstance(q, bool) or int(q) != q or int(q) < 1:
        raise ValueError("ddc: q must be a positive integer, got %r" % (q,))
    q = int(q)
    if taps is not None:
        if np.iscomplexobj(taps):
            raise ValueError("ddc: the taps must be real")
        h = np.asarray(taps, dtype=np.float64)
        if h.ndim != 1 or h.size < 1 or h.size % 2 == 0:
            raise ValueError("ddc: the taps must be a one-dimensional array of odd length")
        if not np.all(np.isfinite(h)):
            raise ValueError("ddc: the taps must be finite")
        if h.size > MAX_TAPS:
            raise Unsupported("ddc: %d taps are beyond the %d one launch takes" % (h.size, MAX_TAPS))
        if q > MAX_Q:
            raise Unsupported("ddc: explicit taps are one stage, q <= %d" % MAX_Q)
        return [(q, h)]
    atten, width = float(atten), float(width)
    if not 0.0 < width < 1.0:
        raise ValueError("ddc: width must lie in (0, 1), got %r" % width)
    if not (math.isfinite(atten) and atten > 0):
        raise ValueError("ddc: atten must be positive, got %r" % atten)
    import scipy.signal as ss
    fp = (1.0 - width) / (2.0 * q)
    stages, Q = [], 1
    factors = _factor(q)
    for i, qi in enumerate(factors):
        last = i == len(factors) - 1
        fstop = 1.0 / (2.0 * q) if last else 1.0 / (Q * qi) - 1.0 / (2.0 * q)
        # in cycles per sample of this stage's own input rate 1 / Q
        lo, hi = fp * Q, fstop * Q
        numtaps, beta = ss.kaiserord(atten, (hi - lo) / 0.5)
        numtaps |= 1
        if numtaps > MAX_TAPS:
            raise Unsupported("ddc: stage %d (q = %d) needs %d taps for atten = %g, width = %g; one launch takes %d" %
                              (i, qi, numtaps, atten, width, MAX_TAPS))
        stages.append((qi, ss.firwin(numtaps, 0.5 * (lo + hi), window=("kaiser", beta), fs=1.0)))
        Q *= qi
    return stages


def ddc(x, fc, q, fs=1.0, *, atten=90.0, width=0.2, taps=None, n0=0, axis=-1):
    """The complex64 baseband signal of x around fc at the rate fs / q, along `axis`: mixed with exp(-2 pi i fc (n0 + n) / fs),
    filtered and decimated by the stages of ddc_plan.  n0 is the absolute index of the first sample, so that the chunks of one
    stream continue the oscillator; with more than one stage it must be a multiple of the decimation of all stages but the last.
    numpy in -> numpy out, device tensor in -> device tensor out; between stages the signal stays on the device."""
    fs, fc, n0 = float(fs), float(fc), int(n0)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("ddc: fs must be positive")
    if not math.isfinite(fc):
        raise ValueError("ddc: fc must be finite")
    stages = ddc_plan(q, atten, width, taps)
    done = 1
    for qi, _ in stages[:-1]:
        done *= qi
    if n0 % done:
        raise ValueError("ddc: n0 = %d is not divisible by %d, the decimation applied before the last stage" % (n0, done))
    dev = _is_torch(x)
    nd = x.dim() if dev else np.ndim(x)
    if nd < 1:
        raise ValueError("ddc: x must have at least one axis")
    if not -nd <= axis < nd:
        raise ValueError("ddc: axis %d is out of range" % axis)
    from . import engine
    last = axis in (-1, nd - 1)
    if dev:
        y = x if last else x.movedim(axis, -1)
    else:
        y = np.asarray(x) if last else np.moveaxis(np.asarray(x), axis, -1)
        if len(stages) > 1 and engine.torch is not None:
            from . import _ffi
            y = engine.torch.as_tensor(_ffi.as_samples(y), device="cuda")       # the intermediates stay on the device
    for i, (qi, h) in enumerate(stages):
        y = engine.ddc(y, fc / fs if i == 0 else 0.0, qi, h, n0 if i == 0 else 0)
    if not dev and _is_torch(y):
        y = y.cpu().numpy()
    if last:
        return y
    return y.movedim(-1, axis) if dev else np.moveaxis(y, -1, axis)


def band_plan(nsig, cplx, fc, q, fs=1.0, window="hann", nperseg=256, noverlap=None, scaling="density", return_onesided=True,
              width=0.2):
    """The validated host plan of a band spectrum (pure numpy, never loads the library): a dict with freq (float64: the kept bins on
    the input's frequency axis), keep (their indices in the fftshift-ed two-sided spectrum), window (float64 [nperseg]), nperseg, hop,
    nframes (of the baseband record of ceil(nsig / q) samples), scale (scipy.signal.welch's at the rate fs / q), amp (scipy.signal.stft's:
    1 / sum w for 'spectrum', 1 / sqrt(fs / q sum w^2) for 'density'), fold (2 for a real input with return_onesided, else 1)."""
    who = "band"
    nsig, q, fs, fc, width = int(nsig), int(q), float(fs), float(fc), float(width)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    if not math.isfinite(fc):
        raise ValueError("%s: fc must be finite" % who)
    if q < 1:
        raise ValueError("%s: q must be a positive integer" % who)
    if not 0.0 < width < 1.0:
        raise ValueError("%s: width must lie in (0, 1), got %r" % (who, width))
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
    pow2 = nperseg & (nperseg - 1) == 0
    if nperseg < 2 or nperseg > (MAX_WG_FFT if pow2 else MAX_WG_FFT // 2):
        raise Unsupported("%s: nperseg = %d is not a length the one-workgroup transforms take (powers of two from 2 to %d, other "
                          "lengths up to %d); a longer segment of the baseband signal means a smaller q" %
                          (who, nperseg, MAX_WG_FFT, MAX_WG_FFT // 2))
    nb = -(-nsig // q)
    if nb < nperseg:
        raise ValueError("%s: the baseband record (%d samples) is shorter than nperseg (%d)" % (who, nb, nperseg))
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap < 0 or noverlap >= nperseg:
        raise ValueError("%s: need 0 <= noverlap < nperseg" % who)
    if scaling not in ("density", "spectrum"):
        raise ValueError("%s: scaling must be 'density' or 'spectrum'" % who)
    s1, s2 = float(np.sum(win)), float(np.sum(win * win))
    if not s2 > 0 or s1 == 0:
        raise ValueError("%s: the window sums to zero" % who)
    fsb = fs / q
    half = (1.0 - width) * fs / (2.0 * q)
    grid = np.fft.fftshift(np.fft.fftfreq(nperseg, q / fs))
    keep = np.nonzero(np.abs(grid) <= half * (1.0 + 1e-12))[0]
    onesided = bool(return_onesided) and not cplx
    if onesided and not (fc - half > 0 and fc + half < fs / 2):
        raise ValueError("%s: a one-sided spectrum lives on [0, fs / 2]; the band [%g, %g] leaves it (return_onesided=False gives "
                         "the two-sided values)" % (who, fc - half, fc + half))
    hop = nperseg - noverlap
    return dict(freq=fc + grid[keep], keep=keep, window=win, nperseg=nperseg, hop=hop, nframes=1 + (nb - nperseg) // hop,
                scale=1.0 / (fsb * s2) if scaling == "density" else 1.0 / (s1 * s1),
                amp=1.0 / s1 if scaling == "spectrum" else 1.0 / math.sqrt(fsb * s2), onesided=onesided,
                fold=2.0 if onesided else 1.0, fs=fs, fsb=fsb, q=q, fc=fc, cplx=bool(cplx))


def _shape(v):
    if _is_torch(v):
        return v.dim(), v.numel(), v.is_complex()
    a = np.asarray(v)
    return a.ndim, a.size, np.iscomplexobj(a)


def _baseband(x, y, fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, atten, width):
    """(plan, zx, zy, to_caller): the plan, the device-resident baseband signals, and the map of a result back to the caller's kind."""
    sigs = [_shape(v) for v in (x, y) if v is not None]
    if any(ndim != 1 for ndim, _, _ in sigs):
        raise ValueError("band: signals must be one-dimensional")
    if len({c for _, _, c in sigs}) != 1:
        raise ValueError("band: x and y must both be real or both be complex")
    if len({n for _, n, _ in sigs}) != 1:
        raise ValueError("band: x and y must have equal lengths")
    p = band_plan(sigs[0][1], sigs[0][2], fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, width)
    ddc_plan(q, atten, width)                                   # its refusals, before the library loads
    from . import engine, _ffi
    dev = _is_torch(x)
    if engine.torch is None:
        raise _ffi.SpectralError("band spectra keep the baseband signal on the device: torch is required")

    def resident(v):
        return v if _is_torch(v) else engine.torch.as_tensor(_ffi.as_samples(v), device="cuda")
    zx = ddc(resident(x), fc, q, fs, atten=atten, width=width)
    zy = None if y is None else ddc(resident(y), fc, q, fs, atten=atten, width=width)
    return p, zx, zy, (lambda a: a) if dev else (lambda a: a.cpu().numpy())


def _cut(a, p):
    """fftshift-ed two-sided bins (last axis) -> the kept ones."""
    from . import engine
    return a[..., engine.torch.as_tensor(p["keep"], device=a.device)]


def band_stft(x, fc, q, fs=1.0, window="hann", nperseg=256, noverlap=None, scaling="density", return_onesided=True, atten=90.0,
              width=0.2):
    """(f, t, Z): scipy.signal.stft(boundary=None, padded=False, return_onesided=False) of the baseband signal of x around fc, on the
    kept bins: complex64 [len(f), nframes], t the segment centres in seconds.  scaling 'density' (scipy.signal.stft's 'psd') or
    'spectrum'.  As in scipy, an STFT is never doubled; return_onesided only asks that the band of a real x lie in (0, fs / 2)."""
    p, zx, _, back = _baseband(x, None, fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, atten, width)
    from . import engine
    Z, _ = engine.stft_frames(zx, p["window"], p["hop"], p["nframes"], detrend=False, sided=engine.SIDED_TWO, amp_scale=p["amp"])
    t = (np.arange(p["nframes"], dtype=np.float64) * p["hop"] + p["nperseg"] / 2.0) / p["fsb"]
    return p["freq"], t, back(_cut(Z, p).transpose(0, 1))


def band_psd(x, fc, q, fs=1.0, window="hann", nperseg=256, noverlap=None, scaling="density", return_onesided=True, atten=90.0,
             width=0.2):
    """(f, Pxx): scipy.signal.welch(detrend=False) of the baseband signal of x around fc on the kept bins, float64; doubled for a real
    x with return_onesided (the band must then lie inside (0, fs / 2))."""
    p, zx, _, back = _baseband(x, None, fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, atten, width)
    from . import engine
    pxx = engine.welch_psd(zx, p["window"], p["hop"], p["nframes"], detrend=False, sided=engine.SIDED_TWO, scale=p["scale"] * p["fold"])
    return p["freq"], back(_cut(pxx, p))


def _cross(x, y, fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, atten, width, who):
    if y is None:
        raise ValueError("%s: y is required" % who)
    p, zx, zy, back = _baseband(x, y, fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, atten, width)
    from . import engine
    pxx, pyy, pxy = engine.welch_csd(zx, zy, p["window"], p["hop"], p["nframes"], detrend=False, sided=engine.SIDED_TWO,
                                     scale=p["scale"] * p["fold"])
    return p, _cut(pxx, p), _cut(pyy[0], p), _cut(pxy[0], p), back


def band_csd(x, y, fc, q, fs=1.0, window="hann", nperseg=256, noverlap=None, scaling="density", return_onesided=True, atten=90.0,
             width=0.2):
    """(f, Pxy): scipy.signal.csd(detrend=False) of the two baseband signals (Pxy = mean conj(X) Y), complex128."""
    p, _, _, pxy, back = _cross(x, y, fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, atten, width, "band_csd")
    return p["freq"], back(pxy)


def band_coherence(x, y, fc, q, fs=1.0, window="hann", nperseg=256, noverlap=None, scaling="density", return_onesided=True,
                   atten=90.0, width=0.2):
    """(f, Cxy): the magnitude-squared coherence |Pxy|^2 / (Pxx Pyy) of the two baseband signals, 0 where the denominator is 0."""
    p, pxx, pyy, pxy, back = _cross(x, y, fc, q, fs, window, nperseg, noverlap, scaling, return_onesided, atten, width,
                                    "band_coherence")
    from . import engine
    torch = engine.torch
    den = pxx * pyy
    num = pxy.real ** 2 + pxy.imag ** 2
    return p["freq"], back(torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den)))
