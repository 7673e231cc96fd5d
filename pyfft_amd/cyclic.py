"""Cyclostationary analysis on the GPU: the spectral correlation density S^alpha(f) and the cyclic coherence gamma^alpha(f) of records whose
statistics are periodic in time (amplitude-modulated turbulence, IQ signals with a symbol or sweep rate, rotating-machinery noise).

The estimator is the averaged cyclic periodogram (Gardner 1986; Antoni, "Cyclic spectral analysis in practice", MSSP 2007): for every
cycle frequency alpha a Welch cross spectrum between the record shifted down and up by alpha / 2,

    S_yx^alpha(f_k) = scale/K sum_g DFT(w (y - m_y) e^{-i pi alpha t / fs})[k] conj(DFT(w (x - m_x) e^{+i pi alpha t / fs})[k])

at f_k = k fs / nperseg (two-sided, fft order): y at f_k + alpha / 2 against x at f_k - alpha / 2.  It holds for ANY alpha, on or off
any grid, and one fused kernel (engine.cyclic, sp_cyclic) runs the whole list of alphas over the frames; a real record, and the
conjugate form of a complex one, take one transform per frame and alpha, the other forms two.  Phases are exact over records of any
length: t is the absolute sample index first + n, and the phase is formed in 64-bit integer arithmetic modulo one turn, so records cut
at frame starts give un-normalised S that add up (pass each part its own `first`).

noverlap defaults to 3/4 of nperseg, not scipy's 1/2: Antoni (2007) shows that the cyclic periodogram under a Hann window at 50 % overlap
leaks cyclic power (the window's own periodicity at fs / hop aliases into alpha); 2/3 or more is needed, 3/4 is the customary choice.

What is not here: the estimators that tile the whole (f, alpha) plane at once (the FFT accumulation method is pyfft_amd.fam, the blind
search that tells which alpha to pass here; the strip spectral correlation analyzer is not built); the cyclic modulation spectrum and Fast-SC (an FFT along the frames of an STFT: compose stft_frames and engine.fft); segments that are no power
of two or longer than 8192; per-segment detrending.  Those raise CyclicRefused, which is a ValueError and a NotImplementedError.
"""
import numpy as np

from .windows import get_window
from . import engine as _engine
from .engine import CyclicRefused, _is_torch

MIN_NPERSEG, MAX_NPERSEG = _engine.CYC_MIN_N, _engine.CYC_MAX_N


def _setup(who, nsig, fs, alphas, window, nperseg, noverlap, detrend, scaling):
    """(win float64, hop, nframes, nu, scale, detrend flag): everything refused here is refused before the library is touched"""
    if not np.isfinite(fs) or fs <= 0:
        raise CyclicRefused("%s: fs must be positive" % who)
    nperseg = int(nperseg)
    if nperseg < MIN_NPERSEG or nperseg > MAX_NPERSEG or nperseg & (nperseg - 1):
        raise CyclicRefused("%s: nperseg = %d must be a power of two from %d to %d: other segment lengths are not built"
                            % (who, nperseg, MIN_NPERSEG, MAX_NPERSEG))
    if isinstance(window, (str, tuple)):
        win = np.asarray(get_window(window, nperseg), dtype=np.float64)
    else:
        win = np.asarray(window, dtype=np.float64)
    if win.shape != (nperseg,) or not np.all(np.isfinite(win)) or not np.sum(win ** 2) > 0:
        raise CyclicRefused("%s: the window must hold nperseg = %d finite values, not all zero" % (who, nperseg))
    noverlap = 3 * nperseg // 4 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < nperseg:
        raise CyclicRefused("%s: need 0 <= noverlap < nperseg" % who)
    if detrend not in (False, None, "none", 0, True, "constant", "mean", 1):
        raise CyclicRefused("%s: detrend must be False or 'constant' (the record's mean): per-segment and linear detrending are not built" % who)
    if scaling not in ("density", "spectrum"):
        raise CyclicRefused("%s: scaling must be 'density' or 'spectrum'" % who)
    hop = nperseg - noverlap
    nframes = (nsig - nperseg) // hop + 1 if nsig >= nperseg else 0
    if nframes < 1:
        raise CyclicRefused("%s: the record of %d samples holds no segment of %d" % (who, nsig, nperseg))
    al = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
    if al.ndim != 1 or al.size < 1:
        raise CyclicRefused("%s: alphas must be one axis of at least one cycle frequency" % who)
    nu = al / float(fs)
    _engine.cyclic_check(who, nperseg, hop, nframes, int(nu.size), 1, nsig, None, nu)
    scale = 1.0 / (fs * np.sum(win ** 2)) if scaling == "density" else 1.0 / np.sum(win) ** 2
    return win, hop, nframes, al, nu, scale / nframes, detrend not in (False, None, "none", 0)


def _run(who, x, alphas, fs, window, nperseg, noverlap, detrend, scaling, y, conjugate, first, want):
    if x is None or getattr(x, "ndim", np.ndim(x)) < 1:
        raise CyclicRefused("%s: x must have at least one axis" % who)
    nsig = int(x.shape[-1]) if hasattr(x, "shape") else int(np.asarray(x).shape[-1])
    win, hop, nframes, al, nu, scale, det = _setup(who, nsig, fs, alphas, window, nperseg, noverlap, detrend, scaling)
    if not _is_torch(x):
        x = np.asarray(x)
        y = None if y is None else np.asarray(y)
    S, Pp, Pm = _engine.cyclic(x, win, hop, nframes, nu, y=y, conj=bool(conjugate), first=int(first), detrend=det, scale=scale,
                               S=want[0], Pp=want[1], Pm=want[2])
    f = np.fft.fftfreq(int(nperseg), 1.0 / fs)
    return f, al, S, Pp, Pm


def _gamma(S, Pp, Pm):
    """S / sqrt(Pp Pm) in float64 (0 where the denominator is 0)"""
    if _is_torch(S):
        import torch
        den = torch.sqrt(Pp.double() * Pm.double())
        return torch.where(den > 0, S.to(torch.complex128) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(S, dtype=torch.complex128))
    den = np.sqrt(Pp.astype(np.float64) * Pm.astype(np.float64))
    return np.where(den > 0, S.astype(np.complex128) / np.where(den > 0, den, 1.0), 0.0)


def scd(x, alphas, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend="constant", scaling="density", y=None, conjugate=False,
        first=0):
    """The spectral correlation density along the last axis: f, alphas, S with S complex64 [..., A, nperseg] at f = fftfreq(nperseg, 1/fs),
    scaled as scipy.signal.csd ('density': per Hz, 'spectrum').  S[a, k] estimates the correlation of y at f_k + alpha_a / 2 with x at
    f_k - alpha_a / 2; y=None: y = x; conjugate=True: x is replaced by its conjugate (the conjugate spectral correlation S_xx*, the one
    that shows carriers and symbol rates of IQ records).  alpha = 0 is the Welch CSD / PSD.  first: the absolute index of x's first sample.
    noverlap defaults to 3 nperseg / 4 (see the module docstring).  numpy in -> numpy out; device tensors in -> device tensors."""
    f, al, S, _, _ = _run("scd", x, alphas, fs, window, nperseg, noverlap, detrend, scaling, y, conjugate, first, (True, False, False))
    return f, al, S


def cyclic_spectra(x, alphas, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend="constant", scaling="density", y=None,
                   conjugate=False, first=0):
    """Everything from one pass: f, alphas, S, Pp, Pm, gamma.  Pp[a, k] is the PSD of y at f_k + alpha_a / 2, Pm that of x at
    f_k - alpha_a / 2 (float32), gamma = S / sqrt(Pp Pm) the cyclic coherence (complex128, formed in float64)."""
    f, al, S, Pp, Pm = _run("cyclic_spectra", x, alphas, fs, window, nperseg, noverlap, detrend, scaling, y, conjugate, first,
                            (True, True, True))
    return f, al, S, Pp, Pm, _gamma(S, Pp, Pm)


def cyclic_coherence(x, alphas, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend="constant", y=None, conjugate=False, first=0):
    """The cyclic coherence gamma^alpha(f) = S / sqrt(Pp Pm): f, alphas, gamma (complex128 [..., A, nperseg], |gamma| <= 1), from one pass.
    |gamma|^2 of a record without cyclostationarity at alpha exceeds cyclic_level(...) with probability p."""
    f, al, S, Pp, Pm = _run("cyclic_coherence", x, alphas, fs, window, nperseg, noverlap, detrend, "density", y, conjugate, first,
                            (True, True, True))
    return f, al, _gamma(S, Pp, Pm)


def cyclic_profile(g, band=None):
    """The alpha-domain profile of gamma (or S) [..., A, nf]: the mean over f of |g|^2, for gamma the enhanced envelope spectrum.  band =
    (lo, hi) keeps the bins lo .. hi - 1 of the last axis.  A reduction on the returned array: no kernel."""
    if band is not None:
        g = g[..., int(band[0]):int(band[1])]
    if _is_torch(g):
        return (g.abs().double() ** 2).mean(dim=-1)
    return np.mean(np.abs(np.asarray(g)).astype(np.float64) ** 2, axis=-1)


def alpha_grid(nsig, fs, amax, oversample=1):
    """Cycle frequencies 0, d, 2 d, .. <= amax at the cyclic resolution d = fs / nsig (/ oversample): what a record of nsig samples
    resolves in alpha, whatever nperseg is."""
    if nsig < 1 or not fs > 0 or amax < 0 or oversample < 1:
        raise CyclicRefused("alpha_grid: need nsig >= 1, fs > 0, amax >= 0 and oversample >= 1")
    d = float(fs) / (int(nsig) * int(oversample))
    return d * np.arange(int(np.floor(amax / d + 1e-9)) + 1)


def effective_segments(nframes, window, hop):
    """Welch's equivalent number of independent segments of K overlapped frames: K / (1 + 2 sum_{m >= 1} (1 - m / K) rho(m)^2),
    rho(m) = sum_j w[j] w[j + m hop] / sum w^2."""
    K, hop = int(nframes), int(hop)
    w = np.asarray(window, dtype=np.float64)
    if K < 1 or hop < 1 or w.ndim != 1 or w.size < 1:
        raise CyclicRefused("cyclic_level: need nframes >= 1, hop >= 1 and a window of one axis")
    den, e = 1.0, float(np.sum(w ** 2))
    for m in range(1, min(K, (w.size - 1) // hop + 1)):
        rho = float(np.sum(w[:w.size - m * hop] * w[m * hop:])) / e
        den += 2.0 * (1.0 - m / K) * rho ** 2
    return K / den


def cyclic_level(nframes, window, hop, p=0.05):
    """The level |gamma|^2 exceeds with probability p where the record is NOT cyclostationary at alpha: 1 - p^(1 / (K_eff - 1)), with
    K_eff = effective_segments(...).  running.coherence_level takes its navg as independent; at 75 % overlap that level is badly
    optimistic (a fifth of the cells of white noise exceed its 5 % level), so this one carries the correction.  window: the taps."""
    if not 0 < p < 1:
        raise CyclicRefused("cyclic_level: p must lie strictly between 0 and 1")
    ke = effective_segments(nframes, window, hop)
    return 1.0 if ke <= 1 else 1.0 - p ** (1.0 / (ke - 1.0))


def cyclic_plan(nsig, alphas, fs=1.0, nperseg=256, noverlap=None, cplx=False, cross=False, conjugate=False, rows=1):
    """What a call will do (host only): nframes, hop and sp_cyclic_plan's figures (fpg, workgroups, alpha_per_pass, passes, transforms)."""
    _, hop, nframes, al, _, _, _ = _setup("cyclic_plan", int(nsig), fs, alphas, "hann", nperseg, noverlap, "constant", "density")
    d = _engine.cyclic_plan(int(nperseg), hop, nframes, al.size, rows=rows, cplx=cplx, cross=cross, conj=conjugate)
    d.update(nframes=nframes, hop=hop)
    return d
