"""Two-point wavenumber-frequency spectra (Beall, Kim & Powers, J. Appl. Phys. 53, 3933 (1982)): two records from probes a distance dx
apart; every frame gives a local wavenumber k(f) = arg(X conj Y) / dx and a power, and the powers of many frames are histogrammed
into S(k, f).

    X_g, Y_g   = FFT(win * (frame g of x, of y, its own mean removed))           hop = nperseg - noverlap
    theta      = arg(X_g[f] conj(Y_g[f]))  in [-pi, pi]                           y[n] = x[n - d] gives theta = +2 pi f d / fs, f > 0
    j          = floor((theta / 2 pi + 1/2) nk) mod nk                           nk equal bins, centred on k_j = (j + 1/2 - nk/2) 2 pi / (nk dx)
    S[f, j]    = scale / M * sum_g p,   p = (|X|^2 + |Y|^2) / 2  ('mean', Beall)  or  |X| |Y|  ('cross')

S is power per k-bin, not divided by the bin width: S.sum(axis=1) is the mean of the two Welch PSDs (scipy.signal.welch's window,
overlap and scaling conventions; real input one-sided with rows 1 .. nperseg/2 - 1 doubled, complex input on an fftshift-ed axis).
From the table come the conditional spectrum s(k|f) = S / P, the statistical dispersion relation kbar(f) and the spectral width
sigma_k(f) (skf_moments).  The histogram is built inside the frame loop of one kernel (k_skf.hip): the two records are read once and
only the table is written.  Segments are powers of two from 32 to 4096: the method wants many realisations per cell."""
import math
import os

import numpy as np

from .engine import _is_torch
from .windows import get_window

MIN_NFFT, MAX_NFFT, MAX_NK = 32, 4096, 1024
LDS_BYTES = 160 * 1024
_POWERS = {"mean": 0, "cross": 1}


class SegmentNotBuilt(ValueError, NotImplementedError):
    """nperseg that is not a power of two in 32 .. 4096: outside the limits, and a path that is not built."""


def _check_shape(who, nperseg, nk):
    if nperseg < MIN_NFFT or nperseg > MAX_NFFT or nperseg & (nperseg - 1):
        raise SegmentNotBuilt("%s: nperseg = %d must be a power of two from %d to %d" % (who, nperseg, MIN_NFFT, MAX_NFFT))
    if nk < 2 or nk > MAX_NK:
        raise ValueError("%s: nk = %d must lie in 2 .. %d" % (who, nk, MAX_NK))


def skf_plan(nperseg, nk, nb=None, cplx=False, cells=None):
    """What a call costs: dict(tiles, tile_bins, lds_bytes, transforms, read, written), the first four as sp_skf_plan reports them.
    The histogram of a band of nb bins (default: all of them) has nb x nk float32 cells and lives in LDS behind the transform
    images.  Where it does not fit, the band is cut into `tiles` frequency tiles of `tile_bins` bins; a workgroup transforms its
    frames whole and bins only its tile, so every frame is transformed and read `tiles` times: transforms = tiles (real input: one
    packed transform per frame) or 2 tiles (complex), read = the bytes of samples a frame loads over all tiles.  written = 0: a frame
    writes nothing, a run of frames leaves one float32 table.  Short segments and limited bands (nperseg 64 .. 1024, where the
    method has the realisations it needs) are a single tile; nperseg = 4096 over the full band with nk = 128 is 10.
    cells: a cap on nk x tile_bins (default: the SP_SKF_CELLS test hook, else none).  Host only."""
    nperseg, nk, cplx = int(nperseg), int(nk), bool(cplx)
    _check_shape("skf_plan", nperseg, nk)
    nbins = nperseg if cplx else nperseg // 2 + 1
    nb = nbins if nb is None else int(nb)
    if not 1 <= nb <= nbins:
        raise ValueError("skf_plan: nb must lie in 1 .. %d" % nbins)
    if cells is None:
        cells = int(os.environ.get("SP_SKF_CELLS", "0") or 0)
    images = max(1, 4096 // nperseg) * (nperseg + 16) * 8 * (2 if cplx else 1)
    room = (LDS_BYTES - images) // 4 // nk
    gran = 32
    while gran > 1 and room < gran:
        gran //= 2
    tb = min(room // gran * gran, nb)
    if cells > 0:
        tb = min(tb, max(1, cells // nk))
    tiles = -(-nb // tb)
    stride = -(-tb // gran) * gran
    esz = 8 if cplx else 4
    return dict(tiles=tiles, tile_bins=tb, lds_bytes=images + 4 * nk * stride, transforms=tiles * (2 if cplx else 1),
                read=2 * esz * nperseg * tiles, written=0)


def _prepare(who, x, y, fs, dx, nperseg, noverlap, window, nk, band, detrend, power, scaling):
    """Every check, before the library is touched -> the engine's arguments, f, k and the per-row fold (or None)."""
    dev = _is_torch(x)
    if dev != _is_torch(y):
        raise ValueError("%s: x and y must both be arrays or both be device tensors" % who)
    if not dev:
        x, y = np.asarray(x), np.asarray(y)
    if len(x.shape) != 1 or len(y.shape) != 1:
        raise ValueError("%s: x and y must be one-dimensional" % who)
    if x.shape[0] != y.shape[0]:
        raise ValueError("%s: x and y must have equal lengths" % who)
    cplx = bool(x.is_complex() if dev else np.iscomplexobj(x))
    if cplx != bool(y.is_complex() if dev else np.iscomplexobj(y)):
        raise ValueError("%s: x and y must both be real or both be complex" % who)
    fs, dx = float(fs), float(dx)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    if not (dx > 0 and math.isfinite(dx)):
        raise ValueError("%s: dx must be positive and finite" % who)
    nperseg, nk, nsig = int(nperseg), int(nk), int(x.shape[0])
    _check_shape(who, nperseg, nk)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < nperseg:
        raise ValueError("%s: need 0 <= noverlap < nperseg" % who)
    if nsig < nperseg:
        raise ValueError("%s: the record (%d samples) is shorter than a segment (%d)" % (who, nsig, nperseg))
    if isinstance(window, (str, tuple)):
        win = np.asarray(get_window(window, nperseg), dtype=np.float64)
    else:
        win = np.asarray(window, dtype=np.float64)
    if win.shape != (nperseg,):
        raise ValueError("%s: window must be a name or nperseg = %d values" % (who, nperseg))
    if not np.all(np.isfinite(win)):
        raise ValueError("%s: the window must be finite" % who)
    if detrend not in ("constant", "none", False, None):
        raise ValueError("%s: detrend must be 'constant' (every segment's own mean) or False" % who)
    if power not in _POWERS:
        raise ValueError("%s: power must be 'mean' or 'cross'" % who)
    if scaling == "density":
        scale = 1.0 / (fs * np.sum(win * win))
    elif scaling == "spectrum":
        scale = 1.0 / np.sum(win) ** 2
    else:
        raise ValueError("%s: scaling must be 'density' or 'spectrum'" % who)
    if not math.isfinite(scale):
        raise ValueError("%s: the window has no weight" % who)
    # the bins: real input 0 .. nperseg/2 in order, complex input fftshift-ed (natural bin nperseg/2 first)
    if cplx:
        f = np.fft.fftshift(np.fft.fftfreq(nperseg, 1.0 / fs))
        first = nperseg // 2
    else:
        f = np.fft.rfftfreq(nperseg, 1.0 / fs)
        first = 0
    lo, hi = 0, f.size
    if band is not None:
        try:
            fmin, fmax = (float(v) for v in band)
        except (TypeError, ValueError):
            raise ValueError("%s: band must be a pair (fmin, fmax)" % who)
        if not (math.isfinite(fmin) and math.isfinite(fmax) and fmin <= fmax):
            raise ValueError("%s: band must be a pair of finite frequencies with fmin <= fmax" % who)
        if fmin < (-0.5 * fs if cplx else 0.0) or fmax > 0.5 * fs:
            raise ValueError("%s: the band (%g, %g) lies outside the spectrum" % (who, fmin, fmax))
        inside = np.nonzero((f >= fmin) & (f <= fmax))[0]
        if inside.size == 0:
            raise ValueError("%s: the band (%g, %g) is empty: no bin lies inside it" % (who, fmin, fmax))
        lo, hi = int(inside[0]), int(inside[-1]) + 1
    f = f[lo:hi]
    b0, nb = (first + lo) % nperseg if cplx else lo, hi - lo
    fold = None
    if not cplx:
        bins = np.arange(lo, hi)
        fold = np.where((bins >= 1) & (bins <= nperseg // 2 - 1), 2.0, 1.0)
    hop = nperseg - noverlap
    k = (np.arange(nk) + 0.5 - 0.5 * nk) * (2.0 * math.pi / (nk * dx))
    args = dict(nfft=nperseg, hop=hop, nframes=1 + (nsig - nperseg) // hop, b0=b0, nb=nb, nk=nk, win=win,
                segmean=detrend == "constant", cross=power == "cross", scale=scale)
    return args, f, k, fold


def skf(x, y, fs, dx, nperseg=256, noverlap=None, window="hann", nk=65, band=None, detrend="constant", power="mean",
        scaling="density"):
    """(f, k, S): the two-point wavenumber-frequency spectrum of two records x, y (both real or both complex, equal lengths) sampled at
    fs by probes dx apart.  S float64 [len(f), nk]; k are the nk bin centres, -pi/dx < k < pi/dx; f = rfftfreq(nperseg, 1/fs) for real
    input (one-sided: rows 1 .. nperseg/2 - 1 doubled), fftshift(fftfreq(nperseg, 1/fs)) for complex input, both cut to
    band=(fmin, fmax) if given (inclusive; for complex input it may run through zero).  noverlap (default nperseg // 2), window
    (a name, a (name, parameter) tuple or nperseg values) and scaling ('density', 'spectrum') as scipy.signal.welch; detrend
    'constant' removes every segment's own mean, False nothing; power 'mean' = (|X|^2 + |Y|^2) / 2 (Beall), 'cross' = |X| |Y|.
    S is power per k-bin: S.sum(axis=1) is the mean of the two Welch PSDs ('mean').  A positive k is a structure that reaches x
    first: y[n] = x[n - d] puts the power of f > 0 at k = +2 pi f d / (fs dx).  numpy in -> numpy out; device tensors in -> S on the
    device (f, k stay numpy)."""
    args, f, k, fold = _prepare("skf", x, y, fs, dx, nperseg, noverlap, window, nk, band, detrend, power, scaling)
    from . import engine
    S = engine.skf(x, y, **args)
    if fold is not None:
        if _is_torch(S):
            import torch
            S = S * torch.as_tensor(fold, dtype=torch.float64, device=S.device)[:, None]
        else:
            S = S * fold[:, None]
    return f, k, S


def skf_moments(k, S):
    """The moments of a table S[nf, nk] over the wavenumbers k[nk], host float64: dict(P = sum_k S (the power at f), s = S / P (the
    conditional spectrum s(k|f), 0 where P = 0), kbar = sum_k k s (the statistical dispersion relation), sigma_k = sqrt(sum_k
    (k - kbar)^2 s) (the spectral width), S_k = sum_f S (the wavenumber spectrum)).  A device tensor is copied to the host."""
    if _is_torch(S):
        S = S.detach().cpu().numpy()
    S, k = np.asarray(S, dtype=np.float64), np.asarray(k, dtype=np.float64)
    if S.ndim != 2 or k.shape != (S.shape[1],):
        raise ValueError("skf_moments: S must be [nf, nk] and k must hold nk values")
    P = S.sum(axis=1)
    s = np.divide(S, P[:, None], out=np.zeros_like(S), where=P[:, None] > 0)
    kbar = s @ k
    var = np.sum((k[None, :] - kbar[:, None]) ** 2 * s, axis=1)
    return dict(P=P, s=s, kbar=kbar, sigma_k=np.sqrt(np.maximum(var, 0.0)), S_k=S.sum(axis=0))


def dispersion(x, y, fs, dx, nperseg=256, noverlap=None, window="hann", nk=65, band=None, detrend="constant", power="mean",
               scaling="density"):
    """(f, kbar, sigma_k, P): the statistical dispersion relation kbar(f), the spectral width sigma_k(f) and the power P(f) of skf's
    table in one call (host float64; arguments as skf)."""
    f, k, S = skf(x, y, fs, dx, nperseg, noverlap, window, nk, band, detrend, power, scaling)
    m = skf_moments(k, S)
    return f, m["kbar"], m["sigma_k"], m["P"]
