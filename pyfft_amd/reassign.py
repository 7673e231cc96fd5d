"""Time-frequency reassignment: the synchrosqueezed STFT (FSST) and the reassignment operators of every STFT cell (Auger & Flandrin,
IEEE Trans. SP 43, 1068 (1995); Daubechies, Lu & Wu, ACHA 30, 243 (2011); Thakur & Wu, SIAM J. Math. Anal. 43, 2078 (2011); Oberlin,
Meignen & Perrier, ICASSP 2014).

Frame g of a record is the n = nperseg samples from first + g hop on (zero outside the record), c = n / 2.  Under the three windows
h, dh = dh/dj and th = (j - c) h:

    X_h, X_d, X_t = FFT(h x), FFT(dh x), FFT(th x)
    khat = k - (n / 2 pi) Im(X_d conj X_h) / |X_h|^2            the instantaneous frequency of cell (g, k), in bins
    that = first + g hop + c + Re(X_t conj X_h) / |X_h|^2        its group delay, in samples
    used = |X_h| > max(gamma, rel * the frame's largest |X_h|)
    T[g, m] = sum over the used k with rint(khat) = m of (-1)^k X_h[g, k]       the synchrosqueezed transform
    P[g, m] = the same sum of |X_h[g, k]|^2                                     the frequency-reassigned spectrogram

The phase of T is referred to the frame's centre, so that a band of T summed over its bins and divided by n h[c] is that band's
analytic waveform at the frame centres: with boundary='zeros' (first = -n/2) and hop = 1 frame g is centred on sample g and the sum is
the waveform at full rate; with hop > 1 it is the same waveform sampled at the frame centres, carrier included (nothing interpolates).
Real records have the bins 0 .. n/2 and the modes are 2 Re of the sums; complex records have all n bins in FFT order, targets modulo n.

Everything runs in one kernel (pyfft_amd/csrc/k_ssq.hip): a real record costs one transform per frame for T or P (h x + i dh x, split by
symmetry), one more for the fields.  The squeeze is a scatter inside the frame, summed exactly in 64-bit fixed point in LDS, so the
results are bitwise reproducible.  Segments are powers of two from 32 to 8192; a band and output set whose accumulators do not fit
the LDS of a workgroup is refused (ssq_plan tells), never shrunk."""
import importlib
import math

import numpy as np

from . import engine as E
from .engine import SsqRefused, _is_torch

W = importlib.import_module(".windows", __package__)     # (the package rebinds the name `windows` to the function)

DEFAULT_THRESHOLD = 1e-4            # relative to the frame's largest cell: -80 dB

_COSINE = {W.hann: (0.5, 0.5), W.hamming: (0.54, 0.46), W.blackman: W._COSINE_SUMS["blackman"], W.nuttall: W._COSINE_SUMS["nuttall"],
           W.blackmanharris: W._COSINE_SUMS["blackmanharris"], W.flattop: W._COSINE_SUMS["flattop"]}


def reassignment_windows(window, nperseg):
    """-> (h, dh, th) float64 [nperseg]: the window (DFT-even), its derivative per sample and (j - nperseg/2) h.  dh is exact for the
    cosine-sum windows of pyfft_amd.windows (hann, hamming, blackman, nuttall, blackmanharris, flattop: the derivative term by term)
    and for ('gaussian', std); every other table, a caller's own included, gets cyclic central differences.  A triple (h, dh, th) of
    arrays is returned as it is."""
    n = int(nperseg)
    if n < 2:
        raise ValueError("reassignment_windows: nperseg must be at least 2")
    j = np.arange(n, dtype=np.float64)
    if isinstance(window, (tuple, list)) and len(window) == 3 and not isinstance(window[0], str):
        tabs = tuple(np.asarray(w, dtype=np.float64) for w in window)
        if any(w.shape != (n,) for w in tabs):
            raise ValueError("reassignment_windows: a triple (h, dh, th) must hold nperseg = %d values each" % n)
        return tabs
    dh = None
    if isinstance(window, (str, tuple)):
        h = np.asarray(W.get_window(window, n), dtype=np.float64)
        name = window if isinstance(window, str) else window[0]
        fn = W._win_equiv.get(name)
        if fn in _COSINE:
            t = -math.pi + 2.0 * math.pi * j / n
            dh = np.zeros(n)
            for k, ak in enumerate(_COSINE[fn]):
                dh -= ak * k * (2.0 * math.pi / n) * np.sin(k * t)
        elif fn is W.gaussian:
            std = float(window[1])
            dh = -(j - n / 2.0) / (std * std) * h
    else:
        h = np.asarray(window, dtype=np.float64)
        if h.shape != (n,):
            raise ValueError("reassignment_windows: window must be a name, a (name, parameter) tuple or nperseg = %d values" % n)
    if dh is None:
        dh = 0.5 * (np.roll(h, -1) - np.roll(h, 1))
    return h, dh, (j - n / 2.0) * h


def _threshold(who, threshold):
    """threshold: rel, or (gamma, rel): a cell is used where |X_h| > max(gamma, rel * the frame's largest |X_h|)"""
    if isinstance(threshold, (tuple, list)):
        gamma, rel = (float(v) for v in threshold)
    else:
        gamma, rel = 0.0, float(threshold)
    if not (math.isfinite(gamma) and math.isfinite(rel) and gamma >= 0 and rel >= 0):
        raise SsqRefused("%s: threshold must be rel or (gamma, rel), finite and not negative" % who)
    return gamma, rel


def _frames(who, nsig, n, noverlap, hop, boundary):
    if hop is not None and noverlap is not None:
        raise ValueError("%s: give hop or noverlap, not both" % who)
    hop = 1 if hop is None and noverlap is None else (int(hop) if hop is not None else n - int(noverlap))
    if hop < 1:
        raise SsqRefused("%s: hop = %d must be at least 1" % (who, hop))
    if boundary == "zeros":
        return hop, -(n // 2), (nsig - 1) // hop + 1 if nsig >= 1 else 0
    if boundary is None:
        return hop, 0, (nsig - n) // hop + 1 if nsig >= n else 0
    raise ValueError("%s: boundary must be 'zeros' or None" % who)


def _band(who, band, fs, n, cplx):
    """band (flo, fhi) in Hz -> (b0, nb): the bins whose frequency lies inside; None: all of them"""
    nbins = n if cplx else n // 2 + 1
    if band is None:
        return 0, nbins
    flo, fhi = float(band[0]), float(band[1])
    lo, hi = int(math.ceil(flo * n / fs - 1e-9)), int(math.floor(fhi * n / fs + 1e-9))
    if hi < lo or (not cplx and (lo < 0 or hi > n // 2)) or (cplx and (hi - lo + 1 > n or lo < -n // 2 or hi >= n)):
        raise SsqRefused("%s: band = %r holds no bins of the spectrum (bins %d .. %d)" % (who, band, lo, hi))
    return lo % n if cplx else lo, hi - lo + 1


def _setup(who, x, fs, window, nperseg, noverlap, hop, boundary, threshold, band):
    n, fs = int(nperseg), float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    if n < E.SSQ_MIN_N or n > E.SSQ_MAX_N or n & (n - 1):
        raise SsqRefused("%s: nperseg = %d must be a power of two from %d to %d" % (who, n, E.SSQ_MIN_N, E.SSQ_MAX_N))
    dev = _is_torch(x)
    if not dev:
        x = np.asarray(x)
    if len(x.shape) < 1:
        raise ValueError("%s: x must have at least one axis" % who)
    cplx = bool(x.is_complex() if dev else np.iscomplexobj(x))
    nsig = int(x.shape[-1])
    hop, first, nframes = _frames(who, nsig, n, noverlap, hop, boundary)
    gamma, rel = _threshold(who, threshold)
    b0, nb = _band(who, band, fs, n, cplx)
    h, dh, th = reassignment_windows(window, n)
    bins = (b0 + np.arange(nb)) % n if cplx else b0 + np.arange(nb)
    f = np.where(bins >= n // 2, bins - n, bins) * fs / n if cplx else bins * fs / n
    t = (first + hop * np.arange(nframes) + n // 2) / fs
    return dict(x=x, n=n, fs=fs, cplx=cplx, hop=hop, first=first, nframes=nframes, gamma=gamma, rel=rel, b0=b0, nb=nb, h=h, dh=dh, th=th,
                f=f, t=t)


def _swap(a):
    """[..., nframes, nb] -> scipy's [..., nb, nframes], a view"""
    return a.transpose(-1, -2) if _is_torch(a) else np.swapaxes(a, -1, -2)


def ssq_stft(x, fs=1.0, window="hann", nperseg=256, noverlap=None, hop=None, boundary="zeros", threshold=DEFAULT_THRESHOLD, band=None):
    """The synchrosqueezed STFT along the last axis -> f, t, Tx.  Tx complex64 [..., nb, nframes] (scipy's orientation, a view of the
    frame-major result); f the bins' frequencies (real records 0 .. fs/2; complex records in FFT order), t the frame centres.
    hop = 1 by default (or nperseg - noverlap); boundary='zeros': frames centred on the samples 0, hop, ..; None: whole frames only.
    threshold: rel or (gamma, rel).  band = (flo, fhi) in Hz keeps the targets inside it.  window: a name, a (name, parameter)
    tuple, nperseg values, or a triple (h, dh, th)."""
    s = _setup("ssq_stft", x, fs, window, nperseg, noverlap, hop, boundary, threshold, band)
    T = E.ssq(s["x"], s["h"], s["dh"], s["hop"], s["first"], s["nframes"], b0=s["b0"], nb=s["nb"], gamma=s["gamma"], rel=s["rel"])[0]
    return s["f"], s["t"], _swap(T)


def squeezed_spectrogram(x, fs=1.0, window="hann", nperseg=256, noverlap=None, hop=None, boundary="zeros", threshold=DEFAULT_THRESHOLD,
                         band=None):
    """The frequency-reassigned spectrogram -> f, t, P float32 [..., nb, nframes]: |X_h|^2 / sum(h)^2 of every used cell moved to the
    bin of its instantaneous frequency -- scipy.signal.spectrogram(scaling='spectrum', mode='psd') before the squeeze.  Real records
    are one-sided: every bin but 0 and nperseg/2 is doubled (by the bin the power lands in)."""
    s = _setup("squeezed_spectrogram", x, fs, window, nperseg, noverlap, hop, boundary, threshold, band)
    P = E.ssq(s["x"], s["h"], s["dh"], s["hop"], s["first"], s["nframes"], b0=s["b0"], nb=s["nb"], T=False, P=True, gamma=s["gamma"],
              rel=s["rel"])[1]
    scale = 1.0 / float(np.sum(s["h"])) ** 2
    if not math.isfinite(scale):
        raise ValueError("squeezed_spectrogram: the window has no weight")
    if s["cplx"]:
        P *= scale
    else:
        bins = s["b0"] + np.arange(s["nb"])
        w = np.where((bins == 0) | (bins == s["n"] // 2), scale, 2.0 * scale).astype(np.float32)
        P *= (E.torch.from_numpy(w).to(P.device) if _is_torch(P) else w)
    return s["f"], s["t"], _swap(P)


def reassignment_fields(x, fs=1.0, window="hann", nperseg=256, noverlap=None, hop=None, boundary="zeros", threshold=DEFAULT_THRESHOLD,
                        band=None):
    """The reassignment operators of every STFT cell -> f, t, f_hat, t_hat [..., nb, nframes]: the instantaneous frequency in Hz
    (float32) and the group delay in seconds (float64: the frame's centre plus the cell's offset -- in float32 the centres of a record
    of 2^20 samples would swallow the offsets) of the cells at the bins f and the frames t, NaN below the threshold.  What a
    two-dimensional reassigned spectrogram or a ridge tracker on the host needs."""
    s = _setup("reassignment_fields", x, fs, window, nperseg, noverlap, hop, boundary, threshold, band)
    _, _, IF, GD = E.ssq(s["x"], s["h"], s["dh"], s["hop"], s["first"], s["nframes"], th=s["th"], b0=s["b0"], nb=s["nb"], T=False, IF=True,
                         GD=True, gamma=s["gamma"], rel=s["rel"])
    IF *= s["fs"] / s["n"]
    tc = s["t"][:, None]
    if _is_torch(GD):
        that = GD.double() / s["fs"] + E.torch.from_numpy(tc).to(GD.device)
    else:
        that = GD.astype(np.float64) / s["fs"] + tc
    return s["f"], s["t"], _swap(IF), _swap(that)


def _centre_gain(who, h, n):
    gain = float(n) * float(h[n // 2])
    if gain == 0.0 or not math.isfinite(gain):
        raise SsqRefused("%s: the window is zero at its centre, h[nperseg/2] == 0: the modes cannot be scaled" % who)
    return gain


def ssq_extract(x, bands, fs=1.0, window="hann", nperseg=256, noverlap=None, hop=None, boundary="zeros", threshold=DEFAULT_THRESHOLD):
    """Modes without forming the transform -> [..., nbands, nframes]: mode b at frame g is the sum of the used cells whose instantaneous
    frequency lies in [lo, hi) of band b, over nperseg h[nperseg/2].  bands in Hz: [nbands, 2] constants, or [nbands, nframes, 2] per
    frame (a ridge +- a half-width); nbands <= 8.  Real records return 2 Re of the sum (float32), complex records the sum.
    At hop = 1 with boundary='zeros' the modes are waveforms at full rate; at a larger hop they are those waveforms sampled at the
    frame centres, carrier included."""
    s = _setup("ssq_extract", x, fs, window, nperseg, noverlap, hop, boundary, threshold, None)
    gain = _centre_gain("ssq_extract", s["h"], s["n"])
    edges = bands * (s["n"] / s["fs"]) if _is_torch(bands) else np.asarray(bands, dtype=np.float64) * (s["n"] / s["fs"])
    out = E.ssq_bands(s["x"], s["h"], s["dh"], s["hop"], s["first"], s["nframes"], edges, scale=(1.0 if s["cplx"] else 2.0) / gain,
                      gamma=s["gamma"], rel=s["rel"])
    return out if s["cplx"] else out.real


def issq_stft(Tx, window="hann", nperseg=256, band=None, fs=1.0, f0=0.0, onesided=True):
    """The way back: a band of an existing Tx [..., nb, nframes] (as ssq_stft returns it, its first bin at the frequency f0) summed over
    its bins and divided by nperseg h[nperseg/2] -> [..., nframes].  band = (flo, fhi) in Hz, None: every bin; for a complex record
    the band may lie at negative frequencies or straddle 0 (the bins are taken modulo nperseg, as ssq_stft lays them out).  onesided (Tx
    of a real record): 2 Re of the sum with the bins 0 and nperseg/2 at half weight, float32; else the complex sum."""
    n, fs = int(nperseg), float(fs)
    h = reassignment_windows(window, n)[0]
    gain = _centre_gain("issq_stft", h, n)
    b0 = int(round(float(f0) * n / fs)) % n
    T = _swap(Tx)
    nb = int(T.shape[-1])
    if band is None:
        edges = [(0.0, float(n))]
    else:
        lo, hi = math.ceil(float(band[0]) * n / fs - 1e-9), math.floor(float(band[1]) * n / fs + 1e-9) + 1
        if hi <= lo or hi - lo > n or lo < -n or hi > n:
            raise SsqRefused("issq_stft: band = %r holds no bins of the spectrum" % (band,))
        # the kernel compares the edges with the bin modulo n: a band below 0 moves up by n, one that straddles 0 is two pieces
        edges = [(lo, hi)] if lo >= 0 else ([(lo + n, hi + n)] if hi <= 0 else [(lo + n, n), (0, hi)])
    out = E.ssq_sum(T if _is_torch(T) else np.ascontiguousarray(T), n, [(float(a), float(b)) for a, b in edges], b0=b0,
                    half=bool(onesided), scale=(2.0 if onesided else 1.0) / gain)
    out = out[..., 0, :] if len(edges) == 1 else out[..., 0, :] + out[..., 1, :]
    return out.real if onesided else out


def ssq_plan(nsig, nperseg=256, noverlap=None, hop=None, boundary="zeros", band=None, fs=1.0, cplx=False, rows=1, T=True, P=False,
             fields=False, bands=False):
    """What a call costs (host only): dict(nframes, hop, first, b0, nb, fpr, workgroups, lds_bytes, transforms, fits).  transforms: per
    frame; fits: whether the LDS of a workgroup holds the transform images and the accumulators of the band."""
    n = int(nperseg)
    if n < E.SSQ_MIN_N or n > E.SSQ_MAX_N or n & (n - 1):
        raise SsqRefused("ssq_plan: nperseg = %d must be a power of two from %d to %d" % (n, E.SSQ_MIN_N, E.SSQ_MAX_N))
    hop, first, nframes = _frames("ssq_plan", int(nsig), n, noverlap, hop, boundary)
    b0, nb = _band("ssq_plan", band, float(fs), n, bool(cplx))
    d = dict(nframes=nframes, hop=hop, first=first, b0=b0, nb=nb)
    d.update(E.ssq_plan(n, nframes, rows=rows, cplx=cplx, nb=nb, T=T, P=P, fields=fields, bands=bands))
    return d
