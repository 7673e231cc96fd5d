"""Time-resolved Welch spectra: the running PSD, CSD, coherence ("coherogram") and cross-phase of records that are not stationary.

    frames     g = 0 .. nframes - 1,  a_g = win * (x[g hop : g hop + nperseg] - its own mean),  hop = nperseg - noverlap
    block      b = 0 .. nblocks - 1 holds the frames b step .. b step + navg - 1,  nblocks = (nframes - navg) // step + 1
    Pxx[b]     = the Welch PSD of those navg frames,  Pxy[b] = their CSD (conj(X) Y, scipy.signal.csd),  Cxy = |Pxy|^2 / (Pxx Pyy)
    t[b]       = the centre of block b: (b step hop + ((navg - 1) hop + nperseg) / 2) / fs

Block b is exactly scipy.signal.welch / csd / coherence of x[s:e], s = b step hop, e = s + (navg - 1) hop + nperseg, with the same
window, nperseg, noverlap, detrend and scaling.  step == navg (the default): disjoint blocks; step < navg: overlapping blocks (a
smoother coherogram at the same statistical weight per block); step > navg: gaps.  Frames left over behind the last block are not used.
One kernel (k_welch_blocks.hip) forms the averages inside its frame loop: every sample is read once per frame overlap, every frame is
transformed once whatever the block overlap, and only the block averages are written -- navg times less than the spectrogram the
composed route (stft of both records, then block means) writes and reads back.

Arrays are [nblocks, nf], the [frame][bin] layout of stft; with several y channels ([nch, nsig]) [nch, nblocks, nf].  Pxx, Pyy are
float32 and Pxy complex64 as the kernel leaves them; coherence is float64.  Pxx never depends on y or on the
number of channels, to the last bit.  Real input: one-sided by default (f = rfftfreq, bins
1 .. nperseg/2 - 1 doubled), two-sided in fftfreq order with return_onesided=False; complex input: always two-sided in fftfreq order.
numpy in -> numpy out; device tensors in -> device tensors (f, t stay numpy).  Segments are powers of two from 32 to 8192 samples,
nfft == nperseg (no zero padding), detrend 'constant' or False."""
import math

import numpy as np

from .windows import get_window
from . import engine as _engine
from .engine import WelchBlocksRefused, _is_torch

MIN_NFFT, MAX_NFFT = _engine.WELCH_BLOCKS_MIN_NFFT, _engine.WELCH_BLOCKS_MAX_NFFT


class RunningSpectra(object):
    """What running_spectra returns: f, t, Pxx, Pyy, Pxy, coherence, phase (= angle(Pxy), radians), navg, step."""
    __slots__ = ("f", "t", "Pxx", "Pyy", "Pxy", "coherence", "phase", "navg", "step")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return "RunningSpectra(nblocks=%d, nf=%d, navg=%d, step=%d)" % (len(self.t), len(self.f), self.navg, self.step)


def coherence_level(navg, alpha=0.05):
    """The level the magnitude-squared coherence of two INDEPENDENT records exceeds with probability alpha when navg independent
    segments are averaged: 1 - alpha^(1 / (navg - 1)) (Carter 1987); 1 for navg = 1, where every coherence is 1.  Overlapped frames
    are not independent (Hann at 50 %: about 0.95 navg effective segments, fewer at more overlap), so for them the level is
    optimistic: too low.  No correction for the effective degrees of freedom is applied."""
    navg, alpha = int(navg), float(alpha)
    if navg < 1:
        raise ValueError("coherence_level: navg must be at least 1")
    if not 0.0 < alpha < 1.0:
        raise ValueError("coherence_level: alpha must lie in (0, 1)")
    return 1.0 if navg == 1 else 1.0 - alpha ** (1.0 / (navg - 1))


def _geometry(who, nsig, nperseg, noverlap, navg, step, nfft, detrend):
    nperseg, navg = int(nperseg), int(navg)
    if nfft is not None and int(nfft) != nperseg:
        raise WelchBlocksRefused("%s: nfft = %d differs from nperseg = %d: zero padding is not built" % (who, int(nfft), nperseg))
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    step = navg if step is None else int(step)
    if not 0 <= noverlap < nperseg and nperseg >= 1:
        raise WelchBlocksRefused("%s: need 0 <= noverlap < nperseg" % who)
    hop = nperseg - noverlap
    nframes = (nsig - nperseg) // hop + 1 if nsig >= nperseg and hop >= 1 else 0
    _engine.welch_blocks_check(who, nsig, nperseg, hop, nframes, navg, step, detrend)
    return nperseg, hop, nframes, navg, step


def running_plan(nsig, nperseg=256, noverlap=None, navg=8, step=None, fs=1.0, nch=1, cplx=False):
    """What a call on records of nsig samples does, host only: dict(nframes, hop, nblocks, nf, q, runs, transforms, scratch, workgroups,
    lds_bytes, t0, t1, bytes_fused, bytes_composed).  nch = the y channels (0: PSD only).  q = the frames of a run (navg, or
    gcd(navg, step) for overlapping blocks); transforms = frames transformed x 2 nch (x and y_c of every pair have their
    own), x 1 without y: every frame once whatever the block overlap.
    t0[b], t1[b] = the first sample's time and the time just behind the last sample of block b.  bytes_fused = samples read
    (once per frame overlap) + run sums written and read + outputs written; bytes_composed = every record read once per
    frame overlap + the complex64 spectrogram of every record written and read back + the outputs."""
    nsig, nch, cplx, fs = int(nsig), int(nch), bool(cplx), float(fs)
    nperseg, hop, nframes, navg, step = _geometry("running_plan", nsig, nperseg, noverlap, navg, step, None, False)
    p = _engine.welch_blocks_plan(nperseg, hop, nframes, navg, step, nch=nch, cplx=cplx)
    b = np.arange(p["nblocks"], dtype=np.float64)
    esz, nrec, nf = (8 if cplx else 4), 1 + nch, p["nb"]
    used = p["runs"] * p["q"]
    rows = 1 if nch < 1 else 2 * nch                                 # records a frame loads: x and y_c for every pair
    read = esz * nperseg * used * rows
    out = p["nblocks"] * nf * (4 + 12 * nch)
    sums = 2 * p["scratch"]
    d = dict(p)
    d.pop("nb")
    d.update(nframes=nframes, hop=hop, nf=nf, t0=b * step * hop / fs, t1=(b * step * hop + (navg - 1) * hop + nperseg) / fs,
             bytes_fused=read + sums + out, bytes_composed=esz * nperseg * nframes * nrec + 2 * 8 * nf * nframes * nrec + out)
    return d


def _prepare(who, x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided, scaling, navg, step):
    dev = _is_torch(x)
    if y is not None and dev != _is_torch(y):
        raise ValueError("%s: x and y must both be arrays or both be device tensors" % who)
    if not dev:
        x = np.asarray(x)
        y = None if y is None else np.asarray(y)
    if len(x.shape) != 1:
        raise ValueError("%s: x must be one-dimensional" % who)
    if y is not None and (len(y.shape) not in (1, 2) or y.shape[-1] != x.shape[0]):
        raise ValueError("%s: y must be [nsig] or [nch, nsig] with x's length" % who)
    cplx = bool(x.is_complex() if dev else np.iscomplexobj(x))
    if y is not None and cplx != bool(y.is_complex() if dev else np.iscomplexobj(y)):
        raise ValueError("%s: x and y must both be real or both be complex" % who)
    fs = float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    nperseg, hop, nframes, navg, step = _geometry(who, int(x.shape[0]), nperseg, noverlap, navg, step, nfft, detrend)
    if isinstance(window, (str, tuple)):
        win = np.asarray(get_window(window, nperseg), dtype=np.float64)
    else:
        win = np.asarray(window, dtype=np.float64)
    if win.shape != (nperseg,) or not np.all(np.isfinite(win)):
        raise ValueError("%s: window must be a name or nperseg = %d finite values" % (who, nperseg))
    if scaling == "density":
        scale = 1.0 / (fs * np.sum(win * win))
    elif scaling == "spectrum":
        scale = 1.0 / np.sum(win) ** 2
    else:
        raise ValueError("%s: scaling must be 'density' or 'spectrum'" % who)
    if not math.isfinite(scale):
        raise ValueError("%s: the window has no weight" % who)
    onesided = bool(return_onesided) and not cplx
    f = np.fft.rfftfreq(nperseg, 1.0 / fs) if onesided else np.fft.fftfreq(nperseg, 1.0 / fs)
    nblocks = (nframes - navg) // step + 1
    t = (np.arange(nblocks) * (step * hop) + 0.5 * ((navg - 1) * hop + nperseg)) / fs
    segmean = detrend is True or (isinstance(detrend, str) and detrend != "none")       # (_geometry has refused every other mode)
    args = dict(win=win, hop=hop, nframes=nframes, navg=navg, step=step, detrend=segmean, scale=scale, doubled=onesided)
    return args, f, t, (not cplx and not onesided), navg, step


def _mirror(a, conj):
    """Bins 0 .. n/2 of a real record -> all n bins in FFT order: bin n - k is bin k (conjugated for a cross spectrum)."""
    tail = a[..., 1:-1]
    if _is_torch(a):
        import torch
        tail = torch.flip(tail, dims=(-1,))
        return torch.cat((a, tail.conj().resolve_conj() if conj else tail), dim=-1)
    tail = tail[..., ::-1]
    return np.concatenate((a, np.conj(tail) if conj else tail), axis=-1)


def _coherence(pxx, pyy, pxy):
    """|Pxy|^2 / (Pxx Pyy) in float64, 0 where the denominator is 0."""
    if _is_torch(pxy):
        import torch
        num = pxy.real.double() ** 2 + pxy.imag.double() ** 2
        den = pxx.double() * pyy.double()
        return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    num = pxy.real.astype(np.float64) ** 2 + pxy.imag.astype(np.float64) ** 2
    den = pxx.astype(np.float64) * pyy.astype(np.float64)
    return np.divide(num, den, out=np.zeros_like(den), where=den > 0)


def _angle(pxy):
    if _is_torch(pxy):
        import torch
        return torch.angle(pxy)
    return np.angle(pxy)


def _run(who, x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided, scaling, navg, step):
    args, f, t, mirror, navg, step = _prepare(who, x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided, scaling, navg,
                                              step)
    pxx, pyy, pxy = _engine.welch_blocks(x, y=y, **args)
    if mirror:
        pxx = _mirror(pxx, False)
        if y is not None:
            pyy, pxy = _mirror(pyy, False), _mirror(pxy, True)
    return f, t, pxx, pyy, pxy, navg, step


def running_psd(x, fs=1.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
                scaling="density", navg=8, step=None):
    """(f, t, Pxx): the Welch PSD of every block of navg frames, Pxx float32 [nblocks, nf]; arguments as scipy.signal.welch, plus navg
    and step (default navg) in frames."""
    f, t, pxx, _, _, _, _ = _run("running_psd", x, None, fs, window, nperseg, noverlap, nfft, detrend, return_onesided, scaling, navg,
                                 step)
    return f, t, pxx


def running_csd(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
                scaling="density", navg=8, step=None):
    """(f, t, Pxy): the cross spectral density conj(X) Y of every block (scipy.signal.csd), complex64 [nblocks, nf] or
    [nch, nblocks, nf] for y[nch, nsig]."""
    f, t, _, _, pxy, _, _ = _run("running_csd", x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided, scaling, navg, step)
    return f, t, pxy


def running_coherence(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant", navg=8, step=None):
    """(f, t, Cxy): the coherogram, Cxy = |Pxy|^2 / (Pxx Pyy) of every block (scipy.signal.coherence), float64, 0 where the denominator
    is 0.  navg = 1 gives 1 everywhere: a single frame carries no cross-spectral information.  coherence_level(navg) is the level
    independent records exceed by chance."""
    f, t, pxx, pyy, pxy, _, _ = _run("running_coherence", x, y, fs, window, nperseg, noverlap, nfft, detrend, True, "density", navg, step)
    return f, t, _coherence(pxx, pyy, pxy)


def running_spectra(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
                    scaling="density", navg=8, step=None):
    """Everything from one pass: a RunningSpectra with f, t, Pxx, Pyy, Pxy, coherence, phase (angle(Pxy)), navg, step."""
    f, t, pxx, pyy, pxy, navg, step = _run("running_spectra", x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided,
                                           scaling, navg, step)
    return RunningSpectra(f=f, t=t, Pxx=pxx, Pyy=pyy, Pxy=pxy, coherence=_coherence(pxx, pyy, pxy), phase=_angle(pxy), navg=navg,
                          step=step)
