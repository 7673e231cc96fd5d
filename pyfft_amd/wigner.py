"""Quadratic time-frequency distributions of Cohen's class with a separable kernel: the Wigner-Ville distribution, its pseudo and
smoothed pseudo forms and the cross distribution (Claasen & Mecklenbraeuker, Philips J. Res. 35, 217 (1980); Flandrin, ICASSP 1984;
Auger & Flandrin, IEEE Trans. SP 43, 1068 (1995)).

With z (and y) complex records that are zero outside themselves, a lag window h and a time window g, both odd and centred, and the
column times n = 0, hop, 2 hop, ..:

    K[n, tau] = h[tau] sum_mu g[mu] z[n + mu + tau] conj(y[n + mu - tau])
    W[n, k]   = (1 / nfft) sum_tau K[n, tau] exp(-2 pi i k tau / nfft)

The lag is 2 tau samples, so bin k stands for the frequency k fs / (2 nfft) and W has the period fs / 2: a real record is made analytic
first (the whole-record Hilbert path of pyfft_amd.hilbert, on the device), and its bins run over 0 .. fs/2.  h smooths in frequency; g
smooths in time and removes the oscillating cross-terms between components.  With h[0] = 1 and sum(g) = 1 (what windows given by name
are scaled to) the sum of a column over its bins is the time-smoothed instantaneous power.

Everything runs in one kernel (pyfft_amd/csrc/k_wvd.hip): the lag products and the smoothing are formed from samples staged in LDS, K
never exists in memory, and in the auto case two columns share one transform.  Results are bitwise reproducible.  nfft is a power of
two from 32 to 8192, time windows have at most 255 taps, and a shape whose staged samples do not fit the LDS of a workgroup is refused
(wvd_plan tells), never split."""
import importlib
import math

import numpy as np

from . import engine as E
from .engine import WvdRefused, _is_torch

_W = importlib.import_module(".windows", __package__)     # (the package rebinds the name `windows` to the function)


def _window(who, what, window, default_len):
    """a name, a (name, length) or (name, parameters.., length) tuple, or an array -> (float64 taps, odd and centred; given by name?)"""
    if isinstance(window, str):
        window = (window, default_len)
    if isinstance(window, tuple) and len(window) >= 1 and isinstance(window[0], str):
        if len(window) < 2:
            raise ValueError("%s: %s = %r must be (name, length)" % (who, what, window))
        n = int(window[-1])
        if n < 1 or not n & 1:
            raise WvdRefused("%s: %s has %d taps: the length must be odd and at least 1" % (who, what, n))
        spec = window[0] if len(window) == 2 else tuple(window[:-1])
        return np.asarray(_W.get_window(spec, n, fftbins=False), dtype=np.float64), True
    w = np.asarray(window, dtype=np.float64)
    if w.ndim != 1 or w.size < 1 or not w.size & 1 or not np.all(np.isfinite(w)):
        raise WvdRefused("%s: %s must be a name, a (name, length) tuple or an odd number of finite taps" % (who, what))
    return w, False


def _windows(who, window, twindow, nfft):
    h, named = _window(who, "window", ("hamming", nfft // 4 | 1) if window is None else window, nfft // 4 | 1)
    if named:
        if h[h.size // 2] == 0:
            raise WvdRefused("%s: the lag window is zero at lag 0" % who)
        h = h / h[h.size // 2]
    g, named = _window(who, "twindow", ("hamming", nfft // 10 | 1) if twindow is None else twindow, nfft // 10 | 1)
    if named:
        if np.sum(g) == 0:
            raise WvdRefused("%s: the time window has no weight" % who)
        g = g / np.sum(g)
    return h, g


def _band(who, band, fs, nfft, signed):
    """band (flo, fhi) in Hz -> (b0, nb): the bins k with flo <= k fs / (2 nfft) <= fhi (negative k for a complex record); None: all"""
    if band is None:
        return 0, nfft
    df = fs / (2.0 * nfft)
    lo, hi = int(math.ceil(float(band[0]) / df - 1e-9)), int(math.floor(float(band[1]) / df + 1e-9))
    if hi < lo or hi - lo + 1 > nfft or (signed and (lo < -nfft // 2 or hi >= nfft)) or (not signed and (lo < 0 or hi >= nfft)):
        raise WvdRefused("%s: band = %r holds no bins of the distribution (bins %d .. %d)" % (who, band, lo, hi))
    return lo % nfft, hi - lo + 1


def analytic(x):
    """The analytic signal of real rows along the last axis, complex64: the whole-record Hilbert path of pyfft_amd.hilbert on the
    device, numpy arrays and device tensors alike."""
    lead, nsig = tuple(x.shape[:-1]), int(x.shape[-1])
    return E.hilbert_rows(x.reshape(-1, nsig), nsig).reshape(lead + (nsig,))


def _setup(who, x, y, fs, window, twindow, nfft, hop, band, analytic_, boundary):
    nfft, hop, fs = int(nfft), int(hop), float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    if boundary != "zeros":
        raise WvdRefused("%s: boundary = %r: only 'zeros' is built (the record is zero outside itself)" % (who, boundary))
    if nfft < E.WVD_MIN_N or nfft > E.WVD_MAX_N or nfft & (nfft - 1):
        raise WvdRefused("%s: nfft = %d must be a power of two from %d to %d" % (who, nfft, E.WVD_MIN_N, E.WVD_MAX_N))
    if hop < 1:
        raise WvdRefused("%s: hop = %d must be at least 1" % (who, hop))
    rec = []
    for a in (x, y):
        if a is None:
            rec.append(None)
            continue
        if not _is_torch(a):
            a = np.asarray(a)
        if len(a.shape) < 1 or a.shape[-1] < 1:
            raise WvdRefused("%s: the record must have at least one axis and one sample" % who)
        rec.append(a)
    x, y = rec
    if y is not None and (tuple(y.shape) != tuple(x.shape) or _is_torch(y) != _is_torch(x)):
        raise WvdRefused("%s: y must share x's shape and kind of array" % who)
    cplx = [None if a is None else bool(a.is_complex() if _is_torch(a) else np.iscomplexobj(a)) for a in (x, y)]
    if y is not None and cplx[0] != cplx[1]:
        raise WvdRefused("%s: x and y must both be real or both complex" % who)
    real = not cplx[0]
    if analytic_ is None:
        analytic_ = real
    if real and not analytic_:
        raise WvdRefused("%s: real rows are not taken directly (the distribution of a real record aliases and carries the cross-terms of "
                         "its negative frequencies): leave analytic at None or True" % who)
    if not real and analytic_:
        raise WvdRefused("%s: analytic=True needs a real record" % who)
    h, g = _windows(who, window, twindow, nfft)
    nsig = int(x.shape[-1])
    ntimes = (nsig - 1) // hop + 1
    b0, nb = _band(who, band, fs, nfft, not real)
    rows = 1
    for d in x.shape[:-1]:
        rows *= int(d)
    E.wvd_check(who, nfft, h.size, g.size, hop, ntimes, rows, nb, b0)
    bins = (b0 + np.arange(nb)) % nfft
    f = (bins if real else np.where(bins >= nfft // 2, bins - nfft, bins)) * fs / (2.0 * nfft)
    t = hop * np.arange(ntimes) / fs
    return dict(x=x, y=y, real=real, nfft=nfft, hop=hop, first=0, nframes=ntimes, b0=b0, nb=nb, h=h, g=g, f=f, t=t, rows=rows, nsig=nsig)


def _swap(a):
    """[..., ntimes, nb] -> scipy's [..., nb, ntimes], a view"""
    return a.transpose(-1, -2) if _is_torch(a) else np.swapaxes(a, -1, -2)


def _samples(a, real):
    if a is None:
        return None
    if real:
        return analytic(a if _is_torch(a) else np.ascontiguousarray(a, dtype=np.float32))
    return a


def _run(who, x, y, fs, window, twindow, nfft, hop, band, analytic_, boundary):
    s = _setup(who, x, y, fs, window, twindow, nfft, hop, band, analytic_, boundary)
    W = E.wvd(_samples(s["x"], s["real"]), s["h"], s["g"], s["hop"], s["first"], s["nframes"], s["nfft"], y=_samples(s["y"], s["real"]),
              b0=s["b0"], nb=s["nb"], scale=1.0 / s["nfft"])
    return s["f"], s["t"], _swap(W)


def spwvd(x, fs=1.0, window=None, twindow=None, nfft=256, hop=1, y=None, band=None, analytic=None, boundary="zeros"):
    """The smoothed pseudo Wigner-Ville distribution along the last axis -> f, t, W.  W float32 [..., nb, ntimes] (scipy's orientation, a
    view of the column-major result; complex64 with y, the cross distribution), t = 0, hop / fs, .. the column times, f the bins'
    frequencies k fs / (2 nfft).
    window: the lag window h, by default ('hamming', nfft // 4 | 1); twindow: the time window g, by default ('hamming', nfft // 10 | 1).
    Either is a name, a (name, length) tuple (parameters of the family go between the two) or an odd number of taps; windows given by
    name are scaled to h[0] = 1 and sum(g) = 1, arrays are used as they are.  With these and the scale 1 / nfft the sum of a column
    over all its bins is the time-smoothed instantaneous power sum_mu g[mu] |z[n + mu]|^2.
    A real record is made analytic first (analytic=None or True) and f runs over 0 .. fs/2.  A complex record is used as it is and f is
    signed, k fs / (2 nfft) below nfft / 2 and (k - nfft) fs / (2 nfft) from there on: the distribution has the period fs / 2, so
    content beyond +- fs / 4 aliases; resample_poly(x, 2, 1) in front removes that.
    band = (flo, fhi) in Hz keeps the bins inside.  boundary: 'zeros' (the record is zero outside itself)."""
    return _run("spwvd", x, y, fs, window, twindow, nfft, hop, band, analytic, boundary)


def pwvd(x, fs=1.0, window=None, nfft=256, hop=1, y=None, band=None, analytic=None, boundary="zeros"):
    """The pseudo Wigner-Ville distribution: spwvd without smoothing in time (twindow = [1])."""
    return _run("pwvd", x, y, fs, window, np.ones(1), nfft, hop, band, analytic, boundary)


def _whole_record(who, x, nfft):
    """-> (nfft, the rectangular lag window): no product of the record has a lag beyond (nsig - 1) / 2 samples either way"""
    nsig = int(x.shape[-1]) if _is_torch(x) else int(np.shape(x)[-1])
    if nfft is None:
        nfft = E.WVD_MIN_N
        while nfft - 2 < nsig and nfft < E.WVD_MAX_N:
            nfft *= 2
    nfft = int(nfft)
    if nsig > min(nfft, E.WVD_MAX_N) - 2:
        raise WvdRefused("%s: a record of %d samples is longer than nfft - 2 = %d, the lags one transform of at most %d points holds: "
                         "use pwvd, whose lag window is shorter than the record" % (who, nsig, min(nfft, E.WVD_MAX_N) - 2, E.WVD_MAX_N))
    return nfft, np.ones(nsig | 1)


def wvd(x, fs=1.0, nfft=None, hop=1, y=None, band=None, analytic=None):
    """The Wigner-Ville distribution itself: pwvd under a rectangular lag window that covers the whole record (nsig taps, one more for
    an even count; nfft by default the next power of two that holds them).  Refused for records longer than nfft - 2 samples at the
    largest nfft, 8192: use pwvd."""
    nfft, h = _whole_record("wvd", x, nfft)
    return _run("wvd", x, y, fs, h, np.ones(1), nfft, hop, band, analytic, "zeros")


def xwvd(x, y, fs=1.0, window=None, twindow=None, nfft=256, hop=1, band=None, analytic=None, boundary="zeros"):
    """The cross smoothed pseudo Wigner-Ville distribution of x and y -> f, t, W complex64 [..., nb, ntimes];
    xwvd(y, x) = conj(xwvd(x, y)), and xwvd(x, x) is spwvd(x) with a vanishing imaginary part."""
    if y is None:
        raise WvdRefused("xwvd: y is required")
    return _run("xwvd", x, y, fs, window, twindow, nfft, hop, band, analytic, boundary)


def wvd_plan(nsig, nfft=256, window=None, twindow=None, hop=1, rows=1, cross=False, band=None, fs=1.0, cplx=False):
    """What a call would launch (host only): the engine plan (cpr = columns per run, workgroups, lds_bytes, transforms per run, fits)
    plus nframes, first, b0 and nb."""
    nsig, nfft, hop = int(nsig), int(nfft), int(hop)
    if nfft < E.WVD_MIN_N or nfft > E.WVD_MAX_N or nfft & (nfft - 1):
        raise WvdRefused("wvd_plan: nfft = %d must be a power of two from %d to %d" % (nfft, E.WVD_MIN_N, E.WVD_MAX_N))
    if nsig < 1 or hop < 1:
        raise WvdRefused("wvd_plan: nsig and hop must be at least 1")
    h, g = _windows("wvd_plan", window, twindow, nfft)
    ntimes = (nsig - 1) // hop + 1
    b0, nb = _band("wvd_plan", band, float(fs), nfft, bool(cplx))
    d = E.wvd_plan(nfft, h.size, g.size, hop, ntimes, rows=rows, cross=cross, nb=nb)
    d.update(nframes=ntimes, first=0, b0=b0, nb=nb)
    return d
