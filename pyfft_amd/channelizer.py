"""Polyphase filter-bank channelizer: a record split into all M uniformly spaced bands at once under a prototype low-pass of
L = taps * M coefficients, longer than the transform (the weighted overlap-add DFT bank; k_pfb.hip).

    X[m, k] = sum_{n<L} h[n] x[s + n] exp(-2 pi i k (n + rho_m) / M),   s = first + m hop,   x = 0 outside the record
    rho_m   = 0 (phase "frame")  or  (n0 + s) mod M (phase "time": every channel is referred to absolute time, so that a tone at
              exactly k / M cycles per sample is a constant in channel k whatever the hop, and chunks of one stream continue)

Channel k is the baseband series of the band around k fs / M at the rate fs / hop; with phase "frame" and first = 0 it is bin
taps * k of scipy.signal.stft(window=h, nperseg=L, noverlap=L - hop, boundary=None, padded=False) before its scaling.  pfb_prototype
designs h, pfb_plan is the host geometry, channelize returns the frames and pfb_psd their mean power, accumulated on the device.

The way back is the synthesis bank (k_pfb_synth.hip), the adjoint of the fold under a synthesis prototype g:

    y[a] = sum_m g[a - s_m] * numpy.fft.ifft(X[m])[(a - s_m + rho_m) mod M]   over the frames with 0 <= a - s_m < len(g)

synthesize runs it on the device, pfb_dual designs the g that reconstructs the record for a given h and hop < M (least squares, with
its residual), pfb_alias_terms gives the terms T[q][r] of analysis followed by synthesis, pfb_synthesis_plan is the host geometry.
"""
import math

import numpy as np

from .baseband import Unsupported, MAX_WG_FFT, _is_torch

MAX_P = 32                          # branches (taps per channel) one launch takes


def pfb_prototype(M, taps=8, window=("kaiser", 8.0), cutoff=1.0):
    """The prototype low-pass of a bank of M channels, float64 [taps * M]: scipy.signal.firwin(taps * M, cutoff / M, window=window),
    so the -6 dB edge sits at cutoff / (2 M) cycles per sample (half the channel spacing at cutoff = 1) and the DC gain is 1.
    Pure scipy, never loads the library."""
    M, taps = int(M), int(taps)
    if M < 1 or taps < 1:
        raise ValueError("pfb_prototype: M and taps must be positive")
    cutoff = float(cutoff)
    if not 0.0 < cutoff < M:
        raise ValueError("pfb_prototype: cutoff must lie in (0, M), got %r" % cutoff)
    import scipy.signal as ss
    return ss.firwin(taps * M, cutoff / M, window=window)


def pfb_plan(nsig, cplx, M, taps=8, hop=None, fs=1.0, h=None, center=False, n0=0, return_onesided=None):
    """The validated host plan of a channelizer run (pure numpy / scipy, never loads the library): a dict with h (float64 [L]), L, P,
    M, hop, first (the index of frame 0's first sample), nframes, r0 = (n0 + first) mod M, f (the channel centres), t (the frame
    centres in seconds: (n0 + first + m hop + (L - 1) / 2) / fs), nb, onesided.  center=False: the frames that lie inside the record;
    center=True: frame m is centred on sample m hop, the record zero-extended.  A real input is one-sided (the bins 0 .. M/2)."""
    who = "pfb"
    nsig, M, n0 = int(nsig), int(M), int(n0)
    fs = float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    if M < 2 or M & (M - 1) or M > MAX_WG_FFT:
        raise Unsupported("%s: M = %d is not a power of two from 2 to %d; other channel counts are not built" % (who, M, MAX_WG_FFT))
    if h is None:
        taps = int(taps)
        if taps < 1:
            raise ValueError("%s: taps must be at least 1" % who)
        if taps > MAX_P:
            raise Unsupported("%s: %d taps per channel are beyond the %d one launch takes" % (who, taps, MAX_P))
        hh = pfb_prototype(M, taps)
    else:
        if np.iscomplexobj(h):
            raise Unsupported("%s: complex taps are not built" % who)
        hh = np.asarray(h, dtype=np.float64)
        if hh.ndim != 1 or hh.size < M or hh.size % M:
            raise ValueError("%s: len(h) must be a positive multiple of M = %d, got %s" % (who, M, hh.shape))
        if not np.all(np.isfinite(hh)):
            raise ValueError("%s: the taps must be finite" % who)
        if hh.size // M > MAX_P:
            raise Unsupported("%s: %d taps per channel are beyond the %d one launch takes" % (who, hh.size // M, MAX_P))
    L = hh.size
    hop = M if hop is None else int(hop)
    if hop < 1:
        raise ValueError("%s: hop must be at least 1" % who)
    cplx = bool(cplx)
    onesided = (not cplx) if return_onesided is None else bool(return_onesided)
    if onesided and cplx:
        raise ValueError("%s: a complex input has no one-sided spectrum" % who)
    if not onesided and not cplx:
        raise Unsupported("%s: a real input gives the bins 0 .. M/2 only (return_onesided=False is not built)" % who)
    if nsig < 1:
        raise ValueError("%s: the record is empty" % who)
    if center:
        first, nframes = -(L // 2), -(-nsig // hop)
    else:
        if nsig < L:
            raise ValueError("%s: the record (%d samples) is shorter than the filter (%d taps); center=True zero-extends it" %
                             (who, nsig, L))
        first, nframes = 0, (nsig - L) // hop + 1
    m = np.arange(nframes, dtype=np.float64)
    t = (n0 + first + m * hop + (L - 1) / 2.0) / fs
    f = np.arange(M // 2 + 1, dtype=np.float64) * (fs / M) if onesided else np.fft.fftfreq(M, 1.0 / fs)
    return dict(h=hh, L=L, P=L // M, M=M, hop=hop, first=first, nframes=nframes, r0=(n0 + first) % M, f=f, t=t, nb=f.size,
                onesided=onesided, fs=fs, cplx=cplx)


def _prepare(x, axis, who):
    """(x with the time axis last, device?, ndim, is complex, nsig)."""
    dev = _is_torch(x)
    if not dev:
        x = np.asarray(x)
    nd = x.dim() if dev else x.ndim
    if nd < 1:
        raise ValueError("%s: x must have at least one axis" % who)
    if not -nd <= axis < nd:
        raise ValueError("%s: axis %d is out of range" % (who, axis))
    last = axis in (-1, nd - 1)
    if not last:
        x = x.movedim(axis, -1) if dev else np.moveaxis(x, axis, -1)
    cplx = x.is_complex() if dev else np.iscomplexobj(x)
    return x, dev, last, cplx, int(x.shape[-1])


def channelize(x, M, taps=8, hop=None, fs=1.0, *, h=None, center=False, phase="time", n0=0, axis=-1, return_onesided=None):
    """(f, t, X): the M-channel polyphase filter bank of x along `axis`.  X is complex64 [..., nb, nframes] (scipy.signal.stft's
    layout, the frames last); f the channel centres (fftfreq order for a complex input, 0 .. fs/2 for a real one), t the frame centres.
    h: the prototype (default pfb_prototype(M, taps)); hop defaults to M (critical sampling).  phase "time" refers every channel to
    absolute time (n0 = the absolute index of the first sample: chunks of one stream continue), "frame" to the frame's first sample.
    numpy in -> numpy out, device tensor in -> device tensor out."""
    if phase not in ("time", "frame"):
        raise ValueError("channelize: phase must be 'time' or 'frame'")
    y, dev, last, cplx, nsig = _prepare(x, axis, "channelize")
    p = pfb_plan(nsig, cplx, M, taps, hop, fs, h, center, n0, return_onesided)
    from . import engine
    X = engine.pfb(y, p["h"], p["M"], p["hop"], p["first"], p["nframes"], phase_ref=1 if phase == "time" else 0,
                   r0=p["r0"] if phase == "time" else 0, out_major=1)
    if not last:                                  # [..., nb, nframes] with the frames last: the bins go where the time axis was
        nd = X.dim() if dev else X.ndim
        src = nd - 2
        dst = axis if axis >= 0 else axis + nd - 1
        X = X.movedim(src, dst) if dev else np.moveaxis(X, src, dst)
    return p["f"], p["t"], X


def _alias_range(Lh, Lg, M):
    """The q for which g[n] h[n + q M] can be non-zero: 0 <= n < Lg and 0 <= n + q M < Lh."""
    return range(-((Lg - 1) // M), (Lh - 1) // M + 1)


def pfb_alias_terms(h, g, M, hop):
    """The alias terms of analysis under h followed by synthesis under g, float64 T[nq][hop]:
    T[q][r] = sum_j g[r + j hop] h[r + j hop + q M] over every q for which the product can be non-zero, ascending; row i holds
    q = i - (len(g) - 1) // M, up to (len(h) - 1) // M.  On the samples whose frames all belong to the call the chain gives
    y[a] = sum_q T[q][(a - first) mod hop] x[a + q M] (first: the index of frame 0's first sample); perfect reconstruction is
    T = delta_q.  Pure numpy."""
    h = np.asarray(h, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    M, hop = int(M), int(hop)
    if h.ndim != 1 or g.ndim != 1 or h.size < 1 or g.size < 1:
        raise ValueError("pfb_alias_terms: h and g must be one-dimensional and not empty")
    if M < 1 or hop < 1:
        raise ValueError("pfb_alias_terms: M and hop must be positive")
    qs = np.array(list(_alias_range(h.size, g.size, M)), dtype=np.int64)
    T = np.zeros((qs.size, hop))
    n = np.arange(g.size)
    for i, q in enumerate(qs):
        k = n + int(q) * M
        ok = (k >= 0) & (k < h.size)
        prod = np.where(ok, g * h[np.clip(k, 0, h.size - 1)], 0.0)
        T[i] = np.bincount(n % hop, weights=prod, minlength=hop)
    return T


def pfb_dual(h, M, hop, taps=None):
    """(g, residual): the least-squares synthesis prototype of taps * M coefficients (default len(h)) for the analysis prototype h
    at this hop, float64, and residual = max |T - delta_q| of pfb_alias_terms(h, g, M, hop).  The conditions T[q][r] = delta_q are
    linear in g and decouple over the residue r = n mod hop into `hop` small problems in the unknowns g[r + j hop], each solved with
    numpy.linalg.lstsq (the minimum-norm solution where the system leaves freedom).  hop <= M / 2 with the default Kaiser prototype
    reconstructs to rounding; towards hop = M the residual grows, and at hop = M (critical sampling) no dual of this length exists.
    Pure numpy, never loads the library."""
    h = np.asarray(h, dtype=np.float64)
    M, hop = int(M), int(hop)
    if h.ndim != 1 or h.size < 1 or not np.all(np.isfinite(h)):
        raise ValueError("pfb_dual: h must be one-dimensional, not empty and finite")
    if M < 1 or hop < 1:
        raise ValueError("pfb_dual: M and hop must be positive")
    Lg = h.size if taps is None else int(taps) * M
    if Lg < 1:
        raise ValueError("pfb_dual: taps must be at least 1")
    qs = np.array(list(_alias_range(h.size, Lg, M)), dtype=np.int64)
    rhs = (qs == 0).astype(np.float64)
    g = np.zeros(Lg)
    for r in range(min(hop, Lg)):
        n = np.arange(r, Lg, hop)
        k = n[None, :] + qs[:, None] * M
        A = np.where((k >= 0) & (k < h.size), h[np.clip(k, 0, h.size - 1)], 0.0)
        g[r::hop] = np.linalg.lstsq(A, rhs, rcond=None)[0]
    T = pfb_alias_terms(h, g, M, hop)
    return g, float(np.max(np.abs(T - rhs[:, None])))


def pfb_synthesis_plan(nframes, onesided, M, taps=8, hop=None, fs=1.0, h=None, g=None, center=False, n0=0, nsig=None):
    """The validated host plan of a synthesis run (pure numpy / scipy, never loads the library), the counterpart of pfb_plan for the
    frames it describes: a dict with g (float64 [L], the synthesis prototype: the caller's, or pfb_dual of h or of
    pfb_prototype(M, taps)), residual (pfb_dual's; None when the caller supplied g), L, P, M, hop, first and r0 as pfb_plan gives them
    (first = 0, or -(L // 2) with center; r0 = (n0 + first) mod M), nframes, nout (nsig, or by default (nframes - 1) hop + L for
    center=False and nframes hop for center=True), t (the output sample times (n0 + a) / fs), nb, onesided and
    valid = (lo, hi): the output samples a in [lo, hi) to which every frame that reaches them belongs to the call,
    lo = max(0, first + L - hop), hi = min(nout, first + nframes hop)."""
    who = "pfb_synthesis"
    nframes, M, n0 = int(nframes), int(M), int(n0)
    fs = float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    if M < 2 or M & (M - 1) or M > MAX_WG_FFT:
        raise Unsupported("%s: M = %d is not a power of two from 2 to %d; other channel counts are not built" % (who, M, MAX_WG_FFT))
    hop = M if hop is None else int(hop)
    if hop < 1:
        raise ValueError("%s: hop must be at least 1" % who)
    if nframes < 1:
        raise ValueError("%s: there are no frames" % who)

    def proto(a, name):
        if np.iscomplexobj(a):
            raise Unsupported("%s: complex taps are not built" % who)
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 1 or a.size < M or a.size % M:
            raise ValueError("%s: len(%s) must be a positive multiple of M = %d, got %s" % (who, name, M, a.shape))
        if not np.all(np.isfinite(a)):
            raise ValueError("%s: the taps must be finite" % who)
        if a.size // M > MAX_P:
            raise Unsupported("%s: %d taps per channel are beyond the %d one launch takes" % (who, a.size // M, MAX_P))
        return a
    residual = None
    if g is not None:
        gg = proto(g, "g")
    else:
        if h is None:
            taps = int(taps)
            if taps < 1:
                raise ValueError("%s: taps must be at least 1" % who)
            if taps > MAX_P:
                raise Unsupported("%s: %d taps per channel are beyond the %d one launch takes" % (who, taps, MAX_P))
            hh = pfb_prototype(M, taps)
        else:
            hh = proto(h, "h")
        gg, residual = pfb_dual(hh, M, hop)
    L = gg.size
    first = -(L // 2) if center else 0
    if nsig is None:
        nout = nframes * hop if center else (nframes - 1) * hop + L
    else:
        nout = int(nsig)
        if nout < 1:
            raise ValueError("%s: nsig must be at least 1" % who)
    t = (n0 + np.arange(nout, dtype=np.float64)) / fs
    valid = (max(0, first + L - hop), min(nout, first + nframes * hop))
    return dict(g=gg, residual=residual, L=L, P=L // M, M=M, hop=hop, first=first, r0=(n0 + first) % M, nframes=nframes, nout=nout,
                t=t, valid=valid, nb=M // 2 + 1 if onesided else M, onesided=bool(onesided), fs=fs)


def synthesize(X, M, taps=8, hop=None, fs=1.0, *, h=None, g=None, center=False, phase="time", n0=0, nsig=None, input_onesided=True,
               scale=1.0, freq_axis=-2, time_axis=-1):
    """(t, y): the polyphase synthesis bank, the way back from channelize's frames to a waveform (sp_pfb_synth).  X: complex
    [..., nb, nframes] in channelize's layout (freq_axis / time_axis say where the two axes are), nb = M // 2 + 1 for
    input_onesided=True (float32 output) or M (fftfreq order, complex64 output).  g: the synthesis prototype; by default the
    least-squares dual pfb_dual(h or pfb_prototype(M, taps), M, hop)[0], which returns the record that channelize(h=h, hop=hop,
    center=center, phase=phase, n0=n0) was given on the samples pfb_synthesis_plan(...)["valid"] to the dual's residual (hop <= M / 2:
    rounding; no dual exists at hop = M).  nsig: the length of the output (the default ends with the last frame).  y is [..., nout]: X's other axes in
    their order, then the samples; t = (n0 + a) / fs.  numpy in -> numpy out, device tensor in -> device tensor out."""
    if phase not in ("time", "frame"):
        raise ValueError("synthesize: phase must be 'time' or 'frame'")
    dev = _is_torch(X)
    if not dev:
        X = np.asarray(X)
    nd = X.dim() if dev else X.ndim
    if nd < 2:
        raise ValueError("synthesize: X must have a bin axis and a frame axis")
    if not (-nd <= freq_axis < nd and -nd <= time_axis < nd) or freq_axis % nd == time_axis % nd:
        raise ValueError("synthesize: freq_axis %d and time_axis %d must be two axes of X" % (freq_axis, time_axis))
    if not (X.is_complex() if dev else np.iscomplexobj(X)):
        raise ValueError("synthesize: the frames must be complex")
    fa, ta = freq_axis % nd, time_axis % nd
    if (fa, ta) != (nd - 2, nd - 1):
        X = X.movedim((fa, ta), (-2, -1)) if dev else np.moveaxis(X, (fa, ta), (-2, -1))
    p = pfb_synthesis_plan(int(X.shape[-1]), input_onesided, M, taps, hop, fs, h, g, center, n0, nsig)
    if int(X.shape[-2]) != p["nb"]:
        raise ValueError("synthesize: X has %d bins, M = %d with input_onesided=%s needs %d" % (X.shape[-2], p["M"], bool(input_onesided),
                                                                                            p["nb"]))
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError("synthesize: scale must be finite")
    from . import engine
    y = engine.pfb_synth(X, p["g"], p["M"], p["hop"], p["first"], p["nout"], phase_ref=1 if phase == "time" else 0,
                         r0=p["r0"] if phase == "time" else 0, onesided=p["onesided"], in_major=1, scale=scale)
    return p["t"], y


def pfb_psd(x, M, taps=8, hop=None, fs=1.0, *, h=None, center=False, scaling="density", axis=-1, return_onesided=None):
    """(f, Pxx): the mean power of every channel over the frames of channelize, accumulated on the device in one pass (the frames
    are never written): float64 [..., nb].  scaling 'density': 1 / (fs sum h^2), 'spectrum': 1 / (sum h)^2, as scipy.signal.welch
    with the window h; for a real input the bins 1 .. M/2 - 1 are doubled."""
    if scaling not in ("density", "spectrum"):
        raise ValueError("pfb_psd: scaling must be 'density' or 'spectrum'")
    y, dev, last, cplx, nsig = _prepare(x, axis, "pfb_psd")
    p = pfb_plan(nsig, cplx, M, taps, hop, fs, h, center, 0, return_onesided)
    s1, s2 = float(np.sum(p["h"])), float(np.sum(p["h"] * p["h"]))
    if not s2 > 0 or (scaling == "spectrum" and s1 == 0):
        raise ValueError("pfb_psd: the taps sum to zero")
    scale = 1.0 / (p["fs"] * s2) if scaling == "density" else 1.0 / (s1 * s1)
    from . import engine
    pxx = engine.pfb(y, p["h"], p["M"], p["hop"], p["first"], p["nframes"], power=True, scale=scale)
    if p["onesided"]:
        pxx[..., 1:p["M"] // 2] *= 2.0
    if not last:
        pxx = pxx.movedim(-1, axis) if dev else np.moveaxis(pxx, -1, axis)
    return p["f"], pxx
