"""Drop-in for the reference's spectrogram.py hot functions: `specgram` (spectrogram.py:49-134) and `stft`
(spectrogram.py:140-168).  Frames are produced by the STFT kernel on the MI355X.  `istft` is the way back: scipy.signal.istft's
signature with the overlap-add synthesis on the GPU (k_istft.hip)."""
import warnings

import numpy as np

from . import engine as _E
from .fft_analysis import fftanal


def specgram(t, s, wl=512, hanning=True, overlap=True, windowAverage=None):
    """(time, fAxis, spectrogram[wl, nWindows]) -- sqrt(8/3)|FFT(hanning(wl) s_i)|^2 / wl per frame with hop
    wl/2 (or |FFT|^2/wl, hop wl, without window/overlap); symmetric np.hanning like the reference (:109).
    windowAverage=k averages k consecutive frames (the reference's branch needs py2 integer division, :116-122)."""
    if windowAverage is not None:
        overlap = False
    s = np.asarray(s).flatten()
    n = len(s)
    dt = np.abs(t[1] - t[0])
    if overlap:
        nWindows = 2 * (n - (n % wl)) // wl - 1
    else:
        nWindows = (n - (n % wl)) // wl - 1
    hop = wl // 2 if overlap else wl
    if hanning:
        win, amp = np.hanning(wl), np.sqrt(8.0 / 3.0) / wl
    else:
        win, amp = np.ones(wl), 1.0 / wl
    out, _ = _E.stft_frames(s, win, hop, nWindows, detrend=False, sided=_E.SIDED_RAW, amp_scale=amp, power=True,
                            bin_major=True)
    spectrogram = out.astype(np.float64)
    fAxis = np.fft.fftfreq(wl, dt)
    if windowAverage is not None:
        k = int(windowAverage)
        nA = nWindows // k
        spectrogram = spectrogram[:, :nA * k].reshape(wl, nA, k).mean(axis=2)
        time = np.linspace(t[0] + wl * dt / 2, t[0] + wl * dt * ((nWindows - 1) + 1 / 2), num=nA)
        return time, fAxis, spectrogram
    if overlap:
        time = np.linspace(t[0] + wl * dt / 2, t[0] + wl * dt * ((nWindows / 2 - 1) + 1 / 2), num=nWindows)
    else:
        time = np.linspace(t[0] + wl * dt / 2, t[0] + wl * dt * ((nWindows - 1) + 1 / 2), num=nWindows)
    return time, fAxis, spectrogram


def stft(tt, y_in, tper=None, returnclass=True, **kwargs):
    """fftanal().init(tt, y_in, tper=tper, **kwargs); .stft()  -> the object, or (twin, freq, Xseg)."""
    tt = np.asarray(tt)
    if tper is None:
        tper = (tt[-1] - tt[0]) / 20
        if tper < tt[2] - tt[1]:
            print("check your stft window size")
    kwargs.setdefault("verbose", False)
    Ystft = fftanal()
    Ystft.init(tt, y_in, tper=tper, **kwargs)
    Ystft.stft()
    if returnclass:
        return Ystft
    twin = np.linspace(tt[0], tt[-1], num=Ystft.Navr, endpoint=True)
    return twin, Ystft.freq, Ystft.Xseg


# ------------------------------------------------------------------------------------------ inverse STFT
def istft_plan(nseg, win, hop, boundary=True, fs=1.0):
    """Host planning of the overlap-add of `nseg` frames of len(win) samples `hop` apart (no library needed): a dict with
    nframes, nfft, hop, L (samples the frames reach), skip and nout (the slice y[skip : skip + nout] that is returned: the
    nfft // 2 extension samples of boundary=True removed at both ends), and the window-square envelope env[n] = sum_g
    win[n - g hop]^2 in float64 as three pieces: `period` (hop values: env[n] = period[n % hop] away from the ends), `head`
    (env[0 : head_len]) and `tail` (env[L - len(tail) : L]).  The ends differ from the periodic part only in the first and
    last nfft - hop samples; when so few frames are given that the two ends meet, `head` is the whole envelope and `tail`
    is empty.  `time` is the time axis of the returned samples."""
    w2 = np.asarray(win, dtype=np.float64) ** 2
    nfft, nseg, hop = int(w2.size), int(nseg), int(hop)
    if nseg < 1 or hop < 1 or hop > nfft:
        raise ValueError("istft_plan: need nseg >= 1 and 1 <= hop <= len(win)")
    L = (nseg - 1) * hop + nfft
    edge = nfft - hop
    period = np.zeros(hop)
    np.add.at(period, np.arange(nfft) % hop, w2)
    if nseg * hop >= edge:
        head = np.zeros(edge)
        tail = np.zeros(edge)
        for k in range(0, edge, hop):                      # frame k / hop starts inside the head; its mirror ends inside the tail
            head[k:] += w2[:edge - k]
            tail[:edge - k] += w2[hop + k:]
    else:
        head = np.zeros(L)
        for g in range(nseg):
            head[g * hop:g * hop + nfft] += w2
        tail = np.zeros(0)
    skip = nfft // 2 if boundary else 0
    nout = L - 2 * skip
    return dict(nframes=nseg, nfft=nfft, hop=hop, L=L, skip=skip, nout=nout, period=period, head=head, head_len=head.size,
                tail=tail, time=np.arange(max(nout, 0)) / float(fs))


def plan_envelope(plan):
    """The full-length envelope env[0 : L] of an istft_plan (period + edges expanded)."""
    L, hop = plan["L"], plan["hop"]
    env = np.resize(plan["period"], L)
    env[:plan["head_len"]] = plan["head"]
    if plan["tail"].size:
        env[L - plan["tail"].size:] = plan["tail"]
    return env


def _plan_nola(plan):
    """True when every returned sample has a non-tiny envelope (scipy's test on `norm`), from the pieces alone."""
    L, hop, lo, hi = plan["L"], plan["hop"], plan["skip"], plan["skip"] + plan["nout"]
    H, T = plan["head_len"], plan["tail"].size
    ok = np.all(plan["head"][lo:min(H, hi)] > 1e-10)
    if T:
        ok = ok and np.all(plan["tail"][max(lo - (L - T), 0):max(hi - (L - T), 0)] > 1e-10)
    a, b = max(lo, H), min(hi, L - T)
    if b > a:
        ok = ok and np.all(plan["period"][np.arange(a, min(b, a + hop)) % hop] > 1e-10)
    return bool(ok)


def _istft_prepare(shape, window, nperseg, noverlap, nfft, input_onesided, boundary, time_axis, freq_axis, scaling, fs):
    """Validate scipy.signal.istft's arguments for spectra of `shape` (before the library loads) ->
    (freq_axis, time_axis, win float64, hop, plan, scale)."""
    freq_axis, time_axis = int(freq_axis), int(time_axis)
    ndim = len(shape)
    if ndim < 2:
        raise ValueError("Input stft must be at least 2d!")
    if not (-ndim <= freq_axis < ndim and -ndim <= time_axis < ndim):
        raise ValueError("freq_axis and time_axis must be axes of the input")
    freq_axis, time_axis = freq_axis % ndim, time_axis % ndim
    if freq_axis == time_axis:
        raise ValueError("Must specify differing time and frequency axes!")
    nseg = int(shape[time_axis])
    n_default = 2 * (int(shape[freq_axis]) - 1) if input_onesided else int(shape[freq_axis])
    if nperseg is None:
        nperseg = n_default
    else:
        nperseg = int(nperseg)
        if nperseg < 1:
            raise ValueError("nperseg must be a positive integer")
    if nfft is None:
        nfft = nperseg if (input_onesided and nperseg == n_default + 1) else n_default
    elif nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    else:
        nfft = int(nfft)
    if noverlap is None:
        noverlap = nperseg // 2
    else:
        noverlap = int(noverlap)
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    if noverlap < 0:
        raise ValueError("noverlap must not be negative.")
    if isinstance(window, str) or type(window) is tuple:
        from .windows import get_window
        win = np.asarray(get_window(window, nperseg), dtype=np.float64)
    else:
        win = np.asarray(window)
        if len(win.shape) != 1:
            raise ValueError("window must be 1-D")
        if win.shape[0] != nperseg:
            raise ValueError("window must have length of %d" % nperseg)
        win = win.astype(np.float64)
    if scaling == "spectrum":
        scale = float(win.sum())
    elif scaling == "psd":
        scale = float(np.sqrt(fs * np.sum(win ** 2)))
    else:
        raise ValueError("Parameter scaling=%r not in ['spectrum', 'psd']!" % (scaling,))
    if nfft != nperseg:
        raise NotImplementedError("istft: nfft (%d) != nperseg (%d) is not supported: frames padded for the transform" % (nfft, nperseg))
    if nperseg < 2:
        raise ValueError("istft: nperseg must be at least 2")
    if nseg < 1:
        raise ValueError("istft: the input holds no segments")
    nb = nfft // 2 + 1 if input_onesided else nfft
    if int(shape[freq_axis]) != nb:
        raise ValueError("istft: %d frequency bins do not match nfft %d" % (shape[freq_axis], nfft))
    plan = istft_plan(nseg, win, nperseg - noverlap, boundary=boundary, fs=fs)
    if plan["nout"] < 1:
        raise ValueError("istft: nothing is left after the boundary extension is removed")
    return freq_axis, time_axis, win, nperseg - noverlap, plan, scale


def istft(Zxx, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, input_onesided=True, boundary=True,
          time_axis=-1, freq_axis=-2, scaling="spectrum"):
    """scipy.signal.istft: (t, x) from the STFT Zxx by windowed overlap-add, normalised by the window-square envelope.
    Same arguments, defaults and conventions as scipy (nperseg from the frequency axis, noverlap = nperseg // 2, the
    nperseg // 2 boundary extension removed, scaling 'spectrum' or 'psd', the NOLA UserWarning); nfft != nperseg is not
    supported.  numpy (or array-like) input returns float64 (input_onesided) or complex128; a device tensor (complex64)
    returns a float32 / complex64 device tensor.  The inverse transforms and the overlap-add run on the GPU (sp_istft)."""
    is_tensor = type(Zxx).__module__.startswith("torch")
    if not is_tensor:
        Zxx = np.asarray(Zxx)
    fa, ta, win, hop, plan, scale = _istft_prepare(tuple(Zxx.shape), window, nperseg, noverlap, nfft, input_onesided, boundary,
                                                   time_axis, freq_axis, scaling, fs)
    if not _plan_nola(plan):
        warnings.warn("NOLA condition failed, STFT may not be invertible."
                      + (" Possibly due to missing boundary" if not boundary else ""), stacklevel=2)
    ndim = len(Zxx.shape)
    outer = [a for a in range(ndim) if a not in (fa, ta)]
    if is_tensor:
        Z = Zxx.permute(*(outer + [fa, ta]))
    else:
        Z = np.transpose(Zxx, outer + [fa, ta])
    x = _E.istft_frames(Z, win, hop, sided=_E.SIDED_HALF if input_onesided else _E.SIDED_RAW, scale=scale, bin_major=True,
                        skip=plan["skip"], nout=plan["nout"])
    if not is_tensor:
        x = x.astype(np.float64 if input_onesided else np.complex128)
    if x.ndim > 1 and ta != ndim - 1:
        dst = ta - 1 if fa < ta else ta
        x = x.movedim(-1, dst) if is_tensor else np.moveaxis(x, -1, dst)
    return np.arange(x.shape[0]) / float(fs), x
