"""Filtering.  The reference's filters.py has scipy IIR wrappers, resamplers and an np.convolve smoother
(filters.py:20-358) and no FFT/overlap-add filter; `fftfilt` is the build-defined hot function for that slot:
causal FIR y = lfilter(b, 1, x) by overlap-save on the MI355X.  The IIR wrappers run on the device as cascades of
second-order sections, evaluated exactly (engine.sos_filter / sos_filtfilt): `sosfilt`, `sosfiltfilt`, `lfilter`,
`filtfilt` with scipy.signal's signatures, and the reference's `butter_bandpass`, `butter_lowpass`,
`butter_lowpass_filter`, `complex_filtfilt`.  The resamplers need the absent pybaseutils.utils.interp."""
import numpy as np
import scipy.signal as _dsp

from . import engine as _E
from .engine import _is_torch
from .notch_filter import apply_notch  # noqa: F401  (notch application lives with the design)


def fftfilt(b, x, nfft=None):
    """y[n] = sum_k b[k] x[n-k], same length as x (float32 math on the GPU; float64 returned for float64 x)."""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("fftfilt: 1-D signal expected")
    y = _E.fir_filter(np.asarray(b, dtype=np.float64), x, nfft=0 if nfft is None else int(nfft))
    return y.astype(np.float64) if x.dtype != np.float32 else y


def smooth(x, window_len=11, window="hanning"):
    """Window-FIR smoother of the reference (filters.py:226-283: reflect-pad, convolve with w/sum(w), 'valid')
    with the convolution done by the GPU FIR kernel."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("smooth only accepts 1 dimension arrays.")
    if x.size < window_len:
        raise ValueError("Input vector needs to be bigger than window size.")
    if window_len < 3:
        return x
    if window not in ("flat", "hanning", "hamming", "bartlett", "blackman"):
        raise ValueError("Window is on of 'flat', 'hanning', 'hamming', 'bartlett', 'blackman'")
    s = np.r_[x[window_len - 1:0:-1], x, x[-2:-window_len - 1:-1]]
    w = np.ones(window_len) if window == "flat" else getattr(np, window)(window_len)
    full = _E.fir_filter(w / w.sum(), s).astype(np.float64)
    return full[window_len - 1:]          # == np.convolve(w/w.sum(), s, mode='valid')


# ------------------------------------------------------------------------------------------ IIR (F3)
def _to_last(x, axis):
    return _E.torch.movedim(x, axis, -1) if _is_torch(x) else np.moveaxis(np.asarray(x), axis, -1)


def _from_last(y, axis):
    return _E.torch.movedim(y, -1, axis) if _is_torch(y) else np.moveaxis(y, -1, axis)


def sosfilt(sos, x, axis=-1, zi=None):
    """scipy.signal.sosfilt on the GPU: y, or (y, zf) when zi is given (zi / zf in scipy's shape: (n_sections, ..., 2)
    with x's shape less `axis` in the middle), so a long record can be filtered in pieces."""
    xl = _to_last(x, axis)
    if zi is None:
        return _from_last(_E.sos_filter(sos, xl), axis)
    # zi's middle axes are x's shape without `axis`, in order: the lead shape of xl, nothing to move
    y, zf = _E.sos_filter(sos, xl, zi=zi)
    return _from_last(y, axis), zf


def _sos_padlen(sos):
    """sosfiltfilt's default padlen: 3 * (2 n_sections + 1 - min(trailing-zero b2 count, trailing-zero a2 count))"""
    s = _E.sos_array(sos)
    ntaps = 2 * s.shape[0] + 1
    ntaps -= min(int((s[:, 2] == 0).sum()), int((s[:, 5] == 0).sum()))
    return 3 * ntaps


def sosfiltfilt(sos, x, axis=-1, padtype="odd", padlen=None):
    """scipy.signal.sosfiltfilt on the GPU (forward and backward in one device sequence, no host round trip between)."""
    if padlen is None:
        padlen = _sos_padlen(sos)
    return _from_last(_E.sos_filtfilt(sos, _to_last(x, axis), padtype=padtype, padlen=padlen), axis)


def _tf_sos(b, a):
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    if a.size < 1 or a[0] == 0.0:
        raise ValueError("a[0] must not be zero")
    if max(b.size, a.size) - 1 > 2 * _E.MAX_SECTIONS:
        raise ValueError("filter order %d: at most %d is supported" % (max(b.size, a.size) - 1, 2 * _E.MAX_SECTIONS))
    return _dsp.tf2sos(b, a)


def lfilter(b, a, x, axis=-1, zi=None):
    """scipy.signal.lfilter for real (b, a) of order <= 16, as second-order sections (scipy.signal.tf2sos) on the GPU."""
    if zi is not None:
        raise NotImplementedError("lfilter: tf-form zi; use sosfilt(tf2sos(b, a), x, zi=...) to filter in pieces")
    return sosfilt(_tf_sos(b, a), x, axis=axis)


def filtfilt(b, a, x, axis=-1, padtype="odd", padlen=None, method="pad", irlen=None):
    """scipy.signal.filtfilt (method 'pad') for real (b, a) of order <= 16, as second-order sections on the GPU; the
    tf-form default padlen = 3 * max(len(a), len(b)) is kept."""
    if method != "pad":
        raise NotImplementedError("filtfilt: method=%r (Gustafsson's method is not provided)" % (method,))
    if padlen is None:
        padlen = 3 * max(np.size(a), np.size(b))
    return sosfiltfilt(_tf_sos(b, a), x, axis=axis, padtype=padtype, padlen=padlen)


def butter_bandpass(x, fs=4e6, lf=1000, hf=500e3, order=3, disp=0):
    """Reference filters.py:323: causal Butterworth band-pass [lf, hf] of `order` (lfilter along the last axis).  The
    sections are designed directly (butter(..., output='sos')): the same filter as the reference's (b, a), better
    conditioned."""
    nyq = 0.5 * fs
    sos = _dsp.butter(order, [lf / nyq, hf / nyq], btype="band", analog=False, output="sos")
    return sosfilt(sos, x)


def butter_lowpass(cutoff, fnyq, order=5):
    """Reference filters.py:336: Butterworth low-pass design (b, a) with the cutoff normalised by `fnyq` (host)."""
    return _dsp.butter(order, cutoff / fnyq, btype="low", analog=False)


def butter_lowpass_filter(data, cutoff, fs, order=5, axis=0):
    """Reference filters.py:344: zero-phase Butterworth low-pass along `axis`.  Like the reference it passes fs where
    butter_lowpass expects the Nyquist frequency, so the cutoff is normalised by fs, not fs / 2.  filtfilt's tf-form
    default padlen (3 (order + 1)) is kept; the sections are designed directly."""
    sos = _dsp.butter(order, cutoff / fs, btype="low", analog=False, output="sos")
    return sosfiltfilt(sos, data, axis=axis, padlen=3 * (order + 1))


def complex_filtfilt(filt_n, filt_d, data):
    """Reference filters.py:351: filtfilt of the real and the imaginary part (the IQ signal of Doppler.py:196-197)."""
    if not (_is_torch(data) and data.is_complex()) and not np.iscomplexobj(data):
        data = np.asarray(data) + 0j
    return filtfilt(filt_n, filt_d, data)


def upsample(u_t, Fs, Fs_new, plotit=False):
    raise NotImplementedError("upsample needs pybaseutils.utils.interp (absent from the reference)")


def downsample(u_t, Fs, Fs_new, plotit=False):
    raise NotImplementedError("downsample needs pybaseutils.utils.interp (absent from the reference)")


def downsample_efficient(u_t, Fs, Fs_new, plotit=False, halforder=2, lowpass=None):
    raise NotImplementedError("downsample_efficient needs pybaseutils.utils.interp (absent from the reference)")
