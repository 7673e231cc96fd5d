"""Bispectrum and bicoherence (Kim & Powers 1979): quadratic phase coupling between the modes at f1, f2 and f1 + f2.

    B(f1, f2) = (1/M) sum_k X_k(f1) Y_k(f2) conj(Z_k(f1 + f2))
    b2(f1, f2) = |B|^2 / ((1/M) sum_k |X_k(f1) Y_k(f2)|^2 * (1/M) sum_k |Z_k(f1 + f2)|^2)      in [0, 1]

over the M windowed frames of nfft samples, hop nfft - noverlap, of records detrended as a whole.  Real input: f = rfftfreq(nfft,
1/fs); complex input: f = fftshift(fftfreq(nfft, 1/fs)).  B[i, j] sits at (f1[i], f2[j]); B and b2 are NaN where f1 + f2 falls
outside the frequency axis, b2 is 0 where the denominator is 0.  The contraction over frames runs on the GPU (k_bispec.hip).
"""
import numpy as np

from .windows import get_window

_DETRENDS = {"none": 0, "mean": 1, "linear": 2}
NFFT_MIN, NFFT_MAX = 8, 4096


def _prepare(x, y, z, fs, nfft, noverlap, window, detrend):
    """Validate the arguments (before the library loads) -> (xs, ys, zs, win, hop, nframes, detrend code, freq)."""
    sigs = [_shape(v) for v in (x, y, z) if v is not None]
    if any(ndim != 1 for ndim, _, _ in sigs):
        raise ValueError("bispectrum: signals must be one-dimensional")
    cplx = [c for _, _, c in sigs]
    if any(cplx) and not all(cplx):
        raise ValueError("bispectrum: x, y and z must all be real or all be complex")
    if len({n for _, n, _ in sigs}) != 1:
        raise ValueError("bispectrum: x, y and z must have equal lengths")
    nfft = int(nfft)
    if not NFFT_MIN <= nfft <= NFFT_MAX:
        raise ValueError("bispectrum: nfft must lie in %d .. %d" % (NFFT_MIN, NFFT_MAX))
    noverlap = nfft // 2 if noverlap is None else int(noverlap)
    if noverlap < 0 or noverlap >= nfft:
        raise ValueError("bispectrum: need 0 <= noverlap < nfft")
    nsig = sigs[0][1]
    if nsig < nfft:
        raise ValueError("bispectrum: the record (%d samples) is shorter than nfft (%d)" % (nsig, nfft))
    if not fs > 0:
        raise ValueError("bispectrum: fs must be positive")
    if detrend not in _DETRENDS:
        raise ValueError("bispectrum: detrend must be 'none', 'mean' or 'linear'")
    if isinstance(window, str) or isinstance(window, tuple):
        win = np.asarray(get_window(window, nfft), dtype=np.float64)
    else:
        win = np.asarray(window, dtype=np.float64)
        if win.shape != (nfft,):
            raise ValueError("bispectrum: a window array must have length nfft")
    hop = nfft - noverlap
    nframes = 1 + (nsig - nfft) // hop
    return win, hop, nframes, _DETRENDS[detrend], freq_axis(nfft, fs, cplx[0])


def freq_axis(nfft, fs, cplx):
    """The frequency of each bin: rfftfreq for real input, fftshift(fftfreq) for complex input."""
    if cplx:
        return np.fft.fftshift(np.fft.fftfreq(nfft, 1.0 / fs))
    return np.fft.rfftfreq(nfft, 1.0 / fs)


def valid_region(nfft, cplx):
    """Boolean [nb, nb]: True where the sum bin of (i, j) lies on the frequency axis."""
    nb = nfft if cplx else nfft // 2 + 1
    c0 = nfft // 2 if cplx else 0
    s = np.arange(nb)[:, None] + np.arange(nb)[None, :] - c0
    return (s >= 0) & (s < nb)


def bispectrum(x, y=None, z=None, fs=1.0, nfft=512, noverlap=None, window="hanning", detrend="mean"):
    """(f1, f2, B, b2): the bispectrum B (complex128 [nb, nb]) and the bicoherence b2 of x (auto) or of x, y, z (cross; y and z
    default to x).  numpy or device-tensor input; device tensors give device tensors."""
    win, hop, nframes, dt, f = _prepare(x, y, z, fs, nfft, noverlap, window, detrend)
    from . import engine
    B, b2, _ = engine.bispectrum(x, win, hop, nframes, y=y, z=z, detrend=dt)
    return f, f.copy(), B, b2


def bicoherence(x, y=None, z=None, fs=1.0, nfft=512, noverlap=None, window="hanning", detrend="mean"):
    """(f1, f2, b2): the bicoherence of bispectrum()."""
    f1, f2, _, b2 = bispectrum(x, y, z, fs=fs, nfft=nfft, noverlap=noverlap, window=window, detrend=detrend)
    return f1, f2, b2


def _shape(v):
    """(ndim, size, complex?) of a numpy array, array-like or device tensor, without copying a tensor to the host."""
    if type(v).__module__.startswith("torch"):
        return v.dim(), v.numel(), v.is_complex()
    a = np.asarray(v)
    return a.ndim, a.size, np.iscomplexobj(a)
