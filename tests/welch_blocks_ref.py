"""Float64 numpy restatement of the time-resolved Welch spectra (sp_welch_blocks), from the definition:

    frames  g = 0 .. nframes - 1,  a_g = win (x[g hop : g hop + nfft] - m_g),  m_g the frame's own mean (segmean) or 0
    blocks  b = 0 .. nblocks - 1 hold the frames b step .. b step + navg - 1,  nblocks = (nframes - navg) // step + 1
    Pxx[b][k] = s_k / navg sum_g |X_g[k]|^2,   Pyy[c][b][k] likewise,   Pxy[c][b][k] = s_k / navg sum_g conj(X_g[k]) Y_g[k]

s_k = scale, doubled on the bins 1 .. nfft/2 - 1 of a real record when `doubled`.  Real records give the bins 0 .. nfft/2, complex
records the natural FFT order.  Also the inputs the host and the GPU tests share."""
import math

import numpy as np


def hann(n):
    """scipy.signal.get_window('hann', n): periodic."""
    return 0.5 - 0.5 * np.cos(2 * math.pi * np.arange(n) / n)


def nframes_of(nsig, nfft, hop):
    return (nsig - nfft) // hop + 1


def nblocks_of(nframes, navg, step):
    return (nframes - navg) // step + 1


def spectra_of(x, nfft, hop, nframes, win, segmean):
    """[nframes, nb] complex128: the transforms of the frames."""
    cplx = np.iscomplexobj(x)
    x = np.asarray(x).astype(np.complex128 if cplx else np.float64)
    a = np.lib.stride_tricks.sliding_window_view(x, nfft)[::hop][:nframes].copy()
    assert a.shape == (nframes, nfft)
    if segmean:
        a -= a.mean(axis=1, keepdims=True)
    if win is not None:
        a *= np.asarray(win, dtype=np.float64)
    return np.fft.fft(a, axis=1) if cplx else np.fft.rfft(a, axis=1)


def block_mean(v, navg, step):
    """[nframes, nb] -> [nblocks, nb]: the mean over the frames b step .. b step + navg - 1."""
    nblocks = nblocks_of(v.shape[0], navg, step)
    return np.stack([v[b * step:b * step + navg].mean(axis=0) for b in range(nblocks)])


def welch_blocks_ref(x, y, nfft, hop, nframes, navg, step, win=None, segmean=True, scale=1.0, doubled=False):
    """-> (Pxx [nblocks, nb], Pyy, Pxy) float64 / complex128; y None: (Pxx, None, None); y [nch, nsig]: Pyy, Pxy [nch, nblocks, nb]."""
    X = spectra_of(x, nfft, hop, nframes, win, segmean)
    s = np.full(X.shape[1], float(scale))
    if doubled and not np.iscomplexobj(x):
        s[1:nfft // 2] *= 2.0
    pxx = block_mean(np.abs(X) ** 2, navg, step) * s
    if y is None:
        return pxx, None, None
    y = np.asarray(y)
    rows = y[None, :] if y.ndim == 1 else y
    pyy, pxy = [], []
    for row in rows:
        Y = spectra_of(row[:len(x)], nfft, hop, nframes, win, segmean)
        pyy.append(block_mean(np.abs(Y) ** 2, navg, step) * s)
        pxy.append(block_mean(np.conj(X) * Y, navg, step) * s)
    if y.ndim == 1:
        return pxx, pyy[0], pxy[0]
    return pxx, np.stack(pyy), np.stack(pxy)


def coherence_ref(pxx, pyy, pxy):
    return np.abs(pxy) ** 2 / (pxx * pyy)


def block_slice(b, nfft, hop, navg, step):
    """The samples [s, e) of block b: the slice scipy.signal.welch / csd sees."""
    s = b * step * hop
    return s, s + (navg - 1) * hop + nfft


def make_pair(nsig, cplx, seed, ax=1.0, ay=1.0, nch=None):
    """Seeded noise plus a common component (so that no reference bin is zero and the coherence is neither 0 nor 1), different
    offsets; float32 / complex64.  nch: y as [nch, nsig], every row with its own noise and share of the common part."""
    rng = np.random.default_rng(seed)

    def noise(*shape):
        v = rng.standard_normal(shape)
        return v + 1j * rng.standard_normal(shape) if cplx else v
    common = noise(nsig)
    x = ax * (common + 0.5 * noise(nsig) + 0.3)
    rows = 1 if nch is None else nch
    y = np.stack([ay * ((0.6 + 0.2 * c) * np.roll(common, 2 + c) + 0.5 * noise(nsig) - 0.2 * (c + 1)) for c in range(rows)])
    dt = np.complex64 if cplx else np.float32
    x, y = np.ascontiguousarray(x, dtype=dt), np.ascontiguousarray(y if nch is not None else y[0], dtype=dt)
    return x, y
