"""Float64 reference of the continuous wavelet transform (numpy), written from the definitions:
    H_s[k] = sqrt(2 pi s') psi0^(s' w_k),  w_k = 2 pi k / L for 0 < k <= L / 2, 0 elsewhere;  scales s' in samples
    Morlet(w0): psi0^(u) = pi^(-1/4) exp(-(u - w0)^2 / 2);   Paul(m): psi0^(u) = 2^m / sqrt(m (2m - 1)!) u^m exp(-u)
    W = ifft(fft(x, N_full)[None, :] * H)[:, :N],  N_full = next_pow2(2 N): a linear convolution, nothing wraps.
Also the float64 / float32 restatement of the overlap-save plan the device runs, the margin rule, and the records the tests share."""
import math

import numpy as np


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def psi_ft(family, param, u):
    u = np.asarray(u, dtype=np.float64)
    pos = u > 0
    us = np.where(pos, u, 1.0)
    if family == "morlet":
        v = math.pi ** -0.25 * np.exp(-0.5 * (us - param) ** 2)
    elif family == "paul":
        m = param
        v = 2.0 ** m / math.sqrt(m * math.gamma(2 * m)) * us ** m * np.exp(-us)
    else:
        raise ValueError(family)
    return np.where(pos, v, 0.0)


def filters(family, param, scales, L):
    s = np.asarray(scales, dtype=np.float64)[:, None]
    k = np.arange(L)
    H = np.sqrt(2 * math.pi * s) * psi_ft(family, param, s * (2 * math.pi * k / L)[None, :])
    H[:, 0] = 0.0
    H[:, k > L // 2] = 0.0
    return H


def cwt_ref(x, scales, family="morlet", param=6.0, n_full=None):
    x = np.asarray(x)
    n = x.shape[-1]
    n_full = next_pow2(2 * n) if n_full is None else n_full
    X = np.fft.fft(x.astype(np.complex128), n_full, axis=-1)
    return np.fft.ifft(X[..., None, :] * filters(family, param, scales, n_full), axis=-1)[..., :n]


def kernel_time(family, param, s, grid):
    """g_s = ifft(H_s) on `grid` points."""
    return np.fft.ifft(filters(family, param, [s], grid)[0])


def margin_ref(family, param, s, tail=1e-6, grid=1 << 18):
    a = np.abs(kernel_time(family, param, s, grid))
    total = a.sum()
    for_dist = a[:grid // 2 + 1].copy()
    for_dist[1:grid // 2] += a[:grid // 2:-1]
    tails = np.cumsum(for_dist[::-1])[::-1]
    ok = np.nonzero(tails <= tail * total)[0]
    return int(ok[0]) if ok.size else grid // 2 + 1


def overlap_save(x, scales, family, param, L, M, dtype=np.float64):
    """The device's plan restated in numpy at `dtype` (float64, or float32 with complex64 transforms): frame g = the L samples from
    g hop - M on, zero outside the record; one forward transform, per scale the filter and an inverse transform; the elements
    M .. M + hop - 1 are the samples g hop .. < N."""
    x = np.asarray(x)
    n = x.shape[-1]
    hop = L - 2 * M
    frames = -(-n // hop)
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    S = len(scales)
    if dtype == np.float64:
        H = filters(family, param, scales, L)
    else:
        # as the kernel forms it: exp(c + p ln u - a d^2 - b d) from float32 constants
        k = np.arange(L, dtype=np.float32)
        sc = np.asarray(scales, dtype=np.float64)
        step = (2 * math.pi * sc / L).astype(np.float32)[:, None]
        if family == "morlet":
            lognorm, p, a, b, u0 = -0.25 * math.log(math.pi), 0.0, 0.5, 0.0, param
        else:
            lognorm, p, a, b, u0 = param * math.log(2) - 0.5 * (math.log(param) + math.lgamma(2 * param)), param, 0.0, 1.0, 0.0
        c = (lognorm + 0.5 * np.log(2 * math.pi * sc)).astype(np.float32)[:, None]
        u = k[None, :] * step
        d = u - np.float32(u0)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = c - np.float32(a) * d * d - np.float32(b) * d
            if p:
                e = e + np.float32(p) * np.log(np.where(u > 0, u, np.float32(1)))
            H = np.exp(e).astype(np.float32)
        kk = np.arange(L)
        H[:, (kk < 1) | (kk > L // 2)] = 0
    W = np.zeros((S, n), dtype=ctype)
    xp = np.zeros(M + frames * hop + L, dtype=ctype)
    xp[M:M + n] = x
    for g in range(frames):
        fr = xp[g * hop:g * hop + L]
        if dtype == np.float64:
            Y = np.fft.ifft(np.fft.fft(fr)[None, :] * H, axis=-1)
        else:
            import scipy.fft as sf
            Y = sf.ifft((sf.fft(fr)[None, :] * H).astype(np.complex64), axis=-1)
        n1 = min(n, (g + 1) * hop)
        W[:, g * hop:n1] = Y[:, M:M + n1 - g * hop]
    return W


def row_err(got, ref):
    """max |got - ref| over the row's rms of ref, per scale row -> the worst."""
    got, ref = np.asarray(got), np.asarray(ref)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1))
    return float(np.max(np.max(np.abs(got - ref), axis=-1) / rms))


def make_signal(n, cplx=False, seed=0, slow=True):
    """Noise plus lines over three decades, so that no scale row is empty (slow=False: without the two slowest lines, mean removed)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.5 * rng.standard_normal(n)
    for f, a in ((0.31, 0.4), (0.11, 0.7), (0.037, 1.0), (0.0091, 0.8), (0.0023, 0.6), (0.0007, 0.9))[:6 if slow else 4]:
        x = x + a * np.cos(2 * math.pi * f * t + 10 * f)
    if not slow:
        x = x - x.mean()
    if cplx:
        y = 0.5 * rng.standard_normal(n)
        for f, a in ((0.27, 0.5), (0.05, 0.6), (0.004, 0.7)):
            y = y + a * np.sin(2 * math.pi * f * t + 3 * f)
        return (x + 1j * y).astype(np.complex64)
    return x.astype(np.float32)


def composed_f32(x, scales, family, param):
    """The whole-record path restated at float32: complex64 transforms of next_pow2(2 N) points, float32 filter rows."""
    import scipy.fft as sf
    x = np.asarray(x)
    n = x.shape[-1]
    n_full = next_pow2(2 * n)
    xp = np.zeros(n_full, dtype=np.complex64)
    xp[:n] = x
    H = filters(family, param, scales, n_full).astype(np.float32)
    return sf.ifft((sf.fft(xp)[None, :] * H).astype(np.complex64), axis=-1)[:, :n]


def cdelta_ref(family, param, scales, dj, psi0, probe="line"):
    """C_delta (dt = 1) through cwt_ref: the factor by which sum_j dj Re W_n(s_j) / (psi0(0) sqrt(s_j)) exceeds the record, read off in
    the middle of the record.  probe 'line': a cosine in the middle of the set's band (u_peak / sqrt(s_min s_max)); 'delta': a unit
    sample, eq. 13 read literally."""
    scales = np.asarray(scales, dtype=np.float64)
    n = 8192
    t = np.arange(n)
    if probe == "line":
        x = np.cos(param / math.sqrt(scales.min() * scales.max()) * (t - n // 2))
    else:
        x = (t == n // 2).astype(np.float64)
    Wd = cwt_ref(x, scales, family, param)[:, n // 2].real
    return dj / psi0 * float(np.sum(Wd / np.sqrt(scales)))


def band_limited(n, periods, seed=0):
    """Lines at the given periods (samples) under a smooth envelope that vanishes at the ends of the record."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    env = np.sin(math.pi * (t + 0.5) / n) ** 2
    x = np.zeros(n)
    for p in periods:
        x += rng.uniform(0.5, 1.0) * np.cos(2 * math.pi * t / p + rng.uniform(0, 2 * math.pi))
    return (env * x).astype(np.float32)
