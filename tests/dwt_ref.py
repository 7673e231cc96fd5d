"""The discrete wavelet transforms restated on the CPU (include/spectral_dwt.h states the formulas): float64 by gathers through the index
maps, an independent form by numpy.pad + numpy.convolve, a float32 restatement, and a rigorous running bound carried beside the
coefficients.  The last axis is the row; every function takes any leading axes.

The bound.  A coefficient is a chain of L float32 FMAs (u = 2^-24): its error against the exact sum over the inputs it read is at most
gamma_L sum |h| |v^| <= (L + 1) u sum |h| |v| (L^2 u << 1 pays for v^ against v), and the inputs' own errors B pass through |h|:
    B_out = (L + 1) u (|h| * |v|) + (|h| * B_in)            on the same index map, B = 0 for float32-exact inputs,
for a synthesis with both filters' sums (two chains of L / 2 and one addition: L / 2 + 1 roundings a term), and with L + 2 for the
inverse MODWT (two chains of L and one addition).  For complex rows |.| is the modulus and the bound holds for the modulus of the
error.  The filters are rounded to float32 first, as the library does, so they carry no error."""
import numpy as np

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
MODES = ("zero", "constant", "symmetric", "reflect", "periodic", "periodization")
PAD = {"zero": "constant", "constant": "edge", "symmetric": "symmetric", "reflect": "reflect", "periodic": "wrap"}


EXACT_FILTERS = False                   # True (a test patches it): the filters stay float64, for perfect reconstruction in float64


def f32(a):
    """a rounded to float32, as float64: what the library does to the filters once"""
    a = np.asarray(a, dtype=np.float64)
    return a if EXACT_FILTERS else a.astype(np.float32).astype(np.float64)


def orth_bank(g):
    g = np.asarray(g, dtype=np.float64)
    rec_hi = g[::-1] * (-1.0) ** np.arange(g.size)
    return g[::-1].copy(), rec_hi[::-1].copy(), g.copy(), rec_hi


def bank_of(L, seed=7):
    """a bank of length L: Haar, db2's closed form, and beyond them four filters from a random g, which no table holds (the formulas take any
    four filters; perfect reconstruction is tested with the Daubechies banks the package computes)"""
    s3 = np.sqrt(3.0)
    if L == 2:
        g = np.array([1.0, 1.0]) / np.sqrt(2.0)
    elif L == 4:
        g = np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0))
    else:
        g = np.random.default_rng(seed + L).standard_normal(L) / np.sqrt(L)
    return orth_bank(g)


def coeff_len(n, L, mode):
    return (n + 1) // 2 if mode == "periodization" else (n + L - 1) // 2


def ext_index(i, n, mode):
    """the extension as a map of the index: where sample i of the extended array is read, -1 for a zero"""
    i = np.asarray(i, dtype=np.int64)
    if mode == "zero":
        return np.where((i < 0) | (i >= n), -1, i)
    if mode == "constant":
        return np.clip(i, 0, n - 1)
    if mode == "symmetric":
        r = np.mod(i, 2 * n)
        return np.where(r < n, r, 2 * n - 1 - r)
    if mode == "reflect":
        if n == 1:
            return np.zeros_like(i)
        r = np.mod(i, 2 * n - 2)
        return np.where(r < n, r, 2 * n - 2 - r)
    if mode == "periodic":
        return np.mod(i, n)
    if mode == "periodization":
        return np.minimum(np.mod(i, n + (n & 1)), n - 1)
    raise ValueError(mode)


def gather(v, idx):
    out = v[..., np.maximum(idx, 0)]
    out[..., idx < 0] = 0
    return out


def _chain32(h, X):
    """sum_m h[m] X[..., m] as a float32 FMA chain, m ascending (the product is exact in float64; the sum is rounded to float32)"""
    acc = np.zeros(X.shape[:-1], dtype=X.dtype)
    for m in range(h.size):
        acc = (h[m] * X[..., m] + acc).astype(np.complex64 if np.iscomplexobj(X) else np.float32).astype(X.dtype)
    return acc


def _sums(X, fa, B, XB, rounds, single):
    """(the sum over the last axis of X with fa, its bound or None)"""
    c = _chain32(fa, X) if single else X @ fa
    if B is None:
        return c, None
    return c, rounds * U * (np.abs(X) @ np.abs(fa)) + XB @ np.abs(fa)


def ana_index(n, L, mode):
    K, c = coeff_len(n, L, mode), (L // 2 if mode == "periodization" else 1)
    return ext_index(2 * np.arange(K)[:, None] + c - np.arange(L)[None, :], n, mode)


def dwt_level(v, lo, hi, mode, B=None, single=False):
    """one analysis level -> (cA, cD, bA, bD); the bounds are None without B (B = 0.0 starts one)"""
    lo, hi = f32(lo), f32(hi)
    idx = ana_index(v.shape[-1], lo.size, mode)
    X = gather(v, idx)
    XB = None if B is None else gather(np.broadcast_to(np.asarray(B, dtype=np.float64), np.abs(v).shape).copy(), idx)
    cA, bA = _sums(X, lo, B, XB, lo.size + 1, single)
    cD, bD = _sums(X, hi, B, XB, lo.size + 1, single)
    return cA, cD, bA, bD


def dwt_level_conv(v, lo, hi, mode):
    """the independent form, one row: numpy.pad with the matching mode, numpy.convolve, every second sample"""
    lo, hi, L = f32(lo), f32(hi), len(lo)
    if mode == "periodization":
        if v.size & 1:
            v = np.concatenate((v, v[-1:]))
        xe = np.pad(v, L - 1, "wrap")
        return tuple(np.convolve(xe, f, "valid")[L // 2::2][:v.size // 2] for f in (lo, hi))
    xe = np.pad(v, L - 1, PAD[mode])
    return tuple(np.convolve(xe, f, "valid")[1::2] for f in (lo, hi))


def wavedec(v, lo, hi, mode, levels, B=None, single=False):
    """-> ([cA_J, cD_J, .., cD_1], their bounds or Nones)"""
    out, bounds, a, b = [], [], v, B
    for _ in range(levels):
        a, d, b, bd = dwt_level(a, lo, hi, mode, b, single)
        if single:
            a = a.astype(np.complex64 if np.iscomplexobj(a) else np.float32).astype(a.dtype)
        out.insert(0, d)
        bounds.insert(0, bd)
    return [a] + out, [b] + bounds


def idwt_level(cA, cD, n, lo, hi, mode, BA=None, BD=None, single=False):
    """one synthesis level of n samples -> (x, its bound or None)"""
    lo, hi = f32(lo), f32(hi)
    L, K = lo.size, cA.shape[-1]
    assert K == coeff_len(n, L, mode) and cD.shape[-1] == K
    t = np.arange(n) + (L // 2 - 1 if mode == "periodization" else L - 2)
    k = (t >> 1)[:, None] - np.arange(L // 2)[None, :]
    k = np.mod(k, K) if mode == "periodization" else k
    assert k.min() >= 0 and k.max() < K
    j = (t & 1)[:, None] + 2 * np.arange(L // 2)[None, :]
    XA, XD = cA[..., k], cD[..., k]
    if single:
        x = np.zeros(XA.shape[:-1], dtype=XA.dtype)
        sa, sd = x.copy(), x.copy()
        st = np.complex64 if np.iscomplexobj(XA) else np.float32
        for q in range(L // 2):
            sa = (lo[j[:, q]] * XA[..., q] + sa).astype(st).astype(XA.dtype)
            sd = (hi[j[:, q]] * XD[..., q] + sd).astype(st).astype(XA.dtype)
        x = (sa + sd).astype(st).astype(XA.dtype)
    else:
        x = np.sum(lo[j] * XA, axis=-1) + np.sum(hi[j] * XD, axis=-1)
    if BA is None:
        return x, None
    BA, BD = (np.broadcast_to(np.asarray(b, dtype=np.float64), np.abs(cA).shape) for b in (BA, BD))
    mag = np.sum(np.abs(lo[j]) * np.abs(XA), axis=-1) + np.sum(np.abs(hi[j]) * np.abs(XD), axis=-1)
    return x, (L + 1) * U * mag + np.sum(np.abs(lo[j]) * BA[..., k], axis=-1) + np.sum(np.abs(hi[j]) * BD[..., k], axis=-1)


def idwt_level_conv(cA, cD, n, lo, hi, mode):
    """the independent form, one row: zero-stuff, convolve, cut (periodization: scatter modulo 2K)"""
    lo, hi = f32(lo), f32(hi)
    L, K = lo.size, cA.size
    if mode == "periodization":
        x = np.zeros(2 * K, dtype=cA.dtype)
        for kk in range(K):
            for j in range(L):
                x[(2 * kk - L // 2 + 1 + j) % (2 * K)] += lo[j] * cA[kk] + hi[j] * cD[kk]
        return x[:n]
    ua, ud = np.zeros(2 * K, dtype=cA.dtype), np.zeros(2 * K, dtype=cA.dtype)
    ua[::2], ud[::2] = cA, cD
    return (np.convolve(ua, lo) + np.convolve(ud, hi))[L - 2:L - 2 + n]


def level_lens(n, L, mode, levels):
    lens = [n]
    for _ in range(levels):
        lens.append(coeff_len(lens[-1], L, mode))
    return lens


def waverec(coeffs, n, lo, hi, mode, bounds=None, single=False):
    """the rows of n samples back from [cA_J, cD_J, .., cD_1] -> (x, its bound or None)"""
    levels = len(coeffs) - 1
    lens = level_lens(n, len(lo), mode, levels)
    a, b = coeffs[0], None if bounds is None else bounds[0]
    for j in range(levels, 0, -1):
        d = coeffs[levels - j + 1]
        a, b = idwt_level(a, d, lens[j - 1], lo, hi, mode, b, None if bounds is None else bounds[levels - j + 1], single)
        if single:
            a = a.astype(np.complex64 if np.iscomplexobj(a) else np.float32).astype(a.dtype)
    return a, b


def modwt_filters(rec_lo, rec_hi):
    s = 0.70710678118654752440
    return f32(np.asarray(rec_lo, dtype=np.float64) * s), f32(np.asarray(rec_hi, dtype=np.float64) * s)


def modwt(v, rec_lo, rec_hi, levels, B=None, single=False):
    """-> (W[levels + 1, ..., n] = W_1 .. W_J, V_J, the bounds alike or None)"""
    g, h = modwt_filters(rec_lo, rec_hi)
    n, L = v.shape[-1], g.size
    out, bounds, a, b = [], [], v, B
    for j in range(1, levels + 1):
        idx = np.mod(np.arange(n)[:, None] - (1 << (j - 1)) * np.arange(L)[None, :], n)
        X = a[..., idx]
        XB = None if b is None else np.broadcast_to(np.asarray(b, dtype=np.float64), np.abs(a).shape)[..., idx]
        w, bw = _sums(X, h, b, XB, L + 1, single)
        a, b = _sums(X, g, b, XB, L + 1, single)
        out.append(w)
        bounds.append(bw)
    return np.stack(out + [a]), (None if B is None else np.stack(bounds + [b]))


def imodwt(W, rec_lo, rec_hi, B=None, single=False):
    """-> (x, its bound or None) from W[levels + 1, ..., n]; B: the bounds of W alike, or 0.0"""
    g, h = modwt_filters(rec_lo, rec_hi)
    levels, n, L = W.shape[0] - 1, W.shape[-1], g.size
    Bw = None if B is None else np.broadcast_to(np.asarray(B, dtype=np.float64), np.abs(W).shape)
    a, b = W[levels], None if B is None else Bw[levels]
    for j in range(levels, 0, -1):
        idx = np.mod(np.arange(n)[:, None] + (1 << (j - 1)) * np.arange(L)[None, :], n)
        XW, XV = W[j - 1][..., idx], a[..., idx]
        if single:
            st = np.complex64 if np.iscomplexobj(W) else np.float32
            a2 = (_chain32(h, XW) + _chain32(g, XV)).astype(st).astype(W.dtype)
        else:
            a2 = XW @ h + XV @ g
        if B is not None:
            b = (L + 2) * U * (np.abs(XW) @ np.abs(h) + np.abs(XV) @ np.abs(g)) + Bw[j - 1][..., idx] @ np.abs(h) + b[..., idx] @ np.abs(g)
        a = a2
    return a, b


def wpdec(v, lo, hi, level, B=None):
    """the packet table in natural order -> (c[..., 2^level, n / 2^level], its bound or None)"""
    c, b = v[..., None, :], None if B is None else np.broadcast_to(np.asarray(B, dtype=np.float64), np.abs(v).shape)[..., None, :]
    for _ in range(level):
        a, d, ba, bd = dwt_level(c, lo, hi, "periodization", b)
        c = np.stack((a, d), axis=-2).reshape(c.shape[:-2] + (2 * c.shape[-2], a.shape[-1]))
        b = None if B is None else np.stack((ba, bd), axis=-2).reshape(c.shape)
    return c, b


def wprec(c, lo, hi, B=None):
    b = None if B is None else np.broadcast_to(np.asarray(B, dtype=np.float64), np.abs(c).shape)
    while c.shape[-2] > 1:
        m = c.shape[-1]
        pair = c.reshape(c.shape[:-2] + (c.shape[-2] // 2, 2, m))
        pb = None if b is None else b.reshape(pair.shape)
        c, b = idwt_level(pair[..., 0, :], pair[..., 1, :], 2 * m, lo, hi, "periodization", None if b is None else pb[..., 0, :], None if b is None else pb[..., 1, :])
    return c[..., 0, :], None if b is None else b[..., 0, :]


def gray(level):
    f = np.arange(1 << level)
    return f ^ (f >> 1)


def signal(n, rows=1, cplx=False, seed=0):
    """float32-exact rows with a trend, a tone and noise, so that no mode's extension is trivial"""
    rng = np.random.default_rng(1000 * seed + n)
    t = np.arange(n)
    x = 0.5 + 0.01 * t + np.cos(0.37 * t + 0.2) + rng.standard_normal((rows, n))
    if cplx:
        x = x + 1j * (np.sin(0.11 * t) - 0.3 + rng.standard_normal((rows, n)))
        return x.astype(np.complex64)
    return x.astype(np.float32)


# ---- the record of the Python layer's test: a known octave structure --------------------------------------------------------------
OCTAVE_N, OCTAVE_LEVEL = 4096, 6
# the errors of the float32 restatement (single=True) against float64 at this shape, db4, measured on the CPU
# (tests/test_host_dwt.py::test_the_recorded_float32_figures re-measures them); the GPU test allows 4 x each
F32_VARIANCE_REL = 1.733e-8      # max_j |nu2_32[j] - nu2_64[j]| / nu2_64[j]
F32_MRA_SUM = 9.73e-7      # max_t |sum_e mra_32[e][t] - x[t]|


def octave_record():
    """a period of 3 samples (level 1: periods 2 .. 4) and, twice as strong, one of 24 (level 4: periods 16 .. 32), in weak noise"""
    t = np.arange(OCTAVE_N)
    x = np.sin(2 * np.pi * t / 3.0) + 2.0 * np.sin(2 * np.pi * t / 24.0 + 0.4) + 0.05 * np.random.default_rng(12).standard_normal(OCTAVE_N)
    return x.astype(np.float32)


def modwt_variance(v, rec_lo, rec_hi, levels, single=False):
    """the unbiased wavelet variance of one row -> (nu2[levels], edof[levels])"""
    W, _ = modwt(v, rec_lo, rec_hi, levels, single=single)
    n, L = v.shape[-1], len(rec_lo)
    nu2, edof = [], []
    for j in range(1, levels + 1):
        Lj = ((1 << j) - 1) * (L - 1) + 1
        M = n - Lj + 1
        nu2.append(np.sum(np.abs(W[j - 1][..., Lj - 1:]) ** 2, axis=-1) / M)
        edof.append(max(M / float(1 << j), 1.0))
    return np.asarray(nu2), np.asarray(edof)


def modwt_mra(W, rec_lo, rec_hi, single=False):
    out = []
    for e in range(W.shape[0]):
        Z = np.zeros_like(W)
        Z[e] = W[e]
        out.append(imodwt(Z, rec_lo, rec_hi, single=single)[0])
    return np.stack(out)


def float32_figures(rec_lo, rec_hi):
    """-> (F32_VARIANCE_REL, F32_MRA_SUM) as measured now"""
    x = octave_record().astype(np.float64)
    v64, _ = modwt_variance(x, rec_lo, rec_hi, OCTAVE_LEVEL)
    v32, _ = modwt_variance(x, rec_lo, rec_hi, OCTAVE_LEVEL, single=True)
    W32, _ = modwt(x, rec_lo, rec_hi, OCTAVE_LEVEL, single=True)
    mra = modwt_mra(W32, rec_lo, rec_hi, single=True)
    return float(np.max(np.abs(v32 - v64) / v64)), float(np.max(np.abs(mra.sum(axis=0) - x)))
