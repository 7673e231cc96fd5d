"""The discrete wavelet transform on the GPU: the decimated pyramid (dwt / idwt, wavedec / waverec in pywt's conventions), the undecimated
MODWT with its multiresolution analysis and the wavelet variance (Percival & Walden), and wavelet packets.

Every coefficient is computed by the kernels of pyfft_amd/csrc/k_dwt.hip through `engine.dwt`, `dwt_level`, `idwt`, `idwt_level`, `modwt`
and `imodwt` (include/spectral_dwt.h states the formulas); this module holds the host side: the filter banks, the bookkeeping of the
lists and axes, and the orderings of the packet nodes.  numpy arrays in -> numpy arrays out; device tensors in -> device tensors out
on the tensor's stream.  There is no CPU implementation behind these functions.

Filter banks are pywt's 4-tuples (dec_lo, dec_hi, rec_lo, rec_hi).  Only the Daubechies family is built in, computed at call time by
spectral factorisation; any other bank (symlets, coiflets, biorthogonal pairs zero-padded to one even length) is passed as a 4-tuple or
as an object with a `filter_bank` attribute, which a pywt.Wavelet is."""
import functools
import math

import numpy as np

from . import engine as E
from .engine import DwtRefused, dwt_coeff_len as _coeff_len

try:
    import torch
except Exception:                       # pragma: no cover
    torch = None

MODES = tuple(E.DWT_MODES)


@functools.lru_cache(maxsize=None)
def daubechies(N):
    """The scaling filter g (= rec_lo) of the Daubechies wavelet with N vanishing moments, 2N taps, minimum phase, sum g = sqrt 2:
    the roots inside the unit circle of P(y) = sum_{k<N} C(N - 1 + k, k) y^k at y = (2 - z - 1 / z) / 4, times (1 + z)^N."""
    N = int(N)
    if N < 1 or N > 32:
        raise DwtRefused("daubechies: N = %d vanishing moments are outside 1 .. 32" % N)
    zs = []
    if N > 1:
        P = [math.comb(N - 1 + k, k) for k in range(N)]
        for y in np.roots(P[::-1]):
            b = 1.0 - 2.0 * y                               # z + 1 / z = 2 - 4 y
            r = np.sqrt(b * b - 1.0 + 0j)
            z = b + r
            zs.append(b - r if abs(z) > 1.0 else z)
    g = np.real(np.poly(np.concatenate((-np.ones(N), np.asarray(zs, dtype=complex)))))
    g = g * (math.sqrt(2.0) / g.sum())
    g.setflags(write=False)
    return g


def orthogonal_bank(g):
    """(dec_lo, dec_hi, rec_lo, rec_hi) of the orthogonal bank with the scaling filter g = rec_lo: dec_lo[m] = g[L - 1 - m],
    rec_hi[k] = (-1)^k g[L - 1 - k], dec_hi[m] = rec_hi[L - 1 - m]"""
    g = np.asarray(g, dtype=np.float64)
    rec_hi = g[::-1] * (-1.0) ** np.arange(g.size)
    return g[::-1].copy(), rec_hi[::-1].copy(), g.copy(), rec_hi


def wavelet_filters(w):
    """-> (dec_lo, dec_hi, rec_lo, rec_hi) as float64 arrays of one even length: from 'haar', 'db1' .. 'db10', a 4-tuple of filters, or
    any object with a `filter_bank` attribute (a pywt.Wavelet)."""
    if isinstance(w, str):
        name = "db1" if w == "haar" else w
        if not (name.startswith("db") and name[2:].isdigit() and 1 <= int(name[2:]) <= 10):
            raise DwtRefused("wavelet_filters: %r is not built in ('haar', 'db1' .. 'db10'): pass the filter bank as a 4-tuple" % (w,))
        return orthogonal_bank(daubechies(int(name[2:])))
    bank = getattr(w, "filter_bank", w)
    try:
        bank = tuple(np.asarray(f, dtype=np.float64) for f in bank)
    except (TypeError, ValueError):
        raise DwtRefused("wavelet_filters: a wavelet is a name, a 4-tuple of filters or an object with a filter_bank") from None
    if len(bank) != 4 or any(f.ndim != 1 or f.size != bank[0].size for f in bank):
        raise DwtRefused("wavelet_filters: a filter bank is four one-dimensional filters of one length")
    E._dwt_filters("wavelet_filters", bank[0], bank[1])
    E._dwt_filters("wavelet_filters", bank[2], bank[3])
    return bank


def dwt_max_level(n, L):
    """pywt.dwt_max_level: floor(log2(n / (L - 1))), 0 where the row is shorter than the filter's support"""
    n, L = int(n), int(L)
    if L < 2 or n < 1:
        raise DwtRefused("dwt_max_level: n and the filter length must be at least 1 and 2")
    lev = 0
    while (L - 1) << (lev + 1) <= n:
        lev += 1
    return lev


def dwt_coeff_len(n, L, mode="symmetric"):
    """pywt.dwt_coeff_len: the coefficients of one level of n samples"""
    E._dwt_code("dwt_coeff_len", E.DWT_MODES, "mode", mode)
    return _coeff_len(int(n), int(L), mode)


def _is_dev(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _to_last(x, axis):
    if not _is_dev(x):
        x = np.asarray(x)
    if x.ndim < 1:
        raise DwtRefused("the array needs at least one axis")
    if not -x.ndim <= axis < x.ndim:
        raise DwtRefused("axis = %d is outside the %d axes of the array" % (axis, x.ndim))
    axis %= x.ndim
    return (x if axis == x.ndim - 1 else (x.movedim(axis, -1) if _is_dev(x) else np.moveaxis(x, axis, -1))), axis


def _from_last(y, axis, ndim):
    if axis == ndim - 1:
        return y
    return y.movedim(-1, axis) if _is_dev(y) else np.moveaxis(y, -1, axis)


def _cat(parts):
    return torch.cat(parts, dim=-1) if _is_dev(parts[0]) else np.concatenate(parts, axis=-1)


def dwt(x, wavelet, mode="symmetric", axis=-1, form="auto"):
    """pywt.dwt: one level -> (cA, cD) along `axis`"""
    dl, dh, _, _ = wavelet_filters(wavelet)
    xl, axis = _to_last(x, axis)
    cA, cD = E.dwt_level(xl, dl, dh, mode, form)
    return _from_last(cA, axis, xl.ndim), _from_last(cD, axis, xl.ndim)


def idwt(cA, cD, wavelet, mode="symmetric", axis=-1, n=None, form="auto"):
    """pywt.idwt: one level back, 2K - L + 2 samples (2K for 'periodization') or the n given, which may be one less"""
    _, _, rl, rh = wavelet_filters(wavelet)
    al, axis = _to_last(cA, axis)
    dl, _ = _to_last(cD, axis)
    K = int(al.shape[-1])
    full = 2 * K if E.DWT_MODES.get(mode, mode) == 5 else 2 * K - rl.size + 2
    n = full if n is None else int(n)
    if n not in (full, full - 1) or n < 1:
        raise DwtRefused("idwt: %d coefficients give %d samples, or one less: not %d" % (K, full, n))
    return _from_last(E.idwt_level(al, dl, n, rl, rh, mode, form), axis, al.ndim)


def wavedec(x, wavelet, mode="symmetric", level=None, axis=-1, form="auto"):
    """pywt.wavedec: the list [cA_J, cD_J, .., cD_1] along `axis`; level=None: dwt_max_level (at least 1).  The list's arrays are views of
    one pyramid, which one launch writes where the row form fits."""
    dl, dh, _, _ = wavelet_filters(wavelet)
    xl, axis = _to_last(x, axis)
    n = int(xl.shape[-1])
    level = max(1, dwt_max_level(max(n, 1), dl.size)) if level is None else int(level)
    out = E.dwt(xl, dl, dh, mode, level, form)
    entries = E.dwt_layout(n, dl.size, E.DWT_MODES[mode] if isinstance(mode, str) else mode, level)[1]
    return [_from_last(out[..., o:o + ln], axis, xl.ndim) for ln, o in entries]


def waverec(coeffs, wavelet, mode="symmetric", axis=-1, n=None, form="auto"):
    """pywt.waverec: the rows back from [cA_J, cD_J, .., cD_1].  n=None gives the 2 K_1 - L + 2 samples pywt returns (one more than an odd
    row had); n = that or one less."""
    _, _, rl, rh = wavelet_filters(wavelet)
    coeffs = list(coeffs)
    if len(coeffs) < 2:
        raise DwtRefused("waverec: the list must hold cA_J and at least one detail")
    parts = [_to_last(c, axis)[0] for c in coeffs]
    axis = _to_last(coeffs[0], axis)[1]
    code = E._dwt_code("waverec", E.DWT_MODES, "mode", mode)
    K1, L, level = int(parts[-1].shape[-1]), rl.size, len(parts) - 1
    full = 2 * K1 if code == 5 else 2 * K1 - L + 2
    n = full if n is None else int(n)
    if n not in (full, full - 1) or n < 1:
        raise DwtRefused("waverec: %d finest details give %d samples, or one less: not %d" % (K1, full, n))
    E.dwt_check("waverec", 1, n, L, code, level, 1)
    entries = E.dwt_layout(n, L, code, level)[1]
    if [int(p.shape[-1]) for p in parts] != [ln for ln, _ in entries]:
        raise DwtRefused("waverec: the lengths %s are not those of a pyramid of %d samples, %s" % ([int(p.shape[-1]) for p in parts], n, [ln for ln, _ in entries]))
    return _from_last(E.idwt(_cat(parts), n, rl, rh, mode, level, form), axis, parts[0].ndim)


def modwt(x, wavelet, level=None, axis=-1, form="auto"):
    """MATLAB's modwt: W[level + 1, ..., n] = W_1 .. W_J, V_J of the rows along `axis` (moved last), circular; level=None:
    floor(log2 n), at least 1."""
    _, _, rl, rh = wavelet_filters(wavelet)
    xl, _ = _to_last(x, axis)
    level = max(1, int(xl.shape[-1]).bit_length() - 1) if level is None else int(level)
    return E.modwt(xl, rl, rh, level, form)


def imodwt(W, wavelet, form="auto"):
    """MATLAB's imodwt: the rows x[..., n] from W[level + 1, ..., n]"""
    _, _, rl, rh = wavelet_filters(wavelet)
    return E.imodwt(W, rl, rh, form)


def modwt_mra(W, wavelet, form="auto"):
    """MATLAB's modwtmra: the details D_1 .. D_J and the smooth S_J, [level + 1, ..., n], which add up to x: level + 1 inverse calls, each
    with every other plane zeroed."""
    _, _, rl, rh = wavelet_filters(wavelet)
    dev = _is_dev(W)
    if not dev:
        W = np.asarray(W)
    if W.ndim < 2 or W.shape[0] < 2:
        raise DwtRefused("modwt_mra: W must be [level + 1, ..., n] with at least one level")
    out = []
    for e in range(int(W.shape[0])):
        Z = torch.zeros_like(W) if dev else np.zeros_like(W)
        Z[e] = W[e]
        out.append(E.imodwt(Z, rl, rh, form))
    return torch.stack(out) if dev else np.stack(out)


def modwt_variance(x, wavelet, level=None, unbiased=True, axis=-1, form="auto"):
    """The wavelet variance of Percival & Walden: nu2[j - 1, ...] = (1 / M_j) sum_{t >= L_j - 1} |W_j[t]|^2 with L_j = (2^j - 1)(L - 1) + 1
    and M_j = n - L_j + 1 the coefficients the circular wrap does not touch (unbiased=False: all n of them, M_j = n) -> (nu2, edof),
    edof[j - 1] = max(M_j / 2^j, 1) the equivalent degrees of freedom of its chi-square law.  The W_j come from `modwt` on the GPU; the
    sums of squares are a float64 torch reduction of the device result (numpy rows: a float64 numpy sum of the returned array)."""
    _, _, rl, rh = wavelet_filters(wavelet)
    xl, _ = _to_last(x, axis)
    n, L = int(xl.shape[-1]), rl.size
    level = max(1, n.bit_length() - 1) if level is None else int(level)
    Lj = [((1 << j) - 1) * (L - 1) + 1 for j in range(1, level + 1)]
    if level < 1 or (unbiased and Lj[-1] > n):
        raise DwtRefused("modwt_variance: at level %d the filter spans %d samples, the row has %d: no coefficient is free of the wrap" % (level, Lj[-1] if Lj else 0, n))
    W = E.modwt(xl, rl, rh, level, form)
    nu2, edof = [], []
    for j in range(1, level + 1):
        t0 = Lj[j - 1] - 1 if unbiased else 0
        M = n - t0
        w = W[j - 1][..., t0:]
        if _is_dev(W):
            p = w.real.double() ** 2 + w.imag.double() ** 2 if w.is_complex() else w.double() ** 2
            nu2.append(p.sum(dim=-1) / M)
        else:
            nu2.append(np.sum(np.abs(w.astype(np.complex128 if np.iscomplexobj(w) else np.float64)) ** 2, axis=-1) / M)
        edof.append(max(M / float(1 << j), 1.0))
    return (torch.stack(nu2) if _is_dev(W) else np.stack(nu2)), np.asarray(edof)


def _gray(level):
    f = np.arange(1 << level)
    return f ^ (f >> 1)


def wpdec(x, wavelet, level, order="natural", form="auto"):
    """The wavelet packet table of depth `level`, mode 'periodization': [..., 2^level, n / 2^level]; n must be a multiple of 2^level.  Node p of
    level j has the children 2p (low) and 2p + 1 (high): order='natural' (Paley).  order='freq' permutes the node axis by the Gray code,
    out[f] = natural[f ^ (f >> 1)], so that the bands ascend in frequency.  One `dwt_level` call per level transforms all its nodes."""
    dl, dh, _, _ = wavelet_filters(wavelet)
    level = int(level)
    if order not in ("natural", "freq"):
        raise DwtRefused("wpdec: order must be 'natural' or 'freq', not %r" % (order,))
    xl, _ = _to_last(x, -1)
    n = int(xl.shape[-1])
    if level < 1 or level > 30 or n % (1 << level):
        raise DwtRefused("wpdec: n = %d must be a multiple of 2^level, level = %d at least 1" % (n, level))
    lead = tuple(xl.shape[:-1])
    c = xl.reshape(lead + (1, n))
    for j in range(level):
        m = n >> (j + 1)
        c = E.dwt_level(c, dl, dh, "periodization", form, interleave=True).reshape(lead + (2 << j, m))
    if order == "freq":
        g = _gray(level)
        c = c[..., torch.as_tensor(g, device=c.device), :] if _is_dev(c) else c[..., g, :]
    return c


def wprec(c, wavelet, order="natural", form="auto"):
    """The inverse of `wpdec`: rows [..., n] from a packet table [..., 2^level, m]"""
    _, _, rl, rh = wavelet_filters(wavelet)
    if order not in ("natural", "freq"):
        raise DwtRefused("wprec: order must be 'natural' or 'freq', not %r" % (order,))
    if not _is_dev(c):
        c = np.asarray(c)
    if c.ndim < 2:
        raise DwtRefused("wprec: the table must be [..., 2^level, m]")
    nodes, m = int(c.shape[-2]), int(c.shape[-1])
    level = nodes.bit_length() - 1
    if level < 1 or nodes != 1 << level or m < 1:
        raise DwtRefused("wprec: %d nodes are not 2^level with level at least 1" % nodes)
    lead = tuple(c.shape[:-2])
    if order == "freq":
        inv = np.argsort(_gray(level))
        c = c[..., torch.as_tensor(inv, device=c.device), :] if _is_dev(c) else c[..., inv, :]
    for j in range(level, 0, -1):
        c = E.idwt_level(c.reshape(lead + (1 << (j - 1), 2, m)), None, 2 * m, rl, rh, "periodization", form)
        m *= 2
    return c.reshape(lead + (m,))


def dwt_plan(what, n, wavelet, mode="symmetric", level=1, rows=1, cplx=False, form="auto"):
    """`engine.dwt_plan` for a wavelet: the form a call takes, its tile, LDS bytes, workgroups, launches, passes, scratch bytes, and the
    (length, offset) of every entry of the output"""
    return E.dwt_plan(what, n, wavelet_filters(wavelet)[0].size, mode, level, rows, cplx, form)
