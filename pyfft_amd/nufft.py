"""The non-uniform FFTs of type 1 and type 2 on the GPU, and what the pair makes possible for an unevenly sampled record.

Type 1, uneven samples to a uniform grid of frequencies, and type 2, its adjoint, a spectrum on a uniform grid to uneven times:

    F[m] = sum_j c_j exp(2 pi i sign (f0 + m df) (t_j - t_ref)),    m = 0 .. M - 1        nufft1
    c[j] = sum_m F_m exp(2 pi i sign (f0 + m df) (t_j - t_ref)),    j = 0 .. N - 1        nufft2

in O(N w + M log M) in place of the O(N M) of the sums themselves (Dutt & Rokhlin 1993; Greengard & Lee 2004; the "exponential of
semicircle" kernel of Barnett, Magland & af Klinteberg 2019 at width w = 8 and upsampling 2).  Type 1 spreads the samples onto a
fine grid, runs one long transform over it and divides every bin by the kernel's transform (engine.nufft1, sp_nufft1); type 2 divides
the modes, places them on the same grid, runs the same transform and lets every sample gather the 8 cells around it (engine.nufft2,
sp_nufft2).  Accuracy: about 1e-7 of a row's sum of |c_j|, under 1e-6 of its sum of |F_m| (float32 kernel values and a complex64
transform; the method's own error is under 4e-8).  Type 1 adds 64-bit integers, so its results are bitwise reproducible AND do not
depend on the order of the samples; an output of type 2 depends on its own sample alone, so a permutation of the samples permutes
them bit for bit.  Times are float64 and may come in any order, with duplicates.  The fast Lomb-Scargle periodogram
(lomb.ls_periodogram(method='fast')) is built on type 1.

    nufft1        any finite f0, any df != 0, rows of strengths over one axis of times
    nufft1_modes  positions in radians, integer modes -M//2 .. (M-1)//2: the convention of FINUFFT's nufft1d1
    nufft2        the same grid of frequencies, rows of modes over one axis of times
    nufft2_modes  the convention of FINUFFT's nufft1d2
    nufft_plan    how a shape is dealt to the device (type=1 or 2; nufft2_plan is type=2)
    nufft_fit     the band-limited least-squares fit of a record: the modes F that minimise
                  sum_j w_j |y_j - sum_m F[m] e((f0 + m df) tau_j)|^2 + ridge sum(w) |F|^2, by conjugate gradients on the normal
                  equations on the device.  Their matrix is Toeplitz: one nufft1 of the weights gives its column, and a product with
                  it is two engine.fft calls over a circulant of next_pow2(2 M) points.  No further kernel.
    regrid        that fit over the harmonics of one period up to fmax, evaluated at any new times through nufft2: an uneven record
                  put onto a uniform grid under a band limit, so that everything for uniformly sampled records applies to it.  The
                  period must close the circle of the samples exactly (span N / (N - 1) by default): at 1.1 x span the normal matrix
                  of 400 jittered samples and 81 modes has a condition number of 8e8, at the default 1.3.

What is not here: type 3; two and three dimensions; float64 strengths on the device; a tolerance argument (there is one kernel
width); rows with times of their own; a preconditioner for the fit (gaps cost iterations: a gap of 3 % of the record takes 12 where
the full record takes 5); non-periodic reconstruction (sinc or Voronoi-weighted); sharding over GPUs (spectra of the parts of a
record add).  A record piled into one tile of 1024 grid cells is correct and slow.  What is refused raises NufftRefused, which is a
ValueError and a NotImplementedError.
"""
import collections
import math

import numpy as np

from . import engine as _engine
from .engine import NufftRefused, _is_torch          # noqa: F401

try:
    import torch
except Exception:                       # pragma: no cover
    torch = None

TWO_PI = 2.0 * np.pi
FIT_MAX_M = 1 << 23                     # the Toeplitz column is one nufft1 at 2 M - 1 frequencies

NufftFit = collections.namedtuple("NufftFit", "F iterations converged residual")


def nufft1(t, c, f0, df, M, sign=1, t_ref=None):
    """F [..., M] (complex64) of the strengths c[..., N] at the times t[N]: frequencies f0 + m df in cycles per unit of t, phases
    taken from t_ref (default t[0]; 0.0 for the origin of t itself).  numpy in -> numpy out, device tensors in -> a device tensor."""
    return _engine.nufft1(t, c, f0, df, M, sign=sign, t_ref=t_ref)


def nufft1_modes(x, c, M, sign=1):
    """F[..., i] = sum_j c[..., j] exp(i sign k x_j) over the modes k = -(M // 2) + i, i = 0 .. M - 1 (that is -M//2 .. (M-1)//2 in
    FINUFFT's words), for positions x[N] in radians (any real values: the transform is periodic in 2 pi)."""
    t = x / TWO_PI if _is_torch(x) else np.asarray(x, dtype=np.float64) / TWO_PI
    return _engine.nufft1(t, c, -float(int(M) // 2), 1.0, M, sign=sign, t_ref=0.0)


def nufft2(t, F, f0, df, sign=1, t_ref=None):
    """c [..., N] (complex64) of the modes F[..., M] at the times t[N]: frequencies f0 + m df in cycles per unit of t, phases taken
    from t_ref (default t[0]; 0.0 for the origin of t itself).  numpy in -> numpy out, device tensors in -> a device tensor."""
    return _engine.nufft2(t, F, f0, df, sign=sign, t_ref=t_ref)


def nufft2_modes(x, F, sign=1):
    """c[..., j] = sum_i F[..., i] exp(i sign k x_j) over the modes k = -(M // 2) + i, i = 0 .. M - 1 (FINUFFT's nufft1d2), for
    positions x[N] in radians; M is the last axis of F."""
    t = x / TWO_PI if _is_torch(x) else np.asarray(x, dtype=np.float64) / TWO_PI
    return _engine.nufft2(t, F, -float(int(F.shape[-1]) // 2), 1.0, sign=sign, t_ref=0.0)


def nufft_plan(N, M, rows=1, type=1):
    """How engine.nufft1 (type=1) or engine.nufft2 (type=2) deals N samples, M frequencies and `rows` rows to the device (host only):
    nf, width, tiles, tile, rows_per_pass, passes, workgroups, and fast_min_pairs (type 1) or row_group (type 2)."""
    if type not in (1, 2):
        raise NufftRefused("nufft_plan: type must be 1 or 2, not %r" % (type,))
    return _engine.nufft_plan(N, M, rows) if type == 1 else _engine.nufft2_plan(N, M, rows)


def nufft2_plan(N, M, rows=1):
    return _engine.nufft2_plan(N, M, rows)


def _device_record(who, t, y, weights):
    """t float64 [N], y complex64 [rows, N], w float64 [N] as device tensors (numpy input is moved once), and what y was"""
    if torch is None:
        raise NufftRefused("%s: needs torch for its device arithmetic" % who)
    was_dev = _is_torch(t)
    if _is_torch(y) != was_dev or (weights is not None and _is_torch(weights) != was_dev):
        raise TypeError("%s: t, y and weights must all be numpy arrays or all device tensors" % who)
    if not was_dev:
        t = np.ascontiguousarray(np.asarray(t), dtype=np.float64)
        y = np.asarray(y)
        if not (np.all(np.isfinite(t)) and np.all(np.isfinite(y))):
            raise NufftRefused("%s: t and y must be finite" % who)
        if weights is not None:
            weights = np.ascontiguousarray(np.asarray(weights), dtype=np.float64)
    ndim, shape = (t.dim(), tuple(t.shape)) if was_dev else (t.ndim, t.shape)
    if ndim != 1 or len(y.shape) < 1 or int(y.shape[-1]) != int(shape[0]) or shape[0] < 1:
        raise NufftRefused("%s: t needs exactly one axis with a sample at least, and the last axis of y its samples" % who)
    if weights is not None and tuple(weights.shape) != tuple(shape):
        raise NufftRefused("%s: weights must have the shape of t" % who)
    if not was_dev:
        if weights is not None and not (np.all(np.isfinite(weights)) and np.all(weights >= 0) and np.sum(weights) > 0):
            raise NufftRefused("%s: weights must be finite, not negative, and not all zero" % who)
        t, y = torch.as_tensor(t, device="cuda"), torch.as_tensor(np.ascontiguousarray(y), device="cuda")
        weights = None if weights is None else torch.as_tensor(weights, device="cuda")
    is_complex = y.is_complex()
    lead = tuple(int(d) for d in y.shape[:-1])
    N = int(shape[0])
    td = t.to(torch.float64).contiguous()
    yd = y.to(torch.complex64).reshape(-1, N).contiguous()
    wd = torch.ones(N, dtype=torch.float64, device=td.device) if weights is None else weights.to(torch.float64).contiguous()
    return was_dev, is_complex, lead, td, yd, wd


def _dot(a, b):
    """sum conj(a) b over the last axis, accumulated in float64: complex128 [rows]"""
    return (a.to(torch.complex128).conj() * b.to(torch.complex128)).sum(dim=-1)


def _fit(who, td, yd, wd, f0, df, M, ridge, rtol, maxiter, t_ref):
    """conjugate gradients on (A^H W A + ridge sum(w) I) F = A^H W y for the rows of yd together -> (F [rows, M], iterations,
    converged [rows] bool tensor, residual [rows] float64 tensor)"""
    rows, N = int(yd.shape[0]), int(yd.shape[1])
    wsum = wd.sum()
    if not bool(torch.isfinite(wsum)) or not bool(wsum > 0) or bool((wd < 0).any()):
        raise NufftRefused("%s: weights must be finite, not negative, and not all zero" % who)
    w32 = wd.to(torch.complex64)
    b = _engine.nufft1(td, yd * w32[None, :], f0, df, M, sign=-1, t_ref=t_ref)                    # A^H W y
    # T[d] = sum_j w_j e(-d df tau_j), d = -(M - 1) .. M - 1: the normal matrix is T[m - n]
    col = _engine.nufft1(td, w32, -(M - 1) * df, df, 2 * M - 1, sign=-1, t_ref=t_ref)
    L = 1
    while L < 2 * M:
        L *= 2
    circ = torch.zeros(L, dtype=torch.complex64, device=td.device)
    circ[:M] = col[M - 1:]                                                                        # d = 0 .. M - 1
    if M > 1:
        circ[L - (M - 1):] = col[:M - 1]                                                          # d = -(M - 1) .. -1
    spec = _engine.fft(circ)
    shift = float(ridge) * float(wsum)
    pad = torch.zeros((rows, L), dtype=torch.complex64, device=td.device)

    def normal(x):
        pad[:, :M] = x
        return _engine.ifft(_engine.fft(pad) * spec[None, :])[:, :M] + shift * x

    F = torch.zeros_like(b)
    r = b.clone()
    p = r.clone()
    rs = _dot(r, r).real
    stop = (float(rtol) ** 2) * rs
    active = rs > stop
    iterations = 0
    while iterations < int(maxiter) and bool(active.any()):
        q = normal(p)
        pq = _dot(p, q).real
        alpha = torch.where(active & (pq > 0), rs / torch.where(pq > 0, pq, torch.ones_like(pq)), torch.zeros_like(rs))
        F = F + (alpha[:, None] * p).to(torch.complex64)
        r = r - (alpha[:, None] * q).to(torch.complex64)
        rs_new = _dot(r, r).real
        beta = torch.where(active & (rs > 0), rs_new / torch.where(rs > 0, rs, torch.ones_like(rs)), torch.zeros_like(rs))
        p = torch.where(active[:, None], r + (beta[:, None] * p).to(torch.complex64), p)
        rs = torch.where(active, rs_new, rs)
        active = active & (rs > stop)
        iterations += 1
    back = _engine.nufft2(td, F.contiguous(), f0, df, sign=1, t_ref=t_ref)
    d = yd.to(torch.complex128) - back.to(torch.complex128)
    residual = torch.sqrt((wd[None, :] * (d.real ** 2 + d.imag ** 2)).sum(dim=-1) / wsum)
    return F, iterations, ~active, residual


def nufft_fit(t, y, f0, df, M, weights=None, ridge=0.0, rtol=1e-6, maxiter=100, t_ref=None):
    """The band-limited least-squares fit of the record y[..., N] at the times t[N]: NufftFit(F [..., M] complex64, iterations,
    converged, residual) with F the minimiser of sum_j w_j |y_j - sum_m F[m] e((f0 + m df)(t_j - t_ref))|^2 + ridge sum(w) |F|^2.
    Conjugate gradients on the normal equations, on the device; rows of y share t and iterate together, each until its residual
    of the normal equations is below rtol times its right-hand side (a row of zeros gives zeros at once).  converged: whether every
    row got there within maxiter iterations (nothing is raised where not).  residual [...]: the weighted rms of y - nufft2(F), formed
    from the fit itself.  numpy input is moved to the device once and F comes back as numpy."""
    who = "nufft_fit"
    f0, df, M = float(f0), float(df), int(M)
    if M < 1 or M > FIT_MAX_M:
        raise NufftRefused("%s: M = %d modes are outside 1 .. 2^23 (the Toeplitz column takes 2 M - 1 frequencies)" % (who, M))
    if not (math.isfinite(ridge) and ridge >= 0 and math.isfinite(rtol) and rtol > 0 and int(maxiter) >= 0):
        raise NufftRefused("%s: ridge must be finite and not negative, rtol positive, maxiter not negative" % who)
    _engine.nufft_check(who, 1, M, 0, None, 0.0 if t_ref is None else float(t_ref), f0, df, 1)
    was_dev, _, lead, td, yd, wd = _device_record(who, t, y, weights)
    t_ref = float(td[0]) if t_ref is None else float(t_ref)
    F, iterations, conv, residual = _fit(who, td, yd, wd, f0, df, M, ridge, rtol, maxiter, t_ref)
    F, residual = F.reshape(lead + (M,)), residual.reshape(lead)
    if not was_dev:
        F, residual = F.cpu().numpy(), residual.cpu().numpy()
    return NufftFit(F, iterations, bool(conv.all()), residual)


def regrid_grid(t_min, t_max, N, fmax, period=None):
    """The harmonics `regrid` fits: (period, K, M, f0, df) with period = span N / (N - 1) by default (the samples close the circle
    exactly: one more sample at the mean spacing would be the first again), K = floor(fmax period), M = 2 K + 1 modes from
    f0 = -K / period on, df = 1 / period apart."""
    span = float(t_max) - float(t_min)
    if period is None:
        if N < 2 or not span > 0:
            raise NufftRefused("regrid: a default period needs two samples at different times at least")
        period = span * N / (N - 1)
    period = float(period)
    if not (math.isfinite(period) and period > 0 and math.isfinite(fmax) and fmax >= 0):
        raise NufftRefused("regrid: period must be positive and fmax not negative, both finite")
    K = int(math.floor(fmax * period))
    M = 2 * K + 1
    if M > N:
        raise NufftRefused("regrid: fmax = %g over a period of %g asks for M = %d modes from N = %d samples: more unknowns than samples"
                           % (fmax, period, M, N))
    return period, K, M, -K / period, 1.0 / period


def regrid(t, y, t_new, fmax, period=None, weights=None, ridge=0.0, rtol=1e-6, maxiter=100, return_fit=False):
    """The record y[..., N] at the uneven times t[N] evaluated at the times t_new, uniform or not, under the band limit fmax: the
    least-squares fit (nufft_fit) of the harmonics k / period, |k| <= floor(fmax period), evaluated through nufft2.  period defaults
    to span N / (N - 1).  A real y gives float32 values (the real part), a complex y complex64; [..., len(t_new)].  Refused: an fmax
    that asks for more modes than there are samples, and t_new outside [min t, max t] (the series is periodic and says nothing
    there).  return_fit: (values, NufftFit)."""
    who = "regrid"
    if _is_torch(t_new) != _is_torch(t):
        raise TypeError("%s: t_new must be of the kind of t" % who)
    if not _is_torch(t):                    # what can be refused is refused before anything moves to the device
        t = np.ascontiguousarray(np.asarray(t), dtype=np.float64)
        t_new = np.ascontiguousarray(np.asarray(t_new), dtype=np.float64)
    if len(t.shape) != 1 or int(t.shape[0]) < 1 or len(t_new.shape) != 1 or int(t_new.shape[0]) < 1:
        raise NufftRefused("%s: t and t_new need exactly one axis each, with a time at least" % who)
    t_min, t_max = float(t.min()), float(t.max())
    period, K, M, f0, df = regrid_grid(t_min, t_max, int(t.shape[0]), float(fmax), period)
    if not bool(((t_new >= t_min) & (t_new <= t_max)).all()):
        raise NufftRefused("%s: t_new must lie within [min t, max t] = [%g, %g]: the series is periodic and says nothing outside" % (who, t_min, t_max))
    if not (math.isfinite(ridge) and ridge >= 0 and math.isfinite(rtol) and rtol > 0 and int(maxiter) >= 0):
        raise NufftRefused("%s: ridge must be finite and not negative, rtol positive, maxiter not negative" % who)
    was_dev, is_complex, lead, td, yd, wd = _device_record(who, t, y, weights)
    tn = t_new.to(torch.float64).contiguous() if was_dev else torch.as_tensor(t_new, device="cuda")
    F, iterations, conv, residual = _fit(who, td, yd, wd, f0, df, M, ridge, rtol, maxiter, t_min)
    vals = _engine.nufft2(tn, F.contiguous(), f0, df, sign=1, t_ref=t_min).reshape(lead + (int(tn.numel()),))
    if not is_complex:
        vals = vals.real.contiguous()
    F, residual = F.reshape(lead + (M,)), residual.reshape(lead)
    if not was_dev:
        vals, F, residual = vals.cpu().numpy(), F.cpu().numpy(), residual.cpu().numpy()
    return (vals, NufftFit(F, iterations, bool(conv.all()), residual)) if return_fit else vals
