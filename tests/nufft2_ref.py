"""The type-2 NUFFT and the band-limited least-squares fit built on it restated in numpy, the cases of tests/test_gpu_nufft2.py and the
allowances they hold the device to.  A helper module, not a test: nothing here is collected.

The definition (include/spectral_nufft2.h): times t[N], modes F[r][M], e(p) = exp(2 pi i p), tau = t - t_ref,

    c_r[j] = sum_m F_r[m] e(sign (f0 + m df) tau_j),    j = 0 .. N - 1.

`direct2` is that sum in float64, the phase product reduced by p - rint(p) (`exact=True`: phases in rational arithmetic, t_ref = 0).
`nufft2_def` is the algorithm in float64 with numpy.fft, over the geometry of nufft_ref (the same p = frac(-sign df tau), first
cells, kernel, kernel's transform and nf as type 1): F[m] / phihat(k) at cell k mod nf, k = m - M // 2, zeros elsewhere, one forward
transform, per sample the 8 cells from its first cell on weighted with phi, times e(sign fc tau); no factor 1 / nf.  `nufft2_def32`
restates the device arithmetic: a float32 offset and kernel values, the grid rounded to complex64 after the float64 division, a
complex64 scipy.fft, the 8-term sum in float32 in the order l = 0 .. 7, a float32 phase.

The cases are the times, grids and t_ref of every entry of nufft_ref.SHAPES, both signs where the entry has both, with random complex64
modes from seed + 100; 'rows-17' keeps its row of zeros and its two rows at 10^3.

The allowance.  METHOD2_DEV and F32_2_DEV are the largest deviations of nufft2_def and nufft2_def32 from direct2 over the cases, every
cell relative to its row's sum of |F[m]|, as measured by tests/test_host_nufft2.py (which prints them and asserts them against these
constants).  The device gets nufft_ref.MARGIN = 4 x the float32 figure for another order of summation inside the transform, fused
multiply-adds in the 8-term sum and the hardware's exponential; it must stay below nufft_ref.PARITY = 2e-4.

The fit.  `fit_def` solves the regularised normal equations (A^H W A + ridge sum(w) I) F = A^H W y in float64 with
numpy.linalg.solve, A[j, m] = e((f0 + m df) tau_j).  `fit_def32` is the conjugate-gradient iteration of pyfft_amd.nufft.nufft_fit in
numpy with complex64 transforms: the right-hand side and the Toeplitz column from nufft_ref.nufft_def32, the product with the
circulant of next_pow2(2 M) points through complex64 scipy.fft, dot products in float64.  FIT_F32_DEV is the largest
||fit_def32 - fit_def|| / ||fit_def|| over the two FIT_CASES; the device gets the same 4 x.  DEVICE_SHARE2 / FIT_DEVICE_SHARE: the largest
shares of those allowances tests/test_gpu_nufft2.py used on an MI355X."""
import functools

import numpy as np
import scipy.fft

import lomb_ref as L
import nufft_ref as R

W = R.W
METHOD2_DEV = 4.0e-8        # measured 3.830e-8 (test_measured_deviations: 'm1')
F32_2_DEV = 8.5e-7          # measured 8.284e-7 ('m1'; 6.1e-7 at 'rows-17', under 2.4e-7 elsewhere)
FIT_F32_DEV = 5.6e-6        # measured 5.511e-6 ('gapped', cond 4.3e2; 'clean', cond 1.3: 9.0e-7, which is the stopping rule's)
ALLOWANCE2 = R.MARGIN * F32_2_DEV
FIT_ALLOWANCE = R.MARGIN * FIT_F32_DEV
DEVICE_SHARE2 = 0.221       # measured on an MI355X: 'm1', sign +1; 0.16 at 'rows-17', 0.14 at 'm-odd', under 0.09 over the other cases
FIT_DEVICE_SHARE = 0.283    # 'gapped' (12 iterations, as the float64 iteration); 'clean' 0.04 (5 iterations), weights and a ridge 0.08


def direct2(t, F, f0, df, sign=1, t_ref=None, exact=False):
    """[R, N] complex128"""
    t = np.asarray(t, dtype=np.float64)
    F = np.atleast_2d(np.asarray(F)).astype(np.complex128)
    f = sign * (f0 + df * np.arange(F.shape[-1]))
    if exact:
        p = L.exact_turns(f, t)
    else:
        t_ref = float(t[0]) if t_ref is None else float(t_ref)
        p = (t - t_ref)[:, None] * f[None, :]
        p -= np.rint(p)
    return F @ L.e(p).T


def nufft2_def(t, F, f0, df, sign=1, t_ref=None):
    """the algorithm in float64: [R, N] complex128"""
    F = np.atleast_2d(np.asarray(F)).astype(np.complex128)
    M = F.shape[-1]
    nf, h, p, a, _, _ = R._geometry(t, f0, df, M, sign, t_ref)
    k = np.arange(M) - h
    grid = np.zeros((F.shape[0], nf), dtype=np.complex128)
    grid[:, k % nf] = F / R.phihat(nf, k)[None, :]
    G = np.fft.fft(grid, axis=-1)
    lo = p * nf - 0.5 * W
    i0 = np.ceil(lo)
    out = np.zeros((F.shape[0], p.size), dtype=np.complex128)
    for l in range(W):
        z = (i0 + l - p * nf) / (0.5 * W)
        kv = np.exp(R.BETA * (np.sqrt(np.maximum(1 - z * z, 0)) - 1))
        out += kv[None, :] * G[:, (i0.astype(np.int64) + l) % nf]
    return out * L.e(a)[None, :]


def nufft2_def32(t, F64, f0, df, sign=1, t_ref=None):
    """the device arithmetic restated: [R, N] complex64"""
    F64 = np.atleast_2d(np.asarray(F64, dtype=np.complex64))
    M = F64.shape[-1]
    nf, h, p, a, i0, dx = R._geometry(t, f0, df, M, sign, t_ref)
    pc, ps = np.cos(2 * np.pi * a).astype(np.float32), np.sin(2 * np.pi * a).astype(np.float32)
    k = np.arange(M) - h
    grid = np.zeros((F64.shape[0], nf), dtype=np.complex64)
    grid[:, k % nf] = (F64.astype(np.complex128) / R.phihat(nf, k)[None, :]).astype(np.complex64)
    G = scipy.fft.fft(grid, axis=-1)
    assert G.dtype == np.complex64
    sr = np.zeros((F64.shape[0], p.size), dtype=np.float32)
    si = np.zeros_like(sr)
    for l in range(W):
        z = (dx + np.float32(l - W // 2)) * np.float32(2.0 / W)
        u = (np.float32(1) - z) * (np.float32(1) + z)
        kv = np.exp(np.float32(R.BETA) * (np.sqrt(np.maximum(u, np.float32(0))) - np.float32(1))).astype(np.float32)
        g = G[:, (i0 + l) % nf]
        sr = sr + kv[None, :] * g.real
        si = si + kv[None, :] * g.imag
    assert sr.dtype == np.float32 and si.dtype == np.float32
    out = np.empty(sr.shape, dtype=np.complex64)
    out.real = sr * pc[None, :] - si * ps[None, :]
    out.imag = sr * ps[None, :] + si * pc[None, :]
    return out


def deviation(got, ref, F):
    """the largest |got - ref| over the cells, each relative to its row's sum of |F[m]|; a row of zeros must be met exactly"""
    return R.deviation(got, ref, F)


def assert_within(got, ref, F, what=""):
    used = deviation(got, ref, F) / ALLOWANCE2
    print("%s: worst cell at %.3f of its allowance" % (what, used))
    assert used <= 1.0, (what, used)
    return used


# ---- the cases ------------------------------------------------------------------------------------------------------------------
SHAPES, CASES, grid_of = R.SHAPES, R.CASES, R.grid_of


@functools.lru_cache(maxsize=None)
def signals(name):
    """(t [N] float64, F [rows, M] complex64, t_ref): the times and origin of nufft_ref.signals(name)"""
    t, _, t_ref = R.signals(name)
    sh = SHAPES[name]
    rng = np.random.default_rng(sh["seed"] + 100)
    F = (rng.standard_normal((sh["rows"], sh["M"])) + 1j * rng.standard_normal((sh["rows"], sh["M"]))).astype(np.complex64)
    if name == "rows-17":
        F[3] += 1e3
        F[11] += 1e3j
        F[7] = 0
    F.setflags(write=False)
    return t, F, t_ref


@functools.lru_cache(maxsize=None)
def reference(name, sign):
    t, F, t_ref = signals(name)
    f0, df = grid_of(name)
    out = direct2(t, F, f0, df, sign, t_ref)
    out.setflags(write=False)
    return out


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
FIT_K, FIT_N, FIT_PERIOD, FIT_SEED, FIT_JITTER, FIT_GAP = 40, 400, 100.0, 7, 0.45, (50.0, 53.0)
FIT_CASES = ("clean", "gapped")
FIT_ITERATIONS = {"clean": (5, 8), "gapped": (12, 16)}       # what the float64 iteration takes with this draw, what the device may take


def fit_grid():
    """(f0, df, M) of the fit cases: the harmonics of the period up to K"""
    return -FIT_K / FIT_PERIOD, 1.0 / FIT_PERIOD, 2 * FIT_K + 1


def design(t, f0, df, M, t_ref=0.0):
    p = (np.asarray(t, dtype=np.float64) - t_ref)[:, None] * (f0 + df * np.arange(M))[None, :]
    return L.e(p - np.rint(p))


@functools.lru_cache(maxsize=None)
def fit_signals(name):
    """(t [N], y [N] complex64 = A F_true, F_true [M]), t_ref = 0"""
    rng = np.random.default_rng(FIT_SEED)
    f0, df, M = fit_grid()
    h = FIT_PERIOD / FIT_N
    t = (np.arange(FIT_N) + rng.uniform(-FIT_JITTER, FIT_JITTER, FIT_N)) * h
    F_true = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    if name == "gapped":
        t = t[~((t > FIT_GAP[0]) & (t < FIT_GAP[1]))]
    y = (design(t, f0, df, M) @ F_true).astype(np.complex64)
    for a in (t, y, F_true):
        a.setflags(write=False)
    return t, y, F_true


def fit_def(t, y, f0, df, M, w=None, ridge=0.0, t_ref=0.0):
    """the regularised normal equations solved in float64: [R, M] complex128"""
    y = np.atleast_2d(np.asarray(y)).astype(np.complex128)
    w = np.ones(len(t)) if w is None else np.asarray(w, dtype=np.float64)
    A = design(t, f0, df, M, t_ref)
    N = (A.conj().T * w[None, :]) @ A + ridge * w.sum() * np.eye(M)
    return np.linalg.solve(N, (A.conj().T * w[None, :]) @ y.T).T


def cg(normal, b, rtol, maxiter, dtype):
    """pyfft_amd.nufft._fit's iteration over the rows of b together -> (F, iterations, converged [R])"""
    dot = lambda u, v: np.sum(u.astype(np.complex128).conj() * v.astype(np.complex128), axis=-1).real
    F, r = np.zeros_like(b), b.copy()
    p = r.copy()
    rs = dot(r, r)
    stop = rtol ** 2 * rs
    active = rs > stop
    it = 0
    while it < maxiter and active.any():
        q = normal(p)
        pq = dot(p, q)
        alpha = np.where(active & (pq > 0), rs / np.where(pq > 0, pq, 1.0), 0.0)
        F = F + (alpha[:, None] * p).astype(dtype)
        r = r - (alpha[:, None] * q).astype(dtype)
        rs_new = dot(r, r)
        beta = np.where(active & (rs > 0), rs_new / np.where(rs > 0, rs, 1.0), 0.0)
        p = np.where(active[:, None], r + (beta[:, None] * p).astype(dtype), p)
        rs = np.where(active, rs_new, rs)
        active = active & (rs > stop)
        it += 1
    return F, it, ~active


def fit_cg(t, y, f0, df, M, w=None, ridge=0.0, rtol=1e-6, maxiter=100, t_ref=0.0, f32=True):
    """the conjugate-gradient fit with complex64 transforms (f32) or in float64 throughout -> (F [R, M], iterations, converged)"""
    y = np.atleast_2d(np.asarray(y))
    w = np.ones(len(t)) if w is None else np.asarray(w, dtype=np.float64)
    dtype = np.complex64 if f32 else np.complex128
    if f32:
        w32 = w.astype(np.complex64)
        b = R.nufft_def32(t, y.astype(np.complex64) * w32[None, :], f0, df, M, -1, t_ref).astype(np.complex64)
        col = R.nufft_def32(t, w32, -(M - 1) * df, df, 2 * M - 1, -1, t_ref)[0].astype(np.complex64)
    else:
        b = R.direct(t, y * w[None, :], f0, df, M, -1, t_ref)
        col = R.direct(t, w, -(M - 1) * df, df, 2 * M - 1, -1, t_ref)[0]
    Lc = 1
    while Lc < 2 * M:
        Lc *= 2
    circ = np.zeros(Lc, dtype=dtype)
    circ[:M] = col[M - 1:]
    if M > 1:
        circ[Lc - (M - 1):] = col[:M - 1]
    spec = scipy.fft.fft(circ)
    shift = ridge * w.sum()

    def normal(x):
        pad = np.zeros((x.shape[0], Lc), dtype=dtype)
        pad[:, :M] = x
        out = scipy.fft.ifft(scipy.fft.fft(pad, axis=-1) * spec[None, :], axis=-1)[:, :M] + dtype(shift) * x
        assert out.dtype == dtype
        return out

    return cg(normal, b, rtol, maxiter, dtype)


def fit_def32(t, y, f0, df, M, w=None, ridge=0.0, rtol=1e-6, maxiter=100, t_ref=0.0):
    return fit_cg(t, y, f0, df, M, w, ridge, rtol, maxiter, t_ref, True)[0]


def fit_deviation(got, ref):
    """the largest ||got_r - ref_r|| / ||ref_r|| over the rows; a row of zeros must be met exactly"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    worst = 0.0
    for g, r in zip(got, ref):
        n = np.linalg.norm(r)
        worst = max(worst, np.linalg.norm(g - r) / n if n > 0 else (0.0 if not g.any() else np.inf))
    return float(worst)
