"""The type-1 NUFFT and the fast Lomb-Scargle sums restated in numpy, the cases of tests/test_gpu_nufft.py and the allowance they hold
the kernels to.  A helper module, not a test: nothing here is collected.

The definition (include/spectral_nufft.h): times t[N], strengths c[r][N], e(p) = exp(2 pi i p), tau = t - t_ref,

    F_r[m] = sum_j c_r[j] e(sign (f0 + m df) tau_j),    m = 0 .. M - 1.

`direct` is that sum in float64, the phase product reduced by p - rint(p) (`exact=True`: phases in rational arithmetic, t_ref = 0).
`nufft_def` is the algorithm of pyfft_amd/csrc/nufft_plan.h in float64 with numpy.fft: positions p = frac(-sign df tau) on a grid of
nf = next_pow2(2 M) cells (at least one tile), strengths times e(sign fc tau), fc = f0 + (M // 2) df, spread over W = 8 cells with
phi(z) = exp(beta (sqrt(1 - z^2) - 1)), beta = 2.30 W, one forward transform, bin k = m - M // 2 divided by the kernel's transform
(a 64-point Gauss-Legendre sum).  `nufft_def32` restates the device arithmetic: float32 kernel values from a float32 offset, complex64
strengths times a float32 phase, llrint(v 2^shift) summed as integers, the grid rounded to float32, a complex64 transform, a float64
pick.  The Lomb forms take w32 and wy32_r (lomb_ref.sums_def32's) as real strengths: A1 and B_r at (f0, df), A2 at (2 f0, 2 df).

The allowance.  METHOD_DEV and F32_DEV are the largest deviations of nufft_def and nufft_def32 from `direct` over CASES -- every cell
relative to its row's sum of |c_j| -- and LS_METHOD_DEV, LS_F32_DEV the same through lomb_ref.finish against lomb_ref.lomb_def with
lomb_ref.deviation, as measured by tests/test_host_nufft.py (which prints them and asserts them against these constants).  The device
gets 4 x the float32 figure, the project's margin, for another order of summation inside the transform and the hardware's exponent; it
must stay below the parity figure of 2e-4.  DEVICE_SHARE / LS_DEVICE_SHARE: the largest share of that allowance tests/test_gpu_nufft.py
used on an MI355X."""
import functools

import numpy as np
import scipy.fft

import lomb_ref as L

W, TILE, RG, QUAD = 8, 1024, 3, 32
BETA = 2.30 * W
METHOD_DEV = 4.0e-8         # measured 3.830e-8 (test_measured_deviations: 'n1', one sample; under 7e-9 where N is in the hundreds)
F32_DEV = 3.7e-7            # measured 3.606e-7 ('n1'; under 6e-8 where N is in the hundreds)
LS_METHOD_DEV = 1.5e-7      # measured 1.407e-7 ('ls-rows-17', equal weights, no floating mean, 'power'): the float64 algorithm on float32 strengths
LS_F32_DEV = 6.5e-7         # measured 6.354e-7 ('ls-rows-17', weights, no floating mean, 'power')
MARGIN = 4.0
PARITY = 2e-4
ALLOWANCE = MARGIN * F32_DEV
LS_ALLOWANCE = MARGIN * LS_F32_DEV
DEVICE_SHARE = 0.206        # measured on an MI355X: 'n1', one sample; 0.02 .. 0.08 over the other cases
LS_DEVICE_SHARE = 0.236     # 'ls-rows-17', equal weights, no floating mean, 'power'; 0.03 .. 0.12 over the other shapes
UNIFORM_TURNS = 1e-9        # method='fast': every |f[k] - (f[0] + k df)| span is at most so many turns
ROWS_HOOK = 2               # SP_NUFFT_ROWS of the rows-17 case


def nf_of(M):
    nf = TILE
    while nf < 2 * M:
        nf *= 2
    return nf


def plan_of(M, rows, grid_bytes=256 << 20, rows_force=0):
    """nufft_plan_of of pyfft_amd/csrc/nufft_plan.h: (nf, W, tiles, TILE, rows per pass, passes, workgroups)"""
    nf = nf_of(M)
    fit = max(1, grid_bytes // (8 * nf))
    if rows_force > 0:
        fit = min(fit, rows_force)
    rpp = 1 if rows < 1 else min(rows, fit)
    passes = 0 if rows < 1 else -(-rows // rpp)
    wgs = sum((nf // TILE) * -(-min(rpp, rows - r0) // RG) for r0 in range(0, rows, rpp))
    return nf, W, nf // TILE, TILE, rpp, passes, wgs


def _two_prod(a, b):
    """a b = p + lo exactly (Dekker), float64 arrays"""
    p = a * b
    s = 134217729.0
    ah = a * s
    ah = ah - (ah - a)
    al = a - ah
    bh = b * s
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def frac(q, tau):
    """frac(q tau) in [0, 1], as nufft_frac forms it"""
    p, lo = _two_prod(np.float64(q), np.asarray(tau, dtype=np.float64))
    r = (p - np.rint(p)) + lo
    return r - np.floor(r)


def cells(p, nf):
    """nufft_cell: the first cell of every footprint, wrapped, and the float32 offset in [0, 1]"""
    lo = p * float(nf) - 0.5 * W
    c = np.ceil(lo)
    i0 = c.astype(np.int64)
    return i0 % nf, (c - lo).astype(np.float32)


def quad(nf):
    x, w = np.polynomial.legendre.leggauss(2 * QUAD)
    x, w = x[QUAD:], w[QUAD:]
    return W * w * np.exp(BETA * (np.sqrt(1 - x * x) - 1)), np.pi * W * x / nf


def phihat(nf, k):
    amp, ang = quad(nf)
    return np.cos(np.asarray(k, dtype=np.float64)[:, None] * ang[None, :]) @ amp


def shift_of(cmax, N):
    """nufft_shift from a row's largest component magnitude"""
    e = int(np.frexp(np.float32(cmax))[1])
    return 60 - e - int(np.ceil(np.log2(N))) if N > 1 else 60 - e


def direct(t, c, f0, df, M, sign=1, t_ref=None, exact=False):
    t = np.asarray(t, dtype=np.float64)
    c = np.atleast_2d(np.asarray(c)).astype(np.complex128)
    f = sign * (f0 + df * np.arange(M))
    if exact:
        p = L.exact_turns(f, t)
    else:
        t_ref = float(t[0]) if t_ref is None else float(t_ref)
        p = (t - t_ref)[:, None] * f[None, :]
        p -= np.rint(p)
    return c @ L.e(p)


def _geometry(t, f0, df, M, sign, t_ref):
    t = np.asarray(t, dtype=np.float64)
    t_ref = float(t[0]) if t_ref is None else float(t_ref)
    tau, nf, h = t - t_ref, nf_of(M), M // 2
    p = frac(-sign * df, tau)
    a = frac(sign * (f0 + h * df), tau)
    i0, dx = cells(p, nf)
    return nf, h, p, a, i0, dx


def nufft_def(t, c, f0, df, M, sign=1, t_ref=None):
    """the algorithm in float64: [R, M] complex128"""
    c = np.atleast_2d(np.asarray(c)).astype(np.complex128)
    nf, h, p, a, _, _ = _geometry(t, f0, df, M, sign, t_ref)
    lo = p * nf - 0.5 * W
    i0 = np.ceil(lo)
    v = c * L.e(a)[None, :]
    grid = np.zeros((c.shape[0], nf), dtype=np.complex128)
    for l in range(W):
        z = (i0 + l - p * nf) / (0.5 * W)
        kv = np.exp(BETA * (np.sqrt(np.maximum(1 - z * z, 0)) - 1))
        for r in range(c.shape[0]):
            np.add.at(grid[r], (i0.astype(np.int64) + l) % nf, v[r] * kv)
    G = np.fft.fft(grid, axis=-1)
    k = np.arange(M) - h
    return G[:, k % nf] / phihat(nf, k)[None, :]


def spread32(t, c64, f0, df, M, sign=1, t_ref=None):
    """the device's integer grid sums: (sums [R, nf, 2] as Python-exact int64, shifts [R], nf, h)"""
    c64 = np.atleast_2d(np.asarray(c64, dtype=np.complex64))
    R, N = c64.shape
    nf, h, p, a, i0, dx = _geometry(t, f0, df, M, sign, t_ref)
    pc, ps = np.cos(2 * np.pi * a).astype(np.float32), np.sin(2 * np.pi * a).astype(np.float32)
    cr, ci = c64.real, c64.imag
    vr = (cr * pc[None, :] - ci * ps[None, :]).astype(np.float32)
    vi = (cr * ps[None, :] + ci * pc[None, :]).astype(np.float32)
    cmax = np.maximum(np.abs(cr), np.abs(ci)).max(axis=-1)
    shifts = np.array([shift_of(m, N) if m > 0 else 0 for m in cmax])
    sums = np.zeros((R, nf, 2), dtype=np.int64)
    for l in range(W):
        z = (dx + np.float32(l - W // 2)) * np.float32(2.0 / W)
        u = (np.float32(1) - z) * (np.float32(1) + z)
        kv = np.exp(np.float32(BETA) * (np.sqrt(np.maximum(u, np.float32(0))) - np.float32(1))).astype(np.float32)
        cell = (i0 + l) % nf
        for r in range(R):
            np.add.at(sums[r, :, 0], cell, np.rint(np.ldexp((vr[r] * kv).astype(np.float64), shifts[r])).astype(np.int64))
            np.add.at(sums[r, :, 1], cell, np.rint(np.ldexp((vi[r] * kv).astype(np.float64), shifts[r])).astype(np.int64))
    return sums, shifts, nf, h


def nufft_def32(t, c64, f0, df, M, sign=1, t_ref=None):
    """the device arithmetic restated: [R, M] complex128, before the last rounding to float32"""
    sums, shifts, nf, h = spread32(t, c64, f0, df, M, sign, t_ref)
    g = np.ldexp(sums.astype(np.float64), -shifts[:, None, None]).astype(np.float32)
    G = scipy.fft.fft((g[..., 0] + 1j * g[..., 1]).astype(np.complex64), axis=-1)
    assert G.dtype == np.complex64
    k = np.arange(M) - h
    return G[:, k % nf].astype(np.complex128) / phihat(nf, k)[None, :]


def _lomb_sums_from(transform, t, w32, wy32, f0, df, M, t_ref):
    rows = np.concatenate([w32[None, :], wy32], axis=0)
    A = transform(t, rows, f0, df, M, 1, t_ref)
    A2 = transform(t, w32[None, :], 2 * f0, 2 * df, M, 1, t_ref)[0]
    common = np.stack([A[0].real, A[0].imag, A2.real, A2.imag], axis=-1)
    return common, np.ascontiguousarray(np.stack([A[1:].real, A[1:].imag], axis=-1))


def lomb_strengths(t, y32, w=None, mean=None, wnorm=None):
    """k_lomb_prep's float32 strengths and float64 totals: (w32, wy32 [R, N], totals, mean)"""
    t = np.asarray(t, dtype=np.float64)
    y32 = np.atleast_2d(np.asarray(y32, dtype=np.float32))
    w = np.ones(t.size) if w is None else np.asarray(w, dtype=np.float64)
    m = y32.astype(np.float64).mean(axis=-1) if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
    inv = 1.0 / (w.sum() if wnorm is None else wnorm)
    d = y32.astype(np.float64) - m[:, None]
    w32 = (w * inv).astype(np.float32)
    wy32 = ((w * inv)[None, :] * d).astype(np.float32)
    totals = np.empty(1 + 2 * y32.shape[0])
    totals[0] = w32.astype(np.float64).sum()
    totals[1::2], totals[2::2] = wy32.astype(np.float64).sum(axis=-1), (wy32.astype(np.float64) * d).sum(axis=-1)
    return w32, wy32, totals, m


def lomb_sums_grid_def(t, y32, f0, df, M, w=None, t_ref=None, mean=None, wnorm=None, f32=False):
    """the fast sums in the layout of lomb_ref.sums_def: the float64 algorithm on the float32 strengths, or (f32) the device arithmetic"""
    w32, wy32, totals, m = lomb_strengths(t, y32, w, mean, wnorm)
    common, rows = _lomb_sums_from(nufft_def32 if f32 else nufft_def, t, w32, wy32, f0, df, M, t_ref)
    return common, rows, totals, m


def deviation(got, ref, c):
    """the largest |got - ref| over the cells, each relative to its row's sum of |c_j|; a row of zeros must be met exactly"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.sum(np.abs(np.atleast_2d(c)), axis=-1, keepdims=True)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    assert not np.any(np.isnan(rel)), "a cell that is not a number"
    return float(np.max(rel))


def assert_within(got, ref, c, what=""):
    used = deviation(got, ref, c) / ALLOWANCE
    print("%s: worst cell at %.3f of its allowance" % (what, used))
    assert used <= 1.0, (what, used)
    return used


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# nufft1 cases: N, M, rows, (f0, df), signs
SHAPES = {
    "tails": dict(N=777, M=257, rows=3, seed=21, signs=(1, -1)),            # not a multiple of anything; both signs
    "tiles": dict(N=1000, M=3000, rows=1, seed=22, signs=(1,)),             # nf 8192: eight tiles, the largest one-workgroup transform
    "long": dict(N=1000, M=5000, rows=1, seed=23, signs=(1,)),              # nf 16384: the multi-pass transform
    "seams": dict(N=64, M=600, rows=2, seed=24, signs=(1,)),                # nf 2048: p = 0, just under 1, on and beside the tile seam
    "pile": dict(N=500, M=300, rows=1, seed=25, signs=(1,)),                # all times equal: one cell takes sum |c|
    "pile-tile": dict(N=500, M=3000, rows=2, seed=26, signs=(1,)),          # all within one tile of eight
    "unsorted": dict(N=400, M=100, rows=1, seed=27, signs=(-1,)),           # a 0.1 grid on both sides of zero, duplicates certain
    "rows-17": dict(N=500, M=130, rows=17, seed=28, signs=(1,)),            # SP_NUFFT_ROWS = 2: nine passes; a row of zeros, rows at 10^3
    "m1": dict(N=300, M=1, rows=1, seed=29, signs=(1, -1)),
    "m-odd": dict(N=300, M=7, rows=2, seed=30, signs=(1,)),
    "n1": dict(N=1, M=33, rows=2, seed=31, signs=(1,)),
    "f0-neg": dict(N=300, M=40, rows=1, seed=32, signs=(1,), grid=(-1.3, 0.07)),
    "f0-zero": dict(N=300, M=40, rows=1, seed=33, signs=(1,), grid=(0.0, 0.05)),
    "df-neg": dict(N=300, M=40, rows=1, seed=34, signs=(1,), grid=(2.0, -0.03)),
}
CASES = [(name, s) for name, sh in SHAPES.items() for s in sh["signs"]]


def grid_of(name):
    """(f0, df): from 1 / span = 0.01 up to 4 where the case does not say otherwise"""
    sh = SHAPES[name]
    if "grid" in sh:
        return sh["grid"]
    return 0.01, (3.99 / (sh["M"] - 1) if sh["M"] > 1 else 1.0)


@functools.lru_cache(maxsize=None)
def signals(name):
    """(t [N] float64, c [rows, N] complex64, t_ref)"""
    sh = SHAPES[name]
    N, M, rows = sh["N"], sh["M"], sh["rows"]
    rng = np.random.default_rng(sh["seed"])
    t = np.sort(rng.uniform(0.0, 100.0, N))
    t_ref = float(t[0])
    f0, df = grid_of(name)
    nf = nf_of(M)
    if name == "seams":
        # positions p = frac(-df tau) chosen, then tau = -p / df (a negative lag is as good as any): 0, just under 1 (tau tiny and
        # positive), and footprint edges nf p - 4 exactly on, one ulp under and one ulp over the cell that starts tile 1, for the
        # footprint's first and last cell
        edge = []
        for cell in (TILE, TILE - W + 1, TILE - W, TILE + 1):
            x = (cell + 0.5 * W) / nf
            edge += [x, np.nextafter(x, 0.0), np.nextafter(x, 1.0)]
        p = np.concatenate([[0.0, 0.0, 1e-12, 1 - 1e-12, 0.5], edge, rng.uniform(0.0, 1.0, N - 5 - len(edge))])
        t = -p / df
        t_ref = 0.0
    if name == "pile":
        t = np.full(N, 37.25)
        t_ref = 30.0
    if name == "pile-tile":
        p = (3.2 + 0.05 * rng.uniform(0.0, 1.0, N)) * TILE / nf        # positions within a twentieth of a tile, well inside tile 3
        t = 30.0 - p / df
        t_ref = 30.0
    if name == "unsorted":
        t = np.round(rng.uniform(-50.0, 50.0, N), 1)
        assert np.unique(t).size < N and t.min() < 0 < t.max() and np.any(np.diff(t) < 0)
        t_ref = float(t[0])
    c = (rng.standard_normal((rows, N)) + 1j * rng.standard_normal((rows, N))).astype(np.complex64)
    if name == "rows-17":
        c[3] += 1e3
        c[11] += 1e3j
        c[7] = 0
    for a in (t, c):
        a.setflags(write=False)
    return t, c, t_ref


@functools.lru_cache(maxsize=None)
def reference(name, sign):
    t, c, t_ref = signals(name)
    f0, df = grid_of(name)
    out = direct(t, c, f0, df, SHAPES[name]["M"], sign, t_ref)
    out.setflags(write=False)
    return out


# the periodogram cases: records of lomb_ref (a line at 1.7 over a floor), frequencies on a uniform grid from 1 / span = 0.01 on
LS_SHAPES = {
    "ls-tails": dict(of="tails", M=257),
    "ls-tiles": dict(of="n1000-m300", M=3000),
    "ls-unsorted": dict(of="unsorted", M=100),
    "ls-rows-17": dict(of="rows-17", M=130),
}
# the normalisations of a shape: a row of zeros has no 'normalize' form (0 / 0 in scipy too)
LS_FORMS_OF = {name: L.NORMALIZE if name != "ls-rows-17" else ("power", "amplitude") for name in LS_SHAPES}
LS_CASES = [(name, (wt, fm, nz)) for name in LS_SHAPES for wt in (False, True) for fm in (False, True) for nz in LS_FORMS_OF[name]]


def ls_grid_of(name):
    M = LS_SHAPES[name]["M"]
    return 0.01, 3.99 / (M - 1)


@functools.lru_cache(maxsize=None)
def ls_signals(name):
    """(t, y32 [R, N] float32, w, f [M], (f0, df))"""
    t, y, w, _ = L.signals(LS_SHAPES[name]["of"])
    f0, df = ls_grid_of(name)
    f = f0 + df * np.arange(LS_SHAPES[name]["M"])
    y32 = y.astype(np.float32)
    for a in (y32, f):
        a.setflags(write=False)
    return t, y32, w, f, (f0, df)


@functools.lru_cache(maxsize=None)
def ls_reference(name, form):
    t, y32, w, f, _ = ls_signals(name)
    wt, fm, nz = form
    out = L.lomb_def(t, y32.astype(np.float64), f, w if wt else None, fm, nz)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ls_sums_ref(name, wt):
    """lomb_ref.sums_def at the row means: what lomb_sums_grid is held to"""
    t, y32, w, f, _ = ls_signals(name)
    y = y32.astype(np.float64)
    return L.sums_def(t, y, f, w if wt else None, float(t[0]), y.mean(axis=-1))


def rows_as_complex(common, rows):
    """(A1, A2 as [2, M], B as [R, M]) complex from the layout of the sums"""
    return np.stack([common[:, 0] + 1j * common[:, 1], common[:, 2] + 1j * common[:, 3]]), rows[..., 0] + 1j * rows[..., 1]
