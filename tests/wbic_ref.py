"""Float64 reference of the wavelet bispectrum and bicoherence (numpy), written from the definitions:
    rows i = 0 .. S - 1 are the frequencies (k_lo + i) df with the scales 1 / (flambda (k_lo + i) df) (samples, dt = 1);
    W = cwt_ref.cwt_ref(record, scales): the linear convolution over the zero-extended record;
    over the block of T samples from a on, with m = i + j + k_lo <= S - 1:
        B(i, j) = (1/T) sum_n Wx[i, n] Wy[j, n] conj(Wz[m, n]),   D(i, j) = (1/T) sum_n |Wx[i, n] Wy[j, n]|^2,
        P(m) = (1/T) sum_n |Wz[m, n]|^2,   b2 = |B|^2 / (D P(m)) (0 where D P = 0),   A(i, j) = (1/T) sum_n |Wx Wy| |Wz|
    B, b2 and A are NaN where m > S - 1.  Also the float32 restatement (cwt_ref.overlap_save at float32 feeding the same sums) and the
    records the tests share.  A helper module, not a test: nothing here is collected."""
import functools
import math

import numpy as np

import cwt_ref


def flambda(family, param):
    """Fourier period / scale (Torrence & Compo 1998, table 1)."""
    if family == "morlet":
        return 4.0 * math.pi / (param + math.sqrt(2.0 + param ** 2))
    if family == "paul":
        return 4.0 * math.pi / (2.0 * param + 1.0)
    raise ValueError(family)


def grid_scales(df, k_lo, k_hi, family="morlet", param=6.0):
    """the scales (samples) of the rows k = k_lo .. k_hi"""
    k = np.arange(k_lo, k_hi + 1)
    return 1.0 / (flambda(family, param) * k * df)


def sums(Wx, Wy, Wz, k_lo, n0, block, step, nblocks):
    """-> (B complex128 [nblocks, S, S], b2, A float64 [nblocks, S, S], P float64 [nblocks, S]) from the three transforms [S, N]"""
    Wx, Wy, Wz = (np.asarray(w).astype(np.complex128) for w in (Wx, Wy, Wz))
    S = Wx.shape[0]
    B = np.full((nblocks, S, S), complex(np.nan, np.nan))
    b2 = np.full((nblocks, S, S), np.nan)
    A = np.full((nblocks, S, S), np.nan)
    P = np.zeros((nblocks, S))
    for b in range(nblocks):
        a = n0 + b * step
        assert 0 <= a and a + block <= Wx.shape[1]
        X, Y, Z = Wx[:, a:a + block], Wy[:, a:a + block], Wz[:, a:a + block]
        T = float(block)
        P[b] = np.sum(np.abs(Z) ** 2, axis=-1) / T
        for i in range(S):
            nj = S - k_lo - i                                   # the pairs (i, j) with j < nj are valid
            if nj <= 0:
                break
            prod = X[i][None, :] * Y[:nj]
            Zm = Z[i + k_lo:i + k_lo + nj]
            Bi = np.sum(prod * np.conj(Zm), axis=-1) / T
            D = np.sum(np.abs(prod) ** 2, axis=-1) / T
            den = D * P[b, i + k_lo:i + k_lo + nj]
            B[b, i, :nj] = Bi
            A[b, i, :nj] = np.sum(np.abs(prod) * np.abs(Zm), axis=-1) / T
            b2[b, i, :nj] = np.where(den > 0, np.abs(Bi) ** 2 / np.where(den > 0, den, 1.0), 0.0)
    return B, b2, A, P


def _transforms(recs, fn):
    """one transform per distinct record (None and a repeated object mean an earlier one)"""
    x, y, z = recs
    Wx = fn(x)
    Wy = Wx if y is None or y is x else fn(y)
    Wz = Wx if z is None or z is x else (Wy if z is y else fn(z))
    return Wx, Wy, Wz


def wbic_ref(x, scales, k_lo, n0, block, step, nblocks, y=None, z=None, family="morlet", param=6.0):
    """the float64 reference -> (B, b2, A, P)"""
    W = _transforms((x, y, z), lambda v: cwt_ref.cwt_ref(np.asarray(v), scales, family, param))
    return sums(*W, k_lo, n0, block, step, nblocks)


def wbic_ref32(x, scales, k_lo, n0, block, step, nblocks, L, M, y=None, z=None, family="morlet", param=6.0):
    """the float32 restatement: the device's overlap-save plan at float32 (complex64 transforms), the same sums in float64"""
    W = _transforms((x, y, z), lambda v: cwt_ref.overlap_save(np.asarray(v), scales, family, param, L, M, np.float32))
    return sums(*W, k_lo, n0, block, step, nblocks)


def parity_bound(A):
    """the bound the project holds k_bispec to: |dB| <= 1e-4 A + 1e-6 max A"""
    return 1e-4 * A + 1e-6 * np.nanmax(A)


# ---- the records --------------------------------------------------------------------------------------------------------------------
QPC_DF, QPC_KLO, QPC_KHI = 1.0 / 400, 3, 72                     # S = 70; Morlet-6: M = 633, L = 4096, hop = 2830
QPC_M, QPC_L, QPC_N, QPC_BURST = 633, 4096, 24000, 400
QPC_COUPLED, QPC_CONTROL = (17, 30, 47), (20, 35, 55)
QPC_SEED = 7


@functools.lru_cache(maxsize=4)
def qpc_record(couple_from=0, n=QPC_N, seed=QPC_SEED):
    """0.3 white noise; unit lines at k = 17 and 30 and a 0.7 line at k = 47 whose phase is the sum of theirs (from sample
    `couple_from` on; an independent phase before it); the control: unit lines at k = 20 and 35 and a 0.7 line at k = 55 with an
    independent phase.  Built burst by burst: every 400-sample burst draws fresh uniform phases.  float32."""
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal(n)
    t = np.arange(QPC_BURST)
    w = 2.0 * math.pi * QPC_DF
    for b0 in range(0, n, QPC_BURST):
        p1, p2, p3, q1, q2, q3 = rng.uniform(0.0, 2.0 * math.pi, 6)
        if b0 >= couple_from:
            p3 = p1 + p2
        m = min(QPC_BURST, n - b0)
        tt = t[:m] + b0
        k1, k2, k3 = QPC_COUPLED
        c1, c2, c3 = QPC_CONTROL
        x[b0:b0 + m] += (np.cos(w * k1 * tt + p1) + np.cos(w * k2 * tt + p2) + 0.7 * np.cos(w * k3 * tt + p3)
                         + np.cos(w * c1 * tt + q1) + np.cos(w * c2 * tt + q2) + 0.7 * np.cos(w * c3 * tt + q3))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def qpc_scales():
    return grid_scales(QPC_DF, QPC_KLO, QPC_KHI)


def qpc_trim():
    """n0 of trim=True: the e-folding time sqrt(2) s_max of the longest scale, rounded up"""
    return int(math.ceil(math.sqrt(2.0) * float(qpc_scales().max())))


def qpc_figures(b2):
    """-> (b2 at the coupled pair, b2 at the control pair, the largest b2 more than 6 rows from the coupled pair or its mirror)"""
    i, j = QPC_COUPLED[0] - QPC_KLO, QPC_COUPLED[1] - QPC_KLO
    ci, cj = QPC_CONTROL[0] - QPC_KLO, QPC_CONTROL[1] - QPC_KLO
    S = b2.shape[-1]
    ii, jj = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    near = ((np.abs(ii - i) <= 6) & (np.abs(jj - j) <= 6)) | ((np.abs(ii - j) <= 6) & (np.abs(jj - i) <= 6))
    far = np.where(near | np.isnan(b2), -np.inf, b2)
    return float(b2[i, j]), float(b2[ci, cj]), float(far.max())


def assert_qpc_whole(b2):
    """the asserts of the first record (one block): what the reference must pass before the device is asked to"""
    c, ctl, far = qpc_figures(b2)
    print("coupled %.3f  control %.3f  largest elsewhere %.3f" % (c, ctl, far))
    assert c > 0.25 and ctl < 0.2 and far < 0.2, (c, ctl, far)


def assert_qpc_switched(b2):
    """the second record: coupling switched on at sample 12 000, four blocks of 6000"""
    c = [qpc_figures(b2[b])[0] for b in range(4)]
    print("coupled pair per block: %s" % ", ".join("%.3f" % v for v in c))
    assert c[0] < 0.1 and c[1] < 0.1 and c[2] > 0.25 and c[3] > 0.25, c


@functools.lru_cache(maxsize=2)
def qpc_reference(switched):
    """(B, b2, A, P) in float64 of the two records: one block over the whole record, or four blocks of 6000 with the coupling
    switched on at 12 000.  Computed once and shared; the arrays are read-only."""
    if switched:
        r = wbic_ref(qpc_record(12000), qpc_scales(), QPC_KLO, 0, 6000, 6000, 4)
    else:
        r = wbic_ref(qpc_record(0), qpc_scales(), QPC_KLO, 0, QPC_N, QPC_N, 1)
    for a in r:
        a.setflags(write=False)
    return r


def noise_record(n, cplx, seed):
    """white noise plus a few lines on the grid of the parity cases, so that no row is empty; float32 or complex64"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.5 * rng.standard_normal(n)
    for f, a in ((0.013, 1.0), (0.041, 0.8), (0.054, 0.6), (0.11, 0.7), (0.23, 0.5)):
        x = x + a * np.cos(2.0 * math.pi * f * t + rng.uniform(0.0, 2.0 * math.pi))
    if cplx:
        y = 0.5 * rng.standard_normal(n)
        for f, a in ((0.021, 0.9), (0.07, 0.6), (0.17, 0.5)):
            y = y + a * np.sin(2.0 * math.pi * f * t + rng.uniform(0.0, 2.0 * math.pi))
        return (x + 1j * y).astype(np.complex64)
    return x.astype(np.float32)
