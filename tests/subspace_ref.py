"""float64 restatements of include/spectral_sub.h (covmat_def, ls_def, pseudo_def), independent forms of the same things (the data
matrix, lstsq, the projector), a restatement of the kernels' arithmetic (covmat_rec: row 0 and the diagonal recursion; ls_chol: Cholesky
from that matrix), the cases of tests/test_gpu_subspace.py, its bounds and the measured figures its allowances rest on.  numpy only."""
import numpy as np

import burg_ref as B
import eigh_ref as EG

MARGIN = 4.0
U = 2.0 ** -53
SEGS_HOOK = 7                   # SP_AR_SEGS of the two-pass test


# ---- the definitions -----------------------------------------------------------------------------------------------------------
def covmat_def(s, m, fb):
    """C[i,j] = (1 / N) sum_{t=m-1}^{n-1} conj(s[t-i]) s[t-j]; fb: (C + J conj(C) J) / 2.  complex128 [m, m]"""
    s = np.asarray(s, dtype=np.complex128)
    n = s.size
    N = n - m + 1
    C = np.empty((m, m), dtype=np.complex128)
    for i in range(m):
        for j in range(i, m):
            C[i, j] = np.sum(np.conj(s[m - 1 - i:n - i]) * s[m - 1 - j:n - j]) / N
            C[j, i] = np.conj(C[i, j])
    if fb:
        C = 0.5 * (C + np.conj(C[::-1, ::-1]))
    return C


def data_matrix(s, m, fb):
    """X with X'X / rows-of-forward = C: MATLAB's corrmtx(s, m - 1, 'covariance' | 'modified') up to its scaling: row t holds
    s[t], s[t-1] .. s[t-m+1]; the backward rows conj(s[t-m+1]) .. conj(s[t])"""
    s = np.asarray(s, dtype=np.complex128)
    n = s.size
    X = np.stack([s[t - np.arange(m)] for t in range(m - 1, n)])
    if fb:
        X = np.concatenate([X, np.conj(X[:, ::-1])]) / np.sqrt(2.0)
    return X


def covmat_rec(s, m, fb):
    """the kernels' arithmetic: row 0 summed, every diagonal walked by C[i+1,j+1] = C[i,j] + conj(s[m-2-i]) s[m-2-j] -
    conj(s[n-1-i]) s[n-1-j], mirrored, folded along the diagonal, divided by N"""
    s = np.asarray(s, dtype=np.complex128)
    n = s.size
    N = n - m + 1
    C = np.zeros((m, m), dtype=np.complex128)
    for d in range(m):
        c = np.sum(np.conj(s[m - 1:n]) * s[m - 1 - d:n - d])
        dg = [c]
        for i in range(m - d - 1):
            j = i + d
            c = c + np.conj(s[m - 2 - i]) * s[m - 2 - j] - np.conj(s[n - 1 - i]) * s[n - 1 - j]
            dg.append(c)
        dg = np.array(dg)
        if d == 0:
            dg = dg.real + 0j
        if fb:
            dg = 0.5 * (dg + dg[::-1])
        dg = dg / N
        for i in range(m - d):
            C[i, i + d] = dg[i]
            C[i + d, i] = np.conj(dg[i])
    return C


def ls_from(C):
    """-> a[m], e, status of sum_j C[i,j] a_j = -C[i,0] by Cholesky, with the kernel's pivot rule"""
    m = C.shape[0]
    p = m - 1
    A = np.array(C[1:, 1:], dtype=np.complex128)
    dg = A.diagonal().real.copy()
    L = np.zeros_like(A)
    for j in range(p):
        d = A[j, j].real
        if not d > m * 2.0 ** -52 * dg[j]:
            return np.eye(1, m, dtype=np.complex128)[0], 0.0, j + 1
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], np.conj(L[j + 1:, j]))
    y = np.zeros(p, dtype=np.complex128)
    b = -np.array(C[1:, 0])
    for j in range(p):
        y[j] = b[j] / L[j, j].real
        b[j + 1:] -= L[j + 1:, j] * y[j]
    a = np.zeros(p, dtype=np.complex128)
    for j in range(p - 1, -1, -1):
        a[j] = y[j] / L[j, j].real
        y[:j] -= np.conj(L[j, :j]) * a[j]
    full = np.concatenate([[1.0], a])
    return full, float((C[0, 0] + np.sum(C[0, 1:] * a)).real), 0


def ls_def(s, p, fb, rec=False):
    """the fit of one detrended segment -> a[p + 1] (float64 for a real segment), e, status; rec: from the kernels' matrix"""
    C = (covmat_rec if rec else covmat_def)(s, p + 1, fb)
    a, e, st = ls_from(C)
    return (a if np.iscomplexobj(s) else a.real.copy()), e, st


def ls_lstsq(s, p, fb):
    """the same fit by numpy.linalg.lstsq on the data matrix: X[:, 1:] a = -X[:, 0]; e = |residual|^2 / N"""
    X = data_matrix(s, p + 1, fb)
    N = np.asarray(s).size - p
    a = np.linalg.lstsq(X[:, 1:], -X[:, 0], rcond=None)[0]
    r = X[:, 0] + X[:, 1:] @ a
    full = np.concatenate([[1.0], a])
    return (full if np.iscomplexobj(s) else full.real.copy()), float(np.sum(np.abs(r) ** 2) / N)


def steering(nu, m):
    nu = np.atleast_1d(nu)
    fr = nu - np.floor(nu)
    ph = np.outer(fr, np.arange(m))
    return np.exp(2j * np.pi * (ph - np.round(ph)))                      # [bins, m]: e(nu)[i] = exp(+2 pi i nu i)


def pseudo_def(V, w, p, nbins, start, step, weighting):
    """P[q] = 1 / sum_{k >= p} g_k |v_k^H e(nu_q)|^2 -> (P float64 [nbins], status)"""
    V, w = np.asarray(V, dtype=np.complex128), np.asarray(w, dtype=np.float64)
    m = V.shape[0]
    Es = steering(start + np.arange(nbins) * step, m)
    g = np.ones(m - p)
    st = 0
    if weighting == "ev":
        wk = w[p:]
        st = int(np.any(~(wk > 0)))
        g = np.where(wk > 0, 1.0 / np.where(wk > 0, wk, 1.0), 0.0)
    # sum_i v_k[i] e^{-2 pi i nu i} = conj(e)^T v_k
    proj = np.abs(np.conj(Es) @ V[:, p:]) ** 2
    den = proj @ g
    return np.where(den > 0, 1.0 / np.where(den > 0, den, 1.0), 0.0), st


def eigh_desc(C):
    w, V = np.linalg.eigh(C)
    return w[::-1].copy(), V[:, ::-1].copy()


def music_projector(C, p, nu):
    """1 / e^H (I - V_s V_s^H) e"""
    w, V = eigh_desc(C)
    m = C.shape[0]
    Pn = np.eye(m) - V[:, :p] @ np.conj(V[:, :p].T)
    Es = steering(nu, m)
    return 1.0 / np.einsum("qi,ij,qj->q", np.conj(Es), Pn, Es).real


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def covmat_bound(s, m, mean_rounding=0.0):
    """per element, absolute: 4 (n + 2 m) 2^-53 (sum |s|^2 / N), the sum of N products and 2 (m - 1) steps of the recursion, each term at
    the most |s[a]| |s[b]| (Cauchy-Schwarz bounds their sum by sum |s|^2).  A mean that differs from the reference's by delta moves
    every sample by delta and an element by (1 / N) sum (|s[t-i]| + |s[t-j]|) delta + delta^2 <= 2 delta sqrt(sum |s|^2 / N) + delta^2"""
    s = np.asarray(s)
    n = s.size
    N = n - m + 1
    pw = float(np.sum(np.abs(s) ** 2)) / N
    return 4.0 * (n + 2 * m) * U * pw + 2.0 * mean_rounding * np.sqrt(pw) + mean_rounding ** 2


def mean_rounding(x):
    """what a float64 mean of n float32 samples summed in any order can differ by from another order's: 2 n 2^-53 mean|x| (each of
    two sums of n terms is off by n u sum|x| / n at the most)"""
    x = np.asarray(x)
    return 2.0 * x.size * U * float(np.mean(np.abs(x)))


def pseudo_bound(V, w, p, nbins, start, step, weighting):
    """relative to P, per bin: a Horner sum over m terms with a unit-circle point good to 2 u is off by 4 m u sum|v_k| (as
    tests/test_gpu_parametric.py derives for k_ar_psd), so |S_k|^2 by 8 m u sum|v_k| |S_k| and, with sum|v_k| <= sqrt(m),
    D = sum g_k |S_k|^2 by 8 m sqrt(m) u sum_k g_k |S_k|; the sum over the m - p vectors and the weights 1 / w_k add (m - p + 2) u D;
    one more term for the reference's own sums: twice that"""
    V, w = np.asarray(V, dtype=np.complex128), np.asarray(w, dtype=np.float64)
    m = V.shape[0]
    Es = steering(start + np.arange(nbins) * step, m)
    g = np.ones(m - p) if weighting == "music" else np.where(w[p:] > 0, 1.0 / np.where(w[p:] > 0, w[p:], 1.0), 0.0)
    S = np.abs(np.conj(Es) @ V[:, p:])
    D = (S ** 2) @ g
    l1 = np.sum(np.abs(V[:, p:]), axis=0)
    err = 8.0 * m * U * (S * l1) @ g + (m - p + 2) * U * D
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(D > 0, 2.0 * err / D, 0.0)


# ---- the cases of the GPU test ---------------------------------------------------------------------------------------------------
COV_CASES = {
    "c2":      dict(n=2, m=2, cplx=False),                              # the smallest; one snapshot
    "c8":      dict(n=8, m=8, cplx=False),                              # a single snapshot
    "c64":     dict(n=64, m=8, cplx=False),
    "c333c":   dict(n=333, m=24, cplx=True),
    "seam":    dict(n=2048 + 7, m=8, cplx=False),                       # a halo across a stage seam
    "seam64":  dict(n=2 * 2048 + 63, m=64, cplx=False),
    "long":    dict(n=100003, m=32, cplx=True),                         # many tiles, a ragged last one
    "frames":  dict(n=200, m=7, cplx=False, rows=3, nframes=5, hop=77, first=13),
    "ragged":  dict(n=64, m=4, cplx=True, rows=1, nframes=11, hop=32, first=0),
}
# the records of burg_ref the fits run on, and their orders
LS_CASES = {"w64": 4, "w333c": 8, "g4096": 63, "frames": 6}


def shape_of(name):
    c = dict(rows=1, nframes=1, hop=1, first=0)
    c.update(COV_CASES[name])
    c["nsig"] = c["first"] + (c["nframes"] - 1) * c["hop"] + c["n"] + (3 if c["first"] else 0)
    return c


_signals = {}


def signals(name):
    """the record of a covmat case, float32 or complex64 [rows, nsig]: two tones in white noise and a constant offset"""
    if name in _signals:
        return _signals[name]
    c = shape_of(name)
    rng = np.random.default_rng(sorted(COV_CASES).index(name) + 300)
    t = np.arange(c["nsig"])
    rows = []
    for r in range(c["rows"]):
        if c["cplx"]:
            y = np.exp(2j * np.pi * (0.11 * t + rng.random())) + 0.5 * np.exp(2j * np.pi * (0.31 * t + rng.random()))
            y = y + 0.3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size)) + (0.7 - 0.4j)
        else:
            y = np.cos(2 * np.pi * (0.11 * t + rng.random())) + 0.5 * np.cos(2 * np.pi * (0.31 * t + rng.random()))
            y = y + 0.3 * rng.standard_normal(t.size) + 0.7
        rows.append(y)
    x = np.stack(rows).astype(np.complex64 if c["cplx"] else np.float32)
    x.setflags(write=False)
    _signals[name] = x
    return x


_cov_refs = {}


def cov_reference(name, fb, detrend=True, mean_value=None):
    """C[rows, nframes, m, m] of the case from the definition, computed once"""
    key = (name, fb, detrend, mean_value)
    if key not in _cov_refs:
        c = shape_of(name)
        x = signals(name)
        _cov_refs[key] = np.stack([np.stack([covmat_def(B.segment(x[r], c["n"], c["first"], g, c["hop"], detrend, mean_value), c["m"], fb)
                                             for g in range(c["nframes"])]) for r in range(c["rows"])])
    return _cov_refs[key]


_ls_refs = {}


def ls_reference(name, fb, kind="lstsq"):
    """(a, e[..., None], k = zeros) of the burg_ref record `name` at LS_CASES' order, every (row, frame) less its own mean: by lstsq on
    the data matrix (the reference) or by Cholesky from the kernels' matrix (kind='chol'); in the layout burg_ref.deviations takes"""
    key = (name, fb, kind)
    if key not in _ls_refs:
        c = B.shape_of(name)
        p = LS_CASES[name]
        x = B.signals(name)
        a = np.zeros((c["rows"], c["nframes"], p + 1), dtype=np.complex128 if c["cplx"] else np.float64)
        e = np.zeros((c["rows"], c["nframes"], 1))
        for r in range(c["rows"]):
            for g in range(c["nframes"]):
                s = B.segment(x[r], c["n"], c["first"], g, c["hop"])
                if kind == "lstsq":
                    a[r, g], e[r, g, 0] = ls_lstsq(s, p, fb)
                else:
                    a[r, g], e[r, g, 0], st = ls_def(s, p, fb, rec=True)
                    assert st == 0
        _ls_refs[key] = (a, e, np.zeros(a.shape[:-1] + (1,)))
    return _ls_refs[key]


def ls_deviations(got, ref):
    """burg_ref.deviations' metrics that a least-squares fit has: (P per bin, a, e)"""
    dP, _, da, dE = B.deviations(got, ref)
    return dP, da, dE


def white(n, cplx, seed=5):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    return y.astype(np.complex64 if cplx else np.float32)


# ---- end to end: two close tones ----------------------------------------------------------------------------------------------------
TONES = (0.200, 0.215)
E2E_N, E2E_M, E2E_GRID = 128, 24, 8192
E2E_CASES = {"real20": (False, 4, 20.0), "real40": (False, 4, 40.0), "cplx20": (True, 2, 20.0), "cplx40": (True, 2, 40.0)}
MIN_GAP = 50.0


def tones(name):
    """two unit tones at TONES cycles per sample in white noise at the case's SNR (per tone), float32 or complex64 [E2E_N].  At 20 dB
    the float64 reference itself puts its peaks within one grid step of the tones for about half of the noise realisations (32 of 60
    seeds tried); the seed is one of those, with the reference 0.6 of a step off at the most, and the test asserts that on the
    reference before it looks at the device"""
    cplx, p, snr = E2E_CASES[name]
    rng = np.random.default_rng(sorted(E2E_CASES).index(name) + 940)
    t = np.arange(E2E_N)
    sig = 10.0 ** (-snr / 20.0)
    if cplx:
        y = sum(np.exp(2j * np.pi * (f * t + rng.random())) for f in TONES)
        y = y + sig * (rng.standard_normal(E2E_N) + 1j * rng.standard_normal(E2E_N)) / np.sqrt(2.0)
        return y.astype(np.complex64)
    y = sum(np.sqrt(2.0) * np.cos(2 * np.pi * (f * t + rng.random())) for f in TONES)
    return (y + sig * rng.standard_normal(E2E_N)).astype(np.float32)


def e2e_axis(cplx):
    """(nbins, start, step): 0 .. 1/2 for a real record, the full circle for a complex one, on the E2E_GRID-point grid"""
    return (E2E_GRID // 2 + 1 if not cplx else E2E_GRID, 0.0, 1.0 / E2E_GRID)


def e2e_reference(name, weighting="music"):
    cplx, p, _ = E2E_CASES[name]
    C = covmat_def(B.segment(tones(name), E2E_N, detrend=False), E2E_M, True)
    w, V = eigh_desc(C)
    return C, w, V, pseudo_def(V, w, p, *e2e_axis(cplx), weighting)[0]


def perturbation_change(name, trials=8, weighting="music"):
    """the worst relative change of the reference P over `trials` Hermitian perturbations of C of 2-norm eigh_ref.tol(m) ||C||_2"""
    cplx, p, _ = E2E_CASES[name]
    C, w, V, P = e2e_reference(name, weighting)
    rng = np.random.default_rng(77)
    worst = 0.0
    for _ in range(trials):
        H = rng.standard_normal(C.shape) + 1j * rng.standard_normal(C.shape)
        H = H + np.conj(H.T)
        H *= EG.tol(E2E_M) * np.linalg.norm(C, 2) / np.linalg.norm(H, 2)
        w2, V2 = eigh_desc(C + H)
        P2 = pseudo_def(V2, w2, p, *e2e_axis(cplx), weighting)[0]
        worst = max(worst, float(np.max(np.abs(P2 - P) / P)))
    return worst


def peaks(P, k):
    """the bins of the k largest local maxima of P (circular), ascending"""
    P = np.asarray(P, dtype=np.float64)
    loc = np.flatnonzero((P > np.roll(P, 1)) & (P >= np.roll(P, -1)))
    return np.sort(loc[np.argsort(P[loc])[-k:]])


# ---- measured on the CPU (tests/test_host_subspace.py holds each to within a factor of two) ------------------------------------------
# the worst (P per bin, a, e) of the Cholesky fit from the kernels' matrix (covmat_rec + ls_from) against lstsq on the data matrix,
# over LS_CASES and both fb (the conditions of the normal matrices run from 20 to 1.6e3); each metric has its own allowance
LS_CHOL_DEV = (1.8e-13, 7.0e-15, 7.7e-15)
LS_ALLOWANCE = tuple(MARGIN * d for d in LS_CHOL_DEV)
# the worst relative change of the reference pseudospectrum under the perturbation above, over E2E_CASES
E2E_PERT = 3.3e-7
E2E_ALLOWANCE = MARGIN * E2E_PERT
# the covariance recursion against the direct sums, relative to the mean power sum |s|^2 / N, over COV_CASES
COV_REC_DEV = 1.4e-15
# the share of the allowances tests/test_gpu_subspace.py used on an MI355X
COV_DEVICE_SHARE = 0.020
LS_DEVICE_SHARE = 0.49
PSEUDO_DEVICE_SHARE = 0.20
E2E_DEVICE_SHARE = 5.2e-7
