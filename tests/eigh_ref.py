"""Float64 numpy restatement of the batched Hermitian eigensolver k_eigh.hip (sp_eigh): the same padding, scaling, round-robin
ordering, skip rule, stopping rule, sort and phase convention, one matrix at a time.  It is not numpy.linalg.eigh: the tests hold it
to that, and the kernel to the same limits.

    a[n][n]   only the lower triangle and the real part of the diagonal are read (numpy's UPLO='L')
    NP        the order padded to 8, 16, 32 or 64 with zero rows and columns
    scale     2^-e with e = ilogb(the largest |re| or |im| read); w is scaled back by 2^e
    sweep     NP - 1 steps of NP / 2 disjoint pairs (schedule()); all rotations of a step come from the matrix before the step
    rotation  g = |a_pq|, skipped unless g >= 2^-1000 (so exact zeros, and with them the padding, never mix with anything);
              tau = (a_qq - a_pp) / 2g, t = sgn(tau) / (|tau| + hypot(1, tau)) (sgn(0) = 1), c = 1 / sqrt(1 + t^2), s = t c,
              ph = a_pq / g;  J = [[c, s ph], [-s conj(ph), c]] on (p, q);  A <- J^H A J, V <- V J
              pair-blocks r <= c are computed, the others are their conjugate mirror; the diagonal block is set to
              a_pp - t g, a_qq + t g, 0
    stop      before each sweep: off^2 = sum_{i<j} |a_ij|^2 <= (n eps)^2 ||A||_F^2 (the finite norm of the scaled input); after
              max_sweeps sweeps without that, sweeps = max_sweeps + 1
    finish    w_i = Re a_ii, descending by counting with ties broken by index; each written vector is turned so that its component of
              largest modulus (the first on ties) is real and positive
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
G_MIN = 2.0 ** -1000
MAX_N = 64


def padded_order(n):
    for NP in (8, 16, 32, 64):
        if n <= NP:
            return NP
    raise ValueError("eigh_ref: n = %d above %d" % (n, MAX_N))


def tol(n):
    """4 n 30 eps: Jacobi's backward error is of order n sweeps eps."""
    return 4.0 * n * 30 * EPS


def schedule(NP):
    """The round-robin tournament: NP - 1 steps, each an int array [NP / 2, 2] of disjoint pairs p < q.  Index NP - 1 stays put and
    meets s at step s; pair k >= 1 of step s is ((s + k) mod (NP - 1), (s - k) mod (NP - 1))."""
    m, R = NP // 2, NP - 1
    steps = []
    for s in range(R):
        a = [R] + [(s + k) % R for k in range(1, m)]
        b = [s] + [(s - k) % R for k in range(1, m)]
        steps.append(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1))
    return steps


def hermitian_from_lower(a):
    """The matrix the solver sees: lower triangle, real diagonal, the upper triangle its mirror ([..., n, n])."""
    a = np.asarray(a, dtype=np.complex128)
    lo = np.tril(a, -1)
    d = np.zeros_like(a)
    idx = np.arange(a.shape[-1])
    d[..., idx, idx] = a[..., idx, idx].real
    return lo + d + np.conj(np.swapaxes(lo, -1, -2))


def _one(a, nvec, max_sweeps):
    n = a.shape[0]
    NP = padded_order(n)
    H = hermitian_from_lower(a)
    with np.errstate(invalid="ignore"):
        comps = np.abs(np.concatenate([H.real.ravel(), H.imag.ravel()]))
        amax = float(np.fmax.reduce(comps, initial=0.0))
    e = int(np.frexp(amax)[1]) - 1 if (amax > 0 and np.isfinite(amax)) else 0
    A = np.zeros((NP, NP), dtype=np.complex128)
    A[:n, :n] = np.ldexp(H.real, -e) + 1j * np.ldexp(H.imag, -e)
    V = np.eye(NP, dtype=np.complex128)
    iu = np.triu_indices(NP, 1)
    norm2 = float(np.sum(A.diagonal().real ** 2) + 2.0 * np.sum(np.abs(A[iu]) ** 2))
    thresh = (n * EPS) ** 2 * norm2
    steps = schedule(NP)
    sweeps = max_sweeps + 1
    with np.errstate(all="ignore"):
        for sw in range(max_sweeps + 1):
            off2 = float(np.sum(A[iu].real ** 2 + A[iu].imag ** 2))
            if off2 <= thresh and np.isfinite(thresh):
                sweeps = sw
                break
            if sw == max_sweeps:
                break
            for pq in steps:
                p, q = pq[:, 0], pq[:, 1]
                apq = A[p, q]
                g = np.hypot(apq.real, apq.imag)
                skip = ~(g >= G_MIN)
                gs = np.where(skip, 1.0, g)
                tau = (A[q, q].real - A[p, p].real) / (2.0 * gs)
                t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.hypot(1.0, tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                ph = apq / gs
                c, s, t, ph = np.where(skip, 1.0, c), np.where(skip, 0.0, s), np.where(skip, 0.0, t), np.where(skip, 1.0, ph)
                tg = t * gs
                sp, sc = s * ph, s * np.conj(ph)
                # rows, then columns: element for element the 2 x 2 pair-block formulas
                Y = A.copy()
                Y[p, :] = c[:, None] * A[p, :] - sp[:, None] * A[q, :]
                Y[q, :] = sc[:, None] * A[p, :] + c[:, None] * A[q, :]
                X = Y.copy()
                X[:, p] = Y[:, p] * c[None, :] - Y[:, q] * sc[None, :]
                X[:, q] = Y[:, p] * sp[None, :] + Y[:, q] * c[None, :]
                blk = np.empty(NP, dtype=np.int64)
                blk[p] = np.arange(p.size)
                blk[q] = np.arange(p.size)
                upper = blk[:, None] <= blk[None, :]
                X = np.where(upper, X, np.conj(X.T))
                dpp, dqq = A[p, p].real - tg, A[q, q].real + tg
                X[p, p], X[q, q], X[p, q], X[q, p] = dpp, dqq, 0.0, 0.0
                Vn = V.copy()
                Vn[:, p] = V[:, p] * c[None, :] - V[:, q] * sc[None, :]
                Vn[:, q] = V[:, p] * sp[None, :] + V[:, q] * c[None, :]
                A, V = X, Vn
        wl = A.diagonal().real[:n].copy()
        rank = np.array([int(np.sum((wl > wl[i]) | ((wl == wl[i]) & (np.arange(n) < i)))) for i in range(n)])
        perm = np.arange(n)
        perm[rank] = np.arange(n)
        w = np.ldexp(wl[perm], e)
        Vo = V[:n, perm[:nvec]].copy()
        for j in range(nvec):
            col = Vo[:, j]
            i = int(np.argmax(col.real ** 2 + col.imag ** 2))
            r = np.hypot(col[i].real, col[i].imag)
            Vo[:, j] = col * (np.conj(col[i]) / r)
            Vo[i, j] = r
    return w, Vo, sweeps


def eigh_ref(a, nvec=None, max_sweeps=30):
    """a [..., n, n] -> (w [..., n] float64 descending, V [..., n, nvec] complex128, sweeps [...] int32)."""
    a = np.asarray(a)
    if a.ndim < 2 or a.shape[-1] != a.shape[-2]:
        raise ValueError("eigh_ref: a must be [..., n, n]")
    n = a.shape[-1]
    nvec = n if nvec is None else int(nvec)
    lead = a.shape[:-2]
    flat = a.reshape((-1, n, n)).astype(np.complex128)
    w = np.empty((flat.shape[0], n))
    V = np.empty((flat.shape[0], n, nvec), dtype=np.complex128)
    sw = np.empty(flat.shape[0], dtype=np.int32)
    for b in range(flat.shape[0]):
        w[b], V[b], sw[b] = _one(flat[b], nvec, int(max_sweeps))
    return w.reshape(lead + (n,)), V.reshape(lead + (n, nvec)), sw.reshape(lead)


# ---- the families of the tests, each [batch, n, n] complex128 (seeded by the caller's generator)
def fam_csd(rng, batch, n, frames=None):
    frames = 3 * n + 2 if frames is None else frames
    X = rng.standard_normal((batch, n, frames)) + 1j * rng.standard_normal((batch, n, frames))
    return X @ np.conj(np.swapaxes(X, -1, -2)) / frames


def fam_rank_deficient(rng, batch, n):
    return fam_csd(rng, batch, n, frames=max(1, n // 4))


def fam_graded(rng, batch, n):
    d = np.logspace(0, -8, n) if n > 1 else np.ones(1)
    return fam_csd(rng, batch, n) * d[None, :, None] * d[None, None, :]


def fam_degenerate(rng, batch, n):
    """Clusters of four equal eigenvalues 1, 2, 3, .. under a random unitary."""
    lam = (np.arange(n) // 4 + 1).astype(np.float64)
    Z = rng.standard_normal((batch, n, n)) + 1j * rng.standard_normal((batch, n, n))
    Q = np.linalg.qr(Z)[0]
    return (Q * lam[None, None, :]) @ np.conj(np.swapaxes(Q, -1, -2))


def fam_real_symmetric(rng, batch, n):
    X = rng.standard_normal((batch, n, 3 * n + 2))
    return (X @ np.swapaxes(X, -1, -2) / (3 * n + 2)).astype(np.complex128)


def fam_diagonal(rng, batch, n):
    out = np.zeros((batch, n, n), dtype=np.complex128)
    idx = np.arange(n)
    out[:, idx, idx] = rng.standard_normal((batch, n))
    return out


def fam_zero(rng, batch, n):
    return np.zeros((batch, n, n), dtype=np.complex128)


def fam_identity(rng, batch, n):
    return np.broadcast_to(np.eye(n, dtype=np.complex128), (batch, n, n)).copy()


def fam_huge(rng, batch, n):
    return fam_csd(rng, batch, n) * 1e150


def fam_tiny(rng, batch, n):
    return fam_csd(rng, batch, n) * 1e-150


FAMILIES = {
    "csd": fam_csd, "rank_deficient": fam_rank_deficient, "graded": fam_graded, "degenerate": fam_degenerate,
    "real_symmetric": fam_real_symmetric, "diagonal": fam_diagonal, "zero": fam_zero, "identity": fam_identity,
    "huge": fam_huge, "tiny": fam_tiny,
}
ORDERS = (1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64)


def limits(a, w, V, sweeps):
    """The figures the tests bound, the worst over a batch a[B, n, n] solved with all n vectors: dict(resid, orth, eig, descending,
    phase, sweeps).  resid = ||A_L V - V diag(w)||_F / ||A||_F, orth = ||V^H V - I||_F, eig = max|w - eigvalsh(A_L)| / ||A||_2
    (a zero matrix: the absolute figures); phase = phase_defect(V)."""
    a, w, V = np.asarray(a), np.asarray(w, dtype=np.float64), np.asarray(V)
    if a.ndim == 2:
        a, w, V = a[None], w[None], V[None]
    n = a.shape[-1]
    H = hermitian_from_lower(a)
    big = np.max(np.abs(H), axis=(1, 2))
    e = np.where((big > 0) & np.isfinite(big), np.frexp(big)[1], 0)       # an exact power of two per matrix, so that the squares
    H = np.ldexp(H.real, -e[:, None, None]) + 1j * np.ldexp(H.imag, -e[:, None, None])     # below neither overflow nor vanish
    w = np.ldexp(w, -e[:, None])
    nf = np.linalg.norm(H, axis=(1, 2))
    ref = np.linalg.eigvalsh(H)[:, ::-1]
    n2 = np.max(np.abs(ref), axis=1)
    resid = np.linalg.norm(H @ V - V * w[:, None, :], axis=(1, 2))
    orth = np.linalg.norm(np.conj(np.swapaxes(V, 1, 2)) @ V - np.eye(n)[None], axis=(1, 2))
    eig = np.max(np.abs(w - ref), axis=1)
    return dict(resid=float(np.max(resid / np.where(nf > 0, nf, 1.0))), orth=float(np.max(orth)),
                eig=float(np.max(eig / np.where(n2 > 0, n2, 1.0))), descending=bool(np.all(np.diff(w, axis=1) <= 0)),
                phase=max(phase_defect(v) for v in V), sweeps=int(np.max(sweeps)))


def phase_defect(V):
    """0 for a matrix of columns whose components of largest modulus are real and positive: max over the columns of
    (|imag| + max(0, -real)) / modulus of the largest component."""
    worst = 0.0
    for j in range(V.shape[1]):
        col = V[:, j]
        m2 = col.real ** 2 + col.imag ** 2
        # any component within rounding of the largest may be the one the solver turned
        cand = np.nonzero(m2 >= m2.max() * (1 - 64 * EPS))[0]
        worst = max(worst, min((abs(col[i].imag) + max(0.0, -col[i].real)) / np.sqrt(m2[i]) for i in cand))
    return worst
