"""The reference of the conditioned spectral analysis (pyfft_amd.mimo; k_cond.hip; include/spectral_mimo.h), numpy only:

  ref_cond       the definitions in numpy.longdouble (the factor, and every output from it)
  restate_cond   the kernel's operation order in float64 (right-looking factor, the flags, every output as the kernel sums it)
  bound_of       a DERIVED elementwise error bound per output of one matrix, from the backward-error results for the Cholesky
                 factorisation and for triangular solves, evaluated in extended precision on the reference
  matrices, GPU_N, gpu_cases   the seeded case tables
  record, scipy_csd, allowance_of   the end-to-end record of three correlated inputs and two outputs, its float64 CSD matrix, and the
                 measured allowance of the end-to-end comparison

The bound.  u = 2^-53, gam(k) = k u / (1 - k u).  A complex inner product of k terms is two real ones of 2k terms whose summands are at
most |a_m| |b_m| each, so its error is at most sqrt(2) gam(2k) sum |a_m| |b_m|; a division by a real number or a real square root adds
two roundings.  Hence cg(k) = sqrt(2) gam(2k + 2) takes the place of gamma_k in Higham, Accuracy and Stability of Numerical Algorithms,
2nd ed.:
  Thm 10.3   the computed factor satisfies  L^ L^H = A + dA,  |dA| <= cg(n + 1) |L^| |L^H|                              =: Ef
  Thm 8.5    a triangular solve T x = b gives (T + dT) x^ = b, |dT| <= cg(n) |T|, in any order of the substitution
  Thm 10.4   the solution through the factor satisfies (A + dA) x^ = b, |dA| <= cg(3n + 1) |L^| |L^H|                  =: Es
(The kernel may fuse a multiplication into the following addition; that removes roundings and the bounds stand.)  With a loading the
kernel's delta and A_ii + delta carry n + 3 roundings, a further diagonal perturbation gam(n + 3) (|G_ii| + delta).  Every output is
a function of A, exact for the perturbed matrix up to the roundings of its own final products, so to first order
  H     dH = (dA_yx - H dA_xx) A_xx^-1                      |dH|   <= (Es_yx + |H| Es_xx) |A_xx^-1|
  Gc    dGc = [-H, 1] dA [-H, 1]^H                          |dGc|  <= [|H|, 1] Ef [|H|, 1]^T + cg(r + 1) |L_yy| |L_yy^H|
  piv   d piv_j = v^H dA v, v = L_jj conj(row j of L^-1)    |dpiv| <= piv_j |W_j| Ef |W_j|^T + 2u piv_j
  mcoh  the numerator is A_ii - Gc_ii of the perturbed A    |dm|   <= (Ef_ii + [|H|, 1] Ef [|H|, 1]^T_ii) / A_ii + gam(2q + 4) mcoh_i
  P     dP = -P dA P; W^ = L^-1 by substitution (Thm 8.5), P^ = fl(W^H W)
                                                            |dP|   <= |P| Ef |P| + 2 cg(n) |W^H| (|W| |L| |W|) + cg(n) |W^H| |W|
and the remainder of the series is covered by the factor 1 / (1 - rho)^2, rho = || |A^-1| Es ||_inf, which the case tables keep below
1e-3 (checked on the CPU by tests/test_host_mimo.py).  |L|, |W|, |H| and |P| are the reference's."""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = LD(2.0) ** -53
WANT = ("H", "Gc", "mcoh", "piv", "P")


def gam(k):
    return LD(k) * U / (LD(1) - LD(k) * U)


def cg(k):
    return np.sqrt(LD(2)) * gam(2 * k + 2)


def _ct(M):
    return np.conj(np.swapaxes(M, -1, -2))


# ---- the definitions, in extended precision --------------------------------------------------------------------------
def ref_cond(G, q, order=None, loading=0.0):
    """one matrix G[n, n] (lower triangle and real diagonal read) -> dict of A, L, W = L^-1, H, Gc, mcoh, piv, P in longdouble.  The
    matrix must be positive definite (the flagged cases are the restatement's)."""
    G = np.asarray(G)
    n = G.shape[0]
    order = np.arange(n) if order is None else np.asarray(order)
    lo = np.tril(G.astype(CLD), -1)
    Gh = lo + _ct(lo) + np.diag(np.real(np.diag(G)).astype(LD)).astype(CLD)
    A = Gh[np.ix_(order, order)].copy()
    tr = np.sum(np.real(np.diag(A)))
    delta = LD(loading) * max(tr, LD(0)) / LD(n)
    A = A + delta * np.eye(n, dtype=CLD)
    L = np.zeros((n, n), dtype=CLD)
    S = A.copy()
    for j in range(n):
        d = np.real(S[j, j])
        assert d > 0, "ref_cond: not positive definite"
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = S[j + 1:, j] / np.sqrt(d)
        S[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], np.conj(L[j + 1:, j]))
    W = np.zeros((n, n), dtype=CLD)
    for c in range(n):
        W[c, c] = 1 / L[c, c]
        for i in range(c + 1, n):
            W[i, c] = -np.sum(L[i, c:i] * W[c:i, c]) / L[i, i]
    r = n - q
    Lyx, Lyy = L[q:, :q], L[q:, q:]
    H = Lyx @ W[:q, :q] if q else np.zeros((r, 0), dtype=CLD)
    Gc = Lyy @ _ct(Lyy)
    Gc = (Gc + _ct(Gc)) / 2
    dg = np.real(np.diag(A))
    mcoh = np.sum(np.abs(Lyx) ** 2, axis=1) / dg[q:] if r else np.zeros(0, dtype=LD)
    piv = np.real(np.diag(L)) ** 2
    P = _ct(W) @ W
    P = (P + _ct(P)) / 2
    return dict(A=A, L=L, W=W, H=H, Gc=Gc, mcoh=np.asarray(mcoh, dtype=LD), piv=piv, P=P, delta=delta, Gdiag=np.real(np.diag(A)) - delta,
                n=n, q=q, loading=loading)


def bound_of(ref):
    """the derived elementwise bounds of one matrix -> dict H, Gc, mcoh, piv, P (longdouble arrays of the outputs' shapes) and rho"""
    n, q = ref["n"], ref["q"]
    r = n - q
    aL, aW, aH, aP = np.abs(ref["L"]), np.abs(ref["W"]), np.abs(ref["H"]), np.abs(ref["P"])
    LLt = aL @ aL.T
    extra = np.zeros((n, n), dtype=LD)
    if ref["loading"] > 0:
        extra = np.diag(gam(n + 3) * (np.abs(ref["Gdiag"]) + ref["delta"]))
    Ef = cg(n + 1) * LLt + extra
    Es = cg(3 * n + 1) * LLt + extra
    rho = np.max(np.sum(aP @ Es, axis=1))
    infl = 1 / (1 - rho) ** 2
    aPxx = np.abs(_ct(ref["W"][:q, :q]) @ ref["W"][:q, :q]) if q else np.zeros((0, 0), dtype=LD)
    bH = (Es[q:, :q] + aH @ Es[:q, :q]) @ aPxx * infl
    T = np.concatenate((aH, np.eye(r, dtype=LD)), axis=1)                 # [|H|, 1]
    first = T @ Ef @ T.T * infl
    aLyy = aL[q:, q:]
    bGc = first + cg(r + 1) * (aLyy @ aLyy.T)
    bpiv = ref["piv"] * np.array([aW[j] @ Ef @ aW[j] for j in range(n)], dtype=LD) * infl + 2 * U * ref["piv"]
    dg = np.real(np.diag(ref["A"]))
    bm = (np.diag(Ef)[q:] + np.diag(first)) / dg[q:] * infl + gam(2 * q + 4) * ref["mcoh"]
    bP = aP @ Ef @ aP * infl + 2 * cg(n) * (aW.T @ (aW @ aL @ aW)) + cg(n) * (aW.T @ aW)
    bP = np.maximum(bP, bP.T)
    return dict(H=bH, Gc=bGc, mcoh=bm, piv=bpiv, P=bP, rho=rho)


# ---- the kernel's operation order, in float64 ------------------------------------------------------------------------
def restate_cond(G, q, order=None, loading=0.0):
    """one matrix -> dict H, Gc, mcoh, piv, P (float64 / complex128) and status, as k_cond.hip computes them"""
    G = np.asarray(G, dtype=np.complex128)
    n = G.shape[0]
    r = n - q
    order = np.arange(n) if order is None else np.asarray(order)
    A = np.zeros((n, n), dtype=np.complex128)
    for i in range(n):
        for k in range(i + 1):
            oi, ok = order[i], order[k]
            A[i, k] = G[oi, ok] if oi >= ok else np.conj(G[ok, oi])
        A[i, i] = A[i, i].real
    tr = 0.0
    for i in range(n):
        tr += A[i, i].real
    delta = loading * (tr if tr > 0 else 0.0) / n                      # fmax(NaN, 0) = 0
    for i in range(n):
        A[i, i] = A[i, i].real + delta
    dg = np.real(np.diag(A)).copy()
    zero = dict(H=np.zeros((r, q), np.complex128), Gc=np.zeros((r, r), np.complex128), mcoh=np.zeros(r), P=np.zeros((n, n), np.complex128))
    st, piv = 0, np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = A[j, j].real
            if not dj > n * 2.0 ** -52 * dg[j]:
                st = st or j + 1
                if j < q:
                    piv[:j] = np.real(np.diag(A))[:j]
                    return dict(zero, piv=piv, status=st)
                A[j:, j] = 0.0
                continue
            s = np.sqrt(dj)
            A[j + 1:, j] = A[j + 1:, j] / s
            for i in range(j + 1, n):
                A[i, j + 1:i] -= A[i, j] * np.conj(A[j + 1:i, j])
                A[i, i] = A[i, i].real - (A[i, j].real ** 2 + A[i, j].imag ** 2)
        piv = np.real(np.diag(A)).copy()
        mcoh = np.zeros(r)
        for i in range(r):
            sm = 0.0
            for k in range(q):
                sm += A[q + i, k].real ** 2 + A[q + i, k].imag ** 2
            mcoh[i] = sm / dg[q + i] if dg[q + i] > 0 else 0.0
        Gc = np.zeros((r, r), np.complex128)
        for i in range(r):
            for j in range(i + 1):
                sm = 0.0
                for m in range(j):
                    sm = sm + A[q + i, q + m] * np.conj(A[q + j, q + m])
                if i == j:
                    Gc[i, i] = np.real(sm) + A[q + i, q + i].real
                else:
                    Gc[i, j] = sm + A[q + i, q + j] * np.sqrt(A[q + j, q + j].real)
                    Gc[j, i] = np.conj(Gc[i, j])
        P = np.zeros((n, n), np.complex128)
        if st == 0:
            W = np.eye(n, dtype=np.complex128)
            for m in range(n):
                W[m, :m + 1] = W[m, :m + 1] / np.sqrt(A[m, m].real)
                for i in range(m + 1, n):
                    W[i, :m + 1] -= A[i, m] * W[m, :m + 1]
            for i in range(n):
                for j in range(i + 1):
                    sm = 0.0
                    for m in range(i, n):
                        sm = sm + W[m, j] * np.conj(W[m, i])
                    P[i, j] = sm
                    P[j, i] = np.conj(sm)
                P[i, i] = P[i, i].real
        X = A.copy()
        for k in range(q - 1, -1, -1):
            X[q:, k] = X[q:, k] / np.sqrt(A[k, k].real)
            X[q:, :k] -= np.outer(X[q:, k], A[k, :k])
        H = X[q:, :q].copy()
    return dict(H=H, Gc=Gc, mcoh=mcoh, piv=piv, P=P, status=st)


# ---- the case tables ------------------------------------------------------------------------------------------------
GPU_N = (1, 2, 3, 5, 16, 17, 33, 45, 46, 64)
SCALES = (1.0, 1e-6, 1e6)


def q_of(n):
    return sorted({0, 1, n // 2, n - 1, n} & set(range(n + 1)))


def spread_of(n):
    """decades between the largest and the smallest row scale of B: the condition number of B B^H grows by 10^spread.  Small matrices
    reach 1e8 and beyond; the large ones are kept where the derived bound stays under 1e-3 of every output's largest element."""
    return 7.0 if n <= 5 else 5.0 if n <= 17 else 3.0 if n <= 33 else 1.0


def eps_of(n):
    """the floor under the eigenvalues, relative to entries of order n"""
    return 1e-8 if n <= 5 else 1e-6 if n <= 17 else 1e-4 if n <= 33 else 1e-3


def matrices(n, seed, spread=None, eps=None):
    """three seeded matrices B B^H + eps I (B complex n x (n + 2), its rows scaled over `spread` decades) at the scales 1, 1e-6, 1e6
    -> complex128 [3, n, n], exactly Hermitian"""
    rng = np.random.default_rng([n, seed])
    spread = spread_of(n) if spread is None else spread
    eps = eps_of(n) if eps is None else eps
    out = np.zeros((3, n, n), dtype=np.complex128)
    for s, scale in enumerate(SCALES):
        B = rng.standard_normal((n, n + 2)) + 1j * rng.standard_normal((n, n + 2))
        if n > 1:
            B *= (10.0 ** (-0.5 * spread * rng.permutation(n) / (n - 1)))[:, None]
        M = B @ np.conj(B.T) + eps * np.eye(n)
        M = (M + np.conj(M.T)) / 2
        out[s] = M * scale
    return out


def order_of(n, seed):
    return np.random.default_rng([n, seed, 7]).permutation(n).astype(np.int32)


def gpu_cases():
    """(n, q, 'identity' | 'random') for every GPU case against the definition"""
    return [(n, q, kind) for n in GPU_N for q in q_of(n) for kind in ("identity", "random")]


def explained_bound(S, q, Hx, E0=None):
    """The derived bounds of the one output S[q] that is an exact combination Hx of the q inputs S[:q, :q] (positive definite), where the
    full matrix is singular and `bound_of` does not apply: the definition gives H = Hx, mcoh = 1, Gc = 0 exactly, the factor is
    [[L_xx, 0], [Hx L_xx, 0]], and the terms are bound_of's with that factor; E0 [q + 1, q + 1] is what the roundings of forming S itself
    may have moved its elements by, a further perturbation of A -> (bound of H [q], of mcoh, of Gc)"""
    n = q + 1
    ref = ref_cond(S[:q, :q], q)
    aL = np.zeros((n, n), dtype=LD)
    aL[:q, :q] = np.abs(ref["L"])
    aL[q, :q] = np.abs(np.asarray(Hx).astype(CLD) @ ref["L"])
    LLt = aL @ aL.T
    E0 = np.zeros((n, n), dtype=LD) if E0 is None else np.asarray(E0).astype(LD)
    Ef, Es = cg(n + 1) * LLt + E0, cg(3 * n + 1) * LLt + E0
    aP, aH = np.abs(ref["P"]), np.abs(np.asarray(Hx)).astype(LD)
    infl = 1 / (1 - np.max(np.sum(aP @ Es[:q, :q], axis=1))) ** 2
    bH = (Es[q, :q] + aH @ Es[:q, :q]) @ aP * infl
    T = np.concatenate((aH, [LD(1)]))
    bGc = T @ Ef @ T * infl
    bm = (Ef[q, q] + bGc) / np.real(S[q, q]) * infl + gam(2 * q + 4)
    return bH, bm, bGc


def explained_output():
    """five channels whose fourth is an exact combination of the first three, which are orthogonal with norms 2, 4, 8: every step of the
    factorisation is exact in float64, so the fourth pivot is exactly zero -> the matrix [5, 5] and the exact H [2, 3]"""
    Z = np.zeros((5, 6))
    Z[0, 0], Z[1, 1], Z[2, 2] = 2.0, 4.0, 8.0
    Hx = np.array([[2.0, -1.0, 0.5], [0.25, 0.5, 1.0]])
    Z[3:] = Hx @ Z[:3]
    Z[4, 3:] = [1.0, -2.0, 0.5]
    return (Z @ Z.T).astype(np.complex128), Hx.astype(np.complex128)


_CACHE = {}


def case(n, q, kind, seed=0):
    """the matrices, the order, and per matrix the reference and its bound, computed once and shared"""
    key = (n, q, kind, seed)
    if key not in _CACHE:
        G = matrices(n, seed)
        order = None if kind == "identity" else order_of(n, seed)
        refs = [ref_cond(G[s], q, order) for s in range(3)]
        _CACHE[key] = (G, order, refs, [bound_of(x) for x in refs])
    return _CACHE[key]


def share_of(got, refs, bounds, names=WANT):
    """the largest |got - ref| / bound per output over the matrices of a case (0 / 0 counts as 0) -> dict"""
    out = {}
    for name in names:
        worst = 0.0
        for s, (ref, bd) in enumerate(zip(refs, bounds)):
            err = np.abs(np.asarray(got[name][s]).astype(CLD if np.iscomplexobj(ref[name]) else LD) - ref[name])
            if err.size:
                with np.errstate(divide="ignore", invalid="ignore"):
                    sh = np.where(err == 0, LD(0), err / bd[name])
                worst = max(worst, float(np.max(sh)))
        out[name] = worst
    return out


# ---- the end-to-end record -------------------------------------------------------------------------------------------
NSIG, NPERSEG, NX, NY = 1 << 16, 256, 3, 2


def record(seed=1):
    """three coloured, mutually correlated inputs and two outputs formed by FIR filters plus noise -> x [3, 2^16], y [2, 2^16] float64,
    h [2][3] the filters"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((NX, NSIG + 64))
    col = np.stack([np.convolve(src[k], [1.0, 0.5, 0.2], mode="full")[:NSIG + 64] for k in range(NX)])
    mix = np.array([[1.0, 0.35, 0.15], [0.25, 1.0, 0.3], [0.1, 0.3, 1.0]])
    xx = mix @ col
    h = [[rng.standard_normal(8) * np.exp(-0.5 * np.arange(8)) for _ in range(NX)] for _ in range(NY)]
    yy = np.zeros((NY, NSIG + 64))
    for i in range(NY):
        for k in range(NX):
            yy[i] += np.convolve(xx[k], h[i][k], mode="full")[:NSIG + 64]
        yy[i] += 0.3 * np.std(yy[i]) * rng.standard_normal(NSIG + 64)
    return np.ascontiguousarray(xx[:, 64:]), np.ascontiguousarray(yy[:, 64:]), h


def true_response(h, nperseg=NPERSEG):
    """H[nb, ny, nx] of the filters on the bins of rfftfreq(nperseg)"""
    return np.stack([[np.fft.rfft(h[i][k], nperseg) for k in range(NX)] for i in range(NY)]).transpose(2, 0, 1)


def scipy_csd(ch, fs=1.0, nperseg=NPERSEG):
    """G[nb, n, n] = E[X_i conj X_j] of the channels ch[n, nsig] in float64 through scipy.signal.csd: Hann, half overlap, the mean of each
    channel's whole record removed (the library's detrend), a one-sided density"""
    from scipy.signal import csd
    ch = np.asarray(ch, dtype=np.float64)
    ch = ch - ch.mean(axis=1, keepdims=True)
    n = ch.shape[0]
    G = np.zeros((nperseg // 2 + 1, n, n), dtype=np.complex128)
    for i in range(n):
        for j in range(i + 1):
            f, pij = csd(ch[j], ch[i], fs=fs, window="hann", nperseg=nperseg, noverlap=nperseg // 2, detrend=False)   # conj(X_j) X_i
            G[:, i, j] = pij
            G[:, j, i] = np.conj(pij)
    for i in range(n):
        G[:, i, i] = G[:, i, i].real
    return f, G


def outputs_of(G, q, want, order=None):
    """the float64 numpy composition of the wanted outputs for every bin of G[nb, n, n] (the end-to-end reference) -> dict.  Beside the
    kernel's outputs `want` may name what partial_coherence makes of P (q = n): 'pc' = |P_ij|^2 / (P_ii P_jj) and 'mc' = 1 - 1 / (G_ii P_ii)"""
    out = {k: [] for k in want}
    for Gb in G:
        x = restate_cond(Gb, q, order)
        if "pc" in want or "mc" in want:
            d = np.real(np.diag(x["P"]))
            x["pc"] = np.abs(x["P"]) ** 2 / (d[:, None] * d[None, :])
            x["mc"] = 1 - 1 / (np.real(np.diag(Gb)) * d)
        for k in want:
            out[k].append(x[k])
    return {k: np.stack(v) for k, v in out.items()}


def allowance_of(G, q, want, order=None, rel=2e-4, trials=32, seed=5):
    """The end-to-end allowance per output and bin, measured: twice the largest change of any element of the output under `trials` seeded
    Hermitian perturbations of G of relative size `rel` per element (the library's parity figure for the CSD matrix, which it forms
    from float32 spectra) -> dict of float64 [nb]"""
    rng = np.random.default_rng(seed)
    base = outputs_of(G, q, want, order)
    worst = {k: np.zeros(G.shape[0]) for k in want}
    n = G.shape[-1]
    for _ in range(trials):
        z = np.sqrt(rng.uniform(size=G.shape)) * np.exp(2j * np.pi * rng.uniform(size=G.shape))    # uniform in the unit disc
        z = np.tril(z, -1)
        z = z + np.conj(np.swapaxes(z, -1, -2)) + np.eye(n) * rng.uniform(-1, 1, size=(G.shape[0], n, 1))
        now = outputs_of(G * (1 + rel * z), q, want, order)
        for k in want:
            worst[k] = np.maximum(worst[k], np.max(np.abs(now[k] - base[k]).reshape(G.shape[0], -1), axis=1))
    return {k: 2 * v for k, v in worst.items()}


# ---- the calls whose bits this family must not change (tests/golden/cond_before.npz) -------------------------------------
def before_calls(pyfft_amd):
    """one spod call and one ar_ls call on seeded records -> dict of numpy arrays"""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((4, 4096)).astype(np.float32)
    x[1] += 0.5 * x[0]
    out = dict(zip(("spod_f", "spod_lam", "spod_phi"), pyfft_amd.spod(x, fs=2.0, nperseg=64, nmodes=2)))
    out.update(zip(("ls_a", "ls_e", "ls_status"), pyfft_amd.engine.ar_ls(x[:2, :1024], 256, 128, 0, 7, 6, fb=True)))
    return {k: np.asarray(v) for k, v in out.items()}
