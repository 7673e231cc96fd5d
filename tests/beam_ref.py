"""float64 definitions, derived bounds and case tables of the array scan (k_beam.hip; include/spectral_array.h), numpy only: the phase rule
with its separate roundings, the four estimators from (w, V), a bound per output without a measured term, the end-to-end records
("ring": a Mirnov-coil ring with uneven coils, "line": a probe rake resolving two waves half a Rayleigh width apart) and their all-float64
chain from the raw record."""
import numpy as np

U = 2.0 ** -53
MARGIN = 4.0
MIN_GAP = 50.0
TQ, KS, WAVES, MAX_M = 64, 32, 8, 64          # beam_plan.h
METHODS = ("bartlett", "capon", "music", "ev")
CSDM_PARITY = 2e-4                             # engine.csd_matrix against float64, relative to a bin's largest element


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def _table(t):
    t = np.asarray(t, dtype=np.float64)
    return t.reshape(-1, 1) if t.ndim == 1 else t


def phase_def(pos, kv, scale=1.0):
    """fr[q, i] in [0, 1]: t = pos[i][0] kv[q][0]; t = t + pos[i][1] kv[q][1]; ..; phi = scale t; fr = phi - floor(phi).  numpy rounds every
    product and every sum on its own, as the kernel's __dmul_rn / __dadd_rn do: the kernel's fr has these bits"""
    pos, kv = _table(pos), _table(kv)
    t = kv[:, 0][:, None] * pos[:, 0][None, :]
    for d in range(1, pos.shape[1]):
        t = t + kv[:, d][:, None] * pos[:, d][None, :]
    ph = np.float64(scale) * t
    return ph - np.floor(ph)


def steer_def(pos, kv, scale=1.0):
    """a[q, i] = (cos 2 pi fr, sin 2 pi fr); fr - round(fr) is exact, so the argument of exp is at most pi"""
    fr = phase_def(pos, kv, scale)
    return np.exp(2j * np.pi * (fr - np.round(fr)))


def first_vector(method, p):
    return p if method in ("music", "ev") else 0


def delta_def(w, loading):
    """loading max(sum_k w_k, 0) / m, the sum in k ascending, as the kernel forms it"""
    tr = np.float64(w[0])
    for x in w[1:]:
        tr = tr + np.float64(x)
    return np.float64(loading) * max(tr, np.float64(0.0)) / np.float64(len(w))


def weights_def(w, method, p, loading):
    """(g[k >= first], status)"""
    w = np.asarray(w, dtype=np.float64)
    k0 = first_vector(method, p)
    wk = w[k0:]
    if method == "bartlett":
        return wk.copy(), 0
    if method == "music":
        return np.ones(len(wk)), 0
    den = wk + delta_def(w, loading) if method == "capon" else wk
    ok = den > 0
    return np.where(ok, 1.0 / np.where(ok, den, 1.0), 0.0), int(np.any(~ok))


def beam_def(V, w, pos, kv, method, p=0, loading=0.0, scale=1.0):
    """(P float64 [nk], status) of one model: D = sum_k g_k |a_q^H v_k|^2; D / m^2 for Bartlett, 1 / D otherwise (0 where D is 0)"""
    V, w = np.asarray(V, dtype=np.complex128), np.asarray(w, dtype=np.float64)
    m = V.shape[0]
    g, st = weights_def(w, method, p, loading)
    S2 = np.abs(np.conj(steer_def(pos, kv, scale)) @ V[:, first_vector(method, p):]) ** 2
    D = S2 @ g
    if method == "bartlett":
        return D / (m * m), st
    return np.where(D > 0, 1.0 / np.where(D > 0, D, 1.0), 0.0), st


SINCOS_U = 16.0   # |a_kernel - a_here| in units of u: sincospi to 2 ulp a component (4 u, 5.7 u for the pair) and here the product 2 pi fr (pi u),
#                   pi itself (pi u / 2 at the most) and exp to 1 ulp a component (2.9 u for the pair): 13.3 u, rounded up


def beam_bound(V, w, pos, kv, method, p=0, loading=0.0, scale=1.0):
    """absolute, per output, between the kernel and beam_def; no measured term.
      a projection S_k = sum_i conj(a_i) v_ik of m terms in float64 (complex products and sums, fused or not) is off by
        (m + 2) sqrt 2 u sum_i |v_ik| <= 2 (m + 2) u l1_k at the most, here and there, and by SINCOS_U u l1_k for the two steering vectors:
        dS_k = (4 (m + 2) + SINCOS_U) u l1_k;
      |S_k|^2 by 2 |S_k| dS_k + dS_k^2 + 3 u |S_k|^2 (two squares and a sum) each side;
      a weight g_k = 1 / (w_k + delta) by 3 u g_k (sum, reciprocal, product with |S|^2) and by what delta is off, (m + 2) u loading sum |w| / m
        over w_k + delta, each side; g_k = w_k and g_k = 1 are exact;
      the sum over the nv vectors in any order (the kernel: within a wave, then over WAVES partial sums) by (nv + WAVES) u sum |g_k| |S_k|^2
        each side;
      the last step (a division by m^2, or a reciprocal) by u P each side; 1 / D moves by dD / D^2 / (1 - dD / D)."""
    V, w = np.asarray(V, dtype=np.complex128), np.asarray(w, dtype=np.float64)
    m = V.shape[0]
    k0 = first_vector(method, p)
    g, _ = weights_def(w, method, p, loading)
    S = np.abs(np.conj(steer_def(pos, kv, scale)) @ V[:, k0:])
    l1 = np.sum(np.abs(V[:, k0:]), axis=0)
    dS = (4.0 * (m + 2) + SINCOS_U) * U * l1
    dS2 = 2.0 * (2.0 * S * dS + dS ** 2 + 3.0 * U * S ** 2)
    grel = np.zeros(len(g))
    if method in ("capon", "ev"):
        grel = np.full(len(g), 2.0 * 3.0 * U)
    if method == "capon" and loading > 0:
        ddelta = (m + 2) * U * loading * np.sum(np.abs(w)) / m
        grel = grel + 2.0 * ddelta * np.abs(g)
    ag = np.abs(g)
    T = (S ** 2) @ ag
    dD = dS2 @ ag + (S ** 2) @ (ag * grel) + 2.0 * (len(g) + WAVES) * U * T
    D = (S ** 2) @ g
    if method == "bartlett":
        return dD / (m * m) + 2.0 * U * np.abs(D) / (m * m)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(D > 0, dD / D, 0.0)
        assert np.all(rel < 0.5), "the bound has no meaning where the sum is lost in its own rounding"
        return np.where(D > 0, (rel / (1.0 - rel) + 2.0 * U) / np.where(D > 0, D, 1.0), 0.0)


# ---- the cases of the GPU test -----------------------------------------------------------------------------------------------------------
DEF_M = (2, 23, 64)
SCALES = (1.0, 0.37, 2.5)                       # three models, three scales
LOADINGS = (0.0, 1e-3)
FAR = 1e6 + 0.37
# (nk, ndim, far): every nk around a tile of TQ, more than one tile with a tail, every ndim, two with the phase 1e6 turns out
GEOMS = ((1, 1, False), (TQ - 1, 2, False), (TQ, 3, False), (TQ + 1, 1, False), (300, 2, False), (300, 3, False), (5, 1, True), (TQ + 1, 3, True))


def variants(m):
    """(method, p, loading) of the definition test: every method, p in {0, 2, m - 1} where it counts, both loadings for Capon"""
    ps = sorted({0, min(2, m - 1), m - 1})
    return [("bartlett", 0, 0.0)] + [("capon", 0, l) for l in LOADINGS] + [(me, p, 0.0) for me in ("music", "ev") for p in ps]


_eig = {}


def eig_of(m, nmodels=3):
    """(w [nmodels, m] descending, V [nmodels, m, m]) by numpy's eigh of fixed positive definite Hermitian matrices, computed once"""
    if m not in _eig:
        rng = np.random.default_rng(1000 + m)
        ws, Vs = [], []
        for s in range(nmodels):
            A = rng.standard_normal((m, 3 * m)) + 1j * rng.standard_normal((m, 3 * m))
            A[:, :2] *= 10.0 * (s + 1)                                   # two strong directions: a gap, as an array's matrix has
            C = A @ np.conj(A.T) / (3 * m)
            w, V = np.linalg.eigh(C)
            ws.append(w[::-1].copy()), Vs.append(V[:, ::-1].copy())
        _eig[m] = (np.stack(ws), np.stack(Vs))
    return _eig[m]


def geometry(m, nk, ndim, far, seed=0):
    """pos [m, ndim] uneven within a few units, kv [nk, ndim] within +- 1 turn per unit (offset by FAR turns per unit for `far`)"""
    rng = np.random.default_rng(50 + 7 * m + nk + 100 * ndim + seed)
    pos = np.arange(m)[:, None] * np.array([1.0, 0.31, -0.17])[None, :ndim] + 0.3 * rng.uniform(-1, 1, (m, ndim))
    kv = rng.uniform(-1, 1, (nk, ndim))
    if far:
        kv = kv + FAR
    return pos, kv


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
NSIG, NPERSEG = 1 << 14, 256
E2E = {
    # sensors, jitter, bin, (mode or wavenumber in cycles per unit, amplitude) of two independent narrow-band processes, noise, seed
    "ring": dict(m=16, jitter=0.35, bin=32, f=0.125, noise=0.05, amps=(1.0, 0.5), seed=11),
    "line": dict(m=12, jitter=0.30, bin=51, f=0.2, noise=0.03, amps=(1.0, 1.0), seed=23),
}
RING_MODES = np.arange(-8, 8)
RING_TRUE = (2, -3)
LINE_GRID = np.linspace(-0.5, 0.5, 1025)        # cycles per unit of position
LINE_K1 = 0.1


def sensors(case):
    c = E2E[case]
    rng = np.random.default_rng(c["seed"])
    j = rng.uniform(-c["jitter"], c["jitter"], c["m"])
    if case == "ring":
        return 2.0 * np.pi * (np.arange(c["m"]) + j) / c["m"]            # angles
    return np.arange(c["m"]) + j


def truth(case):
    """the two sources' k in radians per unit of position (mode numbers for the ring)"""
    if case == "ring":
        return np.array(RING_TRUE, dtype=np.float64)
    r = sensors(case)
    return 2.0 * np.pi * np.array([LINE_K1, LINE_K1 + 0.5 / (r.max() - r.min())])


def scan(case):
    """k of the scan in radians per unit"""
    return RING_MODES.astype(np.float64) if case == "ring" else 2.0 * np.pi * LINE_GRID


_rec = {}


def record(case):
    """x float32 [m, NSIG]: sum_j Re(A_j(t) exp(i (2 pi f t - k_j r_i))) + noise, A_j independent complex envelopes (white noise under a
    64-sample running mean, unit mean square) times the amplitudes"""
    if case not in _rec:
        c = E2E[case]
        rng = np.random.default_rng(c["seed"] + 1)
        r, t = sensors(case), np.arange(NSIG)
        x = c["noise"] * rng.standard_normal((c["m"], NSIG))
        for kj, amp in zip(truth(case), c["amps"]):
            e = rng.standard_normal(NSIG + 63) + 1j * rng.standard_normal(NSIG + 63)
            A = np.convolve(e, np.ones(64), mode="valid")
            A *= amp / np.sqrt(np.mean(np.abs(A) ** 2))
            x = x + np.real(A[None, :] * np.exp(1j * (2.0 * np.pi * c["f"] * t[None, :] - kj * r[:, None])))
        _rec[case] = x.astype(np.float32)
    return _rec[case]


def csd_def(x, win, fs=1.0):
    """G [nb, m, m] in float64 as beamform.array_spectrum scales it: Welch with half overlap, each channel's whole-record mean removed,
    1 / (fs sum w^2), interior bins doubled; G[b][i, j] = mean over the segments of X_i conj(X_j)"""
    x = np.asarray(x, dtype=np.float64)
    x = x - x.mean(axis=1, keepdims=True)
    n = len(win)
    hop = n // 2
    nf = 1 + (x.shape[1] - n) // hop
    G = np.zeros((n // 2 + 1, x.shape[0], x.shape[0]), dtype=np.complex128)
    for g in range(nf):
        X = np.fft.rfft(x[:, g * hop:g * hop + n] * win[None, :], axis=1).T          # [nb, m]
        G += X[:, :, None] * np.conj(X[:, None, :])
    G *= 1.0 / (nf * fs * np.sum(win * win))
    G[1:(n - 1) // 2 + 1] *= 2.0
    return G


def eigh_desc(C):
    w, V = np.linalg.eigh(C)
    return w[::-1].copy(), V[:, ::-1].copy()


_g = {}


def e2e_matrix(case, win):
    """the float64 CSD matrix of the case's bin, and its eigendecomposition"""
    if case not in _g:
        G = csd_def(record(case), win)[E2E[case]["bin"]]
        _g[case] = (G,) + eigh_desc(G)
    return _g[case]


def e2e_reference(case, method, win, G=None):
    Gm, w, V = e2e_matrix(case, win)
    if G is not None:
        w, V = eigh_desc(G)
    return beam_def(V, w, sensors(case), -scan(case) / (2.0 * np.pi), method, 2, 0.0)[0]


def perturbation_change(case, method, win, trials=8):
    """the worst relative change of the reference over `trials` Hermitian perturbations of G of 2-norm CSDM_PARITY ||G||_2"""
    G, w, V = e2e_matrix(case, win)
    P = e2e_reference(case, method, win)
    rng = np.random.default_rng(77)
    worst = 0.0
    for _ in range(trials):
        H = rng.standard_normal(G.shape) + 1j * rng.standard_normal(G.shape)
        H = H + np.conj(H.T)
        H *= CSDM_PARITY * np.linalg.norm(G, 2) / np.linalg.norm(H, 2)
        P2 = e2e_reference(case, method, win, G + H)
        worst = max(worst, float(np.max(np.abs(P2 - P) / P)))
    return worst


def peak_bins(P, n):
    """the grid indices of the n largest local maxima of P (the ends count), largest first"""
    P = np.asarray(P, dtype=np.float64)
    left = np.concatenate(([True], P[1:] > P[:-1]))
    right = np.concatenate((P[:-1] >= P[1:], [True]))
    loc = np.flatnonzero(left & right)
    return loc[np.argsort(-P[loc], kind="stable")][:n]


def nearest(case):
    """the grid indices nearest to the two true sources"""
    return [int(np.argmin(np.abs(scan(case) - k))) for k in truth(case)]


# ---- measured on the CPU (tests/test_host_beam.py holds each to within a factor of two and reprints it) ----------------------------------
# the worst relative change of the reference under the perturbation above, per case and method
E2E_PERT = {
    ("ring", "capon"): 40.7, ("ring", "music"): 0.0908, ("ring", "ev"): 40.7,
    ("line", "capon"): 240.0, ("line", "music"): 0.0527, ("line", "ev"): 240.0,
}
# (Capon and EV weigh every vector by 1 / w_k: a perturbation of 2e-4 of the largest eigenvalue is a third of the noise eigenvalues at a gap
# of 1500 and more than the smallest of them, so between the peaks these two move by many times their value; MUSIC does not look at w.)


def e2e_allowance(case, method):
    return MARGIN * E2E_PERT[(case, method)]
