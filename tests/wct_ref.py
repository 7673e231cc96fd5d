"""Float64 reference of the cross-wavelet transform and the wavelet coherence (numpy), written from the definitions on top of
tests/cwt_ref.py.  Scales s' in samples, Morlet(w0) for the coherence:
    Wx, Wy   = cwt_ref (a linear convolution of the zero-extended records)
    Wxy      = Wx conj(Wy)                                             (no normalisation by the records' standard deviations)
    a, b, c  = |Wx|^2 / s', |Wy|^2 / s', Wxy / s' for 0 <= n < N, zero outside
    time     a linear convolution along n with the kernel whose DFT is exp(-(s' w_k)^2 / 2), w_k = 2 pi k / L for k <= L / 2 and
             2 pi (k - L) / L above: a unit-gain Gaussian of standard deviation s' samples; nothing wraps (the grid is
             next_pow2(max(2 N, N + 9 s'max)): at 9 standard deviations the Gaussian is below 3e-18 of its peak)
    scale    scipy.signal.convolve2d(., win[:, None], 'same'), win = ones of length round(2 dj0 / dj) + 2 with both ends 0.5, sum 1
    R2 = |C|^2 / (A B), phase = atan2(Im C, Re C), both 0 where A B == 0
Also the restatement of the overlap-save plan the device runs, at float64 and at float32 (complex64 transforms, the filter and the
Gaussian from float32 constants as the kernel forms them), the pair of records the tests share, and the checker."""
import math

import numpy as np

import cwt_ref as R


def scale_window(dj, dj0=0.6):
    win = np.ones(int(round(2.0 * dj0 / dj)) + 2)
    win[0] = win[-1] = 0.5
    return win / win.sum()


def gauss_rows(scales, L):
    s = np.asarray(scales, dtype=np.float64)[:, None]
    k = np.arange(L)
    w = 2 * math.pi * np.where(k <= L // 2, k, k - L) / L
    return np.exp(-0.5 * (s * w[None, :]) ** 2)


def smooth_margin_ref(s, tail=1e-6, grid=1 << 18):
    a = np.abs(np.fft.ifft(gauss_rows([s], grid)[0]))
    d = a[:grid // 2 + 1].copy()
    d[1:grid // 2] += a[:grid // 2:-1]
    tails = np.cumsum(d[::-1])[::-1]
    ok = np.nonzero(tails <= tail * a.sum())[0]
    return int(ok[0]) if ok.size else grid // 2 + 1


def make_pair(n, cplx=False, seed=0):
    """x = cwt_ref.make_signal; y = independent noise of std 0.5, the line of x at f = 0.037 (0.9 rad later) and a slow chirp that
    crosses x's line at 0.0091 in the middle of the record.  (The chirp is narrow, 0.95 .. 1.05 of that frequency: a wide one raises
    the row means of the scales it sweeps far above the stretches it has left, and the noise-only stretches of |Wy|^2 then fall
    below assert_conditioned's floor.)"""
    x = R.make_signal(n, cplx, seed)
    rng = np.random.default_rng(seed + 7919)
    t = np.arange(n)
    y = 0.5 * rng.standard_normal(n)
    y = y + 0.8 * np.cos(2 * math.pi * 0.037 * t + 10 * 0.037 + 0.9)
    f0 = 0.0091
    y = y + 0.5 * np.cos(2 * math.pi * f0 * (0.95 * t + 0.05 * t * t / n))         # frequency 0.95 f0 .. 1.05 f0
    if cplx:
        yi = 0.5 * rng.standard_normal(n) + 0.6 * np.sin(2 * math.pi * 0.05 * t + 0.15 + 0.4)
        return x, (y + 1j * yi).astype(np.complex64)
    return x, y.astype(np.float32)


def products(Wx, Wy, scales):
    """-> P [S, N, 3] complex: a, b (real) and c"""
    inv = 1.0 / np.asarray(scales, dtype=np.float64)[:, None]
    return np.stack([np.abs(Wx) ** 2 * inv + 0j, np.abs(Wy) ** 2 * inv + 0j, Wx * np.conj(Wy) * inv], axis=-1)


def smooth_time(P, scales):
    """P [S, N, ...] -> the same shape, every row convolved along n with its Gaussian"""
    n = P.shape[1]
    L = R.next_pow2(max(2 * n, n + int(math.ceil(9 * float(np.max(scales))))))
    G = gauss_rows(scales, L)
    G = G.reshape(G.shape + (1,) * (P.ndim - 2))
    return np.fft.ifft(np.fft.fft(P, L, axis=1) * G, axis=1)[:, :n]


def smooth_scale(T, win):
    """scipy.signal.convolve2d(., win[:, None], 'same') over the first axis of T [S, N, ...]"""
    import scipy.signal as ss
    flat = T.reshape(T.shape[0], -1)
    return ss.convolve2d(flat, np.asarray(win, dtype=np.float64)[:, None], "same").reshape(T.shape)


def coherence(A, B, C):
    den = A * B
    ok = den != 0
    R2 = np.where(ok, np.abs(C) ** 2 / np.where(ok, den, 1.0), 0.0)
    return R2, np.where(ok, np.arctan2(C.imag, C.real), 0.0)


def xwt_ref(x, y, scales, family="morlet", param=6.0):
    return R.cwt_ref(x, scales, family, param) * np.conj(R.cwt_ref(y, scales, family, param))


def as_T(P):
    """[S, N, 3] complex (a, b, c) -> [S, N, 4] float64 (A, B, Re C, Im C)"""
    return np.stack([P[..., 0].real, P[..., 1].real, P[..., 2].real, P[..., 2].imag], axis=-1)


def finish(T, win):
    """T [S, N, 4] -> dict(T, A, B, C, R2, phase)"""
    D = smooth_scale(T, win)
    A, B, C = D[..., 0], D[..., 1], D[..., 2] + 1j * D[..., 3]
    R2, phase = coherence(A, B, C)
    return dict(T=T, A=A, B=B, C=C, R2=R2, phase=phase)


def wct_ref(x, y, scales, w0=6.0, dj=1.0 / 12, dj0=0.6, n_full=None):
    """-> dict: T [S, N, 4] (the time-smoothed A_t, B_t, Re C_t, Im C_t), A, B, C, R2, phase [S, N]; float64 (n_full: cwt_ref's grid)"""
    Wx, Wy = R.cwt_ref(x, scales, "morlet", w0, n_full), R.cwt_ref(y, scales, "morlet", w0, n_full)
    return finish(as_T(smooth_time(products(Wx, Wy, scales), scales)), scale_window(dj, dj0))


def filters_f32(scales, w0, L):
    """Morlet's H_s as k_cwt and k_wct_time form it: exp(c - d^2 / 2), d = k step - w0, from float32 constants (1 / L left to the
    inverse transform)"""
    sc = np.asarray(scales, dtype=np.float64)
    k = np.arange(L, dtype=np.float32)
    step = (2 * math.pi * sc / L).astype(np.float32)[:, None]
    c = (-0.25 * math.log(math.pi) + 0.5 * np.log(2 * math.pi * sc)).astype(np.float32)[:, None]
    d = k[None, :] * step - np.float32(w0)
    H = np.exp(c - np.float32(0.5) * d * d).astype(np.float32)
    kk = np.arange(L)
    H[:, (kk < 1) | (kk > L // 2)] = 0
    return H


def gauss_f32(scales, L):
    sc = np.asarray(scales, dtype=np.float64)
    k = np.arange(L)
    kk = np.where(k <= L // 2, k, k - L).astype(np.float32)
    u = kk[None, :] * (2 * math.pi * sc / L).astype(np.float32)[:, None]
    return np.exp(np.float32(-0.5) * u * u).astype(np.float32)


def overlap_save(x, y, scales, w0, L, Mw, Mg, dtype=np.float64, xwt=False):
    """The device's plan restated in numpy at `dtype`: frame g = the L samples from g hop - M on, M = Mw + Mg, zero outside the
    records; two forward transforms, per scale two filtered inverse transforms, the products masked to the record, and for a + i b and
    c a forward transform, the Gaussian and an inverse transform; the elements M .. M + hop - 1 are the samples g hop .. < N.
    -> T [S, N, 4], or Wxy [S, N] with xwt=True (then Mg = 0 and nothing is smoothed)."""
    import scipy.fft as sf
    x, y = np.asarray(x), np.asarray(y)
    n = x.shape[-1]
    M = Mw + Mg
    hop = L - 2 * M
    frames = -(-n // hop)
    f64 = dtype == np.float64
    ctype, rtype = (np.complex128, np.float64) if f64 else (np.complex64, np.float32)
    S = len(scales)
    H = R.filters("morlet", w0, scales, L) if f64 else filters_f32(scales, w0, L)
    G = gauss_rows(scales, L) if f64 else gauss_f32(scales, L)
    inv = (1.0 / np.asarray(scales, dtype=np.float64)).astype(rtype)[:, None]
    out = np.zeros((S, n), dtype=ctype) if xwt else np.zeros((S, n, 4), dtype=rtype)
    xp, yp = np.zeros(M + frames * hop + L, dtype=ctype), np.zeros(M + frames * hop + L, dtype=ctype)
    xp[M:M + n], yp[M:M + n] = x, y
    for g in range(frames):
        X, Y = sf.fft(xp[g * hop:g * hop + L]), sf.fft(yp[g * hop:g * hop + L])
        Wx, Wy = sf.ifft((X[None, :] * H).astype(ctype), axis=-1), sf.ifft((Y[None, :] * H).astype(ctype), axis=-1)
        n1 = min(n, (g + 1) * hop)
        own = slice(M, M + n1 - g * hop)
        if xwt:
            out[:, g * hop:n1] = (Wx * np.conj(Wy))[:, own]
            continue
        nn = g * hop - M + np.arange(L)
        m = ((nn >= 0) & (nn < n)).astype(rtype)[None, :] * inv
        a = (Wx.real * Wx.real + Wx.imag * Wx.imag) * m
        b = (Wy.real * Wy.real + Wy.imag * Wy.imag) * m
        p1 = (a + 1j * b).astype(ctype)
        p2 = ((Wx * np.conj(Wy)) * m).astype(ctype)
        q1 = sf.ifft((sf.fft(p1, axis=-1) * G).astype(ctype), axis=-1)
        q2 = sf.ifft((sf.fft(p2, axis=-1) * G).astype(ctype), axis=-1)
        out[:, g * hop:n1, 0], out[:, g * hop:n1, 1] = q1.real[:, own], q1.imag[:, own]
        out[:, g * hop:n1, 2], out[:, g * hop:n1, 3] = q2.real[:, own], q2.imag[:, own]
    return out


def composed_f32(x, y, scales, w0, n_smooth):
    """The whole-record path restated at float32: cwt_ref.composed_f32 for Wx and Wy, the products in float32, the Gaussian as float32
    rows on a grid of n_smooth points, complex64 transforms -> T [S, N, 4] float32."""
    import scipy.fft as sf
    n = np.asarray(x).shape[-1]
    Wx, Wy = R.composed_f32(x, scales, "morlet", w0), R.composed_f32(y, scales, "morlet", w0)
    inv = (1.0 / np.asarray(scales, dtype=np.float64)).astype(np.float32)[:, None]
    p1 = ((Wx.real ** 2 + Wx.imag ** 2) * inv + 1j * ((Wy.real ** 2 + Wy.imag ** 2) * inv)).astype(np.complex64)
    p2 = (Wx * np.conj(Wy) * inv).astype(np.complex64)
    G = gauss_rows(scales, n_smooth).astype(np.float32)
    out = np.zeros((len(scales), n, 4), dtype=np.float32)
    for j, p in ((0, p1), (2, p2)):
        pp = np.zeros((len(scales), n_smooth), dtype=np.complex64)
        pp[:, :n] = p
        q = sf.ifft((sf.fft(pp, axis=-1) * G).astype(np.complex64), axis=-1)[:, :n]
        out[..., j], out[..., j + 1] = q.real, q.imag
    return out


def smooth_scale_f32(T, win):
    """k_wct_scale restated: float32, the rows added in ascending order, rows outside the set skipped"""
    T = np.asarray(T, dtype=np.float32)
    w = np.asarray(win, dtype=np.float32)
    K, S = len(w), T.shape[0]
    out = np.zeros_like(T)
    for s in range(S):
        for j in range(K):
            r = s - K // 2 + j
            if 0 <= r < S:
                out[s] = out[s] + w[K - 1 - j] * T[r]
    return out


def row_err(got, ref):
    """max |got - ref| over the row's rms of ref, per scale row (everything behind the first axis is the row) -> the worst"""
    got, ref = np.asarray(got), np.asarray(ref)
    S = ref.shape[0]
    g, r = got.reshape(S, -1), ref.reshape(S, -1)
    return float(np.max(np.max(np.abs(g - r), axis=-1) / np.sqrt(np.mean(np.abs(r) ** 2, axis=-1))))


def component_errs(got, ref):
    """row_err of A, B and C apart, from arrays [S, N, 4] -> (eA, eB, eC)"""
    got, ref = np.asarray(got), np.asarray(ref)
    return (row_err(got[..., 0], ref[..., 0]), row_err(got[..., 1], ref[..., 1]),
            row_err(got[..., 2] + 1j * got[..., 3], ref[..., 2] + 1j * ref[..., 3]))


FLOOR = 0.05


def assert_conditioned(ref):
    """A condition on the INPUTS: the reference's smoothed auto-spectra stay above FLOOR of their row mean everywhere, so that the
    ratio is well conditioned at every point.  Nothing is excluded from a comparison on its account."""
    for k in ("A", "B"):
        lo = float(np.min(ref[k] / np.mean(ref[k], axis=-1, keepdims=True)))
        assert lo >= FLOOR, "%s falls to %.3g of its row mean: these records do not condition the ratio" % (k, lo)


def r2_bound(ref, eps2):
    """The bound on |R2 - R2ref| per scale row that follows from errors of at most eps2 (of the row rms) in A, B and C: with
    delta = eps2 max over the row of (row rms / local value) for A, B and C against sqrt(A B),
        |C|^2 is off by at most (2 delta + delta^2) A B  (|C| <= sqrt(A B)), A B by at most (2 delta + delta^2) A B,
    and R2 <= 1 moves by at most 4 delta + delta^2 -> (bound [S, 1], delta [S, 1])."""
    A, B = ref["A"], ref["B"]
    rms = lambda v: np.sqrt(np.mean(np.abs(v) ** 2, axis=-1, keepdims=True))       # noqa: E731
    worst = lambda v: np.max(v, axis=-1, keepdims=True)                            # noqa: E731
    delta = eps2 * np.maximum(np.maximum(worst(rms(A) / A), worst(rms(B) / B)), worst(rms(ref["C"]) / np.sqrt(A * B)))
    return 4 * delta + delta * delta, delta


def check(got, ref, eps2, what, spectra=True):
    """got: dict with R2, phase and (spectra) A, B, C or T; held to eps2 of the row rms (spectra) and to r2_bound (R2).  The phase is held
    where it is defined to that accuracy: an error of eps2 rms_C in C turns it by at most asin(eps2 rms_C / |C|), compared modulo
    2 pi; points with |C| below 2 eps2 rms_C carry no phase and are only required to be finite.  Prints every figure."""
    assert_conditioned(ref)
    bound, delta = r2_bound(ref, eps2)
    if spectra:
        for k in ("A", "B", "C"):
            e = row_err(got[k], ref[k])
            print("%s %s: %.3g of the row rms (bound %.3g)" % (what, k, e, eps2))
            assert np.all(np.isfinite(got[k])) and e <= eps2, (what, k, e, eps2)
    e = np.max(np.abs(got["R2"] - ref["R2"]), axis=-1, keepdims=True)
    print("%s R2: off by %.3g at most, %.3g of its row's bound at worst (bounds %.3g .. %.3g); R2 spans %.3g .. %.3g"
          % (what, e.max(), (e / bound).max(), bound.min(), bound.max(), ref["R2"].min(), ref["R2"].max()))
    assert np.all(np.isfinite(got["R2"])) and np.all(e <= bound), (what, float((e / bound).max()))
    C = ref["C"]
    rel = eps2 * np.sqrt(np.mean(np.abs(C) ** 2, axis=-1, keepdims=True)) / np.maximum(np.abs(C), 1e-300)
    held = rel < 0.5
    dphi = np.abs(np.angle(np.exp(1j * (np.asarray(got["phase"], dtype=np.float64) - ref["phase"]))))
    pb = np.arcsin(np.minimum(rel, 0.5)) + 1e-6                                    # (+ float32 atan2 and the rounding of pi)
    print("%s phase: %.3g of its bound at worst, %d of %d points held" % (what, float(np.max((dphi / pb)[held])), int(held.sum()), held.size))
    assert np.all(np.isfinite(got["phase"])) and np.all(dphi[held] <= pb[held]), what
