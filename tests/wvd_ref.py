"""The smoothed pseudo Wigner-Ville distribution restated in numpy, the shapes of tests/test_gpu_wvd.py and the allowance they hold the
kernel to.  A helper module, not a test: nothing here is collected.

The definition (include/spectral_quad.h): z and y complex rows that are zero outside 0 .. nsig - 1, h a lag window of 2 Lh + 1 taps,
g a time window of 2 Lg + 1 taps, both odd, centred and indexed from -L; the column times n_j = first + j hop:

    K[j][tau] = h[tau] sum_mu g[mu] z[n_j + mu + tau] conj(y[n_j + mu - tau]),   tau = -Lh .. Lh, 0 for the other lags
    W[j][k]   = scale sum_tau K[j][tau] exp(-2 pi i k tau / nfft)

wvd_ref is that in float64, vectorised over tau and mu (one Python loop, over the columns); wvd_ref32 is the same in float32: float32
inputs, products and sums, then numpy's transform of the complex64 K.

The allowance.  F32_DEV is the largest deviation of wvd_ref32 from wvd_ref over SHAPES, per column and relative to that column's largest
|W|, as measured by tests/test_host_wvd.py (which prints it and asserts it against the constant).  The kernel gets that figure times a
margin of 4 -- a different but legal summation order and the transform's own rounding -- which must stay below the project's parity
figure of 2e-4, plus an absolute term of 1e-6 of the call's largest cell for the columns in the zero padding."""
import functools

import numpy as np

F32_DEV = 1.5e-7          # measured 1.31e-7 (test_float32_restatement_deviation; numpy's complex64 transform is single precision)
MARGIN = 4.0
PARITY = 2e-4
ABS_TERM = 1e-6
ALLOWANCE = MARGIN * F32_DEV


def _gather(a, idx):
    """a[idx] with zeros outside the row"""
    ok = (idx >= 0) & (idx < a.shape[0])
    return np.where(ok, a[np.clip(idx, 0, a.shape[0] - 1)], 0)


def _wvd(z, y, h, g, hop, first, ntimes, nfft, scale, ct, ft):
    z = np.asarray(z).astype(ct)
    y = z if y is None else np.asarray(y).astype(ct)
    h, g = np.asarray(h).astype(ft), np.asarray(g).astype(ft)
    Lh, Lg = h.size // 2, g.size // 2
    assert h.size == 2 * Lh + 1 and g.size == 2 * Lg + 1 and h.size <= nfft - 1
    tau, mu = np.arange(-Lh, Lh + 1)[None, :], np.arange(-Lg, Lg + 1)[:, None]
    W = np.zeros((ntimes, nfft), dtype=ct)
    for j in range(ntimes):
        n = first + j * hop
        prod = (_gather(z, n + mu + tau) * np.conj(_gather(y, n + mu - tau))).astype(ct)
        K = (h * np.sum((g[:, None] * prod).astype(ct), axis=0, dtype=ct)).astype(ct)
        img = np.zeros(nfft, dtype=ct)
        img[tau[0] % nfft] = K
        W[j] = ft(scale) * np.fft.fft(img)
    return W


def wvd_ref(z, h, g, hop, first, ntimes, nfft, y=None, scale=1.0):
    """float64 -> complex128 [ntimes, nfft] (the auto distribution of a symmetric h is real up to rounding: take .real)"""
    return _wvd(z, y, h, g, hop, first, ntimes, nfft, scale, np.complex128, np.float64)


def wvd_ref32(z, h, g, hop, first, ntimes, nfft, y=None, scale=1.0):
    """the same with float32 inputs, products and sums and numpy's transform of the complex64 K"""
    return _wvd(z, y, h, g, hop, first, ntimes, nfft, scale, np.complex64, np.float32)


def wvd_loops(z, h, g, hop, first, ntimes, nfft, y=None, scale=1.0):
    """the definition as a plain triple loop with a direct transform (tiny shapes only)"""
    z = np.asarray(z, dtype=np.complex128)
    y = z if y is None else np.asarray(y, dtype=np.complex128)
    Lh, Lg = len(h) // 2, len(g) // 2
    at = lambda a, i: a[i] if 0 <= i < len(a) else 0.0
    W = np.zeros((ntimes, nfft), dtype=np.complex128)
    for j in range(ntimes):
        n = first + j * hop
        for tau in range(-Lh, Lh + 1):
            k = 0.0
            for mu in range(-Lg, Lg + 1):
                k += g[mu + Lg] * at(z, n + mu + tau) * np.conj(at(y, n + mu - tau))
            W[j] += scale * h[tau + Lh] * k * np.exp(-2j * np.pi * np.arange(nfft) * tau / nfft)
    return W


def hamming(n):
    """the symmetric Hamming window of n taps (n odd: centred)"""
    return np.hamming(n) if n > 1 else np.ones(1)


def column_error(got, ref):
    """per column: max |got - ref| / the column's largest |ref| (columns of zeros: 0 where got is zero too, else inf)"""
    got, ref = np.asarray(got), np.asarray(ref)
    top = np.max(np.abs(ref), axis=-1)
    err = np.max(np.abs(got - ref), axis=-1)
    return np.where(top > 0, err / np.where(top > 0, top, 1.0), np.where(err > 0, np.inf, 0.0))


def assert_within(got, ref, what=""):
    """every cell within ALLOWANCE of its column's largest |ref| plus ABS_TERM of the call's largest cell"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = ALLOWANCE * np.max(np.abs(ref), axis=-1, keepdims=True) + ABS_TERM * np.max(np.abs(ref))
    err = np.abs(got - ref)
    worst = float(np.max(err / bound)) if err.size else 0.0
    print("%s: worst cell at %.3f of its allowance" % (what, worst))
    assert worst <= 1.0, (what, worst)


# the smallest shapes at which each mechanism first engages (test_gpu_wvd.py): rows x nsig samples, x_ld = nsig + pitch
SHAPES = {
    "n32-full-lag": dict(nfft=32, nh=31, ng=1, ntimes=37, hop=1, first=-5, nsig=40, rows=1, pitch=0, b0=0, nb=32),
    "n256-band-wraps": dict(nfft=256, nh=127, ng=9, ntimes=41, hop=7, first=0, nsig=300, rows=1, pitch=0, b0=200, nb=100),
    "n256-long-g": dict(nfft=256, nh=63, ng=255, ntimes=6, hop=300, first=0, nsig=1800, rows=1, pitch=0, b0=0, nb=256),
    "n2048-batch-pitch": dict(nfft=2048, nh=2047, ng=33, ntimes=9, hop=64, first=100, nsig=1500, rows=3, pitch=7, b0=0, nb=2048),
    "n8192-right-of-record": dict(nfft=8192, nh=8191, ng=5, ntimes=5, hop=1000, first=0, nsig=2900, rows=1, pitch=0, b0=0, nb=8192),
}


def windows_of(s):
    """(h with h[0] = 1, g with sum 1) of a shape: Hamming both"""
    h, g = hamming(s["nh"]), hamming(s["ng"])
    return h / h[s["nh"] // 2], g / np.sum(g)


@functools.lru_cache(maxsize=None)
def signals(name):
    """(x, y) complex64 [rows, nsig]: unit noise plus a chirp from 0.02 to 0.2 cycles per sample; y = a delayed, rescaled x plus noise.
    Computed once and shared: read-only."""
    s = SHAPES[name]
    rng = np.random.default_rng(sum(name.encode()))
    n = np.arange(s["nsig"])
    out = []
    for amp, lag in ((2.0, 0), (1.5, 3)):
        ph = 2 * np.pi * (0.02 * (n - lag) + 0.09 * (n - lag) ** 2 / s["nsig"])
        a = amp * np.exp(1j * ph)[None, :] + (rng.standard_normal((s["rows"], s["nsig"])) + 1j * rng.standard_normal((s["rows"], s["nsig"])))
        a = a.astype(np.complex64)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name, cross):
    """float64 W [rows, ntimes, nfft] of a shape on the float32-rounded samples and windows; computed once, read-only"""
    s = SHAPES[name]
    x, y = signals(name)
    h, g = (w.astype(np.float32) for w in windows_of(s))
    W = np.stack([wvd_ref(x[r], h, g, s["hop"], s["first"], s["ntimes"], s["nfft"], y[r] if cross else None) for r in range(s["rows"])])
    W = W if cross else W.real.copy()
    W.setflags(write=False)
    return W


def band(W, s):
    """the nb bins from b0 on, modulo nfft"""
    return W[..., (s["b0"] + np.arange(s["nb"])) % s["nfft"]]
