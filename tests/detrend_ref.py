"""float64 restatement of the frame operations of include/spectral.h under its five detrend modes, for the tests of
the one-workgroup frame kernels (sp_welch_psd, sp_welch_csd, sp_stft, sp_stft_cog).  Written from the header text:

    frame g = win * (x[g*hop : g*hop + nfft] - trend)
    CONST      trend = the given constant
    MEAN       trend = mean of x[0:nsig]                       (samples past the last frame included)
    LINEAR     trend = least-squares line of x[0:nsig]
    SEGMEAN    trend = the frame's own mean
    SEGLINEAR  trend = the frame's own least-squares line
    complex input: real and imaginary parts are fitted separately

numpy only.  A helper module, not a test: nothing here is collected."""
import numpy as np

CONST, MEAN, LINEAR, SEGMEAN, SEGLINEAR = 0, 1, 2, 3, 4
MODES = (CONST, MEAN, LINEAR, SEGMEAN, SEGLINEAR)
MODE_NAMES = {CONST: "const", MEAN: "mean", LINEAR: "linear", SEGMEAN: "segmean", SEGLINEAR: "seglinear"}
SIDED_ONE, SIDED_TWO, SIDED_RAW = 1, 2, 3

TONE = 0.21          # cycles per sample
AMP = 4.0            # tone amplitude
TAIL = 11            # samples the tests leave past the last frame


def wg_transform(nfft):
    """L, the transform one workgroup runs for an nfft-point frame: nfft itself for a power of two, else the Bluestein
    length, the next power of two >= 2 nfft - 1 and at least 16."""
    if nfft & (nfft - 1) == 0:
        return nfft
    L = 16
    while L < 2 * nfft - 1:
        L *= 2
    return L


def fpw_of(L):
    """frame groups per workgroup: radix R = min(L, 16), T = L / R threads per frame, workgroups of max(T, 256) threads"""
    R = min(L, 16)
    T = L // R
    return max(T, 256) // T


# (nfft, hop): each pair selects a different form of segment_detrend / group_mean and of the per-frame reductions
SHAPES = ((2, 1), (3, 2), (8, 3), (16, 16), (32, 7), (64, 16), (30, 7), (512, 100), (1024, 512), (1000, 250), (1023, 511),
          (4096, 1024), (4095, 4095), (8192, 2048))


def frame_counts(nfft):
    """1; a workgroup whose tail groups run on clamped frames; 37.  From 4096 points up one workgroup holds one frame."""
    if nfft >= 4095:
        return (1, 5)
    return tuple(sorted({1, fpw_of(wg_transform(nfft)) + 3, 37}))


def nsig_of(nfft, hop, M):
    return nfft + hop * (M - 1) + TAIL


def signal(seed, n, cplx, nfft=None, offset=3.0):
    """The one input of the detrend tests, n samples cast to float32 / complex64 (references are computed from the cast
    samples): unit white noise + an offset (-offset / 2 on the imaginary part) + a drift of 2 per nfft samples that turns
    round every nfft samples (a triangle between 0 and 2: every frame sees a slope of its own, while offsets stay near the
    noise level and the tone keeps its share of every frame's power) + a quadratic term (t / n)^2 over the record (so that
    the whole-record line is not flat either) + a tone of amplitude 4 at 0.21 cycles per sample (exp(+i) for complex input:
    the centre of gravity sits away from 0; at amplitude 2 the noise cancels it in some 8-point frames, whose band share
    falls to 2.6e-4) + a transient 30 exp(-(n - 1 - t) / 3) on the last samples, which lie past the
    last frame: the whole-record mean and line then differ from a lone frame's own, so a kernel that fitted the framed span
    instead of x[0:nsig] is told apart."""
    nfft = n if nfft is None else nfft
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    slow = 2.0 * np.abs((t / nfft + 0.3 * seed) % 2.0 - 1.0) - 2.0 * (t / n) - (t / n) ** 2 + 80.0 * np.exp(-(n - 1 - t) / 2.0)
    ph = 2.0 * np.pi * TONE * t + 0.4 * seed
    re = rng.standard_normal(n) + offset + slow
    if not cplx:
        return (re + AMP * np.cos(ph)).astype(np.float32)
    im = rng.standard_normal(n) - 0.5 * offset - 0.5 * slow
    return (re + 1j * im + AMP * np.exp(1j * ph)).astype(np.complex64)


def _line(v):
    """least-squares line of v over its own index 0 .. len-1, evaluated there (closed form, centred index)"""
    n = v.shape[-1]
    if n <= 2:
        return v.copy()                       # a line through two points is the points: the residual is exactly zero
    c = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    slope = (v * c).sum(axis=-1, keepdims=True) / np.sum(c * c)
    return v.mean(axis=-1, keepdims=True) + slope * c


def _wide(x):
    x = np.asarray(x)
    return x.astype(np.complex128) if np.iscomplexobj(x) else x.astype(np.float64)


def frames(x, nfft, hop, M, mode, mean_value=None):
    """[M, nfft] detrended frames before the window, float64 / complex128"""
    x = _wide(x)
    if mode == CONST:
        x = x - (0.0 if mean_value is None else mean_value)
    elif mode == MEAN:
        x = x - x.mean()
    elif mode == LINEAR:
        x = x - _line(x)                      # complex: the sums are linear, so real and imaginary parts are fitted separately
    idx = (np.arange(M) * hop)[:, None] + np.arange(nfft)[None, :]
    f = x[idx]
    if mode == SEGMEAN:
        f = f - f.mean(axis=1, keepdims=True)
    elif mode == SEGLINEAR:
        f = f - _line(f)
    return f


def spectra(x, win, hop, M, mode, mean_value=None):
    """X[M, nfft] = FFT(win * frame), natural order"""
    w = np.asarray(win, dtype=np.float64)
    return np.fft.fft(w[None, :] * frames(x, w.size, hop, M, mode, mean_value), axis=1)


def nbins(n, sided):
    if sided == SIDED_ONE:
        return (n + 1) // 2 if n % 2 else n // 2
    return n


def layout(P, sided, amp=False):
    """natural-order bins (last axis) -> the layout of `sided`.  SIDED_ONE: the first nbins bins, [1:-1] of them doubled
    and, for odd n, the last one too (amp: times sqrt(2), for amplitudes); SIDED_TWO: fftshift; SIDED_RAW: as is."""
    n = P.shape[-1]
    if sided == SIDED_RAW:
        return P.copy()
    if sided == SIDED_TWO:
        return np.fft.fftshift(P, axes=-1)
    nb = nbins(n, SIDED_ONE)
    out = P[..., :nb].copy()
    hi = nb if n % 2 else nb - 1
    out[..., 1:hi] *= np.sqrt(2.0) if amp else 2.0
    return out


def psd(x, win, hop, M, mode, sided=SIDED_TWO, mean_value=None, scale=1.0):
    X = spectra(x, win, hop, M, mode, mean_value)
    return layout(scale * np.mean(np.abs(X) ** 2, axis=0), sided)


def csd(x, y, win, hop, M, mode, sided=SIDED_ONE, scale=1.0):
    """(pxx[nb], pyy[nch, nb], pxy[nch, nb] = mean_g Y conj(X)); y[nch, nsig]"""
    X = spectra(x, win, hop, M, mode)
    Y = np.stack([spectra(yc, win, hop, M, mode) for yc in np.atleast_2d(y)])
    pxx = layout(scale * np.mean(np.abs(X) ** 2, axis=0), sided)
    pyy = layout(scale * np.mean(np.abs(Y) ** 2, axis=1), sided)
    pxy = layout(scale * np.mean(Y * np.conj(X)[None], axis=1), sided)
    return pxx, pyy, pxy


def stft(x, win, hop, M, mode, sided=SIDED_ONE, amp=1.0, power=False, mean_value=None):
    """[M, nbins]: amp * X (sqrt(2) on the doubled bins of SIDED_ONE), or with power amp * |X|^2 with nothing doubled"""
    X = spectra(x, win, hop, M, mode, mean_value)
    if power:
        P = np.abs(X) ** 2
        return amp * (P[:, :nbins(P.shape[1], sided)] if sided == SIDED_ONE else layout(P, sided))
    return amp * layout(X, sided, amp=True)


def pseg(x, win, hop, M, mode, mean_value=None):
    """trapezoid of |win * frame|^2 at unit spacing"""
    w = np.asarray(win, dtype=np.float64)
    p = np.abs(w[None, :] * frames(x, w.size, hop, M, mode, mean_value)) ** 2
    return p.sum(axis=1) - 0.5 * (p[:, 0] + p[:, -1])


def band_mask(nfft, fs, fmin, fmax):
    """bins of fftfreq(nfft, 1 / fs) with fmin <= |f_k| <= fmax; a band edge that is a bin centre up to rounding (1e-9 of a
    bin) counts as inside"""
    ka = np.abs(np.fft.fftfreq(nfft, 1.0 / nfft))               # |signed bin index|, exact
    return (ka >= fmin * nfft / fs - 1e-9) & (ka <= fmax * nfft / fs + 1e-9)


def cog(x, win, hop, M, mode, fs, fmin=0.0, fmax=None, mean_value=None):
    """(cog[M], share[M]): sum f_k |X|^2 / sum |X|^2 over the band, 0 where the band holds no power; share = the band's
    part of the frame's power (0 for a frame without power)"""
    w = np.asarray(win, dtype=np.float64)
    n = w.size
    P = np.abs(spectra(x, win, hop, M, mode, mean_value)) ** 2
    keep = band_mask(n, fs, fmin, fs if fmax is None else fmax)
    f = np.fft.fftfreq(n, 1.0 / fs)
    den = (P * keep).sum(axis=1)
    num = (P * keep * f).sum(axis=1)
    tot = P.sum(axis=1)
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0), np.where(tot > 0, den / np.where(tot > 0, tot, 1.0), 0.0)


# ---- the cases both test modules walk (one place, so that the host checks hold for exactly what the GPU test runs) ----------
FS = 250.0                                   # sampling rate of the cog cases (not 1: the scaling by fs is part of the check)
CHANNEL_OFFSETS = (3.0, -2.0, 1.5, 4.5)      # the reference and three channels of the CSD cases


def case_signal(nfft, hop, M, cplx, ch=0):
    return signal(7 * nfft + M + 1000 * ch, nsig_of(nfft, hop, M), cplx, nfft, CHANNEL_OFFSETS[ch])


def const_value(cplx):
    """the non-zero constant of the CONST cases, exactly representable in float32"""
    return (1.25 + 0.75j) if cplx else 1.25


def cog_bands(nfft):
    """(name, fmin, fmax): every bin; the band [0.15 fs, 0.3 fs] around the tone; a band between bin 0 and bin 1, which holds
    no bin whatever nfft is"""
    return (("whole", 0.0, None), ("tone", 0.15 * FS, 0.3 * FS), ("empty", 0.25 * FS / nfft, 0.75 * FS / nfft))


def mode_cases(cplx):
    """(label, detrend argument of pyfft_amd.engine, mean_value, reference mode): the five modes + CONST with a non-zero constant"""
    return (("const", 0, None, CONST), ("const-value", True, const_value(cplx), CONST), ("mean", 1, None, MEAN),
            ("linear", 2, None, LINEAR), ("segmean", 3, None, SEGMEAN), ("seglinear", 4, None, SEGLINEAR))
