"""Dynamic-range records and references for the Welch / CSD tests: a coloured floor with a line 80 dB above it, the float64
references of the estimates, their float32 restatements (what float32 arithmetic costs on such a record) and the per-bin
checkers, which have NO absolute term: every bin is held to its own level, every cross term to sqrt(G_ii G_jj).

    frame g = win * (x[g*hop : g*hop + nfft] - m),   m the mean of the WHOLE record (samples past the last frame included),
                                                     a given constant, or 0
    psd[k]      = 1/M sum_g |X_g[k]|^2                       (scale 1, what engine.welch_psd returns with scale=1.0)
    pxy[c][k]   = 1/M sum_g Y_c,g[k] conj(X_g[k])            (engine.welch_csd)
    G[k][i][j]  = 1/M sum_g X_i,g[k] conj(X_j,g[k])          (engine.csd_matrix, bins 0 .. nfft/2)

The float64 references convert the float32 / complex64 record to float64 FIRST and do everything after that in float64
(oracle.welch_psd_stream subtracts the mean in the input's dtype by design, which alone moves the quiet bins of these records
by 1e-5 of their level).  The float32 restatements take window, mean subtraction and transform in float32 (scipy.fft
transforms float32 natively) and the sums over frames in float64.

numpy and scipy only.  A helper module, not a test: nothing here is collected."""
import numpy as np
import scipy.fft
from scipy.signal import lfilter

POLE = 0.97              # AR(1) floor: ~36 dB between the spectrum's ends
LINE_F = 0.237           # cycles per sample: never on a bin centre of a power-of-two segment
RTOL = 2e-4              # the project's float32 Welch tolerance, here with no absolute term
TAIL = 333               # samples the records carry past the last frame (they count for the mean)
NCU_MI355X = 256         # compute units of the chip the frame counts are derived from (the host tests use this figure)


def floor_at(f):
    """PSD of the unit-variance-innovation AR(1) process at f cycles per sample"""
    return 1.0 / abs(1.0 - POLE * np.exp(-2j * np.pi * f)) ** 2


def weak_pair_of(nch):
    """the two channels that share a weak common component: (3, 7) as in the nfft-256 test, the first and the last channel
    of a record with fewer than 8 channels, none for a single channel"""
    if nch >= 8:
        return (3, 7)
    return (0, nch - 1) if nch >= 2 else ()


def _ar1(rng, nsig):
    return lfilter([1.0], [1.0, -POLE], rng.standard_normal(nsig))


def _floors(rng, nch, nsig, weak_pair, weak_gamma2, cplx=False):
    """independent AR(1) floors, a weak common component added to the channels of weak_pair (gamma^2 = weak_gamma2).  The
    order of the draws for real records is the one the nfft-256 test has always used."""
    x = np.empty((nch, nsig), dtype=np.complex128 if cplx else np.float64)
    for c in range(nch):
        x[c] = _ar1(rng, nsig) + 1j * _ar1(rng, nsig) if cplx else _ar1(rng, nsig)
    a2 = np.sqrt(weak_gamma2) / (1.0 - np.sqrt(weak_gamma2))                 # gamma^2 = (a2 / (1 + a2))^2
    common = (_ar1(rng, nsig) + 1j * _ar1(rng, nsig) if cplx else _ar1(rng, nsig)) * np.sqrt(a2)
    for c in weak_pair:
        x[c] += common
    return x


def coloured_record_256(nch, nsig, seed, line_db=None, weak_pair=(3, 7), weak_gamma2=0.01):
    """The record of test_csd_matrix_per_bin_parity_dynamic_range (nfft 256, periodic Hann), sample for sample what that test
    has always run on: AR(1) floors, the weak pair, optionally a line `line_db` dB over the floor with the amplitude
    1 + 0.1 c and the phase 0.4 c in channel c, and the offset 0.3.  coloured_record() below is its generalisation to any
    segment length and window; it scales the channels differently, so this one is kept for that test."""
    rng = np.random.default_rng(seed)
    x = _floors(rng, nch, nsig, weak_pair, weak_gamma2)
    if line_db is not None:
        k = np.arange(nsig)
        # a sinusoid of amplitude A in a Hann-windowed periodogram stands A^2 S1^2 / (4 S2) over a floor of height floor_at()
        w = 2 * np.pi * LINE_F
        for c in range(nch):
            amp = np.sqrt(floor_at(LINE_F) * 10.0 ** (line_db / 10.0) * 4.0 * 1.5 / 256.0) * (1.0 + 0.1 * c)   # (nfft 256: S1^2/S2 = N/1.5)
            x[c] += amp * np.cos(w * k + 0.4 * c)
        x += 0.3
    return x.astype(np.float32)


def coloured_record(nch, nsig, seed, nfft, win, line_db=80.0, cplx=False, dc=3.0):
    """[nch, nsig] float32 (complex64 with cplx): every channel an independent AR(1) floor (both parts, for complex records);
    the channels weak_pair_of(nch) share a weak common component (gamma^2 ~ 0.01); a line `line_db` dB over the floor at
    LINE_F in every channel, its amplitude taken from the window's S1^2 / S2, scaled by 1 + 0.5 c / nch with the phase 0.4 c in
    channel c (64 channels stay within 4 dB of each other); the offset dc (1 + c) / nch (times 1 - 0.5i for complex records),
    so that the mean corrections of the one-pass kernels are far above any threshold.  line_db=None: floors and offsets only."""
    win = np.asarray(win, dtype=np.float64)
    assert win.size == nfft
    rng = np.random.default_rng(seed)
    x = _floors(rng, nch, nsig, weak_pair_of(nch), 0.01, cplx)
    k = np.arange(nsig)
    w = 2 * np.pi * LINE_F
    s2_s1 = np.sum(win ** 2) / np.sum(win) ** 2
    for c in range(nch):
        if line_db is not None:
            g = (1.0 + 0.5 * c / nch) * np.sqrt(10.0 ** (line_db / 10.0) * s2_s1)
            if cplx:
                # floor 2 floor_at() (two parts); A exp(iwk) stands A^2 S1^2 / S2 over it
                x[c] += g * np.sqrt(2.0 * floor_at(LINE_F)) * np.exp(1j * (w * k + 0.4 * c))
            else:
                # A cos(wk) stands A^2 S1^2 / (4 S2) over the floor
                x[c] += g * np.sqrt(4.0 * floor_at(LINE_F)) * np.cos(w * k + 0.4 * c)
        x[c] += dc * (1 + c) / nch * ((1 - 0.5j) if cplx else 1.0)
    return x.astype(np.complex64 if cplx else np.float32)


def nsig_of(nfft, hop, M):
    return (M - 1) * hop + nfft + TAIL


# ---------------------------------------------------------------------------------------------------------------------
# the estimates, in float64 and in float32
# ---------------------------------------------------------------------------------------------------------------------
def _prepare(x, win, detrend, f32):
    """(record minus its trend constant, window), both in the working precision.  detrend: True -- the mean of every row over
    the whole record; False / None -- nothing; a number (or one per row) -- that constant"""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    if f32:
        assert x.dtype == (np.complex64 if cplx else np.float32), "the restatement starts from the record the GPU gets"
    x64 = x.astype(np.complex128 if cplx else np.float64)
    if detrend is True:
        m = x64.mean(axis=-1, keepdims=True)
    elif detrend is False or detrend is None:
        m = None
    else:
        m = np.asarray(detrend, dtype=x64.dtype).reshape(x64.shape[:-1] + (1,))
    if f32:
        xw = x if m is None else x - m.astype(x.dtype)
        assert xw.dtype == x.dtype
        return xw, np.asarray(win).astype(np.float32)
    return (x64 if m is None else x64 - m), np.asarray(win, dtype=np.float64)


def _chunks(M, rows, nfft):
    """frame ranges that keep rows x frames x nfft samples at or under 2^24 (128 MiB of float64 frames, as much again of
    spectra and of their transposed copy: the working set stays far below 1 GB)"""
    m = max(1, (1 << 24) // (rows * nfft))
    return [(g0, min(M, g0 + m)) for g0 in range(0, M, m)]


def _spectra(xw, w, hop, g0, g1, half):
    """transforms of the frames g0 .. g1 - 1 of every row of xw: [..., g1 - g0, nb], complex128, or complex64 for float32 in"""
    nfft = w.size
    idx = (np.arange(g0, g1) * hop)[:, None] + np.arange(nfft)[None, :]
    seg = w * xw[..., idx]
    assert seg.dtype == xw.dtype
    if seg.dtype in (np.float32, np.complex64):
        X = scipy.fft.rfft(seg, axis=-1) if half else scipy.fft.fft(seg, axis=-1)
        assert X.dtype == np.complex64                                       # the transform really ran in float32
    else:
        X = np.fft.rfft(seg, axis=-1) if half else np.fft.fft(seg, axis=-1)
        assert X.dtype == np.complex128
    return X


def _power(X):
    X = X.astype(np.complex128)
    return X.real ** 2 + X.imag ** 2


def _welch_psd(x, win, hop, M, detrend, f32):
    xw, w = _prepare(x, win, detrend, f32)
    assert xw.ndim == 1
    acc = np.zeros(w.size)
    for g0, g1 in _chunks(M, 1, w.size):
        acc += _power(_spectra(xw, w, hop, g0, g1, False)).sum(axis=0)
    return np.fft.fftshift(acc) / M


def welch_psd64(x, win, hop, M, detrend=True):
    """two-sided, fftshift-ed (SIDED_TWO), scale 1: float64[nfft]"""
    return _welch_psd(x, win, hop, M, detrend, False)


def welch_psd32(x, win, hop, M, detrend=True):
    return _welch_psd(x, win, hop, M, detrend, True)


def one_sided(p_two):
    """SIDED_ONE from SIDED_TWO along the last axis: the bins 0 .. nfft/2 - 1, doubled on [1:-1] (the reference's crop)"""
    n = p_two.shape[-1]
    p = np.fft.ifftshift(p_two, axes=-1)[..., : n // 2].copy()
    p[..., 1:-1] *= 2
    return p


def _welch_csd(x, y, win, hop, M, detrend, f32):
    xw, w = _prepare(x, win, detrend, f32)
    yw, _ = _prepare(y, win, detrend, f32)
    assert xw.ndim == 1 and yw.ndim == 2
    nfft, nch = w.size, yw.shape[0]
    pxx, pyy, pxy = np.zeros(nfft), np.zeros((nch, nfft)), np.zeros((nch, nfft), dtype=np.complex128)
    for g0, g1 in _chunks(M, nch + 1, nfft):
        X = _spectra(xw, w, hop, g0, g1, False).astype(np.complex128)
        Y = _spectra(yw, w, hop, g0, g1, False).astype(np.complex128)
        pxx += _power(X).sum(axis=0)
        pyy += _power(Y).sum(axis=1)
        pxy += (Y * np.conj(X)[None]).sum(axis=1)
    sh = lambda a: np.fft.fftshift(a, axes=-1) / M
    return sh(pxx), sh(pyy), sh(pxy)


def welch_csd64(x, y, win, hop, M, detrend=True):
    """(pxx[nfft], pyy[nch, nfft], pxy[nch, nfft] = Y conj(X)), two-sided, fftshift-ed, scale 1"""
    return _welch_csd(x, y, win, hop, M, detrend, False)


def welch_csd32(x, y, win, hop, M, detrend=True):
    return _welch_csd(x, y, win, hop, M, detrend, True)


def _csd_matrix(x, win, hop, M, detrend, f32):
    xw, w = _prepare(x, win, detrend, f32)
    assert xw.ndim == 2 and not np.iscomplexobj(xw)
    nch, nb = xw.shape[0], w.size // 2 + 1
    G = np.zeros((nb, nch, nch), dtype=np.complex128)
    for g0, g1 in _chunks(M, nch, w.size):
        # [bins, nch, m] @ [bins, m, nch]: the contraction over the frames of the chunk as one batched product
        A = np.ascontiguousarray(_spectra(xw, w, hop, g0, g1, True).astype(np.complex128).transpose(2, 0, 1))
        G += np.matmul(A, np.ascontiguousarray(np.conj(A).transpose(0, 2, 1)))
    return G / M


def csd_matrix64(x, win, hop, M, detrend=True):
    """G[nfft/2 + 1, nch, nch] complex128, scale 1, nothing doubled.  The frames go through in chunks (a few hundred MB at the
    most) and each chunk is contracted by one batched matmul: seconds at 64 channels, where the per-frame broadcast of
    oracle.csd_matrix takes tens of seconds."""
    return _csd_matrix(x, win, hop, M, detrend, False)


def csd_matrix32(x, win, hop, M, detrend=True):
    return _csd_matrix(x, win, hop, M, detrend, True)


# ---------------------------------------------------------------------------------------------------------------------
# the checkers: no absolute term
# ---------------------------------------------------------------------------------------------------------------------
def psd_excess(got, ref, rtol=RTOL):
    """(max_k |got - ref| / (rtol ref), the bin where it is reached): <= 1 passes.  Every bin against its OWN level."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(ref > 0)
    e = np.abs(got - ref) / (rtol * ref)
    k = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[k]), (k[0] if len(k) == 1 else k)


def cross_excess(pxy, pxy_ref, pxx_ref, pyy_ref, rtol=RTOL):
    """a cross-spectrum against rtol sqrt(pxx pyy) per bin, the natural scale of a cross term (|pxy| <= it)"""
    e = np.abs(np.asarray(pxy) - pxy_ref) / (rtol * np.sqrt(pxx_ref * pyy_ref))
    k = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[k]), (k[0] if len(k) == 1 else k)


def csd_excess(G, ref, rtol=RTOL):
    """(max over bins and pairs of |G - ref| / (rtol sqrt(ref_ii ref_jj)), the (bin, i, j) where it is reached): <= 1 passes"""
    G, ref = np.asarray(G), np.asarray(ref)
    assert G.shape == ref.shape
    d = np.sqrt(np.abs(np.einsum("kii->ki", ref).real))                      # [nb, nch]
    assert np.all(d > 0)
    e = np.abs(G - ref) / (rtol * d[:, :, None] * d[:, None, :])
    k = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[k]), tuple(int(v) for v in k)


# ---------------------------------------------------------------------------------------------------------------------
# the cases the GPU tests run and the host tests guard: everything at nfft 4096, the frame counts from the chip's CU count so
# that the DEFAULT dispatch takes the named kernel (the pipeline from 2 frames -- or frame pairs -- per CU on)
# ---------------------------------------------------------------------------------------------------------------------
NFFT = 4096


def psd_cases(ncu):
    """id -> dict(cplx, hop, M, window, detrend ('mean' / 'off' / 'const'), seed, env, kernel).  kernel = (how, text):
    E.profile_last_kernel() must start with / equal / contain the text."""
    mp, mr = 2 * ncu + 88, 4 * ncu + 76
    pipe = ("startswith", "k_welch_pipe")
    cases = {
        "c_hop2048_pipe_hann": dict(cplx=True, hop=2048, M=mp, window="Hanning", detrend="mean", kernel=pipe),
        "c_hop2048_pipe_nuttall": dict(cplx=True, hop=2048, M=mp, window="Nuttall4c", detrend="mean", kernel=pipe),
        "c_hop1024_pipe": dict(cplx=True, hop=1024, M=mp, window="Hanning", detrend="mean", kernel=pipe),
        "c_hop4096_symmetric_onepass": dict(cplx=True, hop=4096, M=mp, window="Hanning", detrend="mean",
                                            kernel=("equals", "k_welch_carry(onepass)")),
        "c_hop4096_pipe_nodetrend": dict(cplx=True, hop=4096, M=mp, window="Hanning", detrend="off", kernel=("equals", "k_welch_pipe")),
        "c_hop2048_carry": dict(cplx=True, hop=2048, M=300, window="Hanning", detrend="mean", kernel=("startswith", "k_welch_carry")),
        "c_hop2048_generic": dict(cplx=True, hop=2048, M=300, window="Hanning", detrend="mean", kernel=("equals", "k_welch"),
                                  env={"SP_WELCH_GENERIC": "1"}),
        "r_hop2048_pipe_realpair": dict(cplx=False, hop=2048, M=mr, window="Hanning", detrend="mean", kernel=("contains", "realpair")),
        "r_hop2048_pipe_realpair_const": dict(cplx=False, hop=2048, M=mr, window="Hanning", detrend="const",
                                              kernel=("contains", "realpair")),
        "r_hop2048_symmetric_realpair": dict(cplx=False, hop=2048, M=301, window="Hanning", detrend="mean",
                                             kernel=("equals", "k_welch_rp")),
    }
    for n, (name, c) in enumerate(cases.items()):
        c.setdefault("env", {})
        c["seed"] = 4100 + n
    return cases


def psd_record(case, window):
    """(x, detrend argument of the references).  'const': the record's mean rounded to float32, so that the constant the kernel
    subtracts and the one the reference subtracts are the same number."""
    x = coloured_record(1, nsig_of(NFFT, case["hop"], case["M"]), case["seed"], NFFT, window, cplx=case["cplx"])[0]
    if case["detrend"] == "mean":
        return x, True
    if case["detrend"] == "off":
        return x, False
    return x, float(np.float32(x.astype(np.float64).mean()))


CSD_PAIR = dict(hop=2048, M=301, seed=4201)                                  # x = channel 0, y = channels 1, 2 (0 and 2 weakly coherent)


def matrix_cases(ncu):
    """64 channels: the smallest record that sends the spectra through the pipeline's packed pair spectra (32 frame pairs per
    run, ceil(ncu / 64) runs per channel), with one more frame so that the last pair is half filled; below 1024 frame pairs:
    the three-piece contraction.  16 channels: from 1024 frame pairs on the two-piece contraction."""
    m64 = 64 * ((ncu + 63) // 64) + 1
    assert (2051 + 1) // 2 >= max(1024, 32 * ((ncu + 15) // 16)), "16 channels: 2051 frames no longer reach the pipeline spectra"
    return {"ch64": dict(nch=64, hop=2048, M=m64, seed=4301), "ch16": dict(nch=16, hop=2048, M=2051, seed=4302)}
