"""The instrument of the loop-seam tests (tests/test_gpu_loop_seams.py), and its own check on the CPU (tests/test_host_seam_ref.py).

The library cuts long work into chunks of frames (long_chunk_frames, the chunks of sp_csd_matrix), batches of long transforms into
slices of rows (dev_fft_any, sp_czt) and rows into batches of 65535 (grid.y).  Each loop carries an offset (f0, b0, r0) into its
kernels, its scratch pointers and its output index; an offset that is dropped or applied to the wrong pointer gives spectra that look
plausible.  Here are

    the budgets            restated from pyfft_amd/csrc/spectral.hip, so that a test derives the smallest shape that crosses a seam;
    the records            not stationary across a seam: a slow chirp + unit noise + an offset and a ramp per row, and a tone burst of
                           BURST times the noise rms in the samples that only the frames of the last chunk cover;
    the row batches        rows that all differ (gain, tone), the rows from 65535 on LOUD times louder than the others;
    the references         float64, chunk-free, from numpy and tests/detrend_ref.py: sums over ANY list of source frames, so that the
                           same code gives the reference (every frame once) and
    the planted defects    PLANTS: the result a wrong offset would give, obtained by re-mapping frames or rows in the reference.

        read_f0_zero       a chunk after the first reads its frames at f0 = 0                  (inputs: chirp, burst)
        drop_last          the last, ragged chunk is never run                                 (inputs: burst)
        write_first        a chunk after the first writes its rows at the first chunk's place  (inputs: chirp, burst; row outputs only)
        trend_unshifted    linear detrend: the line is not re-based to the chunk's first sample (inputs: ramp; sp_csd_matrix only,
                           the one loop that re-bases its trend records)
        batch_from_first   the second row batch reads the rows of the first                    (inputs: the rows' gains and tones)

tests/test_host_seam_ref.py shows that each of them moves an output element by at least 100 tolerances on every input of the GPU tests.
The window is 1 + 0.3 cos: largest at the frame's ends, where the samples of a ragged last chunk at a small hop lie (under a
window that vanishes there, seven frames at a hop of 16 would not count in an average of six thousand).  The frame cases' records
carry a small ramp only: a large one leaks into every bin under mean detrend and raises the absolute term of the tolerance.
A helper module, not a test: nothing here is collected."""
import collections
import functools

import numpy as np

import detrend_ref as R

# ---- the budgets, as spectral.hip has them ------------------------------------------------------------------------------------------
MAX_WG_FFT = 8192                       # SP_MAX_WG_FFT: longer transforms take the multi-pass paths
LONG_CHUNK_BYTES = 192 << 20            # SP_LONG_CHUNK_BYTES
LONG_SLICE_BYTES = 256 << 20            # SP_LONG_SLICE_BYTES
MAX_ROWS_PER_PASS = 32768               # the cap of both
ROW_BATCH = 65535                       # grid.y
NCU_MI355X = 256

BURST = 16.0                            # the burst's amplitude over the noise rms: about 10 times the record's rms
LOUD = 8.0                              # the gain of the rows of the second row batch
ROWS = ROW_BATCH + 3                    # the second batch holds 3 rows
ALONE = (0, ROW_BATCH - 1, ROW_BATCH, ROW_BATCH + 2)       # rows that are also computed alone
PLANTS = ("read_f0_zero", "drop_last", "write_first", "trend_unshifted", "batch_from_first")


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def is_pow2(n):
    return n & (n - 1) == 0


def wg_capable(n):
    if n < 2:
        return False
    return n <= MAX_WG_FFT if is_pow2(n) else max(next_pow2(2 * n - 1), 16) <= MAX_WG_FFT


def long_len(n):
    """the multi-pass transform behind an n-point long transform: n itself, or the Bluestein length"""
    return n if is_pow2(n) else next_pow2(2 * n - 1)


def long_chunk_frames(nfft, nframes, cap=0):
    """long_chunk_frames of spectral.hip; cap = SP_LONG_CHUNK_FRAMES"""
    m = max(1, min(LONG_CHUNK_BYTES // (8 * nfft), MAX_ROWS_PER_PASS, nframes))
    return cap if 0 < cap < m else m


def long_slice_rows(n, cap=0):
    """the rows per slice of dev_fft_any / sp_czt for a transform that runs on long_len(n) points; cap = SP_LONG_SLICE_ROWS"""
    s = max(1, min(LONG_SLICE_BYTES // (8 * long_len(n)), MAX_ROWS_PER_PASS))
    return cap if 0 < cap < s else s


def czt_len(n, m):
    return max(next_pow2(n + m - 1), 512)


def csdm_chunk_frames(nch, nfft, nframes, cap=0):
    """mc of sp_csd_matrix; cap = SP_CSDM_CHUNK_FRAMES"""
    nb = nfft // 2 + 1
    mc = min((1 << 31) // (nch * nb), 16384)
    if 0 < cap < mc:
        mc = cap
    mc = max(mc, 32) & ~31
    nchunks = -(-nframes // mc)
    mc = (-(-nframes // nchunks) + 31) & ~31
    if not wg_capable(nfft):
        mc = min(mc, long_chunk_frames(nfft, nframes))
    return min(mc, nframes)


def passes(n, per):
    return -(-n // per)


def chunks(nframes, mc):
    return [(f0, min(mc, nframes - f0)) for f0 in range(0, nframes, mc)]


def pipe_spec_min_frames(nch, ncu=NCU_MI355X):
    """the fewest frames of a chunk that sp_csd_matrix sends through the nfft-4096 pipeline: 32 pairs per run, ceil(ncu / nch) runs"""
    return 2 * 32 * (-(-ncu // nch)) - 1


# ---- the windows, records and row batches ---------------------------------------------------------------------------------------
def window(n):
    return 1.0 + 0.3 * np.cos(2.0 * np.pi * np.arange(n) / n)


def tail_from(nfft, hop, nframes, mc):
    """the first sample that only the frames of the last chunk cover"""
    f0 = (nframes - 1) // mc * mc
    return (f0 - 1) * hop + nfft if f0 > 0 else 0


def record(seed, n, cplx, burst_from, offset=3.0, ramp=4.0):
    """chirp (0.02 -> 0.12 cycles per sample, amplitude 1.5) + unit noise + offset + a ramp of `ramp` over the record + a tone burst
    (0.31 cycles per sample, amplitude BURST) from sample burst_from on; float32 / complex64, what the device sees"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    ph = 2.0 * np.pi * (0.02 * t + 0.05 * t * t / n)
    bph = 2.0 * np.pi * 0.31 * t + 0.3 * seed
    on = t >= burst_from
    slow = offset + ramp * t / n
    re = rng.standard_normal(n) + slow + 1.5 * np.cos(ph) + BURST * on * np.cos(bph)
    if not cplx:
        return re.astype(np.float32)
    im = rng.standard_normal(n) - 0.5 * slow + 1.5 * np.sin(ph) + BURST * on * np.sin(bph)
    return (re + 1j * im).astype(np.complex64)


def channels(seed, nch, n, burst_from):
    """float32 [nch, n]: record() per channel with offsets and ramps of its own and a common part (the channels are coherent)"""
    common = record(seed + 1000, n, False, burst_from, 0.0, 0.0).astype(np.float64)
    out = [0.4 * common + record(seed + c, n, False, n, 0.5 + 0.25 * (c % 7), 3.0 + (c % 5)).astype(np.float64) for c in range(nch)]
    return np.stack(out).astype(np.float32)


def row_batch(seed, nrows, n, cplx=False):
    """float32 / complex64 [nrows, n]: row r = gain_r (cos(2 pi f_r t + r) + 0.3 noise), gain_r = 1 + (r mod 251) / 251, f_r = 0.05 + 0.4
    (r mod 97) / 97, and LOUD times that from row 65535 on"""
    rng = np.random.default_rng(seed)
    r = np.arange(nrows)[:, None]
    t = np.arange(n)[None, :]
    gain = (1.0 + (r % 251) / 251.0) * np.where(r >= ROW_BATCH, LOUD, 1.0)
    ph = 2.0 * np.pi * (0.05 + 0.4 * (r % 97) / 97.0) * t + r
    if cplx:
        return (gain * (np.exp(1j * ph) + 0.3 * (rng.standard_normal((nrows, n)) + 1j * rng.standard_normal((nrows, n))))).astype(np.complex64)
    return (gain * (np.cos(ph) + 0.3 * rng.standard_normal((nrows, n)))).astype(np.float32)


def pipe_channels(xp, nch, n, device=None):
    """float32 [nch, n] made by the array module xp (numpy, or torch with a device): the pipeline case's record, generated where it is
    used.  A chirp + a hash noise of unit rms (the fractional part of a large sine: no generator state, the same on host and device up
    to the rounding of sin) + an offset per channel + a common part."""
    kw = dict(dtype=xp.float64) if device is None else dict(dtype=xp.float64, device=device)
    t = xp.arange(n, **kw)

    def noise(k):
        v = xp.sin(t * 12.9898 + 78.233 * k) * 43758.5453
        return (v - xp.floor(v) - 0.5) * (12.0 ** 0.5)
    ph = 2.0 * np.pi * (0.02 * t + 0.05 * t * t / n)
    common = noise(100) + 1.5 * xp.cos(ph)
    rows = [0.4 * common + noise(c) + 0.5 + 0.25 * c for c in range(nch)]
    return xp.stack(rows).to(xp.float32) if device is not None else xp.stack(rows).astype(xp.float32)


# ---- the frame map of a planted defect ----------------------------------------------------------------------------------------------
def source_frames(nframes, mc, plant=None):
    """for an accumulated quantity: the frames a chunked run with this defect would sum (every frame once without a defect)"""
    g = np.arange(nframes)
    if plant is None or plant == "trend_unshifted":
        return g
    if plant == "read_f0_zero":
        return g % mc
    if plant == "drop_last":
        return g[:(nframes - 1) // mc * mc]
    raise KeyError(plant)


def plant_rows(ref, mc, plant):
    """for a row output ref[nframes, ...] of a chunked run: what the defect leaves (an output that is never written holds zeros)"""
    out = np.array(ref)
    M = out.shape[0]
    for f0, m in chunks(M, mc)[1:]:
        if plant == "read_f0_zero":
            out[f0:f0 + m] = ref[:m]
        elif plant == "write_first":
            out[:m] = ref[f0:f0 + m]
            out[f0:f0 + m] = 0
        elif plant == "drop_last":
            if f0 + m == M:
                out[f0:] = 0
        else:
            raise KeyError(plant)
    return out


def plant_batches(ref):
    """batch_from_first on rows ref[nrows, ...]: row r >= 65535 holds what row r - 65535 gives"""
    out = np.array(ref)
    out[ROW_BATCH:] = ref[:out.shape[0] - ROW_BATCH]
    return out


def exceeds(ref, planted, tol, factor=100.0):
    """True when the defect moves some element by at least `factor` tolerances (tol: a scalar, or an array like ref)"""
    return bool(np.any(np.abs(np.asarray(planted) - np.asarray(ref)) >= factor * np.asarray(tol)))


# ---- the tolerances: the project's own (DESIGN section 0 and each entry's test file) -------------------------------------------------
def tol_psd(ref):
    return 2e-4 * np.abs(ref) + 1e-6 * np.max(np.abs(ref))


def tol_csd(ref):
    return 2e-4 * np.abs(ref) + 2e-6 * np.max(np.abs(ref))


def tol_rows(ref):
    return 1e-4 * np.max(np.abs(ref))


def tol_fft(n, ref):
    return 4e-6 * np.sqrt(np.log2(n)) * np.max(np.abs(ref))


def tol_csdm(G):
    d = np.sqrt(np.abs(np.einsum("kii->ki", G).real))
    return 2e-4 * d[:, :, None] * d[:, None, :] + 1e-6 * np.max(np.abs(G), axis=(1, 2))[:, None, None]


# ---- float64 references over a list of source frames -----------------------------------------------------------------------------------
def _wide(x):
    x = np.asarray(x)
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def detrended(x, mode):
    """the whole-record part of a detrend mode of tests/detrend_ref.py, float64: (record, slope of the line taken off per sample)"""
    x = _wide(x)
    if mode == R.MEAN:
        return x - x.mean(axis=-1, keepdims=True), 0.0
    if mode == R.LINEAR:
        n = x.shape[-1]
        c = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
        slope = (x * c).sum(axis=-1, keepdims=True) / np.sum(c * c)
        return x - x.mean(axis=-1, keepdims=True) - slope * c, slope[..., 0]
    return x, 0.0


def windowed(xd, win, hop, idx, mode, add=None):
    """[len(idx), nfft]: win * the frames idx of the detrended record (+ add[i], a constant per frame: a line that was not re-based)"""
    w = np.asarray(win, dtype=np.float64)
    f = xd[np.asarray(idx)[:, None] * hop + np.arange(w.size)[None, :]]
    if add is not None:
        f = f + np.asarray(add)[:, None]
    if mode == R.SEGMEAN:
        f = f - f.mean(axis=1, keepdims=True)
    elif mode == R.SEGLINEAR:
        f = f - R._line(f)
    return w[None, :] * f


def spectra_rows(x, win, hop, idx, mode):
    """X[len(idx), nfft], natural order, and the frames' time-domain power (trapezoid, unit spacing)"""
    xd, _ = detrended(x, mode)
    f = windowed(xd, win, hop, idx, mode)
    p = np.abs(f) ** 2
    return np.fft.fft(f, axis=1), p.sum(axis=1) - 0.5 * (p[:, 0] + p[:, -1])


def _blocks(idx, block):
    idx = np.asarray(idx)
    for a in range(0, idx.size, block):
        yield idx[a:a + block]


def psd_sum(x, win, hop, idx, mode, block=256):
    """sum over the frames idx of |X|^2, natural order"""
    xd, _ = detrended(x, mode)
    acc = np.zeros(len(win))
    for b in _blocks(idx, block):
        acc += (np.abs(np.fft.fft(windowed(xd, win, hop, b, mode), axis=1)) ** 2).sum(axis=0)
    return acc


def csd_sums(x, y, win, hop, idx, mode, block=128):
    """(sum |X|^2 [nfft], sum |Y|^2 [nch, nfft], sum Y conj(X) [nch, nfft]) over the frames idx"""
    xd, _ = detrended(x, mode)
    yd = [detrended(yc, mode)[0] for yc in np.atleast_2d(y)]
    n = len(win)
    sxx, syy, sxy = np.zeros(n), np.zeros((len(yd), n)), np.zeros((len(yd), n), dtype=np.complex128)
    for b in _blocks(idx, block):
        X = np.fft.fft(windowed(xd, win, hop, b, mode), axis=1)
        sxx += (np.abs(X) ** 2).sum(axis=0)
        for c, yc in enumerate(yd):
            Y = np.fft.fft(windowed(yc, win, hop, b, mode), axis=1)
            syy[c] += (np.abs(Y) ** 2).sum(axis=0)
            sxy[c] += (Y * np.conj(X)).sum(axis=0)
    return sxx, syy, sxy


def arc(nfft, m, start, step):
    """E[nfft, m] = exp(-2 pi i (start + k step) j): frames @ E is the chirp-z transform on the arc"""
    j = np.arange(nfft, dtype=np.float64)[:, None]
    k = np.arange(m, dtype=np.float64)[None, :]
    return np.exp(-2j * np.pi * (((start + k * step) * j) % 1.0))


def zoom_rows(x, win, hop, idx, mode, E):
    xd, _ = detrended(x, mode)
    return windowed(xd, win, hop, idx, mode) @ E


def zoom_sums(x, y, win, hop, idx, mode, E, block=256):
    """(sum |X|^2, sum |Y|^2, sum conj(X) Y) [m] over the frames idx (y None: the first only)"""
    xd, _ = detrended(x, mode)
    yd = None if y is None else detrended(y, mode)[0]
    m = E.shape[1]
    sxx, syy, sxy = np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.complex128)
    for b in _blocks(idx, block):
        X = windowed(xd, win, hop, b, mode) @ E
        sxx += (np.abs(X) ** 2).sum(axis=0)
        if yd is not None:
            Y = windowed(yd, win, hop, b, mode) @ E
            syy += (np.abs(Y) ** 2).sum(axis=0)
            sxy += (np.conj(X) * Y).sum(axis=0)
    return sxx, syy, sxy


def csdm_sum(x, win, hop, idx, mode, block=2048, unshifted_from=None):
    """sum over the frames idx of X_i conj(X_j) on the rfft bins: complex128 [nb, nch, nch]; x [nch, nsig] real.
    unshifted_from = mc plants trend_unshifted under linear detrend: a frame g of a chunk after the first keeps the line's value at
    the chunk's first sample, slope * (g // mc) * mc * hop, which a trend that was not re-based fails to take off."""
    xd, slope = detrended(x, mode)
    nch, nfft = xd.shape[0], len(win)
    G = np.zeros((nfft // 2 + 1, nch, nch), dtype=np.complex128)
    for b in _blocks(idx, block):
        S = np.empty((nch, b.size, nfft // 2 + 1), dtype=np.complex128)
        for c in range(nch):
            add = None
            if unshifted_from is not None and mode == R.LINEAR:
                add = slope[c] * ((b // unshifted_from) * unshifted_from * hop)
            S[c] = np.fft.rfft(windowed(xd[c], win, hop, b, mode, add), axis=1)
        St = np.ascontiguousarray(S.transpose(2, 0, 1))                      # [k][channel][frame]
        G += St @ np.conj(St.transpose(0, 2, 1))
    return G


def cog_of(X, fs):
    """centre of gravity of every row of the natural-order spectra X over all bins"""
    P = np.abs(X) ** 2
    f = np.fft.fftfreq(X.shape[1], 1.0 / fs)
    return (P * f).sum(axis=1) / P.sum(axis=1)


def rows_of_interest(nframes, seams, stride=61):
    """the rows a long row output is compared on: three on either side of every seam, the first three, the last eight, every
    stride-th"""
    keep = set(range(min(3, nframes))) | set(range(max(0, nframes - 8), nframes)) | set(range(0, nframes, stride))
    for s in seams:
        keep |= set(range(max(0, s - 3), min(nframes, s + 3)))
    return np.array(sorted(keep))


def seams_of(nframes, mc, n):
    """the first rows of every chunk after the first and, inside each chunk, of every slice of its transforms"""
    per = long_slice_rows(n)
    out = []
    for f0, m in chunks(nframes, mc):
        out += [f0 + s for s in range(0, m, per)]
    return sorted(set(out) - {0})


# ---- the frame cases both test modules walk ------------------------------------------------------------------------------------------
FrameCase = collections.namedtuple("FrameCase", "id nfft hop nframes cplx mc cap")


def _frame_case(tag, nfft, hop, cplx, cap=0, extra=7, L=None):
    """a case whose frames make `extra` more than one chunk at the default budget, or 7 frames in chunks of `cap` under the hook"""
    L = nfft if L is None else L
    if cap:
        return FrameCase(tag, nfft, hop, 7, cplx, cap, cap)
    mc = long_chunk_frames(L, 1 << 30)
    return FrameCase(tag, nfft, hop, mc + extra, cplx, mc, 0)


ZOOM_M, ZOOM_START, ZOOM_STEP = 100, 0.1037, 0.3 / 100
W4100 = _frame_case("b4100-f32", 4100, 16, False)                            # 6138 + 7 frames, Bluestein on 16384 points
W16384 = _frame_case("p16384-c64", 16384, 16, True)                           # 1536 + 7 frames, five-pass power of two
Z8100 = _frame_case("z8100-f32", 8100, 16, False, L=czt_len(8100, ZOOM_M))    # 1536 + 7 frames of a chirp-z on 16384 points
TINY = tuple(_frame_case("t%d-%s" % (n, "c64" if c else "f32"), n, n // 4, c, cap=3) for n in (4100, 16384) for c in (False, True))
TINY_ZOOM = tuple(_frame_case("tz8100-%s" % ("c64" if c else "f32"), 8100, 2025, c, cap=3) for c in (False, True))


def nsig_of(case):
    return (case.nframes - 1) * case.hop + case.nfft + 5


@functools.lru_cache(maxsize=None)
def case_record(case, ch=0):
    """the record of a frame case (channel ch of a cross-spectral case): computed once, read-only"""
    n = nsig_of(case)
    x = record(sum(case.id.encode()) + 31 * ch, n, case.cplx, tail_from(case.nfft, case.hop, case.nframes, case.mc), 3.0 - 1.5 * ch, 0.5)
    x.setflags(write=False)
    return x


CsdmCase = collections.namedtuple("CsdmCase", "id nch nfft hop nframes cap")
# 16500 frames: two chunks of 8256 + 8244 at the default budget; k_stft_rp + bf16, k_stft + k_csdm_fused, the transposed fp32 form
CSDM_DEFAULT = (CsdmCase("rp-bf16-2ch", 2, 32, 4, 16500, 0), CsdmCase("fused-3ch", 3, 30, 4, 16500, 0),
                CsdmCase("transposed-65ch", 65, 32, 4, 16500, 0))
# under SP_CSDM_CHUNK_FRAMES: 5 channels at nfft 256 (11, 6 and 4 chunks), and the long path at nfft 9000
CSDM_HOOKED = tuple(CsdmCase("h256-5ch-cap%d" % c, 5, 256, 128, 333, c) for c in (32, 64, 96)) + \
    (CsdmCase("h9000-3ch-cap32", 3, 9000, 2250, 70, 32),)


def csdm_mc(case):
    return csdm_chunk_frames(case.nch, case.nfft, case.nframes, case.cap)


@functools.lru_cache(maxsize=None)
def csdm_record(case):
    n = (case.nframes - 1) * case.hop + case.nfft + 5
    mc = csdm_mc(case)
    x = channels(sum(case.id.encode()), case.nch, n, tail_from(case.nfft, case.hop, case.nframes, mc))
    x.setflags(write=False)
    return x


# ---- rows: the slices of a batch of long transforms, and the row batches of 65535 --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sliding_rows(seed, nrows, n, cplx=True):
    """[nrows, n]: row r = gain_r * noise[r : r + n], one noise record under a sliding window (every row differs, and a row read at the
    wrong offset is another row's samples shifted), gain_r = 1 + (r mod 251) / 251.  Cheap enough for 2049 rows of 16384."""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n + nrows) + (1j * rng.standard_normal(n + nrows) if cplx else 0.0)
    win = np.lib.stride_tricks.sliding_window_view(b, n)[:nrows]
    x = (win * (1.0 + (np.arange(nrows)[:, None] % 251) / 251.0)).astype(np.complex64 if cplx else np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def batch_rows(seed, n, cplx=False, nrows=ROWS):
    x = row_batch(seed, nrows, n, cplx)
    x.setflags(write=False)
    return x


def row_sources(nrows, per, plant):
    """source row of every output row of a run in passes of `per` rows under a defect (-1: never written)"""
    return plant_rows(np.arange(1, nrows + 1), per, plant) - 1


def take_rows(ref_of, x, src):
    """rows of the reference of x[src] with zeros where src is -1; ref_of maps rows [k, n] to their float64 result [k, ...]"""
    src = np.asarray(src)
    out = ref_of(x[np.maximum(src, 0)])
    out[src < 0] = 0
    return out


SOS_N, FILTFILT_PAD = 40, 9


def sos_design(K):
    """K sections: a band-pass of order K (the reference's butter_bandpass shape at K = 3), wide enough to settle within 40 samples"""
    import scipy.signal as ss
    return ss.butter(K, [0.05, 0.3], btype="band", output="sos")


def sos_zi(sos, x64):
    import scipy.signal as ss
    return ss.sosfilt_zi(sos)[:, None, :] * x64[:, 0][None, :, None]         # (K, rows, 2)


PFB_M, PFB_P, PFB_HOP, PFB_FRAMES = 8, 2, 8, 5
DDC_Q, DDC_T, DDC_NU, DDC_N0, DDC_N = 4, 33, 0.1234, 12345, 300
UPF_UP, UPF_DOWN, UPF_T, UPF_N = 3, 2, 31, 200
CZT_N, CZT_M = 8100, 100
CZT_SMALL_N, CZT_SMALL_M = 8, 5
