"""Spectra of unevenly sampled records on the GPU: the generalised Lomb-Scargle periodogram (Lomb 1976; Scargle 1982; Zechmeister &
Kuerster 2009) as scipy.signal.lombscargle of scipy 1.15 defines it, for records with gaps -- dropped blocks, burst-mode lasers,
probe sweeps, merged shots with clocks of their own, housekeeping channels on a jittered clock -- that cannot be resampled to a grid
without inventing data.

At every frequency the periodogram is the least-squares fit of a sinusoid (with `floating_mean`, of a sinusoid and a constant) to the
weighted samples.  One kernel (engine.lomb, sp_lomb) takes three complex sums per frequency in one pass over the samples, one lane
per frequency, and a float64 finish step applies scipy's body to them; scipy's own O(N M) float64 product on the host materialises
N x M arrays.  On a uniform frequency grid the same sums are three type-1 NUFFTs (engine.lomb_sums_grid, sp_lomb_sums_grid; Press &
Rybicki 1989 in its modern form): O(N + M log M), taken with method='fast', or with method='auto' from the measured crossover on.  Times are float64 and may come in any order, with duplicates; the phases are taken from an origin near the record
(`t_ref`, by default the first sample), so a far time origin costs nothing.  Results are bitwise reproducible.

    lombscargle     scipy's signature and semantics (angular frequencies, one row)
    ls_periodogram  Hz, any leading axes of y over one t
    ls_window       the spectral window |sum w e^{2 pi i f t}|^2 of the sampling pattern: what to look at first in a gapped record
    ls_grid         a frequency grid from the record's span and mean rate
    ls_level        the level the normalised periodogram exceeds with probability p under white Gaussian noise
    ls_plan         how a shape is dealt to the device, and which path it takes
    uniform_grid    whether a frequency list is a uniform grid for a record: what method='fast' needs

What is not here: cross spectra and coherence between unevenly
sampled channels (the complex 'amplitude' form of several rows over one t is what to build them from); a segment-averaged
Lomb-Scargle; float64 or complex values on the device; rows with times of their own in one call; multi-term and multi-band models;
bootstrap false-alarm levels.  What is refused raises LombRefused, which is a ValueError and a NotImplementedError.
"""
import numpy as np

from . import engine as _engine
from .engine import LombRefused, _is_torch

TWO_PI = 2.0 * np.pi


def lombscargle(x, y, freqs, precenter=False, normalize=False, *, weights=None, floating_mean=False):
    """scipy.signal.lombscargle (scipy 1.15) on the GPU: sample times x, values y, ANGULAR frequencies freqs (rad per unit of x), all
    with one axis; the same ValueErrors for the same bad inputs.  Host arrays are taken as float64 and centred in float64 before they
    become float32 -- by their mean with `precenter`, by their weighted mean with `floating_mean` (which does not change the result);
    device tensors are x float64, y float32.  The phases are taken from x[0] inside the kernel."""
    dev = _is_torch(x)
    if dev:
        if not (_is_torch(y) and (weights is None or _is_torch(weights))):
            raise TypeError("lombscargle: x, y and weights must all be numpy arrays or all device tensors")
        xs, ys, ws = x, y, weights
        fr = freqs.detach().cpu().numpy() if _is_torch(freqs) else freqs
    else:
        xs, ys = np.asarray(x, dtype=np.float64), np.array(y, dtype=np.float64)
        ws = None if weights is None else np.asarray(weights, dtype=np.float64)
        fr = freqs
    fr = np.asarray(fr, dtype=np.float64)
    wshape = tuple(xs.shape) if ws is None else tuple(ws.shape)
    if not (len(xs.shape) == 1 and int(xs.shape[0]) > 0 and tuple(xs.shape) == tuple(ys.shape) == wshape):
        raise ValueError("Parameters x, y, weights must be 1-D arrays of equal non-zero length!")
    if not (fr.ndim == 1 and fr.size > 0):
        raise ValueError("Parameter freqs must be a 1-D array of non-zero length!")
    if ws is not None and not dev and not (np.all(ws >= 0) and np.sum(ws) > 0):
        raise ValueError("Parameter weights must have only non-negative entries which sum to a positive value!")
    if isinstance(normalize, (bool, np.bool_)):
        normalize = "normalize" if normalize else "power"
    if normalize not in ("power", "normalize", "amplitude"):
        raise ValueError("Normalize must be: False (or 'power'), True (or 'normalize'), or 'amplitude'.")
    if dev:
        if precenter:
            ys = ys - ys.mean()
    elif precenter:
        ys -= ys.mean()
    elif floating_mean:
        ys -= np.average(ys, weights=ws)
    return _engine.lomb(xs, ys, fr / TWO_PI, weights=ws, floating_mean=bool(floating_mean), normalize=normalize)


UNIFORM_TURNS = 1e-9          # method='fast': every f[k] within so many turns over the record's span of f[0] + k df


def _span(t):
    if _is_torch(t):
        return float(t.max() - t.min()) if t.numel() else 0.0
    tt = np.asarray(t, dtype=np.float64)
    return float(np.max(tt) - np.min(tt)) if tt.size else 0.0


def uniform_grid(t, f):
    """(f0, df, M) where the frequencies f are a uniform grid for the record t -- every |f[k] - (f[0] + k df)| span at most 1e-9 turns,
    df = (f[-1] - f[0]) / (M - 1) not zero -- and None where they are not (one frequency is a grid of any step)."""
    fv = np.asarray(f.detach().cpu().numpy() if _is_torch(f) else f, dtype=np.float64)
    if fv.ndim != 1 or fv.size < 1 or not np.all(np.isfinite(fv)):
        return None
    M = int(fv.size)
    if M == 1:
        return float(fv[0]), 1.0, 1
    df = float((fv[-1] - fv[0]) / (M - 1))
    if df == 0 or not np.isfinite(df):
        return None
    span = _span(t)
    if not np.isfinite(span) or np.max(np.abs(fv - (fv[0] + df * np.arange(M)))) * span > UNIFORM_TURNS:
        return None
    return float(fv[0]), df, M


def _path(who, method, t, f):
    """None for the direct sums, (f0, df, M) for the fast ones"""
    if method == "direct":
        return None
    if method not in ("fast", "auto"):
        raise LombRefused("%s: method must be 'direct', 'fast' or 'auto', not %r" % (who, method))
    grid = uniform_grid(t, f)
    if method == "fast":
        if grid is None:
            raise LombRefused("%s: method='fast' needs a uniform frequency grid: every f[k] within 1e-9 turns over the record's span "
                              "of f[0] + k df, df not zero" % who)
        return grid
    if grid is None:
        return None
    N = int(t.shape[-1]) if len(t.shape) else 0
    if N < 1 or N >= 1 << 31 or grid[2] > _engine.NUFFT_MAX_M:
        return None
    return grid if N * grid[2] >= _engine.nufft_plan(N, grid[2])["fast_min_pairs"] else None


def ls_periodogram(t, y, f, weights=None, floating_mean=True, normalize="normalize", t_ref=None, method="direct"):
    """The periodogram P [..., M] of the rows y[..., N] over one axis of times t[N] at the frequencies f[M] in Hz (cycles per unit of
    t); float32, or complex64 for normalize='amplitude': the best-fit a + ib of a cos + b sin referred to the origin of t.
    Accuracy: about 1e-6 of a row's largest value (held on the device to 6e-6) at frequencies from 1 / span on.  Below 1 / span a
    floating-mean fit is nearly degenerate -- the sinusoid, the constant and the record's window are close to collinear -- and
    amplifies the float32 rounding: at 1 / (5 span) the 'amplitude' form is good to 6e-5 of the row's largest value only (float32
    restatement, tests/test_host_lomb.py).  Those bins carry no independent information; scipy's float64 is what to use for them.
    method: 'direct' (the default: one (sample, frequency) pair at a time, any frequencies), 'fast' (three type-1 NUFFTs; f must be a
    uniform grid, see uniform_grid, and the result is that of the grid f[0] + k df itself; it differs from 'direct' by rounding,
    about 1e-6 of a row's largest value) or 'auto' ('fast' where f is uniform and N M is beyond the measured crossover)."""
    grid = _path("ls_periodogram", method, t if _is_torch(t) else np.asarray(t), f)
    if grid is None:
        return _engine.lomb(t, y, f, weights=weights, floating_mean=floating_mean, normalize=normalize, t_ref=t_ref)
    if y is None:
        raise LombRefused("ls_periodogram: y is required (ls_window takes the window's sums without rows)")
    f0, df, M = grid
    sums = _engine.lomb_sums_grid(t, y, f0, df, M, weights=weights, t_ref=t_ref)
    return _engine.lomb_finish(sums, f0 + df * np.arange(M), floating_mean=floating_mean, normalize=normalize)


def ls_window(t, f, weights=None, method="direct"):
    """The spectral window of the sampling pattern, |sum_n wn e^{2 pi i f (t_n - t_0)}|^2 with the weights normalised to sum to one
    (float64 [M]): 1 at f = 0, and near 1 again wherever the sampling repeats -- at the multiples of the rate of an even clock.  A
    line at f0 in the record shows up at f0 plus every peak of the window.  From the device's sums without rows; method as in
    ls_periodogram."""
    grid = _path("ls_window", method, t if _is_torch(t) else np.asarray(t), f)
    s = _engine.lomb_sums(t, None, f, weights=weights) if grid is None else _engine.lomb_sums_grid(t, None, *grid, weights=weights)
    W = s.totals[0]
    return (s.common[:, 0] ** 2 + s.common[:, 1] ** 2) / (W * W)


def ls_grid(t, oversample=5, nyquist_factor=1.0):
    """Frequencies (Hz) from 1 / (oversample span) in steps of as much up to nyquist_factor N / (2 span): `oversample` points per
    independent frequency 1 / span, up to nyquist_factor times the Nyquist frequency of an even clock of the same mean rate.
    The first oversample - 1 points lie below 1 / span, where a floating-mean periodogram in float32 is less accurate (see
    ls_periodogram): drop them (f[f >= 1 / span]) where the lowest bins matter."""
    tt = t.detach().cpu().numpy() if _is_torch(t) else np.asarray(t, dtype=np.float64)
    if tt.ndim != 1 or tt.size < 2 or not np.all(np.isfinite(tt)):
        raise LombRefused("ls_grid: t must be one axis of at least two finite times")
    span = float(np.max(tt) - np.min(tt))
    if not span > 0 or not oversample > 0 or not nyquist_factor > 0:
        raise LombRefused("ls_grid: the record needs a span, and oversample and nyquist_factor must be positive")
    df = 1.0 / (oversample * span)
    n = int(np.floor(nyquist_factor * tt.size / (2.0 * span) / df + 1e-9))
    if n < 1:
        raise LombRefused("ls_grid: the grid is empty")
    return df * np.arange(1, n + 1)


def ls_level(N, p, nindep=1):
    """The value z0 the normalised periodogram of N samples (normalize='normalize', with a floating mean or pre-centred) exceeds with
    probability p under white Gaussian noise.  At one frequency Prob(z > z0) = (1 - z0)^((N - 3) / 2) (Zechmeister & Kuerster 2009);
    over nindep independent frequencies the false-alarm probability is 1 - (1 - p1)^nindep.  nindep is the CALLER'S estimate: about
    span x bandwidth for a well-sampled record, and there is no exact figure for an uneven one."""
    N, nindep = int(N), float(nindep)
    if N < 4 or not 0.0 < p < 1.0 or not nindep >= 1:
        raise LombRefused("ls_level: need N >= 4, 0 < p < 1 and nindep >= 1")
    p1 = -np.expm1(np.log1p(-p) / nindep)                 # 1 - (1 - p)^(1 / nindep)
    return float(1.0 - p1 ** (2.0 / (N - 3)))


def ls_plan(N, M, rows=1, method=None):
    """How engine.lomb deals N samples, M frequencies and `rows` rows to the device (sp_lomb_plan, host only): rows_per_group,
    freqs_per_pass, passes, split (sample runs), workgroups.  With a method ('direct', 'fast', 'auto') also `path`, the path a uniform
    grid of that shape takes ('direct' or 'fast': 'auto' goes by N M against the measured crossover), and under `fast` the plan of the
    fast path's 1 + rows transforms (engine.nufft_plan)."""
    plan = _engine.lomb_plan(N, M, rows)
    if method is None:
        return plan
    if method not in ("direct", "fast", "auto"):
        raise LombRefused("ls_plan: method must be 'direct', 'fast' or 'auto', not %r" % (method,))
    try:
        fast = _engine.nufft_plan(N, M, int(rows) + 1)
    except _engine.NufftRefused as exc:
        raise LombRefused(str(exc))
    take = method == "fast" or (method == "auto" and int(N) * int(M) >= fast["fast_min_pairs"])
    return dict(plan, path="fast" if take else "direct", fast=fast)
