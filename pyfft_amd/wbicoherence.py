"""Wavelet bispectrum and wavelet bicoherence on the GPU (van Milligen, Hidalgo & Sanchez, Phys. Plasmas 2, 3017, 1995): quadratic
phase coupling resolved in time.

The Fourier bicoherence (`bicoherence`) needs hundreds of stationary frames; coupling that comes in bursts of a few wave periods is
averaged away.  Here the record is transformed with an analytic wavelet on a LINEAR frequency grid f_k = k df, k = k_lo .. k_hi (row i of
every array is k = k_lo + i; its scale is 1 / (flambda f_k), so the rows descend in scale), because only then does the sum of two
rows' frequencies lie on a row: m = i + j + k_lo.  Over a block of T samples

    B(i, j)  = (1/T) sum_n Wx[i, n] Wy[j, n] conj(Wz[m, n])
    b2(i, j) = |B|^2 / ( (1/T) sum_n |Wx[i, n] Wy[j, n]|^2  (1/T) sum_n |Wz[m, n]|^2 )      in [0, 1], 0 where the denominator is 0

with Wx, Wy, Wz exactly what `cwt(..., scales=s)` returns (its normalisation, a linear convolution over the zero-extended record).  B
and b2 are NaN where m > S - 1, the convention of `bispectrum`.  The transforms never exist as a whole: engine.wbic walks the record
in passes (k_cwt into scratch, k_wbic_tile over it).  Only scales that fuse are taken -- there is no composed path here -- and one
record (or triple of records) per call.

A significance level is not given: the closed form usually quoted, (fs / 2) / min(f1, f2, f1 + f2) / N, does not scale as stated
(DESIGN section 7); use surrogates.

numpy in -> numpy out; device tensors in -> device tensors on x's stream.  There is no CPU implementation behind these functions.
"""
import math

import numpy as np

from . import engine as E
from . import wavelet as W
from .engine import WbicRefused, _is_torch

try:
    import torch
except Exception:                       # pragma: no cover
    torch = None


def _wv(wavelet):
    if wavelet is None:
        return W.Morlet(6.0)
    if isinstance(wavelet, (W.Morlet, W.Paul)):
        return wavelet
    raise WbicRefused("wavelet %r is not built: Morlet(w0) or Paul(m) (analytic wavelets)" % (wavelet,))


def wbic_freqs(n, dt, df, fmin=None, fmax=None, wavelet=None, tail=1e-6):
    """-> (k_lo, k_hi, freqs, scales): the multiples k df of df inside [fmin, fmax] (defaults: df and the Nyquist frequency) whose
    scales 1 / (flambda k df) fuse by the margin rule of `wavelet.margin` -- the longest run of consecutive k that do, since rows must be
    consecutive multiples.  freqs ascend, scales (units of dt) descend."""
    wv = _wv(wavelet)
    n = int(n)
    if n < 1 or not (dt > 0) or df is None or not (df > 0) or not math.isfinite(df):
        raise WbicRefused("wbic_freqs: n >= 1, dt > 0 and a finite df > 0 are required")
    fmin = df if fmin is None else float(fmin)
    fmax = 0.5 / dt if fmax is None else float(fmax)
    k0 = max(int(math.ceil(fmin / df - 1e-9)), 1)
    k1 = int(math.floor(min(fmax, 0.5 / dt) / df + 1e-9))
    if k1 < k0:
        raise WbicRefused("wbic_freqs: no multiple of df = %g lies in [%g, %g]" % (df, fmin, fmax))
    if k1 - k0 + 1 > 1 << 16:
        raise WbicRefused("wbic_freqs: %d multiples of df lie in the band: choose a coarser df" % (k1 - k0 + 1))
    k = np.arange(k0, k1 + 1)
    sp = 1.0 / (wv.flambda() * k * df * dt)                     # scales in samples
    ok = np.array([W.margin(wv, s, tail) <= W.FUSED_MAX_MARGIN for s in sp])
    best, run = (0, 0), 0
    for i, v in enumerate(ok):
        run = run + 1 if v else 0
        if run > best[1]:
            best = (i - run + 1, run)
    if best[1] < 2:
        raise WbicRefused("wbic_freqs: fewer than two consecutive multiples of df = %g in [%g, %g] have scales that fuse" % (df, fmin, fmax))
    if best[1] > E.WBIC_MAX_S:                                  # the top of the band: the short scales are the cheap ones
        best = (best[0] + best[1] - E.WBIC_MAX_S, E.WBIC_MAX_S)
    k = k[best[0]:best[0] + best[1]]
    return int(k[0]), int(k[-1]), k * df, 1.0 / (wv.flambda() * k * df)


def _setup(who, n, dt, df, fmin, fmax, wavelet, tail, block, step, trim, span):
    wv = _wv(wavelet)
    k_lo, k_hi, f, sc = wbic_freqs(n, dt, df, fmin, fmax, wv, tail)
    plan = W.cwt_plan(n, dt, wavelet=wv, scales=sc, tail=tail)
    if not plan["fused"].all():                                 # (wbic_freqs returns fusing scales only)
        raise WbicRefused("%s: a scale does not fuse" % who)
    if trim and span is not None:
        raise WbicRefused("%s: trim and span exclude one another" % who)
    n0, n1 = 0, n
    if trim:
        n0 = int(math.ceil(wv.coi() * float(sc.max()) / dt))
        n1 = n - n0
    elif span is not None:
        n0, n1 = int(span[0]), int(span[1])
    if n0 < 0 or n1 > n or n1 - n0 < 1:
        raise WbicRefused("%s: the span [%d, %d) is empty or lies outside the %d samples" % (who, n0, n1, n))
    whole = block is None
    if whole:
        if step is not None:
            raise WbicRefused("%s: step without block" % who)
        block, step, nblocks = n1 - n0, n1 - n0, 1
    else:
        block = int(block)
        step = block if step is None else int(step)
        if block < 1 or step < 1 or block > n1 - n0:
            raise WbicRefused("%s: block = %d and step = %d must be at least 1 and a block fit the span of %d samples"
                              % (who, block, step, n1 - n0))
        nblocks = (n1 - n0 - block) // step + 1
    return dict(wavelet=wv, k_lo=k_lo, k_hi=k_hi, freqs=f, scales=sc, M=plan["M"], L=plan["L"], n0=n0, n1=n1, block=block, step=step,
                nblocks=nblocks, whole=whole, t=(n0 + step * np.arange(nblocks) + 0.5 * (block - 1)) * dt)


def wavelet_bispectrum(x, y=None, z=None, dt=1.0, df=None, fmin=None, fmax=None, wavelet=None, tail=1e-6, block=None, step=None,
                       trim=False, span=None):
    """-> (f, t, B, b2): the frequencies k df of the rows (wbic_freqs), the block centres, B complex128 and b2 float64
    [nblocks, S, S] -- [S, S] when block is None: one block over the span.  y and z default to x (the auto form, symmetric in
    (i, j)).  Blocks of `block` samples start every `step` samples (default: block) from the start of the span: the whole record,
    span=(n0, n1), or with trim=True the record without the e-folding time of the longest scale at either end.  Either
    step >= block or block % step == 0."""
    n = int(x.shape[-1]) if hasattr(x, "shape") and len(x.shape) else 0
    s = _setup("wavelet_bispectrum", n, dt, df, fmin, fmax, wavelet, tail, block, step, trim, span)
    wv = s["wavelet"]
    r = E.wbic(x, s["scales"] / dt, s["k_lo"], wv.family, wv.param, s["L"], s["M"], s["n0"], s["block"], s["step"], s["nblocks"], y=y, z=z)
    B, b2 = r["B"], r["b2"]
    if s["whole"]:
        return s["freqs"], float(s["t"][0]), B[0], b2[0]
    return s["freqs"], s["t"], B, b2


def wavelet_bicoherence(x, y=None, z=None, **kw):
    """-> (f, t, b2): wavelet_bispectrum without B."""
    f, t, _, b2 = wavelet_bispectrum(x, y, z, **kw)
    return f, t, b2


def _klo_of(b2):
    """k_lo from the valid region: row 0 holds S - k_lo valid pairs"""
    S = int(b2.shape[-1])
    if b2.ndim < 2 or int(b2.shape[-2]) != S or S < 2:
        raise WbicRefused("b2 must be [..., S, S] with S >= 2")
    row = b2[(0,) * (b2.ndim - 2) + (0,)]
    nan = torch.isnan(row) if _is_torch(b2) else np.isnan(row)
    return int(nan.sum())


def summed_bicoherence(b2):
    """The summed bicoherence of van Milligen et al.: per sum row m the mean of b2 over the valid pairs (i, j) with i + j + k_lo = m,
    [..., S]; NaN at the rows m < k_lo, which no pair sums to.  (i, j) and (j, i) both count, as they do in b2."""
    k_lo = _klo_of(b2)
    S = int(b2.shape[-1])
    dev = _is_torch(b2)
    out = torch.full(tuple(b2.shape[:-1]), float("nan"), dtype=b2.dtype, device=b2.device) if dev else np.full(b2.shape[:-1], np.nan)
    fl = torch.flip(b2, (-2,)) if dev else np.flip(b2, -2)
    for d in range(S - k_lo):                                   # the anti-diagonal i + j = d
        diag = torch.diagonal(fl, d - (S - 1), -2, -1) if dev else np.diagonal(fl, d - (S - 1), -2, -1)
        out[..., d + k_lo] = diag.mean(-1)
    return out


def total_bicoherence(b2):
    """The total bicoherence: the mean of b2 over all valid pairs, [...]."""
    _klo_of(b2)
    if _is_torch(b2):
        return torch.nanmean(b2, dim=(-2, -1))
    return np.nanmean(b2, axis=(-2, -1))


def wbic_plan(n, dt=1.0, df=None, fmin=None, fmax=None, wavelet=None, tail=1e-6, block=None, step=None, trim=False, span=None, nrec=1,
              sym=True):
    """What wavelet_bispectrum would do for a record of n samples (host only): k_lo, k_hi, S, M, L, n0, n1, block, step, nblocks, and
    engine.wbic_plan's cells, cell_len, groups, passes, workgroups, scratch, chunk, tiles."""
    s = _setup("wbic_plan", int(n), dt, df, fmin, fmax, wavelet, tail, block, step, trim, span)
    S = int(s["scales"].size)
    d = dict(k_lo=s["k_lo"], k_hi=s["k_hi"], S=S, M=s["M"], L=s["L"], n0=s["n0"], n1=s["n1"], block=s["block"], step=s["step"],
             nblocks=s["nblocks"])
    d.update(E.wbic_plan(n, S, s["k_lo"], s["L"], s["M"], s["n0"], s["block"], s["step"], s["nblocks"], nrec, sym))
    return d
