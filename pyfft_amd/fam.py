"""The FFT accumulation method (FAM; Roberts, Brown & Loomis 1991): the spectral correlation of the whole (f, alpha) plane on the GPU.

`cyclic.scd` estimates S^alpha(f) at cycle frequencies the caller already knows.  The first question about a record is which alpha it
has, and FAM is the standard blind search: a short channelizer (nchan channels at step hop), the products of channel pairs, and one
P-point transform along the frames of a block per pair.  Pair (k, l) of the plain form stands for f = (f_k + f_l) / 2 and gives the 2Q
cycle frequencies alpha = f_k - f_l + (j - Q) dalpha, dalpha = fs / (P hop), Q = P hop / (2 nchan): the ones within half a channel
spacing of the pair's own.  The conjugate form (conjugate=True, for IQ records) stands for f = (f_k - f_l) / 2 and alpha = f_k + f_l
+ (j - Q) dalpha.  The resolution in f is that of the channelizer, fs / nchan; in alpha it is dalpha, the same as a record of P hop
samples gives `scd`.  FAM tells where to point `scd`, which remains the precise tool at chosen alpha: FAM's cells away from the centre
of a tile are attenuated by the channelizer window's own response, and the tiles of one f row leave every other strip of alpha to the
neighbouring row (f rows lie fs / (2 nchan) apart, strips of one row 2 fs / nchan).

One kernel besides the STFT's (engine.fam, sp_fam, k_fam.hip); float32 sums over the blocks of a pass, float64 across passes, no
atomics: two calls agree bitwise.

What is not here: the strip spectral correlation analyzer (SSCA) and Fast-SC; leading axes (loop over them); channel counts, hops and
block lengths that are no power of two; hop above nchan.  Those raise FamRefused, which is a ValueError and a NotImplementedError.
"""
import collections

import numpy as np

from .windows import get_window
from . import engine as _engine
from .engine import FamRefused, _is_torch

FamPlane = collections.namedtuple("FamPlane", "pairs f alpha S Pw dalpha")
FamPlane.__doc__ = """pairs int32 [npairs, 2] (k, l: channel k of y against channel l of x, fft order); f [npairs] and alpha [npairs, 2Q] in Hz
(float64, numpy); S complex64 [npairs, 2Q]; Pw float32 [2, nchan]: the channel powers of x (row 0) and of y (row 1; the same without
y); dalpha = fs / (P hop).  S and Pw are numpy arrays or device tensors, as the record was."""


def _signed(k, nchan):
    return np.where(k < nchan // 2, k, k - nchan)


def fam_axes(pairs, nchan, Q, fs=1.0, conjugate=False):
    """f [npairs] and alpha [npairs, 2Q] (Hz) of a pair table, with dalpha = fs / (2 Q nchan) = fs / (P hop): the plain form f = (f_k + f_l) / 2,
    alpha = f_k - f_l + (j - Q) dalpha; the conjugate form f = (f_k - f_l) / 2, alpha = f_k + f_l + (j - Q) dalpha."""
    pr = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    ks, ls = _signed(pr[:, 0], nchan), _signed(pr[:, 1], nchan)
    s, d = (ks - ls, ks + ls) if conjugate else (ks + ls, ks - ls)
    f = s * (fs / (2.0 * nchan))
    # in whole bins first: alpha bin = d 2Q + j - Q of width fs / (2Q nchan)
    bins = d[:, None] * (2 * Q) + (np.arange(2 * Q)[None, :] - Q)
    return f, bins * (fs / (2.0 * Q * nchan))


def fam_pairs(nchan, alpha_band=None, f_band=None, real=False, conjugate=False):
    """The pair table int32 [npairs, 2], sorted by k: all nchan^2 pairs by default.  real=True keeps f >= 0 and alpha >= 0, a quarter: a
    real record gives S^{-alpha}(f) = conj S^{alpha}(f), and pair (k, l) repeats pair (-l, -k).  alpha_band = (lo, hi) and f_band =
    (lo, hi), in cycles per sample, keep the pairs whose tile (alpha within 1 / (2 nchan) of the pair's own, f within 1 / (2 nchan))
    meets them."""
    nchan = int(nchan)
    if nchan < _engine.FAM_MIN_N or nchan > _engine.FAM_MAX_N or nchan & (nchan - 1):
        raise FamRefused("fam_pairs: nchan = %d must be a power of two from %d to %d" % (nchan, _engine.FAM_MIN_N, _engine.FAM_MAX_N))
    k, l = np.meshgrid(np.arange(nchan), np.arange(nchan), indexing="ij")
    ks, ls = _signed(k, nchan), _signed(l, nchan)
    s, d = (ks - ls, ks + ls) if conjugate else (ks + ls, ks - ls)
    keep = np.ones((nchan, nchan), dtype=bool)
    if real:
        keep &= (s >= 0) & (d >= 0)
    half = 0.5 / nchan
    for band, centre, name in ((alpha_band, d / float(nchan), "alpha_band"), (f_band, s / (2.0 * nchan), "f_band")):
        if band is None:
            continue
        lo, hi = float(band[0]), float(band[1])
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise FamRefused("fam_pairs: %s must be (lo, hi) with lo <= hi" % name)
        keep &= (centre + half > lo) & (centre - half <= hi)
    pairs = np.stack([k[keep], l[keep]], axis=1).astype(np.int32)
    if pairs.shape[0] < 1 or pairs.shape[0] > _engine.FAM_MAX_PAIRS:
        raise FamRefused("fam_pairs: %d pairs are outside 1 .. 2^22: narrow the bands" % pairs.shape[0])
    return pairs


def _setup(who, nsig, fs, nchan, hop, nblock, window, taper, detrend, scaling):
    """(a, g float64, hop, P, nblocks, scale, detrend flag): everything refused here is refused before the library is touched"""
    if not np.isfinite(fs) or fs <= 0:
        raise FamRefused("%s: fs must be positive" % who)
    nchan = int(nchan)
    if nchan < _engine.FAM_MIN_N or nchan > _engine.FAM_MAX_N or nchan & (nchan - 1):
        raise FamRefused("%s: nchan = %d must be a power of two from %d to %d: other channel counts are not built"
                         % (who, nchan, _engine.FAM_MIN_N, _engine.FAM_MAX_N))
    hop = nchan // 4 if hop is None else int(hop)
    frames = (nsig - nchan) // hop + 1 if nsig >= nchan and hop >= 1 else 0
    if nblock is None:
        P = _engine.FAM_MAX_N
        while P > frames:
            P //= 2
    else:
        P = int(nblock)
    if P < _engine.FAM_MIN_N or (nblock is None and P * hop < 2 * nchan):
        raise FamRefused("%s: the record of %d samples holds no block of %d frames of %d at hop %d" % (who, nsig, max(P, _engine.FAM_MIN_N), nchan, hop))
    nblocks = frames // P if P > 0 else 0
    if nblocks < 1:
        raise FamRefused("%s: the record of %d samples holds no block of %d frames of %d at hop %d" % (who, nsig, P, nchan, hop))
    wins = []
    for w, n, name in ((window, nchan, "window"), (taper, P, "taper")):
        v = np.asarray(get_window(w, n) if isinstance(w, (str, tuple)) else w, dtype=np.float64)
        if v.shape != (n,) or not np.all(np.isfinite(v)) or not np.sum(v ** 2) > 0 or (name == "taper" and not np.sum(v) > 0):
            raise FamRefused("%s: the %s must hold %d finite values, not all zero" % (who, name, n))
        wins.append(v)
    a, g = wins
    if detrend not in (False, None, "none", 0, True, "constant", "mean", 1):
        raise FamRefused("%s: detrend must be False or 'constant' (the record's mean): per-segment and linear detrending are not built" % who)
    if scaling not in ("density", "spectrum"):
        raise FamRefused("%s: scaling must be 'density' or 'spectrum'" % who)
    _engine.fam_check(who, nchan, hop, P, nblocks, 1, nsig)
    scale = 1.0 / (fs * np.sum(a ** 2)) if scaling == "density" else 1.0 / np.sum(a) ** 2
    return a, g, hop, P, nblocks, scale / (nblocks * np.sum(g)), detrend not in (False, None, "none", 0)


def scd_fam(x, fs=1.0, nchan=256, hop=None, nblock=None, window="hamming", taper="hamming", detrend="constant", scaling="density", y=None,
            conjugate=False, alpha_band=None, f_band=None):
    """The spectral correlation of one record over the whole (f, alpha) plane by the FFT accumulation method -> FamPlane(pairs, f, alpha,
    S, Pw, dalpha).  nchan channels (a power of two) under `window` at step hop (default nchan / 4); blocks of nblock frames (a power of
    two, default the largest <= 8192 that fits the record) under `taper`, averaged over the whole blocks the record holds.  Scaled as
    scipy.signal.csd ('density': per Hz, 'spectrum'), so that pair (k, k) at the centre column Q is the Welch PSD of channel k.  A real
    record gets the pairs with f >= 0 and alpha >= 0; alpha_band and f_band (Hz) keep the pairs whose tile meets them.  y: the cross
    form S_yx; conjugate=True: x without the conjugate.  One record per call: loop over leading axes.  numpy in -> numpy out; device
    tensors in -> device tensors."""
    if x is None or getattr(x, "ndim", np.ndim(x)) != 1:
        raise FamRefused("scd_fam: x must be one record: leading axes are not built")
    if not _is_torch(x):
        x = np.asarray(x)
        y = None if y is None else np.asarray(y)
    nsig = int(x.shape[-1])
    a, g, hop, P, nblocks, scale, det = _setup("scd_fam", nsig, fs, nchan, hop, nblock, window, taper, detrend, scaling)
    nchan = int(a.size)
    cplx = x.is_complex() if _is_torch(x) else np.iscomplexobj(x)
    norm = lambda b: None if b is None else (float(b[0]) / fs, float(b[1]) / fs)
    pairs = fam_pairs(nchan, norm(alpha_band), norm(f_band), real=not cplx and y is None and not conjugate, conjugate=conjugate)
    S, Pwx, Pwy = _engine.fam(x, a, hop, g, nblocks, pairs, y=y, conj=bool(conjugate), detrend=det, scale=scale)
    Q = P * hop // (2 * nchan)
    f, alpha = fam_axes(pairs, nchan, Q, fs, conjugate)
    if _is_torch(S):
        import torch
        Pw = torch.stack([Pwx, Pwy])
    else:
        Pw = np.stack([Pwx, Pwy])
    return FamPlane(pairs, f, alpha, S, Pw, fs / (P * hop))


def fam_coherence(plane):
    """gamma = S / sqrt(Pw_y[k] Pw_x[l]) [npairs, 2Q], complex128, formed in float64 (0 where the denominator is 0); on the device when
    the plane is made of tensors."""
    pr = np.asarray(plane.pairs).astype(np.int64)
    S, Pw = plane.S, plane.Pw
    if _is_torch(S):
        import torch
        k, l = (torch.as_tensor(pr[:, i], device=S.device) for i in (0, 1))
        den = torch.sqrt(Pw[1].double()[k] * Pw[0].double()[l])[:, None]
        return torch.where(den > 0, S.to(torch.complex128) / torch.where(den > 0, den, torch.ones_like(den)),
                           torch.zeros_like(S, dtype=torch.complex128))
    Pw = np.asarray(Pw, dtype=np.float64)
    den = np.sqrt(Pw[1][pr[:, 0]] * Pw[0][pr[:, 1]])[:, None]
    return np.where(den > 0, np.asarray(S).astype(np.complex128) / np.where(den > 0, den, 1.0), 0.0)


def fam_profile(plane, reduce="mean"):
    """The alpha-domain profile of a plane: alphas (Hz, ascending, numpy) and the mean (or reduce='max') over f of |gamma|^2 per alpha bin,
    the alpha = 0 cells left out.  The reduction runs where the plane lives."""
    if reduce not in ("mean", "max"):
        raise FamRefused("fam_profile: reduce must be 'mean' or 'max'")
    bins = np.rint(np.asarray(plane.alpha) / plane.dalpha).astype(np.int64).ravel()
    keep = np.nonzero(bins != 0)[0]
    ub, inv = np.unique(bins[keep], return_inverse=True)
    gam = fam_coherence(plane)
    if _is_torch(gam):
        import torch
        g2 = (gam.abs() ** 2).reshape(-1)[torch.as_tensor(keep, device=gam.device)]
        idx = torch.as_tensor(inv, device=gam.device)
        out = torch.zeros(ub.size, dtype=torch.float64, device=gam.device)
        if reduce == "mean":
            out.index_add_(0, idx, g2)
            out /= torch.as_tensor(np.bincount(inv, minlength=ub.size), device=gam.device)
        else:
            out.scatter_reduce_(0, idx, g2, reduce="amax", include_self=True)
        return ub * plane.dalpha, out
    g2 = (np.abs(gam) ** 2).ravel()[keep]
    if reduce == "mean":
        out = np.bincount(inv, weights=g2, minlength=ub.size) / np.bincount(inv, minlength=ub.size)
    else:
        out = np.zeros(ub.size)
        np.maximum.at(out, inv, g2)
    return ub * plane.dalpha, out


def fam_cells(plane):
    """The plane as flat cells (f, alpha, S), each of npairs 2Q entries, for plotting and peak picking."""
    alpha = np.asarray(plane.alpha)
    return np.repeat(np.asarray(plane.f), alpha.shape[1]), alpha.ravel(), plane.S.reshape(-1)


def fam_plan(nsig, fs=1.0, nchan=256, hop=None, nblock=None, cplx=False, cross=False, conjugate=False, alpha_band=None, f_band=None):
    """What a call will do (host only): hop, nblock, nblocks, npairs, dalpha and sp_fam_plan's figures (Q, blocks_per_pass, passes,
    workgroups, scratch)."""
    a, _, hop, P, nblocks, _, _ = _setup("fam_plan", int(nsig), fs, nchan, hop, nblock, "hamming", "hamming", "constant", "density")
    norm = lambda b: None if b is None else (float(b[0]) / fs, float(b[1]) / fs)
    pairs = fam_pairs(a.size, norm(alpha_band), norm(f_band), real=not cplx and not cross and not conjugate, conjugate=conjugate)
    d = _engine.fam_plan(a.size, hop, P, nblocks, pairs.shape[0], cplx=cplx, cross=cross)
    d.update(hop=hop, nblock=P, nblocks=nblocks, npairs=int(pairs.shape[0]), dalpha=fs / (P * hop))
    return d
