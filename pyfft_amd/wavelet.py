"""Continuous wavelet transform on the GPU (Torrence & Compo 1998; the transform the reference package looks for as `pycwt`).

    W_n(s) = sum_k x^_k psi^*(s w_k) exp(i w_k n dt),   psi^(s w) = sqrt(2 pi s / dt) psi0^(s w)

as a LINEAR convolution of the record with every scale's wavelet: the record is zero-extended, nothing wraps around (pycwt pads to
next_pow2(N) only and wraps).  Morlet and Paul wavelets (analytic: the filter is zero at and below 0 and above Nyquist).

Two paths, chosen per scale and reported by cwt_plan:
  fused     engine.cwt (k_cwt): overlap-save frames of L samples with a margin M on either side.  The margin of a scale is measured, not
            assumed: g_s = ifft(H_s) on a grid of 2^18 points in float64, M_s = the smallest M with sum_{|n| >= M} |g_s[n]| <= tail x
            sum |g_s|.  A scale fuses if M_s <= 3072; all fused scales of a call share M = max M_s and the smallest L >= 4 M.
  composed  scales that do not fuse -- the long ones, and the ones so close to Nyquist that the cut of the filter there gives g_s tails
            that fall off like 1 / n (Morlet-6 below s = 3.7 dt) -- take engine.fft of the record zero-padded to next_pow2(2 N), a
            broadcast multiply with the filter rows and batched engine.ifft, a chunk of scales at a time.

Two records: xwt (the cross-wavelet transform Wx conj(Wy)) and wct (wavelet coherence and phase after Torrence & Webster 1999), on the
same frames with the margin of the time-smoothing Gaussian added to the wavelet's (engine.wct_time, engine.wct_scale; k_wct.hip); see
the section at the end of this module.

numpy in -> numpy out; device tensor in -> device tensors on x's stream.  There is no CPU implementation behind these functions.
xwt and wct differ from the rest in one respect: where torch has a GPU, numpy records are copied to torch's current device, run the
device-tensor path on torch's current stream and are copied back (_on_device), so that both calling modes give the same bits -- the
glue between the library calls of the whole-record path is then the same code -- and T never crosses to the host.  Without torch, or
without a GPU visible to it, numpy records take the library's host path with numpy glue, as cwt's do; the results then agree with the
device mode to rounding, not bit for bit.
"""
import functools
import math

import numpy as np

from . import engine as E
from .engine import CwtRefused, _is_torch

try:
    import torch
except Exception:                       # pragma: no cover
    torch = None

MARGIN_GRID = 1 << 18
FUSED_MAX_MARGIN = 3072
COMPOSED_MAX_NFULL = 1 << 26
COMPOSED_CHUNK_BYTES = 256 << 20        # spectra of one chunk of scales on the composed path


class Morlet:
    """Morlet wavelet, psi0^(u) = pi^(-1/4) exp(-(u - w0)^2 / 2) for u > 0."""
    family = "morlet"

    def __init__(self, w0=6.0):
        self.w0 = self.param = float(w0)
        if not (0.0 < self.w0 <= 64.0):
            raise CwtRefused("Morlet: w0 = %r must lie in (0, 64]" % (w0,))

    def psi_ft(self, u):
        u = np.asarray(u, dtype=np.float64)
        return np.where(u > 0, math.pi ** -0.25 * np.exp(-0.5 * (u - self.w0) ** 2), 0.0)

    def flambda(self):
        """Fourier period / scale."""
        return 4.0 * math.pi / (self.w0 + math.sqrt(2.0 + self.w0 ** 2))

    def coi(self):
        """e-folding time / scale."""
        return math.sqrt(2.0)

    def psi0(self):
        """psi0(0)."""
        return math.pi ** -0.25

    def __repr__(self):
        return "Morlet(%g)" % self.w0


class Paul:
    """Paul wavelet, psi0^(u) = 2^m / sqrt(m (2m - 1)!) u^m exp(-u) for u > 0."""
    family = "paul"

    def __init__(self, m=4):
        self.m = self.param = float(m)
        if not (1.0 <= self.m <= 64.0):
            raise CwtRefused("Paul: m = %r must lie in [1, 64]" % (m,))

    def psi_ft(self, u):
        u = np.asarray(u, dtype=np.float64)
        m = self.m
        lognorm = m * math.log(2.0) - 0.5 * (math.log(m) + math.lgamma(2.0 * m))
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.exp(lognorm + m * np.log(np.where(u > 0, u, 1.0)) - u)
        return np.where(u > 0, v, 0.0)

    def flambda(self):
        return 4.0 * math.pi / (2.0 * self.m + 1.0)

    def coi(self):
        return 1.0 / math.sqrt(2.0)

    def psi0(self):
        m = self.m
        return math.exp(m * math.log(2.0) + math.lgamma(m + 1.0) - 0.5 * (math.log(math.pi) + math.lgamma(2.0 * m + 1.0)))

    def __repr__(self):
        return "Paul(%g)" % self.m


def _wavelet(w):
    if isinstance(w, (Morlet, Paul)):
        return w
    raise CwtRefused("wavelet %r is not built: Morlet(w0) or Paul(m) (analytic wavelets; DOG is not)" % (w,))


def filter_rows(wavelet, scales, L):
    """H_s[k] = sqrt(2 pi s') psi0^(s' w_k) on a grid of L points, float64 [S, L]; scales in samples."""
    s = np.asarray(scales, dtype=np.float64).reshape(-1, 1)
    k = np.arange(L)
    w = 2.0 * math.pi * k / L
    H = np.sqrt(2.0 * math.pi * s) * wavelet.psi_ft(s * w[None, :])
    H[:, k > L // 2] = 0.0
    H[:, 0] = 0.0
    return H


@functools.lru_cache(maxsize=4096)
def _margin_cached(family, param, s, tail):
    wv = Morlet(param) if family == "morlet" else Paul(param)
    G = MARGIN_GRID
    a = np.abs(np.fft.ifft(filter_rows(wv, [s], G)[0]))
    c = a[:G // 2 + 1].copy()                      # by distance |n| = 0 .. G / 2
    c[1:G // 2] += a[:G // 2:-1]
    tails = np.cumsum(c[::-1])[::-1]               # tails[M] = sum over |n| >= M
    ok = np.nonzero(tails <= tail * tails[0])[0]
    return int(ok[0]) if ok.size else G // 2 + 1


def margin(wavelet, s, tail=1e-6):
    """The smallest M with sum_{|n| >= M} |g_s[n]| <= tail sum |g_s|, g_s = ifft(H_s) on 2^18 points; s in samples."""
    wv = _wavelet(wavelet)
    return _margin_cached(wv.family, wv.param, float(s), float(tail))


def cwt_scales(n, dt, dj=1.0 / 12, s0=None, J=None, wavelet=None, tail=1e-6):
    """s_j = s0 2^(j dj), j = 0 .. J, in the units of dt.  s0 defaults to the smallest scale the fused path takes for this wavelet (not
    T&C's customary 2 dt, which lies where the Nyquist cut spoils the wavelet's decay), J to log2(n dt / s0) / dj."""
    if not (dt > 0 and dj > 0 and n >= 1):
        raise ValueError("cwt_scales: n >= 1, dt > 0 and dj > 0 are required")
    if s0 is None:
        s0 = smallest_fused_scale(Morlet(6.0) if wavelet is None else wavelet, tail) * dt
    if not s0 > 0:
        raise ValueError("cwt_scales: s0 must be positive")
    if J is None:
        J = max(int(math.floor(math.log2(max(n * dt / s0, 1.0)) / dj)), 0)
    if J < 0:
        raise ValueError("cwt_scales: J must not be negative")
    return s0 * 2.0 ** (np.arange(int(J) + 1) * dj)


@functools.lru_cache(maxsize=64)
def _smallest_fused(family, param, tail):
    wv = Morlet(param) if family == "morlet" else Paul(param)

    def settled(s):                                   # fused, and past the Nyquist step's reach: from here on margins grow with the scale
        m = _margin_cached(family, param, s, tail)
        return m <= FUSED_MAX_MARGIN and m <= _margin_cached(family, param, 2.0 * s, tail)
    lo, hi = 0.25, 32.0
    if not settled(hi):
        raise CwtRefused("%r: no scale up to 32 samples fuses at tail = %g" % (wv, tail))
    for _ in range(24):
        mid = math.sqrt(lo * hi)
        if settled(mid):
            hi = mid
        else:
            lo = mid
    return math.ceil(hi * 1.02 * 100.0) / 100.0      # a little above the threshold, rounded up to 1 / 100 sample


def smallest_fused_scale(wavelet, tail=1e-6):
    """The smallest scale (in samples) from which on the margin rule lets scales fuse and the margins grow with the scale: below it the
    filter's step at Nyquist gives g_s tails that fall off like 1 / n, and the margin is of the order of the grid."""
    wv = _wavelet(wavelet)
    return _smallest_fused(wv.family, wv.param, float(tail))


def cdelta(wavelet, scales, dt, dj):
    """The reconstruction factor C_delta of T&C eq. 11-13, computed from the actual scale set.  A line exp(i w n) has
    W_n(s) = sqrt(2 pi s') psi0^(s' w) exp(i w n), so eq. 11 returns it unchanged when
        C_delta = sqrt(2 pi) dj / (2 psi0(0)) sum_j psi0^(s'_j w)
    (the 2: a real record's line has half its amplitude at +w).  For a set that covers w the sum is (1 / ln 2) int psi0^(u) du / u, whatever
    w: 0.7774 for Morlet-6 and pi / (m ln 2) = 1.133 for Paul-4, T&C's 0.776 and 1.132.  It is evaluated at the middle of the set's band,
    w_c = u_peak / sqrt(s'_min s'_max).  (Eq. 13 read literally, with a unit sample as the probe, gives the same number only for a set
    that covers every frequency up to Nyquist -- scales well below 2 dt -- and 0.70 for Morlet-6 from 2 dt on, 0.36 from 4 dt on:
    reconstructions of anything inside the band would come out too large by that ratio.)"""
    wv = _wavelet(wavelet)
    sp = np.asarray(scales, dtype=np.float64) / dt
    wc = wv.param / math.sqrt(float(sp.min()) * float(sp.max()))
    return math.sqrt(2.0 * math.pi) * dj / (2.0 * wv.psi0()) * float(np.sum(wv.psi_ft(sp * wc)))


def recon_weights(wavelet, scales, dt, dj, cd=None):
    """w_j with x_n = sum_j w_j Re W_n(s_j) (T&C eq. 11)."""
    wv = _wavelet(wavelet)
    s = np.asarray(scales, dtype=np.float64)
    cd = cdelta(wv, s, dt, dj) if cd is None else float(cd)
    return dj * math.sqrt(dt) / (cd * wv.psi0()) / np.sqrt(s)


def cwt_plan(n, dt=1.0, dj=1.0 / 12, s0=None, J=None, wavelet=None, scales=None, tail=1e-6, rows=1):
    """What cwt would do for a record of n samples: the scales (units of dt), every scale's margin (samples) and path ('fused' or
    'composed'), M, L and hop of the fused call (None without fused scales), n_full of the composed path (None without composed
    scales), and the bytes W takes.  Host only."""
    wv = Morlet(6.0) if wavelet is None else _wavelet(wavelet)
    n = int(n)
    if n < 1:
        raise CwtRefused("cwt_plan: the record must hold at least one sample")
    sc = cwt_scales(n, dt, dj, s0, J, wv, tail) if scales is None else np.asarray(scales, dtype=np.float64)
    if sc.ndim != 1 or sc.size < 1 or not np.all(np.isfinite(sc)) or not np.all(sc > 0):
        raise CwtRefused("cwt_plan: scales must be one-dimensional, positive and finite")
    sp = sc / dt
    margins = np.array([margin(wv, s, tail) for s in sp], dtype=np.int64)
    fused = margins <= FUSED_MAX_MARGIN
    plan = dict(scales=sc, margins=margins, fused=fused, path=np.where(fused, "fused", "composed"), M=None, L=None, hop=None,
                n_full=None, frames=None, bytes_written=8 * int(rows) * sc.size * n, wavelet=wv, tail=tail)
    if fused.any():
        M = int(margins[fused].max())
        L = E.CWT_MIN_L
        while L < 4 * M and L < E.CWT_MAX_L:
            L *= 2
        plan.update(M=M, L=L, hop=L - 2 * M, frames=-(-n // (L - 2 * M)))
    if (~fused).any():
        n_full = 1 << max(int(2 * n - 1).bit_length(), 1)
        if n_full > COMPOSED_MAX_NFULL:
            raise CwtRefused("cwt: %d of the scales do not fuse (margins above %d samples: near Nyquist, or long) and their whole-record "
                             "path needs a transform of %d points, above 2^26: decimate the record with resample_poly first"
                             % (int((~fused).sum()), FUSED_MAX_MARGIN, n_full))
        plan["n_full"] = n_full
    return plan


def _prep(x):
    if _is_torch(x):
        if x.dtype not in (torch.float32, torch.complex64):
            raise TypeError("device path takes float32 or complex64 samples, got %s" % x.dtype)
        return x, x.dtype == torch.complex64
    from ._ffi import as_samples
    x = as_samples(x)
    return x, x.dtype == np.complex64


def _filter_rows_device(wv, sp, n_full, device):
    """filter_rows as float32 rows on the device, formed there in float64 (the bins 1 .. n_full / 2; the rest stays zero)"""
    k = torch.arange(1, n_full // 2 + 1, dtype=torch.float64, device=device)
    s = torch.as_tensor(np.asarray(sp, dtype=np.float64), device=device)[:, None]
    u = s * (2.0 * math.pi / n_full) * k[None, :]
    if wv.family == "morlet":
        e = -0.25 * math.log(math.pi) - 0.5 * (u - wv.w0) ** 2
    else:
        e = wv.m * math.log(2.0) - 0.5 * (math.log(wv.m) + math.lgamma(2.0 * wv.m)) + wv.m * torch.log(u) - u
    H = torch.zeros((len(sp), n_full), dtype=torch.float32, device=device)
    H[:, 1:n_full // 2 + 1] = (torch.sqrt(2.0 * math.pi * s) * torch.exp(e)).float()
    return H


def _composed_chunks(x, wv, sp, n_full):
    """The whole-record path: yields (index range, W chunk [..., len, N] complex64) for the scales sp (in samples)."""
    n = int(x.shape[-1])
    dev = _is_torch(x)
    if dev:
        xp = torch.zeros(tuple(x.shape[:-1]) + (n_full,), dtype=torch.complex64, device=x.device)
        xp[..., :n] = x
    else:
        xp = np.zeros(x.shape[:-1] + (n_full,), dtype=np.complex64)
        xp[..., :n] = x
    X = E.fft(xp)
    rows = max(int(np.prod(x.shape[:-1], dtype=np.int64)), 1)
    per = max(int(COMPOSED_CHUNK_BYTES // (8 * n_full * rows)), 1)
    for i0 in range(0, len(sp), per):
        if dev:
            H = _filter_rows_device(wv, sp[i0:i0 + per], n_full, x.device)
        else:
            H = filter_rows(wv, sp[i0:i0 + per], n_full).astype(np.float32)
        yield i0, i0 + H.shape[0], E.ifft(X[..., None, :] * H)[..., :n]


def _ix(x, idx):
    """an index array in the form x's container takes"""
    return torch.as_tensor(idx, device=x.device) if _is_torch(x) else idx


def _fused_args(plan, dt):
    idx = np.nonzero(plan["fused"])[0]
    return idx, plan["scales"][idx] / dt


def cwt(x, dt=1.0, dj=1.0 / 12, s0=None, J=None, wavelet=None, scales=None, tail=1e-6):
    """-> (W, scales, freqs, coi): W complex64 [..., S, N] along the last axis of x, the scales (units of dt), the equivalent Fourier
    frequencies 1 / (flambda s), and the cone of influence as a Fourier period per sample: the period whose e-folding time reaches the
    nearer end of the record."""
    x, _ = _prep(x)
    n = int(x.shape[-1])
    rows = max(int(np.prod(x.shape[:-1], dtype=np.int64)), 1)
    plan = cwt_plan(n, dt, dj, s0, J, wavelet, scales, tail, rows)
    wv, sc = plan["wavelet"], plan["scales"]
    idx, spf = _fused_args(plan, dt)
    Wf = None
    if idx.size:
        Wf = E.cwt(x, spf, wv.family, wv.param, plan["L"], plan["M"], W=True)["W"]
    if idx.size == sc.size:
        W = Wf
    else:
        shape = tuple(x.shape[:-1]) + (sc.size, n)
        W = torch.empty(shape, dtype=torch.complex64, device=x.device) if _is_torch(x) else np.empty(shape, dtype=np.complex64)
        if Wf is not None:
            W[..., _ix(x, idx), :] = Wf
        cidx = np.nonzero(~plan["fused"])[0]
        for a, b, Wc in _composed_chunks(x, wv, sc[cidx] / dt, plan["n_full"]):
            W[..., _ix(x, cidx[a:b]), :] = Wc
    freqs = 1.0 / (wv.flambda() * sc)
    edge = dt * (n / 2.0 - np.abs(np.arange(n) - (n - 1) / 2.0))
    return W, sc, freqs, wv.flambda() * edge / wv.coi()


def icwt(W, scales, dt=1.0, dj=1.0 / 12, wavelet=None, real=True):
    """The reconstruction of T&C eq. 11 from a materialised W [..., S, N]: dj sqrt(dt) / (C_delta psi0(0)) sum_j Re W_n(s_j) / sqrt(s_j),
    C_delta computed from the scale set given.  real=False keeps the complex sum (complex records: their positive-frequency half)."""
    wv = Morlet(6.0) if wavelet is None else _wavelet(wavelet)
    y = E.icwt_sum(W, recon_weights(wv, scales, dt, dj))
    return y.real if real else y


def _band_mask(sc, band):
    if band is None:
        return np.ones(sc.size, dtype=bool)
    lo, hi = band
    m = (sc >= lo) & (sc <= hi)
    if not m.any():
        raise CwtRefused("no scale lies in the band %r" % (band,))
    return m


def cwt_power(x, dt=1.0, dj=1.0 / 12, s0=None, J=None, wavelet=None, scales=None, tail=1e-6, band=None):
    """-> (gws, scales) or, with band=(smin, smax), (gws, scales, bandpow): the global wavelet spectrum (1 / N) sum_n |W_n(s)|^2
    (T&C eq. 22), float64 [..., S], and the scale-averaged power dj dt / C_delta sum_{s_j in band} |W_n(s_j)|^2 / s_j (eq. 24), float32
    [..., N].  W is never materialised for the fused scales; the composed ones are reduced a chunk at a time."""
    x, _ = _prep(x)
    n = int(x.shape[-1])
    rows = max(int(np.prod(x.shape[:-1], dtype=np.int64)), 1)
    plan = cwt_plan(n, dt, dj, s0, J, wavelet, scales, tail, rows)
    wv, sc = plan["wavelet"], plan["scales"]
    dev = _is_torch(x)
    wb = None
    if band is not None:
        wb = np.where(_band_mask(sc, band), dj * dt / (cdelta(wv, sc, dt, dj) * sc), 0.0)
    lead = tuple(x.shape[:-1])
    gws = torch.empty(lead + (sc.size,), dtype=torch.float64, device=x.device) if dev else np.empty(lead + (sc.size,))
    bp = None
    idx, spf = _fused_args(plan, dt)
    if idx.size:
        r = E.cwt(x, spf, wv.family, wv.param, plan["L"], plan["M"], W=False, gws=True, bandpow=None if wb is None else wb[idx])
        gws[..., _ix(x, idx)] = r["gws"]
        bp = r.get("bandpow")
    if idx.size < sc.size:
        cidx = np.nonzero(~plan["fused"])[0]
        for a, b, Wc in _composed_chunks(x, wv, sc[cidx] / dt, plan["n_full"]):
            if dev:
                p = (Wc.real.double() ** 2 + Wc.imag.double() ** 2)
                gws[..., _ix(x, cidx[a:b])] = p.sum(-1)
                add = None if wb is None else (p * torch.from_numpy(wb[cidx[a:b]]).to(x.device)[:, None]).sum(-2).float()
            else:
                p = Wc.real.astype(np.float64) ** 2 + Wc.imag.astype(np.float64) ** 2
                gws[..., cidx[a:b]] = p.sum(-1)
                add = None if wb is None else (p * wb[cidx[a:b], None]).sum(-2).astype(np.float32)
            if add is not None:
                bp = add if bp is None else bp + add
    gws = gws / n
    return (gws, sc) if band is None else (gws, sc, bp)


def cwt_filter(x, dt=1.0, dj=1.0 / 12, s0=None, J=None, wavelet=None, scales=None, tail=1e-6, band=None):
    """The reconstruction (T&C eq. 11, C_delta of the whole scale set) from the scales inside band=(smin, smax) alone: a constant-Q
    band-pass.  Fused scales never form W: the weighted sum is accumulated inside the transform's scale loop.  Real records give a
    real result, complex records the complex sum."""
    x, cplx = _prep(x)
    n = int(x.shape[-1])
    rows = max(int(np.prod(x.shape[:-1], dtype=np.int64)), 1)
    plan = cwt_plan(n, dt, dj, s0, J, wavelet, scales, tail, rows)
    wv, sc = plan["wavelet"], plan["scales"]
    w = np.where(_band_mask(sc, band), recon_weights(wv, sc, dt, dj), 0.0)
    dev = _is_torch(x)
    keep = (w != 0) & plan["fused"]
    y = None
    if keep.any():
        idx = np.nonzero(keep)[0]
        y = E.cwt(x, sc[idx] / dt, wv.family, wv.param, plan["L"], plan["M"], W=False, recon=w[idx])["recon"]
    rest = np.nonzero((w != 0) & ~plan["fused"])[0]
    if rest.size:
        for a, b, Wc in _composed_chunks(x, wv, sc[rest] / dt, plan["n_full"]):
            wc = w[rest[a:b]].astype(np.float32)
            add = (Wc * torch.from_numpy(wc).to(x.device)[:, None]).sum(-2) if dev else (Wc * wc[:, None]).sum(-2)
            y = add if y is None else y + add
    return y if cplx else y.real


# ---- cross-wavelet spectra and wavelet coherence (Torrence & Webster 1999; pycwt.xwt, pycwt.wct) --------------------------------------
#   Wxy = Wx conj(Wy);   a, b, c = |Wx|^2 / s', |Wy|^2 / s', Wxy / s' on the record, zero outside;
#   A, B, C = a, b, c smoothed along time by the unit-gain Gaussian of standard deviation s' samples (a LINEAR convolution: pycwt pads
#   to a power of two and wraps) and then across scales by the boxcar of 2 dj0 / dj rows with half weights at its ends;
#   R2 = |C|^2 / (A B), phase = atan2(Im C, Re C), both 0 where A B == 0.
# Fused scales run in engine.wct_time (k_wct_time): the frames of cwt with the margin Mw + Mg, Mg the Gaussian's reach by the tail rule of
# `margin`.  The others take the whole-record path; both write rows of one T, and one engine.wct_scale call smooths them together.

def gauss_rows(scales, L):
    """exp(-(s' w_k)^2 / 2) on a grid of L points, w_k the signed bin frequency, float64 [S, L]; scales in samples."""
    s = np.asarray(scales, dtype=np.float64).reshape(-1, 1)
    k = np.arange(L)
    w = 2.0 * math.pi * np.where(k <= L // 2, k, k - L) / L
    return np.exp(-0.5 * (s * w[None, :]) ** 2)


@functools.lru_cache(maxsize=4096)
def _smooth_margin_cached(s, tail):
    G = MARGIN_GRID
    a = np.abs(np.fft.ifft(gauss_rows([s], G)[0]))
    c = a[:G // 2 + 1].copy()
    c[1:G // 2] += a[:G // 2:-1]
    tails = np.cumsum(c[::-1])[::-1]
    ok = np.nonzero(tails <= tail * tails[0])[0]
    return int(ok[0]) if ok.size else G // 2 + 1


def smooth_margin(s, tail=1e-6):
    """The reach of the time-smoothing Gaussian of scale s (in samples) by the rule of `margin`: the smallest M with
    sum_{|n| >= M} |g[n]| <= tail sum |g|, g = ifft(exp(-(s w)^2 / 2)) on 2^18 points.  About 4.9 s at tail = 1e-6."""
    s = float(s)
    if not (s > 0 and math.isfinite(s)):
        raise E.WctRefused("smooth_margin: the scale must be positive and finite")
    return _smooth_margin_cached(s, float(tail))


def scale_window(dj, dj0=0.6):
    """The scale-smoothing taps: ones of length round(2 dj0 / dj) + 2 with both ends 0.5, normalised to sum 1."""
    if not (dj > 0 and dj0 > 0):
        raise E.WctRefused("scale_window: dj and dj0 must be positive")
    k = int(round(2.0 * dj0 / dj)) + 2
    if k > E.WCT_MAX_TAPS:
        raise E.WctRefused("scale_window: 2 dj0 / dj = %g rows are more than %d taps" % (2.0 * dj0 / dj, E.WCT_MAX_TAPS))
    win = np.ones(k)
    win[0] = win[-1] = 0.5
    return win / win.sum()


def _pair(x, y, who):
    x, cx = _prep(x)
    y, cy = _prep(y)
    if _is_torch(x) != _is_torch(y):
        raise TypeError("%s: x and y must both be arrays or both be device tensors" % who)
    if tuple(x.shape) != tuple(y.shape):
        raise E.WctRefused("%s: x and y must have equal shapes, got %r and %r" % (who, tuple(x.shape), tuple(y.shape)))
    if cx != cy:                            # one real, one complex: both run as complex
        if _is_torch(x):
            x, y = x.to(torch.complex64), y.to(torch.complex64)
        else:
            x, y = x.astype(np.complex64), y.astype(np.complex64)
    if x.ndim < 1 or x.shape[-1] < 1:
        raise E.WctRefused("%s: the records must hold at least one sample" % who)
    return x, y


def wct_plan(n, dt=1.0, dj=1.0 / 12, s0=None, J=None, wavelet=None, scales=None, tail=1e-6, rows=1):
    """What wct would do for records of n samples: the scales (units of dt), per scale the wavelet's margin, the Gaussian's margin
    (`margins_w`, `margins_g`, samples) and the path ('fused' or 'composed'); Mw, Mg, M = Mw + Mg, L, hop and frames of the fused call
    (None without fused scales); n_full (the wavelet transforms) and n_smooth (the time smoothing) of the composed path (None without
    composed scales); and the bytes of T.  A scale fuses if its own margins sum to at most 3072 samples.  Host only."""
    wv = Morlet(6.0) if wavelet is None else _wavelet(wavelet)
    if wv.family != "morlet":
        raise E.WctRefused("wct: the coherence is built for Morlet wavelets only (the smoothing operator is Torrence & Webster's for "
                           "Morlet; pycwt has none for the others), not %r" % (wv,))
    try:
        base = cwt_plan(n, dt, dj, s0, J, wv, scales, tail, rows)
    except CwtRefused as e:
        raise E.WctRefused(str(e).replace("cwt", "wct")) from None
    n, sc = int(n), base["scales"]
    sp = sc / dt
    mw = base["margins"]
    mg = np.array([smooth_margin(s, tail) for s in sp], dtype=np.int64)
    fused = mw + mg <= FUSED_MAX_MARGIN
    # the call's margins are the largest of either kind: a scale whose wavelet reaches far (near Nyquist) beside one whose Gaussian
    # does may push their sum past the limit; the scale with the longest wavelet then leaves the fused set
    while fused.any() and mw[fused].max() + mg[fused].max() > FUSED_MAX_MARGIN:
        cand = np.nonzero(fused)[0]
        fused[cand[np.argmax(mw[cand])]] = False
    plan = dict(scales=sc, margins_w=mw, margins_g=mg, fused=fused, path=np.where(fused, "fused", "composed"), Mw=None, Mg=None, M=None,
                L=None, hop=None, frames=None, n_full=None, n_smooth=None, bytes_T=16 * int(rows) * sc.size * n, wavelet=wv, tail=tail)
    if fused.any():
        Mw, Mg = int(mw[fused].max()), int(mg[fused].max())
        M = Mw + Mg
        L = E.CWT_MIN_L
        while L < 4 * M and L < E.CWT_MAX_L:
            L *= 2
        plan.update(Mw=Mw, Mg=Mg, M=M, L=L, hop=L - 2 * M, frames=-(-n // (L - 2 * M)))
    if (~fused).any():
        n_full = 1 << max(int(2 * n - 1).bit_length(), 1)
        n_smooth = 1 << max(int(n + int(mg[~fused].max()) - 1).bit_length(), 1)
        if max(n_full, n_smooth) > COMPOSED_MAX_NFULL:
            raise E.WctRefused("wct: %d of the scales do not fuse (margins above %d samples) and their whole-record path needs a transform "
                               "of %d points, above 2^26: decimate the records with resample_poly first"
                               % (int((~fused).sum()), FUSED_MAX_MARGIN, max(n_full, n_smooth)))
        plan.update(n_full=n_full, n_smooth=n_smooth)
    return plan


def _gauss_rows_device(sp, n_full, device):
    """gauss_rows as float32 rows on the device, formed there in float64"""
    k = torch.arange(n_full, dtype=torch.float64, device=device)
    w = (2.0 * math.pi / n_full) * torch.where(k <= n_full // 2, k, k - n_full)
    s = torch.as_tensor(np.asarray(sp, dtype=np.float64), device=device)[:, None]
    return torch.exp(-0.5 * (s * w[None, :]) ** 2).float()


def _smooth_composed(p, sp, n, n_smooth):
    """p [..., len, N] complex64 filtered along the last axis by every scale's Gaussian on a zero-padded grid of n_smooth points"""
    dev = _is_torch(p)
    if dev:
        pp = torch.zeros(tuple(p.shape[:-1]) + (n_smooth,), dtype=torch.complex64, device=p.device)
        G = _gauss_rows_device(sp, n_smooth, p.device)
    else:
        pp = np.zeros(p.shape[:-1] + (n_smooth,), dtype=np.complex64)
        G = gauss_rows(sp, n_smooth).astype(np.float32)
    pp[..., :n] = p
    return E.ifft(E.fft(pp) * G)[..., :n]


def _on_device(x, y):
    """numpy records as device tensors where torch has a GPU: the public functions then run their device path and copy the results
    back, so that both calling modes give the same bits (the glue between the library calls of the whole-record path is then the same
    code) and T never crosses to the host.  -> (x, y, host): host = the results go back to numpy."""
    if _is_torch(x):
        return x, y, False
    if torch is not None and torch.cuda.is_available():
        return torch.as_tensor(x, device="cuda"), torch.as_tensor(y, device="cuda"), True
    return x, y, False


def _back(v, host):
    return v.cpu().numpy() if host else v


def _composed_pairs(x, y, wv, sp, n_full):
    """the whole-record transforms of both records, chunk by chunk: (i0, i1, Wx, Wy)"""
    for (a, b, Wx), (_, _, Wy) in zip(_composed_chunks(x, wv, sp, n_full), _composed_chunks(y, wv, sp, n_full)):
        yield a, b, Wx, Wy


def xwt(x, y, dt=1.0, dj=1.0 / 12, s0=None, J=None, wavelet=None, scales=None, tail=1e-6):
    """The cross-wavelet transform -> (Wxy, scales, freqs, coi): Wxy = Wx conj(Wy), complex64 [..., S, N], of two records of equal
    shape; scales, freqs and coi as cwt gives them.  Morlet or Paul.  Unlike pycwt.xwt the records are NOT divided by their standard
    deviations: normalise them first if that is wanted.  Fused scales form neither Wx nor Wy in memory."""
    x, y = _pair(x, y, "xwt")
    n = int(x.shape[-1])
    rows = max(int(np.prod(x.shape[:-1], dtype=np.int64)), 1)
    plan = cwt_plan(n, dt, dj, s0, J, wavelet, scales, tail, rows)
    wv, sc = plan["wavelet"], plan["scales"]
    x, y, host = _on_device(x, y)
    idx, spf = _fused_args(plan, dt)
    Wf = None
    if idx.size:
        Wf = E.wct_time(x, y, spf, wv.family, wv.param, plan["L"], plan["M"], 0, xwt=True)
    if idx.size == sc.size:
        W = Wf
    else:
        shape = tuple(x.shape[:-1]) + (sc.size, n)
        W = torch.empty(shape, dtype=torch.complex64, device=x.device) if _is_torch(x) else np.empty(shape, dtype=np.complex64)
        if Wf is not None:
            W[..., _ix(x, idx), :] = Wf
        cidx = np.nonzero(~plan["fused"])[0]
        for a, b, Wx, Wy in _composed_pairs(x, y, wv, sc[cidx] / dt, plan["n_full"]):
            W[..., _ix(x, cidx[a:b]), :] = Wx * Wy.conj()
    freqs = 1.0 / (wv.flambda() * sc)
    edge = dt * (n / 2.0 - np.abs(np.arange(n) - (n - 1) / 2.0))
    return _back(W, host), sc, freqs, wv.flambda() * edge / wv.coi()


def wct(x, y, dt=1.0, dj=1.0 / 12, s0=None, J=None, wavelet=None, scales=None, tail=1e-6, dj0=0.6, return_spectra=False):
    """Wavelet coherence -> (R2, phase, scales, freqs, coi), with return_spectra=True followed by (A, B, C): R2 and phase float32
    [..., S, N] of two records of equal shape, the doubly smoothed spectra A, B (float32) and C (complex64).  Morlet only.  The scale
    smoothing spans round(2 dj0 / dj) + 2 rows of the scale set as given (dj is the caller's statement about an explicit `scales`).
    Monte-Carlo significance levels are not computed."""
    x, y = _pair(x, y, "wct")
    n = int(x.shape[-1])
    rows = max(int(np.prod(x.shape[:-1], dtype=np.int64)), 1)
    plan = wct_plan(n, dt, dj, s0, J, wavelet, scales, tail, rows)
    taps = scale_window(dj, dj0)
    wv, sc = plan["wavelet"], plan["scales"]
    x, y, host = _on_device(x, y)
    sp = sc / dt
    idx = np.nonzero(plan["fused"])[0]
    Tf = None
    if idx.size:
        Tf = E.wct_time(x, y, sp[idx], wv.family, wv.param, plan["L"], plan["Mw"], plan["Mg"])
    if idx.size == sc.size:
        T = Tf
    else:
        shape = tuple(x.shape[:-1]) + (sc.size, n, 4)
        T = torch.empty(shape, dtype=torch.float32, device=x.device) if _is_torch(x) else np.empty(shape, dtype=np.float32)
        if Tf is not None:
            T[..., _ix(x, idx), :, :] = Tf
        cidx = np.nonzero(~plan["fused"])[0]
        spc = sp[cidx]
        for a, b, Wx, Wy in _composed_pairs(x, y, wv, spc, plan["n_full"]):
            if _is_torch(x):
                inv = torch.as_tensor((1.0 / spc[a:b]).astype(np.float32), device=x.device)[:, None]
                p1 = torch.complex((Wx.real ** 2 + Wx.imag ** 2) * inv, (Wy.real ** 2 + Wy.imag ** 2) * inv)
            else:
                inv = (1.0 / spc[a:b]).astype(np.float32)[:, None]
                p1 = ((Wx.real ** 2 + Wx.imag ** 2) * inv + 1j * ((Wy.real ** 2 + Wy.imag ** 2) * inv)).astype(np.complex64)
            p2 = Wx * Wy.conj() * inv
            rows_i = _ix(x, cidx[a:b])
            for j, p in ((0, p1), (2, p2)):
                q = _smooth_composed(p, spc[a:b], n, plan["n_smooth"])
                # (through views of one component: an integer beside an index array is an advanced index in numpy, and with a
                # slice between the two the indexed axis would move to the front)
                re, im = T[..., j], T[..., j + 1]
                re[..., rows_i, :] = q.real
                im[..., rows_i, :] = q.imag
    out = tuple(_back(v, host) for v in E.wct_scale(T, taps, spectra=return_spectra))
    freqs = 1.0 / (wv.flambda() * sc)
    edge = dt * (n / 2.0 - np.abs(np.arange(n) - (n - 1) / 2.0))
    head = (out[0], out[1], sc, freqs, wv.flambda() * edge / wv.coi())
    return head + tuple(out[2:]) if return_spectra else head
