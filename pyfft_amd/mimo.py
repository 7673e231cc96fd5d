"""Conditioned spectral analysis of a probe array (Bendat & Piersol, Random Data, ch. 7): what several outputs owe to several correlated
inputs, and what is left of the coupling between two channels once the others are accounted for.  Everything is a solve on the
cross-spectral-density matrix G[i, j] = E[X_i conj X_j] of `engine.csd_matrix`, one matrix per frequency bin:

    A = G[order][:, order] + delta I = L L^H,     L = [[L_xx, 0], [L_yx, L_yy]]     (the first nin channels of `order` are the inputs)
    H    = L_yx L_xx^-1 = G_yx G_xx^-1            the response of the outputs to the inputs in Y = H X + N (the H1 estimator)
    Gc   = L_yy L_yy^H                            the CSD matrix of the outputs with the inputs' linear influence removed (the noise N)
    mcoh = sum_k |L_yx[i, k]|^2 / A_yy[i, i]      the multiple coherence of output i with all the inputs
    piv  = L_jj^2                                 the autospectrum of channel order[j] conditioned on those before it
    P    = A^-1                                   |P_ij|^2 / (P_ii P_jj): the partial coherence of i and j given all the rest

One kernel (k_cond.hip, C entries sp_cond and sp_cond_plan in include/spectral_mimo.h) factors a matrix per workgroup in LDS, in float64,
with every sum in a fixed order: two calls agree bitwise, numpy arrays and device tensors give the same bits, and the matrices of a
device tensor never visit the host.  `cond` is the low-level call on matrices from anywhere; `mimo_frf`, `multiple_coherence`,
`partial_coherence`, `conditioned_spectra` and `ordered_spectra` take records of real channels, at most 64 in total, under the
conventions of `spod` and `array_spectrum`."""
import math

import numpy as np

from . import _ffi
from . import engine as E
from .engine import _is_torch
from .spod import csd_segments, one_sided_csd

COND_MAX_N = 64
COND_WANT = {"H": 1, "Gc": 2, "mcoh": 4, "piv": 8, "P": 16}
COND_PLAN_NAMES = ("pitch", "threads", "lds_bytes", "raised", "workgroups", "items_per_workgroup", "w_offset", "diag_offset")


class CondRefused(ValueError, NotImplementedError):
    """A matrix, a split into inputs and outputs, an order, a loading or a set of outputs that the conditioned analysis does not take:
    outside the limits, and what is not built (more than 64 channels)."""


class CondResult:
    """What `cond` returns: H, Gc, mcoh, piv, P (None where not asked for) and status."""
    __slots__ = ("H", "Gc", "mcoh", "piv", "P", "status")

    def __init__(self, H=None, Gc=None, mcoh=None, piv=None, P=None, status=None):
        self.H, self.Gc, self.mcoh, self.piv, self.P, self.status = H, Gc, mcoh, piv, P, status

    def __repr__(self):
        return "CondResult(%s)" % ", ".join("%s=%s" % (k, None if getattr(self, k) is None else tuple(getattr(self, k).shape))
                                            for k in self.__slots__)


def _want_mask(who, want):
    if isinstance(want, str):
        want = (want,)
    want = tuple(want)
    if not want or any(w not in COND_WANT for w in want):
        raise CondRefused("%s: want must name some of 'H', 'Gc', 'mcoh', 'piv', 'P', not %r" % (who, want))
    mask = 0
    for w in want:
        mask |= COND_WANT[w]
    return mask


def cond_check(who, n, nin, order, loading, want, count=0):
    """The refusals of sp_cond and sp_cond_plan before the library is touched -> (order as int32 [n] or None, the mask of `want`)."""
    n, nin = int(n), int(nin)
    if n > COND_MAX_N:
        raise CondRefused("%s: order n = %d above %d is not built (one matrix lives in the LDS of one CU)" % (who, n, COND_MAX_N))
    if n < 1:
        raise CondRefused("%s: the order must be at least 1" % who)
    if not 0 <= nin <= n:
        raise CondRefused("%s: nin = %d is outside 0 .. n = %d" % (who, nin, n))
    loading = float(loading)
    if not (math.isfinite(loading) and loading >= 0.0):
        raise CondRefused("%s: loading must be finite and not negative" % who)
    mask = _want_mask(who, want)
    if count < 0 or count > 1 << 40:
        raise CondRefused("%s: %d matrices are outside 0 .. 2^40" % (who, count))
    if order is not None:
        if _is_torch(order):
            order = order.detach().cpu().numpy()
        o = np.asarray(order)
        if o.shape != (n,) or o.dtype.kind not in "iu" or sorted(int(v) for v in o) != list(range(n)):
            raise CondRefused("%s: order must be a permutation of 0 .. n - 1 = %d" % (who, n - 1))
        order = np.ascontiguousarray(o, dtype=np.int32)
    return order, mask


def cond(G, nin, order=None, loading=0.0, want=("H", "Gc", "mcoh", "piv"), check=True):
    """Conditioned analysis of the Hermitian matrices G[..., n, n], 1 <= n <= 64 (sp_cond: one Cholesky factor per matrix, in float64,
    one matrix per workgroup) -> CondResult(H, Gc, mcoh, piv, P, status).  The first nin channels of `order` (a permutation of 0 .. n - 1,
    default the identity) are the inputs, the other r = n - nin the outputs; A = G[order][:, order] + delta I with
    delta = loading max(Re trace, 0) / n.
      H      [..., r, nin] complex128   A_yx A_xx^-1, the least-squares response of the outputs to the inputs
      Gc     [..., r, r]   complex128   A_yy - A_yx A_xx^-1 A_xy, exactly Hermitian
      mcoh   [..., r]      float64      the multiple coherence of every output with all the inputs
      piv    [..., n]      float64      the autospectrum of channel order[j] conditioned on the channels before it
      P      [..., n, n]   complex128   A^-1, exactly Hermitian (only with 'P' in want)
      status [...]         int32        0, or the 1-based position in `order` of the first pivot that is not above n 2^-52 A_jj:
                                        <= nin the inputs are collinear (H, Gc, mcoh, P zeros, piv zero from there on, never NaN);
                                        > nin an output is explained completely (that pivot and its column are zero, P is zeros)
                                        (a NaN among the output rows also ends here, and the rows of Gc it touched carry it on)
    Outputs not named in `want` are None.  Only the LOWER triangle and the real part of the diagonal are read.  complex128 is native,
    other dtypes are cast.  check=True reads status back and raises numpy.linalg.LinAlgError naming the first matrix whose inputs are
    collinear; a zero output pivot does not raise.  nin = n is valid: no outputs, the precision matrix and piv only.
    numpy in -> numpy out; device tensors in -> device tensors on torch's current stream; the two agree bitwise."""
    who = "cond"
    shape = tuple(G.shape)
    if len(shape) < 2 or shape[-1] != shape[-2]:
        raise CondRefused("%s: G must be [..., n, n], got %s" % (who, shape))
    n, nin = int(shape[-1]), int(nin)
    lead, count = E._lead_rows(shape, 2)
    order, mask = cond_check(who, n, nin, order, loading, want, count)
    r = n - nin
    md = E._enter(G)
    g = md.cast(G, "complex128")
    out = {}
    for name, tail, dt in (("H", (r, nin), "complex128"), ("Gc", (r, r), "complex128"), ("mcoh", (r,), "float64"), ("piv", (n,), "float64"),
                           ("P", (n, n), "complex128")):
        out[name] = md.empty(lead + tail, dt, g) if mask & COND_WANT[name] else None
    st = md.empty(lead, "int32", g)

    def addr(a):
        return md.addr(a) if a is not None and count > 0 and (a.numel() if md.dev else a.size) > 0 else None
    if count:
        md.call(_ffi.lib().sp_cond, md.addr(g), n * n, n, count, _ffi.ptr(order), nin, mask, float(loading), addr(out["H"]), r * nin,
                addr(out["Gc"]), r * r, addr(out["mcoh"]), r, addr(out["piv"]), n, addr(out["P"]), n * n, md.addr(st))
    if check and count:                     # (the read-back of a device tensor waits for the stream)
        s = st.reshape(-1).cpu().numpy() if md.dev else st.reshape(-1)
        bad = (s > 0) & (s <= nin)
        if bad.any():
            first = int(np.argmax(bad))
            raise np.linalg.LinAlgError("cond: the inputs of matrix %s (flat index %d) are collinear: no pivot at position %d of the order"
                                        % (np.unravel_index(first, lead) if lead else (), first, int(s[first])))
    return CondResult(status=st, **out)


def cond_plan(n, nin, count=1, want=("H", "Gc", "mcoh", "piv")):
    """sp_cond_plan as a dict (host only): pitch (elements between the rows of the matrix in LDS), threads (of a workgroup), lds_bytes,
    raised (1: above 64 KiB, the launch raises the kernel's limit), workgroups (launched), items_per_workgroup (the most matrices one
    walks), w_offset and diag_offset (bytes: where the inverse factor and the kept diagonal lie)."""
    n, nin, count = int(n), int(nin), int(count)
    _, mask = cond_check("cond_plan", n, nin, None, 0.0, want, count)
    return E._plan(_ffi.lib().sp_cond_plan, COND_PLAN_NAMES, CondRefused, "cond_plan", n, nin, count, mask)


# ---- records ---------------------------------------------------------------------------------------------------------
def _channels(who, a, name):
    if len(a.shape) == 1:
        a = a.reshape(1, -1)
    if len(a.shape) != 2 or a.shape[0] < 1:
        raise CondRefused("%s: %s must be [nch, nsig] (or one record [nsig])" % (who, name))
    return a


def _record_csd(who, x, y, fs, window, nperseg, noverlap, detrend, band):
    """f[nb], G[nb, n, n] of the channels of x (then those of y) as `spod` forms it: a one-sided density, interior bins doubled"""
    x = _channels(who, x, "x")
    nx, ny = int(x.shape[0]), 0
    if y is not None:
        y = _channels(who, y, "y")
        ny = int(y.shape[0])
        if _is_torch(x) != _is_torch(y) or int(y.shape[1]) != int(x.shape[1]):
            raise CondRefused("%s: x and y must be of one kind and one length" % who)
    if nx + ny > COND_MAX_N:
        raise CondRefused("%s: %d channels in all; at most %d are built" % (who, nx + ny, COND_MAX_N))
    if y is not None:
        if _is_torch(x):
            import torch
            x = torch.cat((x, y.to(dtype=x.dtype, device=x.device)), dim=0)
        else:
            x = np.concatenate((np.asarray(x), np.asarray(y, dtype=np.asarray(x).dtype)), axis=0)
    win, hop, nframes, freq, b0, b1 = csd_segments(who, CondRefused, int(x.shape[1]), fs, window, nperseg, noverlap, band)
    return freq, one_sided_csd(x, win, hop, nframes, float(fs), detrend, b0, b1), nx, ny


def mimo_frf(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=True, band=None, loading=0.0):
    """f, H[nb, ny, nx], mcoh[nb, ny], Gnn[nb, ny, ny]: the frequency responses of the outputs y[ny, nsig] to the correlated inputs
    x[nx, nsig] in Y = H X + N (the H1 estimator G_yx G_xx^-1, MATLAB's tfestimate(.., 'mimo')), the multiple coherence of every output
    with all the inputs (mscohere(.., 'mimo')) and the CSD matrix of the noise N.  Real channels, nx + ny <= 64; the CSD matrix is
    `spod`'s: segments of nperseg under `window` every nperseg - noverlap samples (noverlap defaults to nperseg // 2), a one-sided
    density with the interior bins doubled; detrend is `engine.csd_matrix`'s (the mean of each channel's whole record);
    band = (f1, f2) keeps the bins f1 <= f <= f2.  Raises numpy.linalg.LinAlgError where the inputs are collinear at a bin; a loading
    (relative to the mean autospectrum) repairs that at the price of a bias."""
    f, G, nx, _ = _record_csd("mimo_frf", x, y, fs, window, nperseg, noverlap, detrend, band)
    res = cond(G, nx, None, loading, ("H", "Gc", "mcoh"))
    return f, res.H, res.mcoh, res.Gc


def multiple_coherence(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=True, band=None, loading=0.0):
    """f, mcoh[nb, ny]: the multiple coherence of every output of y[ny, nsig] with all the inputs x[nx, nsig] together: the share of the
    output's autospectrum that the best linear combination of the inputs explains.  Conventions as `mimo_frf`."""
    f, G, nx, _ = _record_csd("multiple_coherence", x, y, fs, window, nperseg, noverlap, detrend, band)
    return f, cond(G, nx, None, loading, ("mcoh",)).mcoh


def conditioned_spectra(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=True, band=None, loading=0.0):
    """f, Gyy_x[nb, ny, ny]: the CSD matrix of the outputs y with the linear influence of the inputs x removed (the residual, or noise,
    spectra: G_yy - G_yx G_xx^-1 G_xy), exactly Hermitian.  Conventions as `mimo_frf`."""
    f, G, nx, _ = _record_csd("conditioned_spectra", x, y, fs, window, nperseg, noverlap, detrend, band)
    return f, cond(G, nx, None, loading, ("Gc",)).Gc


def ordered_spectra(x, order=None, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=True, band=None, loading=0.0):
    """f, S[nb, n]: the ordered conditioned autospectra of the channels x[n, nsig]: S[:, j] is the autospectrum of channel order[j] with
    the linear influence of order[0 .. j - 1] removed (Bendat & Piersol's G_jj.(j-1)!); S[:, 0] is the plain autospectrum.
    Conventions as `mimo_frf`."""
    f, G, nx, _ = _record_csd("ordered_spectra", x, None, fs, window, nperseg, noverlap, detrend, band)
    return f, cond(G, nx, order, loading, ("piv",), check=False).piv


def partial_coherence(x, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend=True, band=None, loading=0.0):
    """f, pc[nb, n, n], mc[nb, n] of the channels x[n, nsig] from the precision matrix P = G^-1 at every bin:
    pc[:, i, j] = |P_ij|^2 / (P_ii P_jj), the coherence of channels i and j with the linear influence of all the others removed (1 on
    the diagonal) -- whether two probes are coupled, or only both driven by a third -- and mc[:, i] = 1 - 1 / (G_ii P_ii), the
    multiple coherence of channel i with all the others.  Conventions as `mimo_frf`; raises numpy.linalg.LinAlgError where the
    channels are collinear at a bin."""
    f, G, n, _ = _record_csd("partial_coherence", x, None, fs, window, nperseg, noverlap, detrend, band)
    P = cond(G, n, None, loading, ("P",)).P
    if _is_torch(P):
        import torch
        d = torch.diagonal(P, dim1=-2, dim2=-1).real
        gd = torch.diagonal(G, dim1=-2, dim2=-1).real
        gd = gd + float(loading) * torch.clamp(gd.sum(-1, keepdim=True), min=0.0) / n
        pc = (P.real ** 2 + P.imag ** 2) / (d[:, :, None] * d[:, None, :])
    else:
        d = np.diagonal(P, axis1=-2, axis2=-1).real
        gd = np.diagonal(G, axis1=-2, axis2=-1).real
        gd = gd + float(loading) * np.maximum(gd.sum(-1, keepdims=True), 0.0) / n
        pc = (P.real ** 2 + P.imag ** 2) / (d[:, :, None] * d[:, None, :])
    return f, pc, 1.0 - 1.0 / (gd * d)


def multiple_coherence_level(nd, nin, p=0.95):
    """The level the sample multiple coherence of an output with nin inputs exceeds with probability 1 - p when the true value is 0
    and nd INDEPENDENT segments are averaged: the sample value is Beta(nin, nd - nin) distributed (Goodman 1963), so the level is
    its p quantile; at nin = 1 that is `running.coherence_level(nd, 1 - p)`.  1 for nd <= nin, where every sample value is 1.
    Overlapped segments are not independent (Hann at 50 %: about 0.95 nd effective segments, fewer at more overlap), so for them the
    level is optimistic: too low.  No correction for the effective degrees of freedom is applied."""
    nd, nin, p = int(nd), int(nin), float(p)
    if nd < 1 or nin < 1:
        raise ValueError("multiple_coherence_level: nd and nin must be at least 1")
    if not 0.0 < p < 1.0:
        raise ValueError("multiple_coherence_level: p must lie in (0, 1)")
    if nd <= nin:
        return 1.0
    if nin == 1:
        from .running import coherence_level
        return coherence_level(nd, 1.0 - p)
    from scipy.special import betaincinv
    return float(betaincinv(nin, nd - nin, p))
