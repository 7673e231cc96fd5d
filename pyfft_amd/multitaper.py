"""Thomson multitaper spectra: every segment is windowed with K orthogonal tapers v_k (Slepian sequences by default) and the K
eigenspectra are averaged with weights c_k >= 0, sum c_k = 1.

    X_{g,k}[f] = FFT_nfft(v_k * xd[g*hop : g*hop + nfft])              xd = x detrended as a whole, hop = nfft - noverlap
    S_k[f]     = 1 / (M fs sum_n v_k[n]^2) * sum_g |X_{g,k}[f]|^2       eigenspectrum k over the M frames
    Pxx[f]     = sum_k c_k S_k[f]
    Pxy[f]     = sum_k c_k / (M fs sum_n v_k[n]^2) * sum_g conj(X_{g,k}[f]) Y_{g,k}[f]
    Cxy[f]     = |Pxy|^2 / (Pxx Pyy)                                    0 where the denominator is 0

Output conventions are scipy.signal.welch / csd / coherence with scaling='density': real input -> one-sided, f = rfftfreq(nfft, 1/fs),
every bin doubled but DC and (even nfft) Nyquist; complex input -> two-sided in natural FFT order, f = fftfreq(nfft, 1/fs).  S_k is
scipy.signal.welch(xd, window=v_k, detrend=False) by construction.  All K transforms of a frame run in one kernel that reads the
record once (k_mtaper.hip); the doubling is done here in float64.
"""
import numpy as np

from .windows import dpss

_DETRENDS = {"none": 0, "mean": 1, "linear": 2}
NFFT_MIN, MAX_WG_FFT, K_MAX = 8, 8192, 32          # MAX_WG_FFT: sp_max_wg_fft(), the largest one-workgroup transform


class SegmentTooLong(ValueError, NotImplementedError):
    """nfft beyond one workgroup transform: outside the limits, and a path that is not built."""


def _shape(v):
    """(ndim, size, complex?) of a numpy array, array-like or device tensor, without copying a tensor to the host."""
    if type(v).__module__.startswith("torch"):
        return v.dim(), v.numel(), v.is_complex()
    a = np.asarray(v)
    return a.ndim, a.size, np.iscomplexobj(a)


def multitaper_plan(nsig, cplx, fs=1.0, nfft=None, noverlap=0, NW=4.0, Kmax=None, weights="unity", tapers=None, detrend="mean"):
    """The validated host plan of a multitaper call (pure numpy, never loads the library): a dict with tapers (float64 [K, nfft]),
    weights (c_k, sum 1), energy (sum_n v_k^2), nfft, hop, nframes (M), detrend (device code), freq and, for the one-sided
    layout, fold (the factor of each bin: 2, but 1 at DC and at the Nyquist bin of an even nfft; ones for complex input)."""
    nsig = int(nsig)
    nfft = nsig if nfft is None else int(nfft)
    pow2 = nfft >= 1 and nfft & (nfft - 1) == 0
    if nfft < NFFT_MIN:
        raise ValueError("multitaper: nfft must be at least %d" % NFFT_MIN)
    if nfft > (MAX_WG_FFT if pow2 else MAX_WG_FFT // 2):
        raise SegmentTooLong("multitaper: segments beyond one workgroup transform (nfft %d; powers of two up to %d, other lengths "
                             "up to %d) are not supported" % (nfft, MAX_WG_FFT, MAX_WG_FFT // 2))
    noverlap = int(noverlap)
    if noverlap < 0 or noverlap >= nfft:
        raise ValueError("multitaper: need 0 <= noverlap < nfft")
    if nsig < nfft:
        raise ValueError("multitaper: the record (%d samples) is shorter than nfft (%d)" % (nsig, nfft))
    if not fs > 0:
        raise ValueError("multitaper: fs must be positive")
    if detrend not in _DETRENDS:
        raise ValueError("multitaper: detrend must be 'none', 'mean' or 'linear'")
    lam = None
    if tapers is None:
        NW = float(NW)
        if not 0 < NW < nfft / 2:
            raise ValueError("multitaper: need 0 < NW < nfft / 2")
        K = int(2 * NW) - 1 if Kmax is None else int(Kmax)
        if K > 2 * NW:
            raise ValueError("multitaper: Kmax must not exceed 2 NW")
        if not 1 <= K <= K_MAX:
            raise ValueError("multitaper: the number of tapers must lie in 1 .. %d" % K_MAX)
        v, lam = dpss(nfft, NW, K, sym=True, norm=2, return_ratios=True)
        v, lam = np.asarray(v, dtype=np.float64).reshape(K, nfft), np.asarray(lam, dtype=np.float64).reshape(K)
    else:
        v = np.asarray(tapers, dtype=np.float64)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2 or v.shape[1] != nfft:
            raise ValueError("multitaper: tapers must be a [K, nfft] array")
        K = v.shape[0]
        if not 1 <= K <= K_MAX:
            raise ValueError("multitaper: the number of tapers must lie in 1 .. %d" % K_MAX)
        if not np.all(np.isfinite(v)):
            raise ValueError("multitaper: tapers must be finite")
    energy = np.sum(v * v, axis=1)
    if not np.all(energy > 0):
        raise ValueError("multitaper: a taper is identically zero")
    if isinstance(weights, str):
        if weights == "unity":
            c = np.full(K, 1.0 / K)
        elif weights == "eigen":
            if lam is None:
                raise ValueError("multitaper: weights='eigen' needs the Slepian tapers (tapers=None)")
            c = lam / np.sum(lam)
        else:
            raise ValueError("multitaper: weights must be 'unity', 'eigen' or K numbers")
    else:
        c = np.asarray(weights, dtype=np.float64)
        if c.shape != (K,):
            raise ValueError("multitaper: weights must be 'unity', 'eigen' or K numbers")
        if not np.all(np.isfinite(c)) or np.any(c < 0) or not np.sum(c) > 0:
            raise ValueError("multitaper: weights must be non-negative, finite and not all zero")
        c = c / np.sum(c)
    hop = nfft - noverlap
    if cplx:
        freq, fold = np.fft.fftfreq(nfft, 1.0 / fs), np.ones(nfft)
    else:
        freq, fold = np.fft.rfftfreq(nfft, 1.0 / fs), np.full(nfft // 2 + 1, 2.0)
        fold[0] = 1.0
        if nfft % 2 == 0:
            fold[-1] = 1.0
    return dict(tapers=v, weights=c, energy=energy, eigenvalues=lam, nfft=nfft, hop=hop, nframes=1 + (nsig - nfft) // hop,
                detrend=_DETRENDS[detrend], freq=freq, fold=fold, fs=float(fs), cplx=bool(cplx))


def _plan_for(x, y, kw):
    sigs = [_shape(v) for v in (x, y) if v is not None]
    if any(ndim != 1 for ndim, _, _ in sigs):
        raise ValueError("multitaper: signals must be one-dimensional")
    if len({c for _, _, c in sigs}) != 1:
        raise ValueError("multitaper: x and y must both be real or both be complex")
    if len({n for _, n, _ in sigs}) != 1:
        raise ValueError("multitaper: x and y must have equal lengths")
    return multitaper_plan(sigs[0][1], sigs[0][2], **kw)


def _run(x, y, eigen, kw):
    """-> (plan, pxx, pyy, pxy, skx, sky) in the output layout (folded one-sided for real input)."""
    p = _plan_for(x, y, kw)
    from . import engine
    unit = p["tapers"] / np.sqrt(p["energy"])[:, None]
    if eigen:
        out = engine.multitaper(x, unit, p["hop"], p["nframes"], y=y, detrend=p["detrend"], weights=p["weights"], scale=1.0 / p["fs"])
    else:
        use = p["weights"] > 0                               # a taper of weight 0 adds nothing: not transformed
        rows = unit[use] * np.sqrt(p["weights"][use])[:, None]
        out = engine.multitaper(x, rows, p["hop"], p["nframes"], y=y, detrend=p["detrend"], scale=1.0 / p["fs"])
    fold = p["fold"]
    if not p["cplx"]:
        if type(out[0]).__module__.startswith("torch"):
            import torch
            fold = torch.as_tensor(fold, dtype=torch.float64, device=out[0].device)
        out = tuple(None if a is None else a * fold for a in out)
    return (p,) + tuple(out)


def _kw(fs, nfft, noverlap, NW, Kmax, weights, tapers, detrend):
    return dict(fs=fs, nfft=nfft, noverlap=noverlap, NW=NW, Kmax=Kmax, weights=weights, tapers=tapers, detrend=detrend)


def multitaper_psd(x, fs=1.0, nfft=None, noverlap=0, NW=4.0, Kmax=None, weights="unity", tapers=None, detrend="mean",
                   return_eigenspectra=False):
    """(f, Pxx[, Sk]): the multitaper PSD of x; Sk [K, nbins] are the unweighted eigenspectra, Pxx = sum_k c_k Sk[k].  nfft=None:
    one segment over the whole record.  numpy or array-like in -> numpy float64 out; device tensors in -> device tensors out."""
    p, pxx, _, _, skx, _ = _run(x, None, return_eigenspectra, _kw(fs, nfft, noverlap, NW, Kmax, weights, tapers, detrend))
    return (p["freq"], pxx, skx) if return_eigenspectra else (p["freq"], pxx)


def multitaper_spectra(x, y, fs=1.0, nfft=None, noverlap=0, NW=4.0, Kmax=None, weights="unity", tapers=None, detrend="mean",
                       return_eigenspectra=False):
    """(f, Pxx, Pyy, Pxy[, Skx, Sky]) of two records of equal length and kind from one transform pass; Pxy = sum conj(X) Y
    (scipy.signal.csd's convention), complex128."""
    if y is None:
        raise ValueError("multitaper_spectra: y is required")
    p, pxx, pyy, pxy, skx, sky = _run(x, y, return_eigenspectra, _kw(fs, nfft, noverlap, NW, Kmax, weights, tapers, detrend))
    return (p["freq"], pxx, pyy, pxy, skx, sky) if return_eigenspectra else (p["freq"], pxx, pyy, pxy)


def multitaper_csd(x, y, fs=1.0, nfft=None, noverlap=0, NW=4.0, Kmax=None, weights="unity", tapers=None, detrend="mean"):
    """(f, Pxy): the multitaper cross spectral density."""
    f, _, _, pxy = multitaper_spectra(x, y, fs, nfft, noverlap, NW, Kmax, weights, tapers, detrend)
    return f, pxy


def multitaper_coherence(x, y, fs=1.0, nfft=None, noverlap=0, NW=4.0, Kmax=None, weights="unity", tapers=None, detrend="mean"):
    """(f, Cxy): the magnitude-squared coherence |Pxy|^2 / (Pxx Pyy), 0 where the denominator is 0."""
    f, pxx, pyy, pxy = multitaper_spectra(x, y, fs, nfft, noverlap, NW, Kmax, weights, tapers, detrend)
    den = pxx * pyy
    if type(den).__module__.startswith("torch"):
        import torch
        num = pxy.real ** 2 + pxy.imag ** 2
        return f, torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    num = pxy.real ** 2 + pxy.imag ** 2
    return f, np.divide(num, den, out=np.zeros_like(den), where=den > 0)
