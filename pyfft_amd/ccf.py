"""Drop-in for the reference's ccf.ccf (ccf.py:66-77): normalised cross-covariance at all 2N-1 lags.
The reference uses np.correlate (O(N^2)); the device path is the equivalent zero-padded FFT product.

ccf_sh is the reference's short-time form: the correlation inside a sliding window, averaged over the windows.  The reference takes
its window indices from the absent pybaseutils.utils.sliding_window_1d; the layout here is this build's stated choice, the one cogspec
made: `nav` is the window length (as the docstring says), windows are complete, they step by `hop` (default nav: no overlap), and a
trailing partial window is dropped.  Per window the defaults are the reference's ccf: mean removed, boxcar, / (nav sigma1 sigma2).
ccf_frames returns the time-resolved correlogram and delay_track the delay read off its peak; all three run one kernel
(k_xcorr_frames.hip) that writes nothing but what was asked for.  Windows with nav + maxlag beyond 8192 are outside one workgroup
transform and refused: the whole-record ccf is the long path."""
import math

import numpy as np

from . import engine as _E
from .engine import _is_torch
from .windows import get_window

MAX_L = 8192                        # one workgroup transform
_NORMS = ("coeff", "raw", "biased", "unbiased")


class WindowTooLong(ValueError, NotImplementedError):
    """nav + maxlag beyond one workgroup transform: a path that is not built."""


def ccf(x1, x2, fs):
    """(tau, co): tau = -lags/fs, lags = -N+1..N-1; co = correlate(x1-m1, x2-m2, 'full') / (N std1 std2)."""
    x1 = np.asarray(x1)
    x2 = np.asarray(x2)
    npts = len(x1)
    lags = np.arange(-npts + 1, npts)
    tau = -lags / float(fs)
    co = _E.xcorr_normalised(x1, x2).astype(np.float64)
    return tau, co


def _xc_len(who, nav, maxlag):
    """The transform length of sp_xcorr_frames_len, with its refusals."""
    if nav < 2:
        raise ValueError("%s: nav must be at least 2" % who)
    if not 0 <= maxlag <= nav - 1:
        raise ValueError("%s: maxlag must lie in 0 .. nav - 1 = %d" % (who, nav - 1))
    if nav + maxlag > MAX_L:
        raise WindowTooLong("%s: nav + maxlag = %d is beyond one workgroup transform (%d points); the whole-record ccf is the long path"
                            % (who, nav + maxlag, MAX_L))
    L = 32
    while L < nav + maxlag:
        L *= 2
    return L


def ccf_plan(nav, maxlag=None, cplx=False):
    """What one frame costs: dict(L = the transform length max(32, next_pow2(nav + maxlag)), nlags = 2 maxlag + 1, transforms per frame
    (real records: 2, complex: 3), read = the bytes of samples a frame loads from the two records (the part a hop shares with the
    frame before comes from cache), written = the bytes a frame writes for each output: the whole row of lags for 'frames', 8 for
    'peak', none for 'avg' (one partial row of L per transform group for the whole run).  Host only."""
    nav = int(nav)
    maxlag = nav - 1 if maxlag is None else int(maxlag)
    L = _xc_len("ccf_plan", nav, maxlag)
    esz = 8 if cplx else 4
    nl = 2 * maxlag + 1
    return dict(L=L, nlags=nl, transforms=3 if cplx else 2, read=2 * esz * nav, written=dict(frames=esz * nl, avg=0, peak=8))


def band_weight(L, fs, band):
    """The 0 / 1 table on the L bins in FFT order: 1 where f_lo <= |f| <= f_hi."""
    try:
        f_lo, f_hi = (float(v) for v in band)
    except (TypeError, ValueError):
        raise ValueError("band must be a pair (f_lo, f_hi)")
    if not (math.isfinite(f_lo) and math.isfinite(f_hi) and 0 <= f_lo <= f_hi):
        raise ValueError("band must be a pair of finite frequencies with 0 <= f_lo <= f_hi")
    f = np.abs(np.fft.fftfreq(L, 1.0 / fs))
    return ((f >= f_lo) & (f <= f_hi)).astype(np.float32)


def _prepare(who, x1, x2, fs, nav, hop, maxlag, window, detrend, norm, phat, weight, band):
    """Every check, before the library is touched.  -> the engine's arguments, the lags and the per-lag scale (or None)."""
    dev = _is_torch(x1)
    if dev != _is_torch(x2):
        raise ValueError("%s: x1 and x2 must both be arrays or both be device tensors" % who)
    if not dev:
        x1, x2 = np.asarray(x1), np.asarray(x2)
    if len(x1.shape) != 1 or len(x2.shape) != 1:
        raise ValueError("%s: x1 and x2 must be one-dimensional" % who)
    if x1.shape[0] != x2.shape[0]:
        raise ValueError("%s: x1 and x2 must have equal lengths" % who)
    c1 = x1.is_complex() if dev else np.iscomplexobj(x1)
    c2 = x2.is_complex() if dev else np.iscomplexobj(x2)
    if c1 != c2:
        raise ValueError("%s: x1 and x2 must both be real or both be complex" % who)
    fs = float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("%s: fs must be positive" % who)
    nsig, nav = int(x1.shape[0]), int(nav)
    maxlag = nav - 1 if maxlag is None else int(maxlag)
    L = _xc_len(who, nav, maxlag)
    if nsig < nav:
        raise ValueError("%s: the record (%d samples) is shorter than nav (%d)" % (who, nsig, nav))
    hop = nav if hop is None else int(hop)
    if hop < 1:
        raise ValueError("%s: hop must be at least 1" % who)
    win = None
    if window is not None and not (isinstance(window, str) and window in ("boxcar", "rect", "rectangular")):
        if isinstance(window, (str, tuple)):
            win = np.asarray(get_window(window, nav), dtype=np.float64)
        else:
            win = np.asarray(window, dtype=np.float64)
        if win.shape != (nav,):
            raise ValueError("%s: window must be a name or nav = %d values" % (who, nav))
        if not np.all(np.isfinite(win)):
            raise ValueError("%s: the window must be finite" % who)
    if detrend not in (True, False, None, "mean", "segmean", "constant", "none"):
        raise ValueError("%s: detrend must be True (every window's own mean) or False" % who)
    segmean = detrend not in (False, None, "none")
    if norm not in _NORMS:
        raise ValueError("%s: norm must be one of %s" % (who, ", ".join(_NORMS)))
    phat = float(phat)
    if not (phat >= 0 and math.isfinite(phat)):
        raise ValueError("%s: phat must be finite and not negative" % who)
    if phat > 0 and norm != "coeff":
        raise ValueError("%s: phat > 0 takes norm='coeff'" % who)
    W = None
    if weight is not None:
        W = np.asarray(weight, dtype=np.float64)
        if W.shape != (L,):
            raise ValueError("%s: weight must hold L = %d values (ccf_plan), in FFT order" % (who, L))
        if not np.all(np.isfinite(W)):
            raise ValueError("%s: the weight must be finite" % who)
        if not c1 and not np.array_equal(W[1:], W[1:][::-1]):
            raise ValueError("%s: the weight must be even for real input (W[k] == W[L - k])" % who)
    if band is not None:
        B = band_weight(L, fs, band)
        W = B if W is None else W * B
    lags = np.arange(-maxlag, maxlag + 1)
    scale = None
    if norm == "biased":
        scale = np.full(lags.size, 1.0 / nav)
    elif norm == "unbiased":
        scale = 1.0 / (nav - np.abs(lags))
    nframes = 1 + (nsig - nav) // hop
    args = dict(nw=nav, hop=hop, nframes=nframes, maxlag=maxlag, win=win, segmean=segmean, coeff=norm == "coeff", beta=phat, weight=W)
    t = (np.arange(nframes) * hop + 0.5 * (nav - 1)) / fs
    return args, -lags / fs, t, scale


def _scaled(out, scale):
    if scale is None:
        return out
    if _is_torch(out):
        return out * out.new_tensor(scale, dtype=out.real.dtype)
    return out * scale.astype(out.real.dtype)


def ccf_sh(x1, x2, fs, nav, hop=None, maxlag=None, window=None, detrend=True, norm="coeff", phat=0.0, weight=None, band=None):
    """(tau, csh): the correlation inside windows of nav samples stepping by hop (default nav), averaged over the complete windows.
    tau = -lags/fs, lags = -maxlag .. maxlag (default nav - 1); csh float64 (complex128 for complex input), accumulated on the device
    -- the per-window correlations are never written.  Per window, by default, the reference's ccf: correlate(a - mean a, b - mean b)
    / (nav std a std b).  window: a taper applied after the mean removal; detrend=False keeps the means; norm: 'coeff', 'raw',
    'biased' (raw / nav), 'unbiased' (raw / (nav - |lag|)); phat = beta > 0: the regularised phase transform S / (|S| + beta E) on the
    cross spectrum (GCC-PHAT; E = sqrt(sum |a|^2 sum |b|^2)); weight: L real weights on the cross spectrum in FFT order (L from
    ccf_plan), band=(f_lo, f_hi): the 0 / 1 weight on f_lo <= |f| <= f_hi.  numpy in -> numpy out, device tensors in -> device out."""
    args, tau, _, scale = _prepare("ccf_sh", x1, x2, fs, nav, hop, maxlag, window, detrend, norm, phat, weight, band)
    _, avg, _ = _E.xcorr_frames(x1, x2, avg=True, **args)
    return tau, _scaled(avg, scale)


def ccf_frames(x1, x2, fs, nav, hop=None, maxlag=None, window=None, detrend=True, norm="coeff", phat=0.0, weight=None, band=None):
    """(tau, t, co): the time-resolved correlogram, co[g, :] = the correlation of window g at the lags of tau (float32, complex64 for
    complex input); t = the window centres in seconds.  Arguments as ccf_sh."""
    args, tau, t, scale = _prepare("ccf_frames", x1, x2, fs, nav, hop, maxlag, window, detrend, norm, phat, weight, band)
    co, _, _ = _E.xcorr_frames(x1, x2, frames=True, **args)
    return tau, t, _scaled(co, scale)


def delay_track(x1, x2, fs, nav, hop=None, maxlag=None, window=None, detrend=True, norm="coeff", phat=0.0, weight=None, band=None):
    """(t, delay, peak): per window the delay of the correlation's top, delay = -(l* + delta) / fs in tau's sign convention, and the
    top's height; l* is the lag of the largest value (of the largest modulus for complex input), delta and the height come from the
    parabola through the three lags around it (delta = 0 at the ends of the lag range).  Eight bytes per window leave the kernel; the
    correlogram is never written.  norm 'biased' / 'unbiased' rescale per lag and would move the top: they are refused here."""
    if norm in ("biased", "unbiased"):
        raise ValueError("delay_track: norm must be 'coeff' or 'raw' (a per-lag scale is applied after the search)")
    args, _, t, _ = _prepare("delay_track", x1, x2, fs, nav, hop, maxlag, window, detrend, norm, phat, weight, band)
    _, _, pk = _E.xcorr_frames(x1, x2, peak=True, **args)
    if _is_torch(pk):
        return t, -pk[:, 0] / float(fs), pk[:, 1]
    return t, -pk[:, 0].astype(np.float64) / float(fs), pk[:, 1].astype(np.float64)
