"""Rational resampling: scipy.signal.upfirdn and scipy.signal.resample_poly on the GPU, one streaming pass of k_upfirdn.hip.

    xu[i up] = x[i], 0 elsewhere;    y[m] = sum_j h[j] xu[m down - j] = sum_p h[phi + p up] x[i0 - p]
    i0 = floor(m down / up),  phi = (m down) mod up

upfirdn is the primitive (zero boundaries only).  resample_poly designs scipy's low-pass (or takes the caller's taps), centres it the way
scipy does -- `pre` zeros in front of the taps, then the outputs m0 .. m0 + nout - 1 -- and asks the device for exactly those outputs.
resample_rate turns a pair of sample rates into up / down.  resample_plan is the host-side bookkeeping, for tools and tests.
The filter is designed on the host in float64; the samples and taps are float32 on the device, and the dtype of the input is kept:
real rows stay real (engine.ddc, the up = 1 special case with a mixer in front, always returns complex64).
"""
import math
from fractions import Fraction

import numpy as np

from .baseband import Unsupported, _is_torch

MAX_FACTOR = 256                    # one launch takes reduced factors up to this
MAX_TAPS = 8191                     # and this many taps, the zeros put in front included
BACKGROUNDS = ("mean", "median", "minimum", "maximum")
PADTYPES = ("constant", "line") + BACKGROUNDS
DEFAULT_WINDOW = ("kaiser", 5.0)


def _factors(up, down, who):
    for name, v in (("up", up), ("down", down)):
        if isinstance(v, bool) or v != int(v):
            raise ValueError("%s: %s must be an integer, got %r" % (who, name, v))
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("%s: up and down must be >= 1" % who)
    return up, down


def _limits(up, down, ntaps, who):
    if up > MAX_FACTOR or down > MAX_FACTOR:
        raise Unsupported("%s: the reduced ratio %d / %d is beyond the factors <= %d of one launch (no cascade is built)" %
                          (who, up, down, MAX_FACTOR))
    if not 1 <= ntaps <= MAX_TAPS:
        raise Unsupported("%s: %d taps are outside the 1 .. %d one launch takes" % (who, ntaps, MAX_TAPS))


def _taps(h, who):
    if np.iscomplexobj(h):
        raise Unsupported("%s: complex taps are not built" % who)
    h = np.asarray(h, dtype=np.float64)
    if h.ndim != 1 or h.size < 1:
        raise ValueError("%s: the taps must be a one-dimensional, non-empty array" % who)
    if not np.all(np.isfinite(h)):
        raise ValueError("%s: the taps must be finite" % who)
    return h


def _axis(x, axis, who):
    nd = x.dim() if _is_torch(x) else np.ndim(x)
    if nd < 1:
        raise ValueError("%s: x must have at least one axis" % who)
    if isinstance(axis, bool) or axis != int(axis) or not -nd <= axis < nd:
        raise ValueError("%s: axis %r is out of range for %d dimensions" % (who, axis, nd))
    return int(axis) % nd, nd


def _to_last(x, axis, nd):
    if axis == nd - 1:
        return x
    return x.movedim(axis, -1) if _is_torch(x) else np.moveaxis(x, axis, -1)


def _from_last(y, axis, nd):
    if axis == nd - 1:
        return y
    return y.movedim(-1, axis) if _is_torch(y) else np.moveaxis(y, -1, axis)


def upfirdn(h, x, up=1, down=1, axis=-1, mode="constant", cval=0):
    """scipy.signal.upfirdn(h, x, up, down, axis, mode='constant', cval=0) on the GPU: all ceil(((n - 1) up + len(h)) / down) outputs.
    Only zero boundaries are built; up and down are taken as they are (scipy does not reduce them either) and must lie in 1 .. 256,
    len(h) in 1 .. 8191.  float32 / complex64 out, like the input; numpy in -> numpy out, device tensor in -> device tensor out."""
    if mode != "constant" or cval != 0:
        raise Unsupported("upfirdn: only mode='constant' with cval=0 is built, got mode=%r, cval=%r" % (mode, cval))
    up, down = _factors(up, down, "upfirdn")
    h = _taps(h, "upfirdn")
    _limits(up, down, h.size, "upfirdn")
    if not _is_torch(x):
        x = np.asarray(x)
    axis, nd = _axis(x, axis, "upfirdn")
    from . import engine
    return _from_last(engine.upfirdn(_to_last(x, axis, nd), h, up, down), axis, nd)


def _design(up, down, window):
    """(taps scaled by up, float64; half) for reduced up, down: the caller's taps, or scipy's firwin(2 * 10 * max + 1, 1 / max)."""
    if isinstance(window, (list, np.ndarray)):
        h = _taps(window, "resample_poly").copy()
    else:
        import scipy.signal as ss
        mx = max(up, down)
        h = ss.firwin(2 * 10 * mx + 1, 1.0 / mx, window=window)
    return h * up, (h.size - 1) // 2


def resample_plan(n, up, down, window=DEFAULT_WINDOW, cplx=False):
    """The bookkeeping of resample_poly for n samples (host only): the reduced 'up' and 'down', 'taps' (float64, scaled by up, without
    the zeros in front), 'pre' (zeros in front), 'm0' and 'nout' (the outputs m0 .. m0 + nout - 1 of upfirdn are the result), 'tile'
    (outputs per workgroup) and 'workgroups' (per row).  up = down = 1 after reduction is a copy: taps, tile are None."""
    up, down = _factors(up, down, "resample_poly")
    n = int(n)
    if n < 1:
        raise ValueError("resample_poly: need at least one sample along the axis")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down == 1:
        return dict(up=1, down=1, taps=None, pre=0, m0=0, nout=n, tile=None, workgroups=0)
    _limits(up, down, 1, "resample_poly")
    h, half = _design(up, down, window)
    pre = down - half % down
    _limits(up, down, h.size + pre, "resample_poly")
    nout = -(-n * up // down)
    from . import engine
    tile = engine.upfirdn_tile(up, down, h.size + pre, cplx)
    return dict(up=up, down=down, taps=h, pre=pre, m0=(half + pre) // down, nout=nout, tile=tile, workgroups=-(-nout // tile))


def _phase_sums(h, up, down, m0, nout):
    """What an endless constant 1 and an endless ramp i give at the outputs m0 .. m0 + nout - 1: (A[phi_m], i0_m A[phi_m] - B[phi_m])
    with A[phi] = sum_p h[phi + p up], B[phi] = sum_p p h[phi + p up], in float64."""
    P = -(-h.size // up)
    hp = np.zeros(P * up)
    hp[:h.size] = h
    hp = hp.reshape(P, up)
    A, B = hp.sum(axis=0), (np.arange(P)[:, None] * hp).sum(axis=0)
    md = (m0 + np.arange(nout, dtype=np.int64)) * down
    phi, i0 = md % up, md // up
    return A[phi], i0 * A[phi] - B[phi]


def resample_poly(x, up, down, axis=0, window=DEFAULT_WINDOW, padtype="constant", cval=None):
    """scipy.signal.resample_poly on the GPU: x resampled by up / down along `axis` with a zero-phase low-pass FIR, ceil(n up / down)
    samples.  window: scipy's window specification for firwin(2 * 10 * max(up, down) + 1, 1 / max(up, down)), or an array of taps.
    padtype 'constant' (with cval), 'line', 'mean', 'median', 'minimum', 'maximum' as in scipy: the background of every row is taken
    off before the kernel and put back after it; scipy's other boundary modes are not built.  up = down after reduction returns a copy.
    float32 / complex64 out; numpy in -> numpy out, device tensor in -> device tensor out."""
    up, down = _factors(up, down, "resample_poly")
    if cval is not None and padtype != "constant":
        raise ValueError("resample_poly: cval has no effect when padtype is %r" % (padtype,))
    if padtype not in PADTYPES:
        raise Unsupported("resample_poly: padtype %r is not built; built are %s" % (padtype, ", ".join(PADTYPES)))
    dev = _is_torch(x)
    if not dev:
        x = np.asarray(x)
    axis, nd = _axis(x, axis, "resample_poly")
    n = int(x.shape[axis])
    cplx = bool(x.is_complex()) if dev else np.iscomplexobj(x)
    if dev and cplx and padtype in ("median", "minimum", "maximum"):
        raise Unsupported("resample_poly: padtype %r of a complex device tensor is not built" % padtype)
    plan = resample_plan(n, up, down, window, cplx)
    if plan["taps"] is None:
        return x.clone() if dev else x.copy()
    up, down, m0, nout = plan["up"], plan["down"], plan["m0"], plan["nout"]
    h = np.concatenate([np.zeros(plan["pre"]), plan["taps"]])
    from . import engine
    v = _to_last(x, axis, nd)
    back = add = None                              # taken off every row before the kernel; added to the outputs after it
    if padtype in BACKGROUNDS:
        if dev:
            if padtype == "median":
                s = v.sort(dim=-1).values
                back = 0.5 * (s[..., (n - 1) // 2:(n - 1) // 2 + 1] + s[..., n // 2:n // 2 + 1])
            else:
                wide = engine.torch.complex128 if cplx else engine.torch.float64      # the mean is accumulated in float64
                back = {"mean": lambda a: a.mean(dim=-1, keepdim=True, dtype=wide).to(a.dtype), "minimum": lambda a: a.amin(dim=-1, keepdim=True),
                        "maximum": lambda a: a.amax(dim=-1, keepdim=True)}[padtype](v)
        else:
            back = {"mean": np.mean, "median": np.median, "minimum": np.amin, "maximum": np.amax}[padtype](v, axis=-1, keepdims=True)
        add = back
    elif padtype == "line" or (cval is not None and cval != 0):
        # the row continues as first + slope i (line) or as cval beyond its ends: taken off, the rest continues as zeros, and what the
        # filter makes of the endless line is added back
        A, R = _phase_sums(h, up, down, m0, nout)
        if padtype == "line":
            first = v[..., :1]
            slope = (v[..., -1:] - first) / (n - 1) if n > 1 else first * 0
        else:
            first, slope = cval, 0.0
        if dev:
            # the offset goes first (nearly exact in the tensor's own precision), then the small ramp; what is added back is
            # worked out in float64 and rounded once
            torch = engine.torch
            wide = torch.complex128 if cplx else torch.float64
            A, R = (torch.as_tensor(t, device=v.device) for t in (A, R))
            ramp = torch.arange(n, device=v.device, dtype=torch.float64 if v.dtype in (torch.float64, torch.complex128) else torch.float32)
            if padtype == "line":
                v = (v - first) - slope * ramp
                add = first.to(wide) * A + slope.to(wide) * R
            else:
                v = v - cval
                add = cval * A
        else:
            back = first + slope * np.arange(n, dtype=np.float64)
            add = first * A + slope * R
    if back is not None:
        v = v - back
    if dev and v.dtype not in (engine.torch.float32, engine.torch.complex64):
        v = v.to(engine.torch.complex64 if cplx else engine.torch.float32)
    y = engine.upfirdn(v, h, up, down, m0=m0, nout=nout)
    if add is not None:
        y = (y + add).to(y.dtype) if dev else (y + add).astype(y.dtype)
    return _from_last(y, axis, nd)


def resample_rate(x, fs, fs_new, max_factor=MAX_FACTOR, axis=-1, **kw):
    """x resampled from the rate fs to fs_new: (y, fs_out) with up / down the best ratio with both factors <= max_factor and
    fs_out = fs up / down the exact rate delivered.  Unless exact=False is passed, a ratio that misses fs_new / fs by more than 1e-9
    relative is refused.  The other keywords go to resample_poly."""
    exact = kw.pop("exact", True)
    fs, fs_new = float(fs), float(fs_new)
    if not (math.isfinite(fs) and math.isfinite(fs_new) and fs > 0 and fs_new > 0):
        raise ValueError("resample_rate: fs and fs_new must be positive and finite")
    max_factor = int(max_factor)
    if not 1 <= max_factor <= MAX_FACTOR:
        raise Unsupported("resample_rate: max_factor = %d must lie in 1 .. %d" % (max_factor, MAX_FACTOR))
    ratio = Fraction(fs_new) / Fraction(fs)
    if ratio <= 1:
        fr = ratio.limit_denominator(max_factor)
    else:
        fr = (1 / ratio).limit_denominator(max_factor)
        fr = 1 / fr if fr else fr
    up, down = fr.numerator, fr.denominator
    if up < 1 or down < 1:
        raise Unsupported("resample_rate: no ratio with factors <= %d comes near fs_new / fs = %g" % (max_factor, fs_new / fs))
    if exact and abs(Fraction(up, down) / ratio - 1) > Fraction(1, 10 ** 9):
        raise Unsupported("resample_rate: no ratio with factors <= %d matches fs_new / fs = %.12g to 1e-9 (nearest: %d / %d); "
                          "pass exact=False to take the nearest" % (max_factor, fs_new / fs, up, down))
    return resample_poly(x, up, down, axis=axis, **kw), fs * up / down
