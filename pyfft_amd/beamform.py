"""Array wavenumber-frequency spectra: what wavenumbers, mode numbers or slownesses a sensor array sees at each frequency, by the four
classical estimators on the array's cross-spectral-density (CSD) matrix G[i, j] = E[X_i conj(X_j)] (Capon 1969; Schmidt 1986; Johnson &
DeGraaf 1982; Johnson & Dudgeon, Array Signal Processing):

    bartlett   a^H G a / nch^2                   the conventional beamformer: a density per scan point, resolution 1 / aperture
    capon      1 / a^H (G + delta I)^-1 a        minimum variance (MVDR), delta = loading trace(G) / nch
    music      1 / sum_{k >= p} |a^H v_k|^2      the noise-subspace pseudospectrum for p sources: no units
    ev         1 / sum_{k >= p} |a^H v_k|^2 / w_k the eigenvector method: `music` with each noise vector weighted by 1 / its eigenvalue

Convention, that of `wavenumber.skf`: a wave that reaches the sensor at larger r LATER has k > 0 at f > 0.  A plane wave
x(r, t) = cos(2 pi f t - k . r) gives G proportional to a a^H with the steering vector a_i = exp(-i k . r_i); k is in radians per
unit of `positions`, a mode number in radians per radian of `angles`, a slowness in time per unit of `positions`.  The engine counts
the phase in turns with the opposite sign, a = exp(+2 pi i pos . kv), so this module passes kv = -k / (2 pi).

The chain stays on the device: `engine.csd_matrix` (Welch's estimate, matrix cores), `engine.eigh` (one bin per workgroup) and
`engine.beamscan` (k_beam.hip: all four estimators are one contraction over the eigenvectors).  Sensor positions need not be evenly
spaced: a Mirnov-coil ring with uneven coils or a probe rake are the cases in mind; `array_pattern` shows what the geometry alone does
to a single wave.  At most 64 sensors (the eigensolver's order).  For the number of sources `subspace.subspace_order` (MDL / AIC on the
eigenvalues) is used as it is: the snapshots are the averaged segments.  numpy in -> numpy out; device tensors in -> device tensors
(axes are numpy arrays)."""
import math

import numpy as np

from . import engine as E
from .engine import BeamRefused, _is_torch                         # noqa: F401
from .spod import csd_segments, one_sided_csd

METHODS = ("bartlett", "capon", "music", "ev")
TWO_PI = 2.0 * math.pi


def _table(who, name, t):
    if _is_torch(t):
        t = t.detach().cpu().numpy()
    t = np.asarray(t, dtype=np.float64)
    if t.ndim == 1:
        t = t.reshape(-1, 1)
    if t.ndim != 2 or not 1 <= t.shape[1] <= 3 or t.shape[0] < 1 or not np.all(np.isfinite(t)):
        raise BeamRefused("%s: %s must be finite, [n] or [n, ndim] with ndim 1 .. 3" % (who, name))
    return t


def _judge(who, nch, positions, k, method, nsources, loading):
    """what every front end refuses before the library is touched -> (pos, kv = -k / 2 pi, p)"""
    if method not in METHODS:
        raise BeamRefused("%s: method must be one of %s, not %r" % (who, ", ".join(METHODS), method))
    pos, kk = _table(who, "positions", positions), _table(who, "k", k)
    if pos.shape[1] != kk.shape[1]:
        raise BeamRefused("%s: positions and k must share ndim" % who)
    if nch < 2 or nch > E.BEAM_MAX_M:
        raise BeamRefused("%s: %d sensors are outside 2 .. %d (the eigensolver's order)" % (who, nch, E.BEAM_MAX_M))
    if pos.shape[0] != nch:
        raise BeamRefused("%s: %d positions for %d sensors" % (who, pos.shape[0], nch))
    p = 0
    if method in ("music", "ev"):
        if nsources is None:
            raise BeamRefused("%s: method %r needs nsources (subspace.subspace_order estimates it from the eigenvalues)" % (who, method))
        p = int(nsources)
        if p < 0 or p > nch - 1:
            raise BeamRefused("%s: nsources = %d is outside 0 .. nch - 1 = %d" % (who, p, nch - 1))
    loading = float(loading)
    if not (math.isfinite(loading) and loading >= 0.0):
        raise BeamRefused("%s: loading must be finite and not negative" % who)
    return pos, -kk / TWO_PI, p


def beam_scan(G, positions, k, method="capon", nsources=None, loading=0.0, out64=False, _who="beam_scan", _scale=None):
    """The scan of CSD matrices from anywhere (`engine.csd_matrix`, `dist.csd_matrix_sharded`, `multitaper_csd`, the sample matrix of a
    complex IQ array): G[..., nch, nch] Hermitian (the lower triangle is read, as `engine.eigh` does), positions[nch] or [nch, ndim],
    k[nk] or [nk, ndim] in radians per unit of positions -> P[..., nk], float32 or float64 with out64.  nsources for 'music' and 'ev'."""
    shape = tuple(G.shape)
    if len(shape) < 2 or shape[-1] != shape[-2]:
        raise BeamRefused("%s: G must be [..., nch, nch]" % _who)
    pos, kv, p = _judge(_who, int(shape[-1]), positions, k, method, nsources, loading)
    w, V, _ = E.eigh(G)
    P, _ = E.beamscan(V, w, pos, kv, method, p, loading, _scale, out64)
    return P


def slowness_scan(G, f, positions, slowness, method="capon", nsources=None, loading=0.0, out64=False):
    """`beam_scan` over slowness vectors for a broadband scan: matrix [..] belongs to the frequency f[..] and is scanned at
    k = 2 pi f slowness, slowness[ns] or [ns, ndim] in time per unit of positions -> P[..., ns].  The engine forms f . slowness per bin
    (scale = f), so one slowness table serves every bin."""
    who = "slowness_scan"
    if _is_torch(f):
        f = f.detach().cpu().numpy()
    f = np.asarray(f, dtype=np.float64)
    if tuple(f.shape) != tuple(G.shape[:-2]) or not np.all(np.isfinite(f)):
        raise BeamRefused("%s: f must be finite and hold one frequency per matrix" % who)
    s = _table(who, "slowness", slowness)
    return beam_scan(G, positions, TWO_PI * s, method, nsources, loading, out64, _who=who, _scale=f)


def array_spectrum(x, positions, k, fs=1.0, method="capon", nsources=None, loading=0.0, window="hann", nperseg=256, noverlap=None, detrend=True,
                   band=None, out64=False):
    """f, P[nb, nk]: the wavenumber-frequency spectrum of the real channels x[nch, nsig], 2 <= nch <= 64, sampled at fs, from sensors at
    positions[nch] or [nch, ndim] over the scan vectors k[nk] or [nk, ndim] (radians per unit of positions).  The CSD matrix is
    `spod`'s: segments of nperseg under `window` every nperseg - noverlap samples (noverlap defaults to nperseg // 2), scaled to a
    one-sided density 1 / (fs sum w^2) with the interior bins doubled, so 'bartlett' is a density per scan point.  detrend is
    `engine.csd_matrix`'s (the mean of each channel's whole record).  band = (f1, f2) decomposes and scans only the bins f1 <= f <= f2.
    nsources is needed for 'music' and 'ev'."""
    who = "array_spectrum"
    if len(x.shape) != 2:
        raise BeamRefused("%s: x must be [nch, nsig]" % who)
    nch, nsig = int(x.shape[0]), int(x.shape[1])
    pos, kv, p = _judge(who, nch, positions, k, method, nsources, loading)
    win, hop, nframes, freq, b0, b1 = csd_segments(who, BeamRefused, nsig, fs, window, nperseg, noverlap, band)
    G = one_sided_csd(x, win, hop, nframes, float(fs), detrend, b0, b1)
    w, V, _ = E.eigh(G)
    P, _ = E.beamscan(V, w, pos, kv, method, p, loading, None, out64)
    return freq, P


def mode_spectrum(x, angles, modes, fs=1.0, method="capon", nsources=None, loading=0.0, window="hann", nperseg=256, noverlap=None, detrend=True,
                  band=None, out64=False):
    """f, P[nb, nmodes]: the mode-number spectrum of sensors on a ring at `angles` (radians; uneven spacing is the point) over the
    integer mode numbers `modes`: `array_spectrum` with positions = angles and k = modes.  A perturbation cos(2 pi f t - n theta),
    which turns towards larger theta, has mode number n > 0."""
    n = np.asarray(modes)
    if n.ndim != 1 or n.size < 1 or not np.all(np.isfinite(n)) or not np.all(n == np.round(n)):
        raise BeamRefused("mode_spectrum: modes must be integer mode numbers")
    a = np.asarray(angles.detach().cpu().numpy() if _is_torch(angles) else angles, dtype=np.float64)
    if a.ndim != 1:
        raise BeamRefused("mode_spectrum: angles must be [nch]")
    return array_spectrum(x, a, n.astype(np.float64), fs, method, nsources, loading, window, nperseg, noverlap, detrend, band, out64)


def array_pattern(positions, k, k0=0.0):
    """The Bartlett response of the geometry alone to one unit plane wave at k0: |a(k)^H a(k0)|^2 / nch^2 over k[nk] or [nk, ndim], 1 at
    k = k0: the array's spectral window, with the sidelobes and grating lobes that an uneven or sparse geometry brings (compare
    `lomb.ls_window`).  Host arithmetic in float64."""
    who = "array_pattern"
    pos, kk = _table(who, "positions", positions), _table(who, "k", k)
    if pos.shape[1] != kk.shape[1]:
        raise BeamRefused("%s: positions and k must share ndim" % who)
    k0 = np.broadcast_to(np.asarray(k0, dtype=np.float64), (pos.shape[1],))
    if not np.all(np.isfinite(k0)):
        raise BeamRefused("%s: k0 must be finite" % who)
    ph = (kk - k0[None, :]) @ pos.T                                   # [nk, nch]: (k - k0) . r_i
    return np.abs(np.exp(1j * ph).sum(axis=1)) ** 2 / pos.shape[0] ** 2


def beam_peaks(P, k, n):
    """The n largest local maxima of every row of P[..., nk] over the 1-D grid k[nk] -> (k_peak[..., n], P_peak[..., n]), largest
    first, NaN where a row has fewer.  An interior maximum is refined by the parabola through it and its neighbours; a maximum on the
    edge of the grid is returned as it is.  A host finish."""
    if _is_torch(P):
        P = P.detach().cpu().numpy()
    P, k, n = np.asarray(P, dtype=np.float64), np.asarray(k, dtype=np.float64), int(n)
    if k.ndim != 1 or P.ndim < 1 or P.shape[-1] != k.size or k.size < 2 or n < 1:
        raise BeamRefused("beam_peaks: P must be [..., nk] over a 1-D grid k[nk] of at least two points, n at least 1")
    flat = P.reshape(-1, k.size)
    kp, pp = np.full((flat.shape[0], n), np.nan), np.full((flat.shape[0], n), np.nan)
    for r, y in enumerate(flat):
        left = np.concatenate(([True], y[1:] > y[:-1]))
        right = np.concatenate((y[:-1] >= y[1:], [True]))
        idx = np.nonzero(left & right & np.isfinite(y))[0]
        idx = idx[np.argsort(-y[idx], kind="stable")][:n]
        for j, i in enumerate(idx):
            kp[r, j], pp[r, j] = k[i], y[i]
            if 0 < i < k.size - 1:
                den = y[i - 1] - 2.0 * y[i] + y[i + 1]
                if den < 0.0:
                    d = 0.5 * (y[i - 1] - y[i + 1]) / den
                    kp[r, j] = k[i] + d * 0.5 * (k[i + 1] - k[i - 1])
                    pp[r, j] = y[i] - 0.25 * (y[i - 1] - y[i + 1]) * d
    return kp.reshape(P.shape[:-1] + (n,)), pp.reshape(P.shape[:-1] + (n,))


def beam_plan(nch, nk, nb=1, method="capon", nsources=0, ndim=1):
    """What the scan of nb matrices of nch sensors over nk scan vectors runs as (engine.beam_plan; host only)."""
    return E.beam_plan(nch, nk, nb, method, nsources, ndim)
