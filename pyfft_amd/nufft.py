"""The non-uniform FFT of type 1 on the GPU: the spectrum of an unevenly sampled complex record on a uniform grid of frequencies,

    F[m] = sum_j c_j exp(2 pi i sign (f0 + m df) (t_j - t_ref)),    m = 0 .. M - 1,

in O(N w + M log M) in place of the O(N M) of the sum itself (Dutt & Rokhlin 1993; Greengard & Lee 2004; the "exponential of
semicircle" kernel of Barnett, Magland & af Klinteberg 2019 at width w = 8 and upsampling 2).  The samples are spread onto a fine
grid, one long transform runs over it, and every bin is divided by the kernel's transform (engine.nufft1, sp_nufft1).  Accuracy:
about 1e-7 of a row's sum of |c_j| (float32 kernel values and a complex64 transform; the method's own error is under 4e-8).  The
spread adds 64-bit integers, so results are bitwise reproducible AND do not depend on the order of the samples.  Times are float64
and may come in any order, with duplicates.  The fast Lomb-Scargle periodogram (lomb.ls_periodogram(method='fast')) is built on it.

    nufft1        any finite f0, any df != 0, rows of strengths over one axis of times
    nufft1_modes  positions in radians, integer modes -M//2 .. (M-1)//2: the convention of FINUFFT's nufft1d1
    nufft_plan    how a shape is dealt to the device

What is not here: the type-2 transform (uniform modes to uneven times) and type 3; two and three dimensions; float64 strengths on the
device; a tolerance argument (there is one kernel width); rows with times of their own; sharding over GPUs (spectra of the parts of a
record add).  A record piled into one tile of 1024 grid cells is correct and slow.  What is refused raises NufftRefused, which is a
ValueError and a NotImplementedError.
"""
import numpy as np

from . import engine as _engine
from .engine import NufftRefused, _is_torch          # noqa: F401

TWO_PI = 2.0 * np.pi


def nufft1(t, c, f0, df, M, sign=1, t_ref=None):
    """F [..., M] (complex64) of the strengths c[..., N] at the times t[N]: frequencies f0 + m df in cycles per unit of t, phases
    taken from t_ref (default t[0]; 0.0 for the origin of t itself).  numpy in -> numpy out, device tensors in -> a device tensor."""
    return _engine.nufft1(t, c, f0, df, M, sign=sign, t_ref=t_ref)


def nufft1_modes(x, c, M, sign=1):
    """F[..., i] = sum_j c[..., j] exp(i sign k x_j) over the modes k = -(M // 2) + i, i = 0 .. M - 1 (that is -M//2 .. (M-1)//2 in
    FINUFFT's words), for positions x[N] in radians (any real values: the transform is periodic in 2 pi)."""
    t = x / TWO_PI if _is_torch(x) else np.asarray(x, dtype=np.float64) / TWO_PI
    return _engine.nufft1(t, c, -float(int(M) // 2), 1.0, M, sign=sign, t_ref=0.0)


def nufft_plan(N, M, rows=1):
    """How engine.nufft1 deals N samples, M frequencies and `rows` rows to the device (sp_nufft1_plan, host only): nf, width, tiles,
    tile, rows_per_pass, passes, workgroups, fast_min_pairs."""
    return _engine.nufft_plan(N, M, rows)
