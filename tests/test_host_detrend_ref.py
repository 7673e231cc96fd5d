"""The float64 detrend reference of the GPU matrix (tests/detrend_ref.py) held to independent implementations, and the
conditions its inputs must satisfy for tests/test_gpu_detrend_matrix.py to mean something: the five modes give spectra that
differ by far more than the GPU tolerance (a kernel that ran another mode fails), and every centre-of-gravity case has power
in its band (a quotient of two rounding residues is not a check).  No GPU."""
import itertools

import numpy as np
import pytest
from scipy import signal as sps

import detrend_ref as R
from oracle import cpu_ref as O

IDS = ["%dx%d" % s for s in R.SHAPES]


def _raw_frames(x, nfft, hop, M):
    return R.frames(x, nfft, hop, M, R.CONST)


def _close(a, b, rel):
    scale = max(float(np.max(np.abs(b))), 1e-300)
    assert float(np.max(np.abs(a - b))) <= rel * scale


@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_detrends_against_scipy_and_oracle(nfft, hop):
    """per-segment and whole-record mean / line removal == scipy.signal.detrend == oracle.cpu_ref.detrend to 1e-12 of the
    largest sample (real and complex; complex parts fitted separately)"""
    M = R.frame_counts(nfft)[-1]
    for cplx in (False, True):
        x = R.case_signal(nfft, hop, M, cplx)
        xw = x.astype(np.complex128 if cplx else np.float64)
        raw = _raw_frames(x, nfft, hop, M)
        top = float(np.max(np.abs(xw)))
        for mode, kind, style in ((R.SEGMEAN, "constant", 1), (R.SEGLINEAR, "linear", -1)):
            got = R.frames(x, nfft, hop, M, mode)
            assert np.max(np.abs(got - sps.detrend(raw, axis=1, type=kind))) <= 1e-12 * top
            assert np.max(np.abs(got - O.detrend(raw.T, style).T)) <= 1e-12 * top
            if cplx:                         # parts fitted separately
                sep = sps.detrend(raw.real, axis=1, type=kind) + 1j * sps.detrend(raw.imag, axis=1, type=kind)
                assert np.max(np.abs(got - sep)) <= 1e-12 * top
        for mode, kind, style in ((R.MEAN, "constant", 1), (R.LINEAR, "linear", -1)):
            got = R.frames(x, nfft, hop, M, mode)
            assert np.max(np.abs(got - _raw_frames(sps.detrend(xw, type=kind), nfft, hop, M))) <= 1e-12 * top
            assert np.max(np.abs(got - _raw_frames(O.detrend(xw, style), nfft, hop, M))) <= 1e-12 * top
        c = R.const_value(cplx)
        assert np.array_equal(R.frames(x, nfft, hop, M, R.CONST, c), raw - c)


def test_whole_record_modes_use_the_tail():
    """MEAN and LINEAR are fitted over x[0:nsig], the samples past the last frame included: changing only those samples
    changes every frame"""
    nfft, hop, M = 64, 16, 5
    x = R.case_signal(nfft, hop, M, False)
    y = x.copy()
    y[-R.TAIL:] += 7.0
    for mode in (R.MEAN, R.LINEAR):
        assert np.min(np.abs(R.frames(x, nfft, hop, M, mode) - R.frames(y, nfft, hop, M, mode))) > 1e-3
    for mode in (R.CONST, R.SEGMEAN, R.SEGLINEAR):
        assert np.array_equal(R.frames(x, nfft, hop, M, mode), R.frames(y, nfft, hop, M, mode))


@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_psd_mean_against_oracle_stream(nfft, hop):
    """the helper's PSD under MEAN == oracle welch_psd_stream (given float64 samples) to 1e-10"""
    win = O.windows("Hanning", nwins=nfft)
    S2 = float(np.sum(win ** 2))
    for cplx in (False, True):
        for M in R.frame_counts(nfft):
            x = R.case_signal(nfft, hop, M, cplx)
            ref = O.welch_psd_stream(x.astype(np.complex128 if cplx else np.float64), win, nfft, hop, M, 1.0)
            _close(R.psd(x, win, hop, M, R.MEAN, R.SIDED_TWO, scale=1.0 / S2), ref, 1e-10)


def test_sided_layouts():
    """one-sided: the first nfft/2 (even) or (nfft+1)/2 (odd) bins, [1:-1] doubled and for odd nfft the last one too;
    two-sided: fftshift; raw: natural order"""
    for n in (2, 3, 8, 9):
        P = np.arange(1.0, n + 1.0)
        one = R.layout(P, R.SIDED_ONE)
        nb = (n + 1) // 2 if n % 2 else n // 2
        assert one.shape == (nb,) and one[0] == P[0]
        for k in range(1, nb):
            doubled = k <= nb - 2 or (n % 2 == 1 and k == nb - 1)
            assert one[k] == (2.0 if doubled else 1.0) * P[k]
        assert np.array_equal(R.layout(P, R.SIDED_TWO), np.fft.fftshift(P))
        assert np.array_equal(R.layout(P, R.SIDED_RAW), P)


def test_pseg_and_cog_by_hand():
    x = np.array([1.0, 2.0, 4.0, 8.0, 0.0], dtype=np.float32)
    w = np.array([1.0, 0.5, 2.0])
    # frames (hop 1): [1 2 4], [2 4 8]; no detrend; trapezoid of (w f)^2
    assert np.allclose(R.pseg(x, w, 1, 2, R.CONST), [0.5 * 1 + 1 + 0.5 * 64, 0.5 * 4 + 4 + 0.5 * 256])
    # a complex exponential on bin 2 of 8: the whole power sits at f = 2 fs / 8
    z = np.exp(2j * np.pi * 2 * np.arange(8) / 8).astype(np.complex64)
    c, share = R.cog(z, np.ones(8), 8, 1, R.CONST, fs=80.0)
    assert abs(c[0] - 20.0) < 1e-5 and abs(share[0] - 1.0) < 1e-12
    c, share = R.cog(z, np.ones(8), 8, 1, R.CONST, fs=80.0, fmin=25.0, fmax=35.0)      # bin 3 only: no power
    assert c[0] == 0.0 or share[0] < 1e-12
    c, share = R.cog(z, np.ones(8), 8, 1, R.CONST, fs=80.0, fmin=2.5, fmax=7.5)        # no bin at all
    assert c[0] == 0.0 and share[0] == 0.0


@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_modes_are_told_apart(nfft, hop):
    """For every shape, dtype and frame count of the GPU matrix, the reference PSDs of CONST (0), CONST (the given constant),
    MEAN, LINEAR, SEGMEAN and SEGLINEAR differ pairwise, in at least one bin, by more than 100 times the GPU tolerance
    2e-4 ref + 1e-6 max(ref) (taken from whichever of the two spectra gives the larger tolerance).  No pair is excepted: no two
    modes are mathematically identical on this input (the tail past the last frame separates the whole-record fits from a lone
    frame's own), and nfft = 2 under SEGLINEAR, where the line fits both points, is the zero spectrum, which differs from every
    other."""
    win = O.windows("Hanning", nwins=nfft)
    for cplx in (False, True):
        for M in R.frame_counts(nfft):
            x = R.case_signal(nfft, hop, M, cplx)
            P = {label: R.psd(x, win, hop, M, mode, mean_value=mv) for label, _, mv, mode in R.mode_cases(cplx)}
            if nfft == 2:
                assert not P["seglinear"].any()
            for a, b in itertools.combinations(sorted(P), 2):
                tol = np.maximum(2e-4 * P[a] + 1e-6 * P[a].max(), 2e-4 * P[b] + 1e-6 * P[b].max())
                ratio = float(np.max(np.abs(P[a] - P[b]) / tol))
                assert ratio > 100.0, (nfft, hop, cplx, M, a, b, ratio)


@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_cog_cases_are_conditioned(nfft, hop):
    """In every cog case of the GPU matrix the band holds at least 1 % of the frame's power, in every frame.  Not cases: the
    band that is empty by construction; the band [0.15 fs, 0.3 fs] at nfft 2 and 3, which holds no bin there (the GPU test
    asserts exactly 0 for it, like the empty one); nfft = 2 under SEGLINEAR, where the frame itself is zero."""
    for wname in ("Hanning", "Boxcar"):
        win = O.windows(wname, nwins=nfft)
        for cplx in (False, True):
            for M in R.frame_counts(nfft):
                x = R.case_signal(nfft, hop, M, cplx)
                for name, fmin, fmax in R.cog_bands(nfft):
                    holds = R.band_mask(nfft, R.FS, fmin, R.FS if fmax is None else fmax).any()
                    if name == "empty":
                        assert not holds
                    if name == "tone":
                        assert holds == (nfft > 3)
                    for label, _, mv, mode in R.mode_cases(cplx):
                        c, share = R.cog(x, win, hop, M, mode, R.FS, fmin, fmax, mv)
                        if not holds or (nfft == 2 and mode == R.SEGLINEAR):
                            assert not c.any()
                        else:
                            assert share.min() >= 0.01, (nfft, hop, wname, cplx, M, name, label, share.min())
