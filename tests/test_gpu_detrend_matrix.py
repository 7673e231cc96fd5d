"""Every detrend mode of the one-workgroup frame kernels (sp_welch_psd, sp_welch_csd, sp_stft, sp_stft_cog) against the
float64 restatement of include/spectral.h in tests/detrend_ref.py, at the transform lengths where segment_detrend / group_mean
and the per-frame reductions take another form (kernels.h): one thread per frame (nfft <= 16), several frame groups per
workgroup with tail groups on clamped frames (nfft < 4096), Bluestein lengths whose padded slots must stay out of the sums
(3, 30, 1000, 1023, 4095), sub-wave, one-wave and many-wave frames.  Frame counts: 1, one workgroup plus three frames, 37
(1 and 5 from 4095 points up); eleven samples lie past the last frame, so MEAN / LINEAR must be fitted over nsig.

Tolerances are the project's stated ones: spectra rtol 2e-4 + 1e-6 max(ref); pxy 2e-4 sqrt(pxx pyy) +
1e-6 max; STFT frames 1e-4 of the call's largest reference magnitude; pseg rtol 1e-4; cog 2e-4 fs.  Where the reference is
identically zero (nfft = 2 under SEGLINEAR: the line fits both points) the output must be finite and its power at most
(16 2^-24 max|x| sum|w|)^2, the float32 rounding of the subtraction.  tests/test_host_detrend_ref.py holds the reference to
scipy and the oracle and shows that on these inputs the modes differ by more than 100 tolerances and that every cog band holds
at least 1 % of its frame's power.  Every test prints its worst error / tolerance: on the MI355X at most 2.2 % of the bound,
except pseg at nfft 2 and 3 (0.96 and 0.85 of it): a frame there is one or two windowed samples, and where the detrended
sample nearly cancels, the float32 rounding of the subtraction shows at full relative size."""
import contextlib
import os

import numpy as np
import pytest

import detrend_ref as R
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

IDS = ["%dx%d" % s for s in R.SHAPES]
DTYPES = (False, True)                       # float32, complex64


@pytest.fixture(scope="module")
def E():
    from pyfft_amd import engine
    from pyfft_amd import _ffi
    _ffi.init()
    return engine


@contextlib.contextmanager
def forced(*names):
    """the library's A/B switches (read on every call), set for the duration of the block"""
    for k in names:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k in names:
            del os.environ[k]


def zero_bound(x, win):
    """power bound where the reference is identically zero: (16 2^-24 max|x| sum|w|)^2"""
    return (16.0 * 2.0 ** -24 * float(np.max(np.abs(x))) * float(np.sum(np.abs(win)))) ** 2


class Worst:
    """largest error / tolerance seen, and where"""

    def __init__(self, what):
        self.what, self.ratio, self.where = what, 0.0, None

    def check(self, got, ref, tol, where):
        got = np.asarray(got)
        assert got.shape == np.shape(ref), (where, got.shape, np.shape(ref))
        assert np.all(np.isfinite(got)), where
        r = float(np.max(np.abs(got - ref) / tol))
        if r > self.ratio:
            self.ratio, self.where = r, where
        assert r <= 1.0, "%s %s: error %.3g tolerances" % (self.what, where, r)

    def report(self):
        print("%s: worst error %.3g of the tolerance at %s" % (self.what, self.ratio, self.where))


def spec_tol(ref):
    return 2e-4 * np.abs(ref) + 1e-6 * float(np.max(np.abs(ref)))


# ------------------------------------------------------------------------------------------ sp_welch_psd
@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_welch_psd(E, nfft, hop):
    win = O.windows("Hanning", nwins=nfft)
    scale = 1.0 / float(np.sum(win ** 2))
    sides = ((E.SIDED_TWO, R.SIDED_TWO), (E.SIDED_ONE, R.SIDED_ONE), (E.SIDED_RAW, R.SIDED_RAW))
    worst = Worst("welch_psd %dx%d" % (nfft, hop))
    for cplx in DTYPES:
        for M in R.frame_counts(nfft):
            x = R.case_signal(nfft, hop, M, cplx)
            for label, det, mv, mode in R.mode_cases(cplx):
                P = scale * np.mean(np.abs(R.spectra(x, win, hop, M, mode, mv)) ** 2, axis=0)
                # MEAN also through the generic kernel: the mean in a pass of its own and one frame per transform, then k_welch itself
                switches = [()]
                if mode == R.MEAN:
                    switches += [("SP_WELCH_TWOPASS", "SP_NO_REALPAIR"), ("SP_WELCH_TWOPASS", "SP_NO_REALPAIR", "SP_WELCH_GENERIC")]
                for sw in switches:
                    for es, rs in sides:
                        where = (label, "c64" if cplx else "f32", M, "sided %d" % es) + sw
                        with forced(*sw):
                            got = E.welch_psd(x, win, hop, M, detrend=det, sided=es, scale=scale, mean_value=mv)
                            kern = E.profile_last_kernel()
                        if mode in (R.SEGMEAN, R.SEGLINEAR) or "SP_WELCH_GENERIC" in sw:
                            assert kern == "k_welch", where
                        elif sw:
                            assert "onepass" not in kern and kern != "k_welch_rp", where
                        ref = R.layout(P, rs)
                        if not ref.any():
                            assert nfft == 2 and mode == R.SEGLINEAR
                            assert np.all(np.isfinite(got)) and got.shape == ref.shape, where
                            assert float(np.max(got)) <= scale * zero_bound(x, win), where
                        else:
                            worst.check(got, ref, spec_tol(ref), where)
    worst.report()


# ------------------------------------------------------------------------------------------ sp_welch_csd
@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_welch_csd(E, nfft, hop):
    """the reference channel against 3 channels (seeds and offsets of their own): pxx, pyy and pxy = Y conj(X)"""
    win = O.windows("Hanning", nwins=nfft)
    scale = 1.0 / float(np.sum(win ** 2))
    worst = Worst("welch_csd %dx%d" % (nfft, hop))
    for cplx in DTYPES:
        for M in R.frame_counts(nfft):
            x = R.case_signal(nfft, hop, M, cplx)
            y = np.stack([R.case_signal(nfft, hop, M, cplx, ch) for ch in (1, 2, 3)])
            for mode in R.MODES:
                X = R.spectra(x, win, hop, M, mode)
                Y = np.stack([R.spectra(yc, win, hop, M, mode) for yc in y])
                nat = (scale * np.mean(np.abs(X) ** 2, axis=0), scale * np.mean(np.abs(Y) ** 2, axis=1),
                       scale * np.mean(Y * np.conj(X)[None], axis=1))
                for sw in ((),) if cplx else ((), ("SP_NO_REALPAIR",)):
                    for es, rs in ((E.SIDED_ONE, R.SIDED_ONE), (E.SIDED_TWO, R.SIDED_TWO)):
                        where = (R.MODE_NAMES[mode], "c64" if cplx else "f32", M, "sided %d" % es) + sw
                        with forced(*sw):
                            pxx, pyy, pxy = E.welch_csd(x, y, win, hop, M, detrend=mode, sided=es, scale=scale)
                        rxx, ryy, rxy = (R.layout(a, rs) for a in nat)
                        if not rxx.any():
                            assert nfft == 2 and mode == R.SEGLINEAR
                            bx = scale * zero_bound(x, win)
                            by = scale * np.array([zero_bound(yc, win) for yc in y])[:, None]
                            for got, ref, bound in ((pxx, rxx, bx), (pyy, ryy, by), (np.abs(pxy), rxy, np.sqrt(bx * by))):
                                assert got.shape == ref.shape and np.all(np.isfinite(got)), where
                                assert np.all(got <= bound), where
                            continue
                        worst.check(pxx, rxx, spec_tol(rxx), where + ("pxx",))
                        worst.check(pyy, ryy, 2e-4 * ryy + 1e-6 * ryy.max(axis=1, keepdims=True), where + ("pyy",))
                        geo = np.sqrt(rxx[None, :] * ryy)
                        worst.check(pxy, rxy, 2e-4 * geo + 1e-6 * geo.max(axis=1, keepdims=True), where + ("pxy",))
    worst.report()


# ------------------------------------------------------------------------------------------ sp_stft
@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_stft_frames(E, nfft, hop):
    """complex frames (frame-major, one- and two-sided), power (bin-major) and pseg, in every mode; real input through the
    two-frames-per-transform kernel and, with SP_NO_REALPAIR, through the generic one"""
    win = O.windows("Hanning", nwins=nfft)
    amp = 1.0 / float(np.sum(win))
    worst = Worst("stft_frames %dx%d" % (nfft, hop))
    wseg = Worst("pseg %dx%d" % (nfft, hop))
    for cplx in DTYPES:
        for M in R.frame_counts(nfft):
            x = R.case_signal(nfft, hop, M, cplx)
            for label, det, mv, mode in R.mode_cases(cplx):
                Xn = R.spectra(x, win, hop, M, mode, mv)
                rseg = R.pseg(x, win, hop, M, mode, mv)
                zero = not Xn.any()
                if zero:
                    assert nfft == 2 and mode == R.SEGLINEAR
                bound = zero_bound(x, win)
                for sw in ((),) if cplx else ((), ("SP_NO_REALPAIR",)):
                    tag = (label, "c64" if cplx else "f32", M) + sw
                    with forced(*sw):
                        one, pseg = E.stft_frames(x, win, hop, M, detrend=det, sided=E.SIDED_ONE, amp_scale=amp, want_pseg=True,
                                                  mean_value=mv)
                        two, pseg2 = E.stft_frames(x, win, hop, M, detrend=det, sided=E.SIDED_TWO, amp_scale=amp, want_pseg=True,
                                                   mean_value=mv)
                        pw, pseg3 = E.stft_frames(x, win, hop, M, detrend=det, sided=E.SIDED_TWO, amp_scale=amp, power=True,
                                                  bin_major=True, want_pseg=True, mean_value=mv)
                    assert one.dtype == np.complex64 and two.dtype == np.complex64 and pw.dtype == np.float32
                    r1 = amp * R.layout(Xn, R.SIDED_ONE, amp=True)
                    r2 = amp * R.layout(Xn, R.SIDED_TWO)
                    rp = (amp * R.layout(np.abs(Xn) ** 2, R.SIDED_TWO)).T
                    if zero:
                        for got, ref, b in ((np.abs(one) ** 2, r1, 2 * amp ** 2 * bound), (np.abs(two) ** 2, r2, amp ** 2 * bound),
                                            (pw, rp, amp * bound), (pseg, rseg, bound), (pseg2, rseg, bound), (pseg3, rseg, bound)):
                            assert got.shape == ref.shape and np.all(np.isfinite(got)), tag
                            assert float(np.max(got)) <= b, tag
                        continue
                    worst.check(one, r1, 1e-4 * float(np.max(np.abs(r1))), tag + ("one-sided",))
                    worst.check(two, r2, 1e-4 * float(np.max(np.abs(r2))), tag + ("two-sided",))
                    worst.check(pw, rp, 1e-4 * float(np.max(rp)), tag + ("power, bin-major",))
                    for p in (pseg, pseg2, pseg3):
                        wseg.check(p, rseg, 1e-4 * rseg, tag + ("pseg",))
    worst.report()
    wseg.report()


# ------------------------------------------------------------------------------------------ sp_stft_cog
@pytest.mark.parametrize("nfft,hop", R.SHAPES, ids=IDS)
def test_stft_cog(E, nfft, hop):
    """whole band, the band [0.15 fs, 0.3 fs] and a band that holds no bin (exactly 0; so is the middle band at nfft 2 and
    3), Hann and boxcar windows"""
    fs = R.FS
    worst = Worst("stft_cog %dx%d" % (nfft, hop))
    for wname in ("Hanning", "Boxcar"):
        win = O.windows(wname, nwins=nfft)
        for cplx in DTYPES:
            for M in R.frame_counts(nfft):
                x = R.case_signal(nfft, hop, M, cplx)
                for label, det, mv, mode in R.mode_cases(cplx):
                    for band, fmin, fmax in R.cog_bands(nfft):
                        where = (wname, label, "c64" if cplx else "f32", M, band)
                        got = E.stft_cog(x, win, hop, M, fs, fmin=fmin, fmax=fmax, detrend=det, mean_value=mv)
                        assert got.shape == (M,) and got.dtype == np.float64, where
                        holds = R.band_mask(nfft, fs, fmin, fs if fmax is None else fmax).any()
                        if not holds:
                            assert band == "empty" or (band == "tone" and nfft <= 3)
                            assert not got.any(), where                      # exactly 0
                        elif nfft == 2 and mode == R.SEGLINEAR:              # the frame itself is zero: any quotient of residues
                            assert np.all(np.isfinite(got)) and float(np.max(np.abs(got))) <= 0.5 * fs, where
                        else:
                            ref, _ = R.cog(x, win, hop, M, mode, fs, fmin, fmax, mv)
                            worst.check(got, ref, 2e-4 * fs, where)
    worst.report()
