"""The schedule of k_welch_pipe's middle and back roles (pyfft_amd/csrc/k_welch_pipe.hip): the periods that both gather and
transform run in a loop of their own, two per trip and without the fill / drain guards; the fill and drain periods run the
guarded form around that loop.  What can go wrong is the seam: a frame
dropped, doubled or taken from the wrong register set or image where the guarded periods hand over to the steady loop and back,
or a wave that runs one barrier more or less than the others.  So: the smallest frame counts (1 ... 7 frames per run: zero, one and
two trips of the steady loop, odd and even), counts that leave workgroups without work, and every mode that shares the two roles
(plain, one-pass detrend with lobe sums and with block sums, real pairs, moments per frame, packed spectra for the CSD matrix).
At these frame counts one frame is 14 % or more of the result.  SP_WELCH_PIPE=2 forces the pipeline at any frame count; the switch
is read once per process, hence the child processes.  Every result is held to 2e-4 |ref| + 1e-6 max|ref| of oracle.cpu_ref."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRELUDE = r"""
import numpy as np, sys
sys.path.insert(0, %r)
from pyfft_amd import engine as E
from oracle import cpu_ref as O
nfft = 4096
hann = O.windows("Hanning", nwins=nfft)
worst = 0.0
def excess(got, ref):
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got) - ref) / (2e-4 * np.abs(ref) + 1e-6 * np.abs(ref).max())))
def check(got, ref, *case):
    global worst
    err = excess(got, ref)
    print("excess %%.4f" %% err, case, E.profile_last_kernel())
    worst = max(worst, err)
    assert E.profile_last_kernel().startswith("k_welch_pipe"), (E.profile_last_kernel(), case)
    assert err <= 1.0, (case, err)
def csig(rng, n, dc):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) + np.complex64(dc)
def psd(s, win, hop, M, detrend):
    return E.welch_psd(s, win, hop, M, detrend=detrend, sided=E.SIDED_TWO, scale=1.0 / float(np.sum(win ** 2)))
""" % ROOT


def _run(body, timeout=300):
    env = dict(os.environ, SP_WELCH_PIPE="2")
    r = subprocess.run([sys.executable, "-c", PRELUDE + body + '\nprint("schedule ok worst/allowance %.4f" % worst)\n'],
                       env=env, capture_output=True, text=True, timeout=timeout)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "schedule ok" in r.stdout


def test_complex_one_to_seven_frames_every_hop():
    """modes 9 / 1 (mean detrend) and 0 (none) at 1 ... 7 frames, hops 1024, 2048, 4096; 17 samples behind the last frame count
    in the mean"""
    _run(r"""
rng = np.random.default_rng(21)
for hop in (1024, 2048, 4096):
    for M in (1, 2, 3, 4, 5, 6, 7):
        s = csig(rng, (M - 1) * hop + nfft + 17, 0.7 - 0.2j)
        for det in (True, False):
            check(psd(s, hann, hop, M, det), O.welch_psd_stream(s, hann, nfft, hop, M, 1.0, detrend_style=1 if det else 0), hop, M, det)
""")


def test_complex_odd_and_even_trips_blackman_and_real_pairs():
    """257 and 515 frames at hop 2048 (odd and even trips of a run, workgroups without work); a Blackman window, whose spectrum
    is not confined to the lobe bins: mode 1 with the block sums instead of mode 9; real input, two frames per transform, at
    2, 3, 8, 9 frames (the front role of modes 3 / 4 is another one, the middle and back roles are these)"""
    _run(r"""
rng = np.random.default_rng(22)
hop = 2048
for M in (257, 515):
    s = csig(rng, (M - 1) * hop + nfft + 17, -0.4 + 0.9j)
    for det in (True, False):
        check(psd(s, hann, hop, M, det), O.welch_psd_stream(s, hann, nfft, hop, M, 1.0, detrend_style=1 if det else 0), hop, M, det)
black = O.windows("Blackman", nwins=nfft)
for M in (3, 6, 257):
    s = csig(rng, (M - 1) * hop + nfft + 17, 0.7 - 0.2j)
    check(psd(s, black, hop, M, True), O.welch_psd_stream(s, black, nfft, hop, M, 1.0, detrend_style=1), "blackman", M)
    assert E.profile_last_kernel() == "k_welch_pipe(onepass)", E.profile_last_kernel()
for M in (2, 3, 8, 9):
    s = (rng.standard_normal((M - 1) * hop + nfft + 5) + 1.7).astype(np.float32)
    for det in (True, False):
        check(psd(s, hann, hop, M, det), O.welch_psd_stream(s, hann, nfft, hop, M, 1.0, detrend_style=1 if det else 0), "real", M, det)
        assert "realpair" in E.profile_last_kernel(), E.profile_last_kernel()
""")


def test_moments_per_frame():
    """stft_cog (modes 2 / 8: the back role reduces every frame's moments) at 5 and 131 frames, with and without the mean
    detrend.  The line sweeps 180 ... 320 Hz of fs = 1000 Hz, so that |ref| in the allowance is the line's frequency in every
    frame."""
    _run(r"""
rng = np.random.default_rng(23)
fs, hop = 1.0e3, 2048
for M in (5, 131):
    n = (M - 1) * hop + nfft
    tt = np.arange(n) / fs
    f_inst = 250.0 + 70.0 * np.sin(2 * np.pi * tt / (n / fs))
    s = (np.exp(2j * np.pi * np.cumsum(f_inst) / fs) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    _, ref = O.cog_frames(tt, s, fs, win=nfft, ov=0.5, window=hann)
    check(E.stft_cog(s, hann, hop, M, fs), ref, "cog", M)
    s = s + np.complex64(0.8 - 0.6j)
    s64 = s.astype(np.complex128)
    _, ref = O.cog_frames(tt, s64 - s64.mean(), fs, win=nfft, ov=0.5, window=hann)
    check(E.stft_cog(s, hann, hop, M, fs, detrend=True), ref, "cog, mean detrend", M)
""")


def test_csd_matrix_packed_spectra():
    """the CSD matrix of 3 channels at hop 2048: from 32 frame pairs per run on the spectra stage is the pipeline (modes 5 / 7:
    the back role writes the packed pair spectra), 86 runs per channel on 256 CUs; an odd frame count (a lone last frame).  The
    channels share a component, so that no cross spectrum averages to nothing and |ref| carries the allowance in every entry"""
    _run(r"""
rng = np.random.default_rng(24)
nch, M, hop = 3, 6001, 2048
nsig = (M - 1) * hop + nfft + 300
x = (0.5 * rng.standard_normal((nch, nsig), dtype=np.float32) + rng.standard_normal(nsig, dtype=np.float32)[None, :]
     + np.array([0.4, -1.1, 2.0], dtype=np.float32)[:, None]).astype(np.float32)
S2 = float(np.sum(hann ** 2))
for det in (True, False):
    G = E.csd_matrix(x, hann, hop, M, detrend=det, scale=1.0)
    ref = O.csd_matrix(x, hann, nfft, hop, M, 1.0, detrend_style=1 if det else 0) * S2
    check(G, ref, "csd matrix", nch, M, det)
""", timeout=600)
