"""Host side of the time-resolved Welch spectra (running_psd / csd / coherence / spectra, engine.welch_blocks, sp_welch_blocks): the
float64 restatement of tests/welch_blocks_ref.py against scipy.signal.welch / csd / coherence on the blocks' slices, the block, run
and transform arithmetic of the plan, every refusal of the C entry before the device is touched and of the Python side before the
library loads, the exports and the significance level.  No GPU needed.  tests/test_gpu_welch_blocks.py takes the cases from here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
from pyfft_amd import _ffi, engine as E, _running_mod as RN
from test_host_multitaper import no_library        # noqa: F401  (a fixture)
from welch_blocks_ref import (hann, nframes_of, nblocks_of, welch_blocks_ref, coherence_ref, block_slice, make_pair)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AVG_STEP = [(1, 1), (2, 2), (8, 8), (5, 2), (6, 4), (8, 2), (4, 6)]
AVG_IDS = ["navg%d-step%d" % c for c in AVG_STEP]


def scipy_block(x, y, b, fs, win, nfft, hop, navg, step, detrend, scaling, onesided):
    """scipy's welch / csd / coherence of block b's slice."""
    s, e = block_slice(b, nfft, hop, navg, step)
    kw = dict(fs=fs, window=win, nperseg=nfft, noverlap=nfft - hop, detrend=detrend, return_onesided=onesided, scaling=scaling)
    xs = np.asarray(x[s:e]).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    pxx = ss.welch(xs, **kw)[1]
    if y is None:
        return pxx, None, None
    ys = np.asarray(y[s:e]).astype(xs.dtype)
    return pxx, ss.welch(ys, **kw)[1], ss.csd(xs, ys, **kw)[1]


@pytest.mark.parametrize("navg,step", AVG_STEP, ids=AVG_IDS)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("detrend", ["constant", False], ids=["segmean", "none"])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
def test_reference_is_scipy_on_the_slices(navg, step, cplx, detrend, scaling):
    nfft, hop, fs = 64, 24, 50.0
    nsig = 21 * hop + nfft + 5                       # 22 frames, 5 samples left over
    nframes = nframes_of(nsig, nfft, hop)
    x, y = make_pair(nsig, cplx, 3)
    win = hann(nfft)
    scale = 1.0 / (fs * np.sum(win ** 2)) if scaling == "density" else 1.0 / np.sum(win) ** 2
    pxx, pyy, pxy = welch_blocks_ref(x, y, nfft, hop, nframes, navg, step, win, detrend == "constant", scale, doubled=not cplx)
    nblocks = nblocks_of(nframes, navg, step)
    assert pxx.shape == (nblocks, nfft if cplx else nfft // 2 + 1) and pxy.shape == pxx.shape and nblocks >= 2
    for b in range(nblocks):
        rxx, ryy, rxy = scipy_block(x, y, b, fs, win, nfft, hop, navg, step, detrend, scaling, not cplx)
        np.testing.assert_allclose(pxx[b], rxx, rtol=1e-12, atol=0)
        np.testing.assert_allclose(pyy[b], ryy, rtol=1e-12, atol=0)
        np.testing.assert_allclose(pxy[b], rxy, rtol=1e-12, atol=0)
        s, e = block_slice(b, nfft, hop, navg, step)
        xs, ys = np.asarray(x[s:e], dtype=pxy.dtype if cplx else np.float64), np.asarray(y[s:e], dtype=pxy.dtype if cplx else np.float64)
        coh = ss.coherence(xs, ys, fs=fs, window=win, nperseg=nfft, noverlap=nfft - hop, detrend=detrend)[1]
        np.testing.assert_allclose(coherence_ref(pxx[b], pyy[b], pxy[b]), coh, rtol=1e-12, atol=0)


def test_reference_channels_and_psd_only():
    nfft, hop, nsig = 32, 16, 400
    nframes = nframes_of(nsig, nfft, hop)
    x, y = make_pair(nsig, False, 5, nch=3)
    pxx, pyy, pxy = welch_blocks_ref(x, y, nfft, hop, nframes, 4, 2, hann(nfft))
    assert pyy.shape == pxy.shape == (3,) + pxx.shape
    for c in range(3):
        one = welch_blocks_ref(x, y[c], nfft, hop, nframes, 4, 2, hann(nfft))
        np.testing.assert_array_equal(one[1], pyy[c])
        np.testing.assert_array_equal(one[2], pxy[c])
    only = welch_blocks_ref(x, None, nfft, hop, nframes, 4, 2, hann(nfft))
    np.testing.assert_array_equal(only[0], pxx)
    assert only[1] is None and only[2] is None


# (nfft, hop, nframes, navg, step, nch, cplx) -> (nblocks, q, runs, frames transformed)
PLANS = [
    ((256, 128, 40, 8, 8, 1, False), (5, 8, 5, 40)),
    ((256, 128, 40, 8, 2, 1, False), (17, 2, 20, 40)),
    ((256, 128, 40, 5, 2, 1, False), (18, 1, 39, 39)),          # one frame left over
    ((256, 128, 40, 6, 4, 1, False), (9, 2, 19, 38)),           # two left over
    ((256, 128, 40, 4, 6, 1, False), (7, 4, 7, 28)),            # step > navg: gaps, the frames between the blocks are not transformed
    ((256, 128, 40, 1, 1, 1, False), (40, 1, 40, 40)),
    ((256, 128, 40, 2, 2, 1, False), (20, 2, 20, 40)),
    ((1024, 385, 8, 8, 3, 1, False), (1, 1, 8, 8)),             # nframes == navg
    ((1024, 385, 8, 8, 8, 1, False), (1, 8, 1, 8)),
    ((32, 16, 4096, 8, 2, 3, False), (2045, 2, 2048, 4096)),
    ((8192, 4096, 41, 6, 4, 2, True), (9, 2, 19, 38)),
    ((256, 128, 40, 8, 2, 0, False), (17, 2, 20, 40)),          # PSD only
    ((256, 128, 40, 8, 2, 0, True), (17, 2, 20, 40)),
]


@pytest.mark.parametrize("shape,want", PLANS, ids=[str(p[0]) for p in PLANS])
def test_plan_arithmetic(shape, want):
    nfft, hop, nframes, navg, step, nch, cplx = shape
    nblocks, q, runs, used = want
    p = E.welch_blocks_plan(nfft, hop, nframes, navg, step, nch=nch, cplx=cplx)
    # transforms per frame: one without y, two per pair (x and y_c each have their own); twice that for a complex pair at 8192 points,
    # whose bins are split over two workgroups
    pairs, per_frame = max(nch, 1), 1 if nch < 1 else 2 * nch * (2 if cplx and nfft >= 8192 else 1)
    nb = nfft if cplx else nfft // 2 + 1
    assert (p["nblocks"], p["nb"], p["q"], p["runs"]) == (nblocks, nb, q, runs)
    assert nblocks == (nframes - navg) // step + 1 and runs * q == used
    # every frame is transformed once, whatever the overlap of the blocks: never more transforms than frames x pairs
    assert p["transforms"] == used * per_frame <= nframes * per_frame
    if step <= navg:                                            # no gaps: all frames but the leftovers
        assert used == (nblocks - 1) * step + navg and nframes - used < step
    planes = 4 if nch >= 1 else 1
    assert p["scratch"] == (0 if step >= navg else 4 * pairs * runs * planes * nb)
    images = max(1, 4096 // nfft) * (nfft + 16) * 8 * (2 if nch >= 1 else 1)
    assert p["lds_bytes"] == images <= 160 * 1024
    teams = max(1, 256 // nfft)
    assert 1 <= p["workgroups"] <= -(-runs // teams)


def test_running_plan_axes():
    fs, nperseg, noverlap, navg, step = 200.0, 256, 160, 6, 4
    hop = nperseg - noverlap
    nsig = 40 * hop + nperseg + 7
    p = RN.running_plan(nsig, nperseg, noverlap, navg, step, fs=fs, nch=2)
    assert (p["nframes"], p["hop"], p["nblocks"], p["nf"], p["q"]) == (41, 96, 9, 129, 2)
    b = np.arange(9)
    np.testing.assert_allclose(p["t0"], b * step * hop / fs, rtol=1e-15)
    np.testing.assert_allclose(p["t1"], (b * step * hop + (navg - 1) * hop + nperseg) / fs, rtol=1e-15)
    assert p["t1"][-1] * fs <= nsig
    assert p["transforms"] == 38 * 4 and p["bytes_composed"] > p["bytes_fused"] > 0
    # noverlap defaults to half a segment, step to navg
    p = RN.running_plan(1 << 16, 1024, navg=8)
    assert (p["hop"], p["nframes"], p["nblocks"], p["q"], p["scratch"]) == (512, 127, 15, 8, 0)
    # complex: all nperseg bins
    assert RN.running_plan(1 << 12, 64, cplx=True)["nf"] == 64


def _c_entry():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    fn = lib.sp_welch_blocks
    fn.restype, fn.argtypes = _ffi.SIGNATURES["sp_welch_blocks"]
    lib.sp_last_error.restype = ctypes.c_char_p
    return lib, fn


GOOD = dict(dtype=0, nsig=1000, nch=2, y_ld=1000, nfft=64, hop=32, nframes=20, navg=4, step=2, detrend=3, scale=1.0, doubled=1)
C_REFUSALS = [
    (dict(nfft=48), "nfft"), (dict(nfft=16), "nfft"), (dict(nfft=16384), "nfft"), (dict(nfft=0), "nfft"),
    (dict(hop=0), "hop"), (dict(hop=65), "hop"), (dict(hop=-3), "hop"),
    (dict(navg=0), "navg"), (dict(step=0), "step"), (dict(step=-1), "step"),
    (dict(nframes=3), "nframes"), (dict(nframes=0), "nframes"),
    (dict(nsig=19 * 32 + 63), "nsig"), (dict(nsig=10), "nsig"),
    (dict(nch=0), "nch"), (dict(nch=-1), "nch"),
    (dict(y_ld=999), "y_ld"),
    (dict(detrend=1), "detrend"), (dict(detrend=2), "detrend"), (dict(detrend=4), "detrend"), (dict(detrend=7), "detrend"),
    (dict(dtype=5), "dtype"),
    (dict(scale=float("nan")), "scale"),
    (dict(pxx=None), "pxx"), (dict(pyy=None), "pyy"), (dict(pxy=None), "pxy"), (dict(x=None), "x is required"),
]


@pytest.mark.parametrize("kw,name", C_REFUSALS, ids=["%s-%d" % (n.split()[0], i) for i, (_, n) in enumerate(C_REFUSALS)])
def test_c_entry_refuses_before_the_device(kw, name):
    """< 0, the message names sp_welch_blocks and the argument, the outputs are untouched.  (Without a GPU a call that got past its
    checks fails too, but with the runtime's message, not the argument's.)"""
    lib, fn = _c_entry()
    a = dict(GOOD)
    a.update({k: v for k, v in kw.items() if k in GOOD})
    x = np.ones(1000, dtype=np.float32)
    y = np.ones((2, 1000), dtype=np.float32)
    win = np.ones(64, dtype=np.float32)
    nb, nblocks = 33, 9
    bufs = dict(pxx=np.full((nblocks, nb), 7.0, np.float32), pyy=np.full((2, nblocks, nb), 7.0, np.float32),
                pxy=np.full((2, nblocks, nb), 7.0 + 7.0j, np.complex64))
    ptrs = {k: (None if (k in kw and kw[k] is None) else _ffi.ptr(v)) for k, v in bufs.items()}
    xp = None if ("x" in kw and kw["x"] is None) else _ffi.ptr(x)
    rc = fn(xp, _ffi.ptr(y), a["dtype"], a["nsig"], a["nch"], a["y_ld"], _ffi.ptr(win), a["nfft"], a["hop"], a["nframes"], a["navg"],
            a["step"], a["detrend"], a["scale"], a["doubled"], ptrs["pxx"], ptrs["pyy"], ptrs["pxy"], 0)
    msg = (lib.sp_last_error() or b"").decode()
    assert rc < 0, msg
    assert msg.startswith("sp_welch_blocks: " + name), msg
    assert np.all(bufs["pxx"] == 7.0) and np.all(bufs["pyy"] == 7.0) and np.all(bufs["pxy"] == 7.0 + 7.0j)


def test_c_plan_refuses():
    lib, _ = _c_entry()
    fn = lib.sp_welch_blocks_plan
    fn.restype, fn.argtypes = _ffi.SIGNATURES["sp_welch_blocks_plan"]
    out = np.zeros(8, dtype=np.int64)
    assert fn(0, 64, 32, 20, 4, 2, 1, out.ctypes.data) == 0 and out[0] == 9
    for bad in ((0, 48, 32, 20, 4, 2, 1), (0, 64, 0, 20, 4, 2, 1), (0, 64, 65, 20, 4, 2, 1), (0, 64, 32, 3, 4, 2, 1), (0, 64, 32, 20, 0, 2, 1),
                (0, 64, 32, 20, 4, 0, 1), (0, 64, 32, 20, 4, 2, -1), (0, 16384, 32, 20, 4, 2, 1)):
        assert fn(*bad, out.ctypes.data) < 0, bad
    assert fn(0, 64, 32, 20, 4, 2, 1, None) < 0


X2000, C2000 = np.zeros(2000), np.zeros(2000, complex)
PY_REFUSALS = [
    (dict(nperseg=300), "power of two"), (dict(nperseg=16), "power of two"), (dict(nperseg=16384, x=np.zeros(40000)), "power of two"),
    (dict(nfft=512), "zero padding"),
    (dict(detrend="linear"), "detrend"), (dict(detrend=2), "detrend"),
    (dict(noverlap=256), "noverlap"), (dict(noverlap=-1), "noverlap"),
    (dict(navg=0), "navg"), (dict(step=0), "step"), (dict(navg=50), "nframes"),
    (dict(nperseg=4096), "nframes"),
]


@pytest.mark.parametrize("kw,text", PY_REFUSALS, ids=[str(i) for i in range(len(PY_REFUSALS))])
def test_python_refusals_carry_both_types(no_library, kw, text):
    kw = dict(kw)
    x = kw.pop("x", X2000)
    calls = [lambda: RN.running_psd(x, **kw), lambda: RN.running_csd(x, x, **kw), lambda: RN.running_coherence(x, x, **kw),
             lambda: RN.running_spectra(x, x, **kw)]
    for call in calls:
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert isinstance(ei.value, ValueError) and isinstance(ei.value, E.WelchBlocksRefused) and text in str(ei.value)


def test_python_refusals_of_the_arguments(no_library):
    for kw, text in ((dict(y=C2000), "both be real or both be complex"), (dict(y=np.zeros(1999)), "x's length"),
                     (dict(fs=0.0), "fs must be positive"), (dict(scaling="psd"), "scaling must be"),
                     (dict(window=np.ones(255)), "window must be")):
        kw = dict(kw)
        y = kw.pop("y", X2000)
        with pytest.raises(ValueError) as ei:
            RN.running_spectra(X2000, y, **kw)
        assert text in str(ei.value)
    with pytest.raises(ValueError):
        RN.running_psd(np.zeros((2, 1000)))


def test_engine_refusals_carry_both_types(no_library):
    w = np.ones(64, dtype=np.float32)
    x = np.zeros(1000, dtype=np.float32)
    for args, kw, text in (((x, w, 0, 20, 4), {}, "hop"), ((x, w, 65, 10, 4), {}, "hop"), ((x, w, 32, 20, 0), {}, "navg"),
                           ((x, w, 32, 20, 4), dict(step=0), "step"), ((x, w, 32, 3, 4), {}, "nframes"), ((x, w, 32, 40, 4), {}, "shorter"),
                           ((x, np.ones(48), 24, 10, 4), {}, "power of two"), ((x, w, 32, 20, 4), dict(detrend="linear"), "detrend"),
                           ((x, w, 32, 20, 4), dict(detrend=2), "detrend"),
                           ((x, w, 32, 20, 4), dict(y=np.zeros((2, 999), dtype=np.float32)), "shorter than x")):
        with pytest.raises(NotImplementedError) as ei:
            E.welch_blocks(*args, **kw)
        assert isinstance(ei.value, ValueError) and text in str(ei.value)
    with pytest.raises(ValueError):
        E.welch_blocks(x, None, 32, 20, 4)                      # no window and no nfft


def test_exported():
    for name in ("running_psd", "running_csd", "running_coherence", "running_spectra", "running_plan", "coherence_level"):
        assert getattr(pyfft_amd, name) is getattr(RN, name)
    assert callable(E.welch_blocks) and callable(E.welch_blocks_plan)
    assert issubclass(E.WelchBlocksRefused, ValueError) and issubclass(E.WelchBlocksRefused, NotImplementedError)
    assert RN.WelchBlocksRefused is E.WelchBlocksRefused


def test_coherence_level():
    assert RN.coherence_level(1) == 1.0
    assert RN.coherence_level(2) == pytest.approx(0.95, rel=1e-15)
    assert RN.coherence_level(8) == pytest.approx(1 - 0.05 ** (1 / 7.0), rel=1e-15)
    assert RN.coherence_level(8, alpha=0.01) == pytest.approx(1 - 0.01 ** (1 / 7.0), rel=1e-15)
    assert RN.coherence_level(100) == pytest.approx(1 - math.exp(math.log(0.05) / 99), rel=1e-12)
    levels = [RN.coherence_level(n) for n in (2, 4, 8, 16, 64)]
    assert all(a > b for a, b in zip(levels, levels[1:]))
    assert "optimistic" in RN.coherence_level.__doc__
    for bad in (dict(navg=0), dict(navg=4, alpha=0.0), dict(navg=4, alpha=1.0)):
        with pytest.raises(ValueError):
            RN.coherence_level(**bad)


def test_axes_handed_to_the_engine(no_library, monkeypatch):
    """f, t, scale, doubling and the frame arithmetic running_spectra hands down, and the two-sided mirror of a real record."""
    seen = {}

    def fake(x, y=None, **kw):
        seen.update(kw)
        nframes, navg, step, nfft = kw["nframes"], kw["navg"], kw["step"], len(kw["win"])
        nb = nfft if np.iscomplexobj(x) else nfft // 2 + 1
        shape = ((nframes - navg) // step + 1, nb)
        k = np.arange(nb, dtype=np.float32)
        pxx = np.broadcast_to(1 + k, shape).copy()
        return pxx, 2 * pxx, (pxx * (1 + 1j)).astype(np.complex64)
    monkeypatch.setattr(E, "welch_blocks", fake)
    fs, nperseg, noverlap, navg, step = 100.0, 64, 40, 6, 4
    hop = nperseg - noverlap
    nsig = 30 * hop + nperseg + 3
    r = RN.running_spectra(np.zeros(nsig), np.zeros(nsig), fs=fs, nperseg=nperseg, noverlap=noverlap, navg=navg, step=step)
    w = hann(nperseg)
    assert (seen["hop"], seen["nframes"], seen["navg"], seen["step"], seen["detrend"], seen["doubled"]) == (24, 31, 6, 4, True, True)
    assert np.isclose(seen["scale"], 1.0 / (fs * np.sum(w * w)), rtol=1e-14) and np.allclose(seen["win"], w, atol=1e-15)
    np.testing.assert_allclose(r.f, np.fft.rfftfreq(nperseg, 1 / fs))
    nblocks = (31 - 6) // 4 + 1
    np.testing.assert_allclose(r.t, (np.arange(nblocks) * step * hop + ((navg - 1) * hop + nperseg) / 2.0) / fs, rtol=1e-15)
    assert r.Pxx.shape == (nblocks, 33) and (r.navg, r.step) == (6, 4)
    np.testing.assert_allclose(r.coherence, np.ones(r.Pxx.shape), rtol=1e-6)            # |Pxx (1 + i)|^2 / (Pxx 2 Pxx)
    assert r.coherence.dtype == np.float64
    np.testing.assert_allclose(r.phase, np.full(r.Pxy.shape, math.pi / 4), rtol=1e-6)
    # two-sided from a real record: fftfreq order, bin n - k mirrors bin k, the cross spectrum conjugated; nothing doubled
    f, t, pxy = RN.running_csd(np.zeros(nsig), np.zeros(nsig), fs=fs, nperseg=nperseg, noverlap=noverlap, navg=navg, step=step,
                               return_onesided=False, scaling="spectrum", detrend=False)
    assert (seen["doubled"], seen["detrend"]) == (False, False) and np.isclose(seen["scale"], 1.0 / np.sum(w) ** 2, rtol=1e-14)
    np.testing.assert_allclose(f, np.fft.fftfreq(nperseg, 1 / fs))
    assert pxy.shape == (nblocks, 64)
    k = np.arange(1, 32)
    np.testing.assert_array_equal(pxy[:, 64 - k], np.conj(pxy[:, k]))
    # complex records: fftfreq order, all bins, nothing doubled, navg and step defaults
    f, t, pxx = RN.running_psd(np.zeros(nsig, complex), fs=fs, nperseg=nperseg)
    assert (seen["doubled"], seen["hop"], seen["navg"], seen["step"]) == (False, 32, 8, 8) and pxx.shape[1] == 64
    np.testing.assert_allclose(f, np.fft.fftfreq(nperseg, 1 / fs))


def test_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("sp_welch_blocks", 19), ("sp_welch_blocks_plan", 8)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt, "%s is not declared in include/spectral.h" % name
        nargs = len([a for a in mt.group(1).split(",") if a.strip()])
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs == want
        assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)
