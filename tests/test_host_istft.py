"""Host side of the inverse STFT: argument refusals and the NOLA warning of spectrogram.istft (raised before the library loads),
the host plan (frames, skip, nout, time axis, envelope pieces) against a float64 overlap-add and scipy.signal.istft, and the
declaration / binding of sp_istft.  No GPU needed."""
import os
import re
import warnings

import numpy as np
import pytest
import scipy.signal as ss

from pyfft_amd import spectrogram as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = ["hann", "hamming", "blackman", ("tukey", 0.5), "boxcar"]
SHAPES = [(32, 8), (256, 64), (1024, 512), (1024, 256), (4096, 1024), (8192, 2048), (1000, 250), (3640, 910), (777, 111),
          (64, 64), (64, 1)]


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the refusals must come first."""
    from pyfft_amd import _ffi

    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "load_library", boom)
    monkeypatch.setattr(_ffi, "init", boom)


def test_exported():
    import pyfft_amd
    assert pyfft_amd.istft is S.istft
    assert callable(pyfft_amd.engine.istft_frames) and callable(pyfft_amd.fftanal.scipy_istft)


@pytest.mark.parametrize("kw,exc,text", [
    (dict(Z=np.zeros(5, complex)), ValueError, "at least 2d"),
    (dict(time_axis=-2), ValueError, "differing time and frequency axes"),
    (dict(nperseg=0), ValueError, "nperseg must be a positive integer"),
    (dict(nperseg=256, nfft=128), ValueError, "nfft must be greater than or equal to nperseg"),
    (dict(noverlap=256), ValueError, "noverlap must be less than nperseg"),
    (dict(window=np.ones((2, 128))), ValueError, "window must be 1-D"),
    (dict(window=np.ones(100)), ValueError, "window must have length of 256"),
    (dict(scaling="power"), ValueError, "not in ['spectrum', 'psd']"),
    (dict(window="no_such_window"), ValueError, "Unknown window type"),
    (dict(nperseg=200), NotImplementedError, "nfft"),
    (dict(nfft=512), NotImplementedError, "nfft"),
])
def test_refusals_before_the_library(no_library, kw, exc, text):
    kw = dict(kw)
    Z = kw.pop("Z", np.zeros((129, 9), complex))
    with pytest.raises(exc) as ei:
        S.istft(Z, **kw)
    assert text in str(ei.value)
    if exc is ValueError and "Z" not in kw and text != "Unknown window type":          # scipy refuses the same call
        with pytest.raises(ValueError):
            ss.istft(Z, **kw)


def test_nola_warning_text(no_library, monkeypatch):
    """A window / hop pair that fails NOLA warns with scipy's text, then goes on to the engine (stubbed here)."""
    from pyfft_amd import engine
    monkeypatch.setattr(engine, "istft_frames", lambda Z, win, hop, **k: np.zeros(Z.shape[:-2] + (k["nout"],), np.float32))
    win = np.ones(64)
    win[::2] = 0.0
    Z = np.zeros((33, 12), complex)
    for boundary in (True, False):
        with warnings.catch_warnings(record=True) as ours:
            warnings.simplefilter("always")
            t, x = S.istft(Z, window=win, nperseg=64, noverlap=32, boundary=boundary)
        with warnings.catch_warnings(record=True) as ref:
            warnings.simplefilter("always")
            tr, xr = ss.istft(Z, window=win, nperseg=64, noverlap=32, boundary=boundary)
        assert len(ours) == 1 and len(ref) == 1 and issubclass(ours[0].category, UserWarning)
        assert str(ours[0].message) == str(ref[0].message)
        assert x.shape == xr.shape and x.dtype == xr.dtype and np.array_equal(t, tr)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        S.istft(Z, window="hann", nperseg=64, noverlap=32)          # NOLA holds: no warning


@pytest.mark.parametrize("nfft,hop", SHAPES)
@pytest.mark.parametrize("wname", WINDOWS, ids=lambda w: w if isinstance(w, str) else w[0])
def test_plan_against_overlap_add_and_scipy(nfft, hop, wname):
    win = ss.get_window(wname, nfft)
    for nseg in (1, 2, 3, 41):
        env = np.zeros((nseg - 1) * hop + nfft)
        for g in range(nseg):
            env[g * hop:g * hop + nfft] += win ** 2
        for boundary in (True, False):
            p = S.istft_plan(nseg, win, hop, boundary=boundary, fs=250.0)
            assert p["L"] == env.size and p["nframes"] == nseg
            assert p["period"].size == hop and p["head_len"] == p["head"].size
            assert p["head"].size + p["tail"].size <= max(2 * (nfft - hop), env.size)      # pieces, not a full-length array
            got = S.plan_envelope(p)
            assert got.shape == env.shape and np.max(np.abs(got - env)) <= 1e-12 * env.max()
            assert p["skip"] == (nfft // 2 if boundary else 0) and p["nout"] == env.size - 2 * p["skip"]
            if p["nout"] < 1 or (nfft > 1024 and nseg == 41 and wname != "hann"):
                continue                                                                   # (scipy reference: a subset is enough)
            nb = nfft // 2 + 1
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t, x = ss.istft(np.zeros((nb, nseg), complex), fs=250.0, window=win, nperseg=nfft, noverlap=nfft - hop,
                                nfft=nfft, boundary=boundary)
            assert x.size == p["nout"] and np.allclose(t, p["time"], rtol=1e-15, atol=0)
            kept = env[p["skip"]:p["skip"] + p["nout"]]
            assert S._plan_nola(p) == bool(np.all(kept > 1e-10))


def test_prepare_defaults_match_scipy():
    """nperseg from the frequency axis, noverlap = nperseg // 2, odd nperseg, two-sided input, axes, psd scaling."""
    fa, ta, win, hop, plan, scale = S._istft_prepare((129, 9), "hann", None, None, None, True, True, -1, -2, "spectrum", 1.0)
    assert (fa, ta, win.size, hop, plan["nframes"]) == (0, 1, 256, 128, 9) and scale == pytest.approx(ss.get_window("hann", 256).sum())
    fa, ta, win, hop, plan, scale = S._istft_prepare((3, 9, 129), "hann", 257, 64, None, True, False, 1, 2, "psd", 4.0)
    assert (fa, ta, win.size, hop, plan["nframes"], plan["skip"]) == (2, 1, 257, 193, 9, 0)
    assert scale == pytest.approx(np.sqrt(4.0 * np.sum(ss.get_window("hann", 257) ** 2)))
    fa, ta, win, hop, plan, scale = S._istft_prepare((100, 7), np.ones(100), None, 75, None, False, True, -1, -2, "spectrum", 1.0)
    assert (win.size, hop, plan["nout"]) == (100, 25, 6 * 25 + 100 - 100)


def test_declared_and_bound():
    from pyfft_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    m = re.search(r"int sp_istft\(([^;]*)\);", hdr)
    assert m, "sp_istft is not declared in include/spectral.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert "sp_istft" in _ffi.SIGNATURES and len(_ffi.SIGNATURES["sp_istft"][1]) == nargs == 13
    if os.path.exists(_ffi.LIB_PATH):
        import ctypes
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "sp_istft")
