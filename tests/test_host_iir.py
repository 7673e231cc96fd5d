"""CPU checks of the IIR surface (cascaded second-order sections): the reference's names exist, its host designs match
the fixture, the fixture is pinned to scipy.signal, and bad arguments are refused before any device work."""
import numpy as np
import pytest
import scipy.signal as ss

from conftest import load_golden

import pyfft_amd
from pyfft_amd import _ffi, engine as E, filters as F


def test_reference_filter_names_exist():
    for name in ("butter_lowpass_filter", "butter_bandpass"):
        assert callable(getattr(pyfft_amd, name)), name
    for name in ("butter_bandpass", "butter_lowpass", "butter_lowpass_filter", "complex_filtfilt", "sosfilt", "sosfiltfilt",
                 "lfilter", "filtfilt"):
        assert callable(getattr(F, name)), name
    assert pyfft_amd.butter_bandpass is F.butter_bandpass
    for name in ("upsample", "downsample", "downsample_efficient"):      # need the absent pybaseutils.utils.interp
        with pytest.raises(NotImplementedError):
            getattr(F, name)(np.zeros(8), 1.0, 0.5)


def test_butter_lowpass_matches_reference_design():
    g = load_golden("filters")
    i = 0
    while "lp_args_%d" % i in g:
        cut, fnyq, order = g["lp_args_%d" % i]
        b, a = F.butter_lowpass(cut, fnyq, order=int(order))
        np.testing.assert_allclose(b, g["lp_b_%d" % i], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(a, g["lp_a_%d" % i], rtol=1e-12, atol=1e-300)
        i += 1
    assert i >= 3


def test_fixture_is_the_scipy_calls():
    """The reference's functions are scipy's lfilter / filtfilt on its (b, a) designs: the fixture says so to 1e-12."""
    g = load_golden("filters")
    x = g["bp_x"].astype(np.float64)
    b, a = ss.butter(3, [1000 / 2e6, 500e3 / 2e6], btype="band")
    np.testing.assert_allclose(g["bp_default"], ss.lfilter(b, a, x), rtol=0, atol=1e-12 * np.abs(g["bp_default"]).max())
    fs, lf, hf, order = g["bp_other_args"]
    b, a = ss.butter(int(order), [lf / (fs / 2), hf / (fs / 2)], btype="band")
    np.testing.assert_allclose(g["bp_other"], ss.lfilter(b, a, x), rtol=0, atol=1e-12 * np.abs(g["bp_other"]).max())
    cutoff, fs, order = g["lpf_args"]
    b, a = ss.butter(int(order), cutoff / fs)                      # normalised by fs, not fs / 2 (filters.py:345)
    want = ss.filtfilt(b, a, g["lpf_x"].astype(np.float64), axis=0)
    np.testing.assert_allclose(g["lpf_y"], want, rtol=0, atol=1e-12 * np.abs(want).max())
    z = g["cf_x"].astype(np.complex128)
    want = ss.filtfilt(g["cf_b"], g["cf_a"], z.real) + 1j * ss.filtfilt(g["cf_b"], g["cf_a"], z.imag)
    np.testing.assert_allclose(g["cf_y"], want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_sosfiltfilt_default_padlen_rule():
    sos5 = ss.butter(5, 0.1, output="sos")                          # last section first order: b2 = a2 = 0
    assert F._sos_padlen(sos5) == 3 * (2 * 3 + 1 - 1)
    sos6 = ss.butter(6, 0.1, output="sos")
    assert F._sos_padlen(sos6) == 3 * (2 * 3 + 1)


def test_refusals_before_device_work():
    x = np.zeros(64, dtype=np.float32)
    good = ss.butter(3, 0.1, output="sos")
    with pytest.raises(ValueError):
        E.sos_filter(np.tile(good[:1], (9, 1)), x)                  # 9 sections
    unstable = good.copy()
    unstable[0, 3:] = [1.0, -2.2, 1.21]                             # double pole at 1.1
    with pytest.raises(ValueError):
        E.sos_filter(unstable, x)
    bad = good.copy()
    bad[1, 3] = 0.0
    with pytest.raises(ValueError):
        E.sos_filter(bad, x)
    bad = good.copy()
    bad[0, 1] = np.nan
    with pytest.raises(ValueError):
        E.sos_filtfilt(bad, x, "odd", 3)
    with pytest.raises(ValueError):
        F.sosfiltfilt(good, np.zeros(12))                           # n <= padlen = 3 * (2 * 2 + 1 - 1)
    with pytest.raises(ValueError):
        E.sos_filtfilt(good, x, "reflect", 3)
    with pytest.raises(ValueError):
        E.sos_filter(good, x, zi=np.zeros((3, 2)))                  # zi shape: (2 sections, 2)
    with pytest.raises(NotImplementedError):
        F.lfilter([1.0, 0.5], [1.0, -0.5], x, zi=np.zeros(1))
    with pytest.raises(NotImplementedError):
        F.filtfilt([1.0, 0.5], [1.0, -0.5], x, method="gust")
    b, a = ss.butter(17, 0.2)
    with pytest.raises(ValueError):
        F.lfilter(b, a, x)                                           # order 17 > 16


def test_library_refuses_bad_sections_without_a_device():
    """sp_sosfilt / sp_sosfiltfilt check their sections before they initialise the device: -1 and the reason."""
    lib = _ffi.load_library()
    x = np.zeros(64, dtype=np.float32)
    y = np.empty_like(x)
    sos = np.ascontiguousarray(np.tile(ss.butter(2, 0.1, output="sos"), (9, 1)))
    assert lib.sp_sosfilt(_ffi.ptr(sos), 9, _ffi.ptr(x), 1, 64, None, _ffi.ptr(y), None, 0) == -1
    assert b"sections" in lib.sp_last_error()
    sos = np.ascontiguousarray(ss.butter(4, 0.1, output="sos"))
    sos[1, 3:] = [1.0, 0.0, -1.0001]                                 # poles at +-1.00005
    assert lib.sp_sosfiltfilt(_ffi.ptr(sos), 2, _ffi.ptr(x), 1, 64, 1, 10, _ffi.ptr(y), 0) == -1
    assert b"unstable" in lib.sp_last_error()
    sos[1, 3:] = [0.0, 0.0, 0.0]
    assert lib.sp_sosfilt(_ffi.ptr(sos), 2, _ffi.ptr(x), 1, 64, None, _ffi.ptr(y), None, 0) == -1
    assert b"a0" in lib.sp_last_error()
    sos = np.ascontiguousarray(ss.butter(2, 0.1, output="sos"))
    assert lib.sp_sosfiltfilt(_ffi.ptr(sos), 1, _ffi.ptr(x), 1, 10, 1, 10, _ffi.ptr(y), 0) == -1
    assert b"padlen" in lib.sp_last_error()
