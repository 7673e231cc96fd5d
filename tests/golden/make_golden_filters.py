#!/usr/bin/env python3
"""Golden vectors for the reference's IIR wrappers (filters.py:323-358): butter_bandpass, butter_lowpass,
butter_lowpass_filter, complex_filtfilt.

TEST INFRASTRUCTURE, run where the reference checkout is (make_golden.REF).  Loads the reference's filters.py unmodified with the
pybaseutils stand-in of make_golden.py and the Agg matplotlib backend, runs it on seeded float32-valued inputs and stores
inputs + outputs in tests/golden/filters.npz.
Usage:  python tests/golden/make_golden_filters.py
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import scipy.signal
from make_golden import _install_shims, _load, save

# butter_lowpass(cutoff, fnyq, order) designs recorded as (b, a)
LOWPASS = [(100e3, 1e6, 5), (50.0, 500.0, 3), (0.2, 1.0, 8), (1.0e3, 4.0e6, 5)]
BANDPASS_OTHER = dict(fs=1e6, lf=20e3, hf=200e3, order=4)
LP_FILTER = dict(cutoff=50e3, fs=1e6, order=5)          # normalised by fs (the reference's quirk): wn = 0.05


def main():
    _install_shims()
    F = _load("filters")
    rng = np.random.default_rng(0x5EED1117)
    d = {}
    x = rng.standard_normal(8192).astype(np.float32)
    d["bp_x"] = x
    d["bp_default"] = F.butter_bandpass(x.astype(np.float64))
    d["bp_other"] = F.butter_bandpass(x.astype(np.float64), **BANDPASS_OTHER)
    d["bp_other_args"] = np.array([BANDPASS_OTHER[k] for k in ("fs", "lf", "hf", "order")], dtype=np.float64)
    for i, (cut, fnyq, order) in enumerate(LOWPASS):
        b, a = F.butter_lowpass(cut, fnyq, order=order)
        d["lp_args_%d" % i] = np.array([cut, fnyq, order], dtype=np.float64)
        d["lp_b_%d" % i] = b
        d["lp_a_%d" % i] = a
    data = (rng.standard_normal((8192, 4)) + np.linspace(-1.0, 2.0, 4)).astype(np.float32)
    d["lpf_x"] = data
    d["lpf_args"] = np.array([LP_FILTER["cutoff"], LP_FILTER["fs"], LP_FILTER["order"]], dtype=np.float64)
    d["lpf_y"] = F.butter_lowpass_filter(data.astype(np.float64), LP_FILTER["cutoff"], LP_FILTER["fs"],
                                         order=LP_FILTER["order"], axis=0)
    k = np.arange(4096)
    z = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096) + 2.0 * np.exp(2j * np.pi * 0.01 * k)).astype(np.complex64)
    b, a = scipy.signal.butter(4, 0.1)
    d["cf_x"] = z
    d["cf_b"] = b
    d["cf_a"] = a
    d["cf_y"] = F.complex_filtfilt(b, a, z.astype(np.complex128))
    save("filters", **d)


if __name__ == "__main__":
    main()
