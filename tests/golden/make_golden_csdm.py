#!/usr/bin/env python3
"""Golden vectors that pin oracle.csd_matrix to the reference: the reference has no matrix entry point, its fft_pwelch
(fft_analysis.py:36-648, homebrew branch :339-446) takes one x against the channels of y, so the matrix is its own fft_pwelch
looped over all ORDERED pairs of 4 seeded channels.  nfft 256 (Navr=7 over 1024 samples), Hann at 50 % overlap, mean detrend,
two-sided output; tbounds ends one sample short of the record, so the reflection branch (:197-205) stays off.

Only inputs and outputs are stored; the inputs are float32 values held as float64 (they compress, and the file stays small).
The archive is written with fixed zip timestamps, so running this again reproduces tests/golden/csd_matrix_4ch.npz bit for bit.

TEST INFRASTRUCTURE, build container only (needs /root/reference).
Usage:  python tests/golden/make_golden_csdm.py
"""
import os
import sys
import zipfile

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

NCH, NSIG, NAVR = 4, 1024, 7


def inputs():
    """4 channels: a common line with per-channel gain and phase, a shared noise component, independent noise, offsets"""
    rng = np.random.default_rng(20240611)
    n = NSIG + 1                                  # one extra sample: tbounds = [t[0], t[-2]] selects NSIG samples, no reflection
    k = np.arange(n, dtype=np.float64)
    t = k / 1024.0                                # (a power of two: the sample times and Fs are exact)
    common = rng.standard_normal(n)
    x = np.stack([(1.0 + 0.3 * c) * np.sin(2 * np.pi * 0.093 * k + 0.7 * c) + 0.4 * np.roll(common, c)
                  + rng.standard_normal(n) + 0.5 * c - 0.8 for c in range(NCH)], axis=1)
    return t, x.astype(np.float32).astype(np.float64)                        # [n, NCH]


def save_fixed(path, **arrs):
    """np.savez_compressed with every member's timestamp fixed: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrs):
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with z.open(zi, "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrs[name]), allow_pickle=False)
    print("wrote %-28s %8.1f KiB" % (os.path.basename(path), os.path.getsize(path) / 1024.0))


def main():
    from make_golden import _install_shims, _load, OUT
    _install_shims()
    _load("windows")
    fa = _load("fft_analysis")
    t, x = inputs()
    tb = [t[0], t[-2]]
    P = None
    for i in range(NCH):
        for j in range(NCH):
            freq, Pxy, Pxx, Pyy, Cxy, phi, info = fa.fft_pwelch(t, x[:, i].copy(), x[:, j].copy(), tbounds=tb, Navr=NAVR,
                                                                windowoverlap=0.5, windowfunction="Hanning", detrend_style=1,
                                                                onesided=False, plotit=False, verbose=False)
            if P is None:
                P = np.zeros((NCH, NCH, np.size(freq)), dtype=np.complex128)
                f0 = np.asarray(freq).copy()
                meta = dict(nwins=np.int64(info.nwins), noverlap=np.int64(info.noverlap), Navr=np.int64(info.Navr),
                            Fs=np.float64(info.Fs), S2=np.float64(info.S2), ibnds=np.asarray(info.ibnds))
            P[i, j] = np.asarray(Pxy).ravel()                                 # fft_pwelch(x = channel i, y = channel j)
            if i == j:
                assert np.array_equal(np.asarray(Pxx).ravel(), np.asarray(Pyy).ravel())
    assert int(meta["nwins"]) == 256
    save_fixed(os.path.join(OUT, "csd_matrix_4ch.npz"), t=t, x=x, freq=f0, Pxy=P, **meta)


if __name__ == "__main__":
    main()
