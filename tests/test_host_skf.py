"""Host side of the two-point wavenumber-frequency spectrum S(k, f) (skf, skf_moments, dispersion, skf_plan): the float64 oracle from
the definition with its bin-edge bounds, the moments, the plan, every Python-side refusal before the library loads, and the declaration
and binding of sp_skf / sp_skf_plan.  No GPU needed.  tests/test_gpu_skf.py imports the oracle, the inputs and the shapes from here.

A histogram is discontinuous: a float32 phase within its error of a bin edge may land next door.  So the oracle returns three tables:
the float64 histogram, `lower` (the sure samples only) and `upper` (every unsure sample added to every bin its interval touches).  A
sample (g, f) is sure when theta +- delta lies in one bin, delta = 4e-6 + 1e-4 (max_f |X_g| / |X_g[f]| + max_f |Y_g| / |Y_g[f]|): the
project's bound for a frame's spectrum (1e-4 of its largest bin, as in the STFT and correlation parity tests) turned into a phase, plus
atan2f and the float32 index arithmetic.  The unsure samples may carry at most 5 % of the band's power in every case (asserted here on
the oracle alone); the pairs are the same noise delayed by 3 samples plus 0.3 of independent noise, different offsets."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import pyfft_amd
from pyfft_amd import _ffi, _wavenumber_mod as WN
from test_host_multitaper import no_library        # noqa: F401  (a fixture)
from test_host_xcorr_frames import make_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nfft, hop, nk, (b0, nb), complex).  The bands of real records leave out bins 0 and nfft/2: there X conj Y is real and the phase
# sits exactly on a bin edge for even nk.
SHAPES = [(32, 16, 16, (1, 15), False), (64, 24, 33, (1, 31), False), (256, 100, 64, (1, 127), False), (256, 128, 65, (200, 112), True),
          (1024, 300, 63, (100, 300), False), (1024, 512, 64, (1, 511), False), (4096, 2048, 128, (1, 2047), False),
          (4096, 2048, 64, (3000, 2192), True)]
SHAPE_IDS = ["%d-%d-nk%d-b%d+%d-%s" % (n, h, nk, b[0], b[1], "cplx" if c else "real") for n, h, nk, b, c in SHAPES]
CASES = [(k, nf) for k in range(len(SHAPES)) for nf in (1, 37)] + [(2, 3000)]
CASE_IDS = ["%s-%dfr" % (SHAPE_IDS[k], nf) for k, nf in CASES]
SEEDS = {}                                          # (shape, frames) -> seed, where a single frame misses the cap with the default
CAP = 0.05
POWERS = ("mean", "cross")


def frames_of(x, nfft, hop, nframes, win, segmean):
    """[nframes, nfft] float64 / complex128: the frames, their own means removed, tapered."""
    x = np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    a = np.lib.stride_tricks.sliding_window_view(x, nfft)[::hop][:nframes].copy()
    assert a.shape == (nframes, nfft)
    if segmean:
        a -= a.mean(axis=1, keepdims=True)
    if win is not None:
        a *= np.asarray(win, dtype=np.float64)
    return a


def band_bins(nfft, b0, nb):
    return (b0 + np.arange(nb)) % nfft


def skf_ref(x, y, nfft, hop, nframes, nk, b0, nb, win=None, segmean=True, power="mean", scale=1.0):
    """The float64 oracle of sp_skf -> (hist, lower, upper, unsure), each table [nb, nk] scaled by scale / nframes; unsure = the
    share of the band's power carried by the samples whose phase interval crosses a bin edge."""
    X = np.fft.fft(frames_of(x, nfft, hop, nframes, win, segmean), axis=1)
    Y = np.fft.fft(frames_of(y, nfft, hop, nframes, win, segmean), axis=1)
    mx, my = np.abs(X).max(axis=1, keepdims=True), np.abs(Y).max(axis=1, keepdims=True)
    bins = band_bins(nfft, b0, nb)
    X, Y = X[:, bins], Y[:, bins]
    th = np.angle(X * np.conj(Y))
    p = 0.5 * (np.abs(X) ** 2 + np.abs(Y) ** 2) if power == "mean" else np.abs(X) * np.abs(Y)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = 4e-6 + 1e-4 * (mx / np.abs(X) + my / np.abs(Y))
    delta = np.where(np.isfinite(delta), delta, 4.0 * math.pi)

    def row(t):
        return np.floor((t / (2 * math.pi) + 0.5) * nk).astype(np.int64)
    j, jlo, jhi = row(th) % nk, row(th - delta), row(th + delta)
    col = np.broadcast_to(np.arange(nb)[None, :], th.shape)
    hist, lower = np.zeros((nb, nk)), np.zeros((nb, nk))
    np.add.at(hist, (col, j), p)
    sure = jlo == jhi
    np.add.at(lower, (col[sure], jlo[sure] % nk), p[sure])
    upper = lower.copy()
    uc, ulo, up = col[~sure], jlo[~sure], p[~sure]
    span = np.minimum(jhi[~sure] - ulo, nk - 1)
    for s in range(int(span.max()) + 1 if span.size else 0):
        m = span >= s
        np.add.at(upper, (uc[m], (ulo[m] + s) % nk), up[m])
    f = scale / nframes
    return hist * f, lower * f, upper * f, float(np.sum(up) / np.sum(p)) if np.sum(p) > 0 else 0.0


def welch_mean_psd(x, y, nfft, hop, nframes, b0, nb, win, segmean, scale):
    """(Pxx + Pyy) / 2 on the band, float64, nothing doubled."""
    bins = band_bins(nfft, b0, nb)
    X = np.fft.fft(frames_of(x, nfft, hop, nframes, win, segmean), axis=1)[:, bins]
    Y = np.fft.fft(frames_of(y, nfft, hop, nframes, win, segmean), axis=1)[:, bins]
    return 0.5 * scale * (np.mean(np.abs(X) ** 2, axis=0) + np.mean(np.abs(Y) ** 2, axis=0))


def hann(n):
    return 0.5 - 0.5 * np.cos(2 * math.pi * np.arange(n) / n)


@functools.lru_cache(maxsize=None)
def shape_case(k, nframes):
    """Inputs, window, scale and the oracle's tables for both powers of shape k at a frame count, computed once and shared."""
    nfft, hop, nk, (b0, nb), cplx = SHAPES[k]
    x, y = make_pair((nframes - 1) * hop + nfft + 3, cplx, SEEDS.get((k, nframes), 11 + k), d=3)
    win = hann(nfft).astype(np.float32)
    scale = 1.0 / float(np.sum(win.astype(np.float64) ** 2))
    ref = {pw: skf_ref(x, y, nfft, hop, nframes, nk, b0, nb, win, True, pw, scale) for pw in POWERS}
    psd = welch_mean_psd(x, y, nfft, hop, nframes, b0, nb, win, True, scale)
    for arr in (x, y, win, psd) + tuple(t for pw in POWERS for t in ref[pw][:3]):
        arr.setflags(write=False)
    return x, y, win, scale, ref, psd


def exact_pair():
    """nfft 64: unit cosines on the odd bins 1 .. 31 with fixed phases, period 64, 8 periods; y[n] = x[n - 1].  Every sample of bin f
    has theta = 2 pi f / 64 exactly, the centre of cell floor(f / 2 + 16) of nk = 32."""
    n = np.arange(8 * 64 + 1)
    f = np.arange(1, 32, 2)
    ph = 0.37 + 1.1 * np.arange(f.size)
    s = np.sum(np.cos(2 * math.pi * f[None, :] * n[:, None] / 64.0 + ph[None, :]), axis=1)
    return _ffi.as_samples(s[1:]), _ffi.as_samples(s[:-1])


def bandlimited_pair(nsig, delay=2.3, seed=21):
    """Noise in 0.02 .. 0.15 cycles per sample; y = x delayed by `delay` samples through a phase ramp, 0.05 of independent noise each."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(nsig)
    Z = np.fft.rfft(rng.standard_normal(nsig)) * ((f >= 0.02) & (f <= 0.15))
    x = np.fft.irfft(Z, nsig)
    y = np.fft.irfft(Z * np.exp(-2j * math.pi * f * delay), nsig)
    amp = x.std()
    return (_ffi.as_samples(x / amp + 0.05 * rng.standard_normal(nsig)), _ffi.as_samples(y / amp + 0.05 * rng.standard_normal(nsig)))


def test_exported():
    for name in ("skf", "skf_moments", "dispersion", "skf_plan"):
        assert getattr(pyfft_amd, name) is getattr(WN, name)
    assert callable(pyfft_amd.engine.skf)


@pytest.mark.parametrize("k,nframes", CASES, ids=CASE_IDS)
def test_oracle_bounds_and_cap(k, nframes):
    nfft, hop, nk, (b0, nb), cplx = SHAPES[k]
    x, y, win, scale, ref, psd = shape_case(k, nframes)
    for pw in POWERS:
        hist, lower, upper, unsure = ref[pw]
        print("%s %s: unsure samples carry %.2f %% of the power" % (CASE_IDS[CASES.index((k, nframes))], pw, 100 * unsure))
        assert unsure <= CAP
        tiny = 1e-12 * hist.max()
        assert np.all(lower <= hist + tiny) and np.all(hist <= upper + tiny) and np.all(lower >= 0)
    np.testing.assert_allclose(ref["mean"][0].sum(axis=1), psd, rtol=1e-12, atol=0)
    # |X| |Y| <= (|X|^2 + |Y|^2) / 2, row by row
    assert np.all(ref["cross"][0].sum(axis=1) <= psd * (1 + 1e-12))


def test_oracle_exact_case():
    x, y = exact_pair()
    hist, lower, upper, unsure = skf_ref(x, y, 64, 64, 8, 32, 0, 33, None, False, "mean", 1.0)
    assert unsure < 1e-6                                   # (the even rows hold rounding noise only)
    top = hist.max()
    for f in range(1, 32, 2):
        j = f // 2 + 16
        assert abs(hist[f, j] - 32.0 ** 2) <= 1e-5 * top and abs(lower[f, j] - hist[f, j]) <= 1e-12 * top
        assert np.all(np.delete(hist[f], j) <= 1e-6 * top)
    # swapping the records mirrors the table
    swapped = skf_ref(y, x, 64, 64, 8, 32, 0, 33, None, False, "mean", 1.0)[0]
    odd = np.arange(1, 32, 2)
    np.testing.assert_allclose(swapped[odd], hist[odd][:, ::-1], rtol=0, atol=1e-6 * top)


def test_moments():
    k = np.array([-1.5, -0.5, 0.5, 1.5])
    S = np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 2.0, 2.0, 0.0], [1.0, 0.0, 0.0, 3.0], [0.0, 0.0, 5.0, 0.0]])
    m = WN.skf_moments(k, S)
    assert set(m) == {"P", "s", "kbar", "sigma_k", "S_k"}
    np.testing.assert_allclose(m["P"], [0.0, 4.0, 4.0, 5.0], atol=0)
    np.testing.assert_allclose(m["s"], [[0, 0, 0, 0], [0, 0.5, 0.5, 0], [0.25, 0, 0, 0.75], [0, 0, 1, 0]], atol=1e-15)
    np.testing.assert_allclose(m["kbar"], [0.0, 0.0, 0.75, 0.5], atol=1e-15)
    np.testing.assert_allclose(m["sigma_k"], [0.0, 0.5, math.sqrt(0.25 * 2.25 ** 2 + 0.75 * 0.75 ** 2), 0.0], atol=1e-15)
    np.testing.assert_allclose(m["S_k"], [1.0, 2.0, 7.0, 3.0], atol=0)
    assert all(np.all(np.isfinite(v)) for v in m.values())
    with pytest.raises(ValueError):
        WN.skf_moments(k[:3], S)


@pytest.mark.parametrize("nk", [65, 64, 33])
def test_oracle_dispersion(nk):
    """kbar of the oracle on the band-limited pair, within a quarter bin of the truth 2 pi f 2.3 (measured 0.11 - 0.20 bins)."""
    nfft, hop, nframes = 256, 100, 500
    x, y = bandlimited_pair((nframes - 1) * hop + nfft)
    hist = skf_ref(x, y, nfft, hop, nframes, nk, 0, nfft // 2 + 1, hann(nfft), True, "mean", 1.0)[0]
    kth = (np.arange(nk) + 0.5 - 0.5 * nk) * (2 * math.pi / nk)                # dx = 1
    f = np.fft.rfftfreq(nfft)
    use = (f >= 0.03) & (f <= 0.15)
    err = np.abs(WN.skf_moments(kth, hist)["kbar"] - 2 * math.pi * f * 2.3)[use] / (2 * math.pi / nk)
    print("nk %d: kbar off by at most %.3f bins" % (nk, err.max()))
    assert err.max() <= 0.25


def test_plan():
    p = WN.skf_plan(256, 65)
    images = 16 * 272 * 8
    assert p == dict(tiles=1, tile_bins=129, lds_bytes=images + 4 * 65 * 160, transforms=1, read=2048, written=0)
    p = WN.skf_plan(256, 65, nb=112, cplx=True)
    assert p == dict(tiles=1, tile_bins=112, lds_bytes=2 * images + 4 * 65 * 128, transforms=2, read=4096, written=0)
    p = WN.skf_plan(4096, 128)
    assert (p["tiles"], p["tile_bins"], p["transforms"], p["read"]) == (10, 224, 10, 10 * 32768) and p["lds_bytes"] <= 160 * 1024
    p = WN.skf_plan(4096, 64, nb=2192, cplx=True)
    assert p["tiles"] == 7 and p["tile_bins"] == 352 and p["transforms"] == 14 and p["lds_bytes"] == 2 * 4112 * 8 + 4 * 64 * 352
    # every shape of the tests: the tile fits, the tiles cover the band, a single tile up to 1024 points but for the full band at nk = 64
    for nfft, _, nk, (_, nb), cplx in SHAPES:
        p = WN.skf_plan(nfft, nk, nb=nb, cplx=cplx)
        assert p["lds_bytes"] <= 160 * 1024 and (p["tiles"] - 1) * p["tile_bins"] < nb <= p["tiles"] * p["tile_bins"]
    assert [WN.skf_plan(n, nk, nb=nb, cplx=c)["tiles"] for n, _, nk, (_, nb), c in SHAPES] == [1, 1, 1, 1, 1, 2, 10, 7]
    # the cap on cells of the tiling tests, and the narrowest LDS: 32 points complex with nk = 1024
    assert WN.skf_plan(256, 64, nb=127, cells=64 * 64)["tiles"] == 2 and WN.skf_plan(1024, 63, nb=300, cells=63 * 48)["tiles"] == 7
    p = WN.skf_plan(32, 1024, cplx=True)
    assert p["tiles"] == 2 and p["tile_bins"] == 16 and p["lds_bytes"] == 160 * 1024
    with pytest.raises(ValueError):
        WN.skf_plan(256, 65, nb=130)
    with pytest.raises(ValueError):
        WN.skf_plan(256, 1)


def test_plan_function_of_the_library():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    fn = ctypes.CDLL(_ffi.LIB_PATH).sp_skf_plan
    fn.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    out = np.zeros(4, dtype=np.int64)
    combos = [(n, nk, nb, c) for n, _, nk, (_, nb), c in SHAPES]
    combos += [(32, 1024, 32, True), (32, 2, 1, False), (4096, 1024, 2049, False), (4096, 1024, 4096, True), (512, 100, 257, False)]
    for n, nk, nb, c in combos:
        assert fn(int(c), n, nb, nk, out.ctypes.data) == 0
        p = WN.skf_plan(n, nk, nb=nb, cplx=c, cells=0)
        assert tuple(out) == (p["tiles"], p["tile_bins"], p["lds_bytes"], p["transforms"]), (n, nk, nb, c)
    for c, n, nb, nk in ((0, 16, 4, 8), (0, 8192, 4, 8), (0, 48, 4, 8), (0, 256, 0, 8), (0, 256, 130, 8), (1, 256, 257, 8), (0, 256, 4, 1),
                         (0, 256, 4, 1025)):
        assert fn(c, n, nb, nk, out.ctypes.data) < 0
    assert fn(0, 256, 4, 8, None) < 0


X600, C600 = np.zeros(600), np.zeros(600, complex)
REFUSALS = [
    (dict(x=np.zeros((2, 300))), "one-dimensional"),
    (dict(y=np.zeros(599)), "equal lengths"),
    (dict(y=C600), "both be real or both be complex"),
    (dict(dx=0.0), "dx must be positive"),
    (dict(dx=-1.0), "dx must be positive"),
    (dict(dx=np.inf), "dx must be positive"),
    (dict(dx=np.nan), "dx must be positive"),
    (dict(fs=0.0), "fs must be positive"),
    (dict(fs=-2.0), "fs must be positive"),
    (dict(nk=1), "nk"),
    (dict(nk=1025), "nk"),
    (dict(band=(30.0, 10.0)), "band"),
    (dict(band=(10.0,)), "band"),
    (dict(band=(10.2, 10.3)), "empty"),
    (dict(band=(10.0, 60.0)), "outside the spectrum"),
    (dict(band=(-5.0, 10.0)), "outside the spectrum"),
    (dict(band=(np.nan, 10.0)), "band"),
    (dict(window=np.ones(255)), "window must be"),
    (dict(window=np.r_[np.nan, np.ones(255)]), "finite"),
    (dict(nperseg=1024), "shorter than a segment"),
    (dict(noverlap=256), "noverlap"),
    (dict(detrend="linear"), "detrend"),
    (dict(power="coherent"), "power must be"),
    (dict(scaling="psd"), "scaling must be"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_before_the_library(no_library, kw, text):
    kw = dict(kw)
    x, y, fs, dx = kw.pop("x", X600), kw.pop("y", X600), kw.pop("fs", 100.0), kw.pop("dx", 0.01)
    for fn in (WN.skf, WN.dispersion):
        with pytest.raises(ValueError) as ei:
            fn(x, y, fs, dx, **kw)
        assert text in str(ei.value)


def test_segment_not_built_is_value_and_not_implemented(no_library):
    x = np.zeros(10000)
    for fn in (WN.skf, WN.dispersion):
        for nperseg in (8192, 300, 16, 4097):
            with pytest.raises(NotImplementedError) as ei:
                fn(x, x, 1.0, 1.0, nperseg=nperseg)
            assert isinstance(ei.value, ValueError) and "power of two from 32 to 4096" in str(ei.value)
    with pytest.raises(NotImplementedError):
        WN.skf_plan(8192, 65)
    # a complex band may run through zero; a real one may not go below it
    with pytest.raises(ValueError):
        WN.skf(x, x, 1.0, 1.0, band=(-0.1, 0.1))


def test_axes_and_band(no_library, monkeypatch):
    """The arguments skf hands to the engine: bins, scale, doubling, the fftshift-ed axis and a band through zero."""
    seen = {}

    def fake(x, y, **kw):
        seen.update(kw)
        return np.ones((kw["nb"], kw["nk"]))
    monkeypatch.setattr(pyfft_amd.engine, "skf", fake)
    f, k, S = WN.skf(X600, X600, 100.0, 0.5, nperseg=64, nk=8)
    w = hann(64)
    assert (seen["b0"], seen["nb"], seen["hop"], seen["nframes"], seen["segmean"], seen["cross"]) == (0, 33, 32, 17, True, False)
    assert np.isclose(seen["scale"], 1.0 / (100.0 * np.sum(w * w))) and np.allclose(seen["win"], w, atol=1e-15)
    np.testing.assert_allclose(f, np.fft.rfftfreq(64, 0.01))
    np.testing.assert_allclose(k, (np.arange(8) - 3.5) * 2 * math.pi / (8 * 0.5))
    assert S.shape == (33, 8) and np.all(S[0] == 1) and np.all(S[32] == 1) and np.all(S[1:32] == 2)
    f, _, S = WN.skf(X600, X600, 100.0, 0.5, nperseg=64, nk=8, band=(10.0, 20.0), scaling="spectrum", detrend=False, power="cross",
                     noverlap=0, window="boxcar")
    assert (seen["b0"], seen["nb"], seen["hop"], seen["nframes"], seen["segmean"], seen["cross"]) == (7, 6, 64, 9, False, True)
    assert np.isclose(seen["scale"], 1.0 / 64.0 ** 2) and f[0] == 7 * 100.0 / 64 and f[-1] == 12 * 100.0 / 64 and np.all(S == 2)
    f, _, S = WN.skf(C600, C600, 64.0, 0.5, nperseg=64, nk=8)
    assert (seen["b0"], seen["nb"]) == (32, 64) and f[0] == -32.0 and f[-1] == 31.0 and np.all(S == 1)
    f, _, S = WN.skf(C600, C600, 64.0, 0.5, nperseg=64, nk=8, band=(-8.0, 5.0))
    assert (seen["b0"], seen["nb"]) == (56, 14) and f[0] == -8.0 and f[-1] == 5.0


def test_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("sp_skf", 16), ("sp_skf_plan", 5)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt, "%s is not declared in include/spectral.h" % name
        nargs = len([a for a in mt.group(1).split(",") if a.strip()])
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs == want
        assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    assert re.search(r"#define SP_SKF_MEAN 0\b", hdr) and re.search(r"#define SP_SKF_CROSS 1\b", hdr)
    assert re.search(r"#define SP_DETREND_NONE 0\b", hdr) and re.search(r"#define SP_DETREND_SEGMEAN 3\b", hdr)
    assert (_ffi.SKF_MEAN, _ffi.SKF_CROSS, _ffi.DETREND_NONE, _ffi.DETREND_SEGMEAN) == (0, 1, 0, 3)
