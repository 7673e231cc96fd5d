"""The FFT accumulation method without a GPU: the float64 reference of tests/fam_ref.py (the demodulation as a shift, block additivity, the
Welch estimate on the diagonal, the cycle frequency of amplitude-modulated noise), the float32 restatement behind the allowance, the
geometry of the pair table, the plan arithmetic of sp_fam_plan, the refusals of the C entries and of the Python fronts, and the declared
set of include/spectral_fam.h."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import fam_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, fam as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_float32_restatement_deviation():
    """fam_def32 against fam_def over the GPU shapes: the figure behind F32_DEV"""
    worst = {}
    for name in R.SHAPES:
        worst[name] = R.deviation(R.reference32(name), R.reference(name), R.pairs_of(name))
        print("%s: float32 restatement deviates by %.3e" % (name, worst[name]))
    top = max(worst.values())
    print("largest deviation %.3e against F32_DEV = %.3e; the kernel's allowance %.3e" % (top, R.F32_DEV, R.ALLOWANCE))
    assert top <= R.F32_DEV and R.F32_DEV <= 1.5 * top          # the constant is the measurement, rounded up
    assert R.ALLOWANCE == 4 * R.F32_DEV and R.ALLOWANCE < R.PARITY


def _small(cplx=False, nblocks=3, seed=5):
    rng = np.random.default_rng(seed)
    n, hop, P = 32, 8, 64
    x = R.CR.am_noise(rng, (nblocks * P - 1) * hop + n, cplx)
    return x, R.hamming(n), hop, R.hamming(P), nblocks, R.all_pairs(n)


@pytest.mark.parametrize("cplx,conj", [(False, False), (True, False), (True, True)])
def test_the_demodulation_is_a_shift(cplx, conj):
    x, a, hop, g, nb, pairs = _small(cplx)
    y = np.roll(x, 3) if cplx else None
    ref = R.fam_def(x, a, hop, g, nb, pairs, y, conj, 0.1)
    got = R.fam_def(x, a, hop, g, nb, pairs, y, conj, 0.1, shift=True)
    dev = R.deviation(got, ref, pairs)
    print("shift against demodulation: %.2e" % dev)
    assert dev <= 1e-12


def test_block_additivity_is_exact():
    x, a, hop, g, nb, pairs = _small()
    P = g.size
    whole = R.fam_def(x, a, hop, g, nb, pairs, shift=True)
    parts = [R.fam_def(x[b * P * hop:], a, hop, g, 1, pairs, shift=True) for b in range(nb)]
    # the un-normalised parts add up in the order of the whole's own sum: exactly
    for i in range(3):
        acc = parts[0][i].copy()
        for p in parts[1:]:
            acc = acc + p[i]
        if i == 0:
            assert np.array_equal(acc, whole[i])                   # S: the difference is exactly 0
        else:
            np.testing.assert_allclose(acc, whole[i], rtol=1e-13)    # the powers are one sum over all frames in the whole
    # and with the demodulation written out, to rounding
    whole_d = R.fam_def(x, a, hop, g, nb, pairs)
    parts_d = sum(R.fam_def(x[b * P * hop:], a, hop, g, 1, pairs)[0] for b in range(nb))
    assert np.max(np.abs(parts_d - whole_d[0])) <= 1e-12 * np.max(np.abs(whole_d[0]))


def test_diagonal_at_q0_is_the_welch_estimate():
    x, a, hop, _, nb, _ = _small()
    n, P = a.size, 64
    nframes = nb * P
    diag = np.stack([np.arange(n), np.arange(n)], axis=1)
    scale = 1.0 / (np.sum(a ** 2) * nframes)
    S, Pwx, _ = R.fam_def(x, a, hop, np.ones(P), nb, diag, scale=scale)
    used = x[:(nframes - 1) * hop + n].astype(np.float64)
    _, pxx = ss.welch(used, 1.0, window=a, nperseg=n, noverlap=n - hop, detrend=False, return_onesided=False, scaling="density")
    Q = P * hop // (2 * n)
    np.testing.assert_allclose(S[:, Q].real, pxx, rtol=1e-12)
    np.testing.assert_allclose(Pwx, pxx, rtol=1e-12)
    assert np.max(np.abs(S[:, Q].imag)) <= 1e-15 * pxx.max()


@pytest.fixture(scope="module")
def am_plane():
    """the plane of the amplitude-modulated record from the float64 reference, as scd_fam lays it out"""
    x = R.am_record()
    a, g = R.hamming(R.AM["np"]), R.hamming(R.AM["P"])
    assert R.tile_offset_loss(a, R.NU_AM - 1 / 32) > 0.96 > 0.89 > R.tile_offset_loss(R.hamming(64), R.NU_AM - 2 / 64)
    assert R.tile_offset_loss(ss.get_window(R.AM_GPU["window"], 64), R.NU_AM - 2 / 64) > 0.96
    pairs = F.fam_pairs(R.AM["np"], real=True)
    S, Pwx, Pwy = R.fam_def(x, a, R.AM["hop"], g, R.AM["nblocks"], pairs, mx=R.CR.row_mean(x))
    Q = R.AM["P"] * R.AM["hop"] // (2 * R.AM["np"])
    f, alpha = F.fam_axes(pairs, R.AM["np"], Q)
    return F.FamPlane(pairs, f, alpha, S, np.stack([Pwx, Pwy]), 1.0 / (R.AM["P"] * R.AM["hop"]))


def test_profile_of_am_noise_peaks_at_the_modulation_rate(am_plane):
    alphas, prof = F.fam_profile(am_plane)
    assert np.all(np.diff(alphas) > 0) and not np.any(alphas == 0) and prof.shape == alphas.shape
    R.assert_am_profile(alphas, prof)
    amax, pmax = F.fam_profile(am_plane, "max")
    assert np.array_equal(amax, alphas) and np.all(pmax >= prof - 1e-15)
    gam = F.fam_coherence(am_plane)
    assert gam.dtype == np.complex128 and np.max(np.abs(gam)) <= 1 + 1e-9
    f, al, S = F.fam_cells(am_plane)
    assert f.shape == al.shape == S.shape == (am_plane.S.size,) and f[0] == am_plane.f[0] and al[1] == am_plane.alpha[0, 1]


# ---- the pair table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conj", [False, True])
def test_pair_tiles_cover_the_alpha_axis_once(conj):
    """Per f row no alpha bin is met twice; the tiles of one diagonal (k - l, or k + l in the conjugate form) are one strip of 2Q bins,
    the strips of neighbouring diagonals abut, and over all diagonals every alpha bin of (-1, 1) is covered exactly once per pair of
    neighbouring f rows (a row holds the diagonals of its own parity)."""
    n, hop, P = 32, 8, 64
    Q = P * hop // (2 * n)
    pairs = F.fam_pairs(n, conjugate=conj)
    assert pairs.shape == (n * n, 2) and pairs.dtype == np.int32 and np.all(np.diff(pairs[:, 0]) >= 0)
    f, alpha = F.fam_axes(pairs, n, Q, conjugate=conj)
    dalpha = 1.0 / (P * hop)
    bins = np.rint(alpha / dalpha).astype(int)
    rows = np.rint(f * 2 * n).astype(int)
    for r in np.unique(rows):
        b = bins[rows == r].ravel()
        assert np.unique(b).size == b.size                       # once per f row
    strips = {}
    for r, b in zip(rows, bins):
        strips.setdefault(b[Q] // (2 * Q), set()).add((r, tuple(b)))
    # the signed channels run over -n/2 .. n/2 - 1: their differences over -(n - 1) .. n - 1, their sums over -n .. n - 2
    dlo, dhi = (-n, n - 2) if conj else (-(n - 1), n - 1)
    for d, cells in strips.items():
        assert len(cells) == n - abs(d + 1 if conj else d)       # the pairs of a diagonal lie in different f rows, on one strip
        assert all(t == tuple(range(d * 2 * Q - Q, d * 2 * Q + Q)) for _, t in cells)
        assert all((r - d) % 2 == 0 for r, _ in cells)
    assert sorted(strips) == list(range(dlo, dhi + 1))
    lo, hi = dlo * 2 * Q - Q, dhi * 2 * Q + Q
    assert np.isclose(lo * dalpha, dlo / n - 0.5 / n) and np.isclose(hi * dalpha, dhi / n + 0.5 / n)
    every = np.sort(np.concatenate([np.array(next(iter(c))[1]) for c in strips.values()]))
    assert np.array_equal(every, np.arange(lo, hi))


def test_real_pairs_are_a_quarter_and_bands_select():
    n = 64
    q = F.fam_pairs(n, real=True)
    assert q.shape[0] == n * n // 4
    f, alpha = F.fam_axes(q, n, 4)
    assert np.all(f >= 0) and np.all(alpha[:, 4] >= 0)
    # pair (k, l) repeats pair (-l, -k): the quarter and its mirror image and the two axes make up the whole
    b = F.fam_pairs(n, alpha_band=(0.1, 0.2), f_band=(0.0, 0.25), real=True)
    fb, ab = F.fam_axes(b, n, 4)
    half = 0.5 / n
    assert 0 < b.shape[0] < q.shape[0] and np.all(ab[:, 4] + half > 0.1) and np.all(ab[:, 4] - half <= 0.2) and np.all(fb - half <= 0.25)
    inside = (alpha[:, 4] >= 0.1) & (alpha[:, 4] <= 0.2) & (f <= 0.25)
    assert set(map(tuple, q[inside])) <= set(map(tuple, b))
    for bad in (lambda: F.fam_pairs(48), lambda: F.fam_pairs(16), lambda: F.fam_pairs(64, alpha_band=(0.3, 0.2)),
                lambda: F.fam_pairs(64, alpha_band=(2.0, 3.0))):
        with pytest.raises(E.FamRefused):
            bad()


# ---- the C entries ----------------------------------------------------------------------------------------------------------------
SENT = np.float32(-7.5)
GOOD = dict(dtype=0, nsig=(2 * 32 - 1) * 8 + 32, np=32, hop=8, P=32, nblocks=2, npairs=4, conj=0, scale=1.0, x=True, y=False, a=True, g=True,
            pairs=True, S=True, Pwx=True, Pwy=True, mx=None, my=None, pair0=(0, 0))


def _call(**over):
    p = dict(GOOD, **over)
    lib = _ffi.load_library()
    n = max(int(p["nsig"]), 1)
    x = np.ones(n, dtype=np.complex64 if p["dtype"] == 1 else np.float32)
    y = x.copy()
    a, g = np.ones(max(p["np"], 1), dtype=np.float32), np.ones(max(p["P"], 1), dtype=np.float32)
    pairs = np.zeros((max(int(p["npairs"]), 1), 2), dtype=np.int32)
    pairs[0] = p["pair0"]
    outs = [np.full(1 << 12, SENT, dtype=np.complex64), np.full(1 << 13, SENT), np.full(1 << 13, SENT)]
    m = lambda v: None if v is None else _ffi.ptr(np.array(v, dtype=np.float64))
    rc = lib.sp_fam(_ffi.ptr(x) if p["x"] else None, _ffi.ptr(y) if p["y"] else None, p["dtype"], p["nsig"], _ffi.ptr(a) if p["a"] else None,
                    p["np"], p["hop"], _ffi.ptr(g) if p["g"] else None, p["P"], p["nblocks"], _ffi.ptr(pairs) if p["pairs"] else None, p["npairs"],
                    p["conj"], m(p["mx"]), m(p["my"]), p["scale"], *(_ffi.ptr(o) if p[k] else None for o, k in zip(outs, ("S", "Pwx", "Pwy"))), 0)
    return rc, lib.sp_last_error().decode(), outs


REFUSALS = [(dict(np=48), "np"), (dict(np=16), "np"), (dict(np=16384), "np"), (dict(P=16), "P must"), (dict(P=48), "P must"),
            (dict(P=16384), "P must"), (dict(hop=0), "hop"), (dict(hop=6), "hop"), (dict(hop=64), "hop"), (dict(hop=1), "P hop"),
            (dict(nblocks=-1), "nblocks"), (dict(nblocks=3), "nsig"), (dict(nsig=535), "nsig"), (dict(nsig=10), "nsig"), (dict(npairs=0), "npairs"),
            (dict(npairs=(1 << 22) + 1), "npairs"), (dict(pair0=(0, 32)), "pairs"), (dict(pair0=(-1, 0)), "pairs"), (dict(dtype=2), "dtype"),
            (dict(dtype=-1), "dtype"), (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"), (dict(mx=(np.nan, 0.0)), "mean"),
            (dict(y=True, my=(0.0, np.inf)), "mean"), (dict(x=False), "x is"), (dict(a=False), "a is"), (dict(g=False), "g is"),
            (dict(pairs=False), "pairs is"), (dict(S=False, Pwx=False, Pwy=False), "output")]
PLAN_KEYS = {"np", "P", "hop", "nblocks", "npairs", "dtype"}


@pytest.mark.parametrize("over,word", REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(REFUSALS)])
def test_c_refusals(over, word):
    """every refusal: < 0, the message starts with the entry's name and names the argument, the outputs untouched; no device is needed,
    because a refusal comes before the device is touched"""
    rc, msg, outs = _call(**over)
    assert rc < 0 and msg.startswith("sp_fam: ") and word in msg, (rc, msg)
    assert all(np.all(o == SENT) for o in outs)
    p = dict(GOOD, **over)
    if set(over) <= PLAN_KEYS and "nsig" not in word:           # what the plan judges as well
        out = np.full(5, -3, dtype=np.int64)
        assert _ffi.load_library().sp_fam_plan(p["dtype"], 0, p["np"], p["hop"], p["P"], p["nblocks"], p["npairs"], _ffi.ptr(out)) < 0
        assert np.all(out == -3)


def test_no_blocks_is_no_work():
    rc, msg, outs = _call(nblocks=0)
    assert rc == 0 and all(np.all(o == SENT) for o in outs)
    out = np.zeros(5, dtype=np.int64)
    assert _ffi.load_library().sp_fam_plan(0, 0, 32, 8, 32, 0, 4, _ffi.ptr(out)) == 0 and list(out) == [4, 0, 0, 0, 0]
    assert _ffi.load_library().sp_fam_plan(0, 0, 32, 8, 32, 1, 4, None) < 0


def _plan_restated(cross, n, hop, P, nblocks, npairs, cap=0):
    fpw = max(256 // (P // 16), 1)
    bpp = max(1, (256 << 20) // (8 * (2 if cross else 1) * n * P))
    if 0 < cap < bpp:
        bpp = cap
    bpp = min(bpp, nblocks)
    passes = -(-nblocks // bpp)
    return dict(Q=P * hop // (2 * n), blocks_per_pass=bpp, passes=passes, workgroups=passes * -(-npairs // fpw),
                scratch=8 * (2 if cross else 1) * n * P * bpp)


@pytest.mark.parametrize("cross,n,hop,P,nblocks,npairs,cap", [(False, 32, 8, 32, 3, 1024, 0), (False, 32, 8, 32, 7, 1024, 3), (True, 256, 64, 8192, 40, 16384, 0),
                                                             (False, 256, 64, 8192, 2, 16384, 0), (True, 8192, 8192, 8192, 3, 5, 0),
                                                             (False, 64, 16, 2048, 1, 1, 0), (False, 64, 4, 32, 2, 4096, 5)])
def test_plan_against_its_arithmetic(cross, n, hop, P, nblocks, npairs, cap, monkeypatch):
    if cap:
        monkeypatch.setenv("SP_FAM_BLOCKS", str(cap))
    else:
        monkeypatch.delenv("SP_FAM_BLOCKS", raising=False)
    assert E.fam_plan(n, hop, P, nblocks, npairs, cross=cross) == _plan_restated(cross, n, hop, P, nblocks, npairs, cap)


def test_many_passes_of_many_cells_are_refused(monkeypatch):
    monkeypatch.setenv("SP_FAM_BLOCKS", "1")
    rc, msg, outs = _call(np=32, hop=32, P=8192, nblocks=2, nsig=(2 * 8192 - 1) * 32 + 32, npairs=1 << 15)
    assert rc < 0 and msg.startswith("sp_fam: ") and "2 GiB" in msg and all(np.all(o == SENT) for o in outs)
    with pytest.raises(E.FamRefused):
        E.fam_plan(32, 32, 8192, 2, 1 << 15)


# ---- the Python fronts ------------------------------------------------------------------------------------------------------------
def _both(exc):
    return isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(E, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    x = np.ones((2 * 32 - 1) * 8 + 32, dtype=np.float32)
    ok = dict(a=np.ones(32), hop=8, g=np.ones(32), nblocks=2, pairs=[[0, 0], [1, 2]], detrend=False)
    call = lambda v=x, **over: (lambda: E.fam(v, **dict(ok, **over)))
    bad = [call(a=np.ones(48)), call(a=np.ones(16)), call(g=np.ones(16)), call(g=np.ones(48)), call(hop=0), call(hop=6), call(hop=64), call(hop=1),
           call(nblocks=-1), call(nblocks=3), call(x[:-1]), call(pairs=np.zeros((0, 2))), call(pairs=[[0, 32]]), call(pairs=[[-1, 0]]),
           call(pairs=[0, 1, 2]), call(scale=float("nan")), call(S=False, Pw=False), call(np.ones((2, x.size), dtype=np.float32)),
           call(a=np.where(np.arange(32) == 3, np.nan, 1.0)), call(y=x[:-1]), call(y=x.astype(np.complex64)), call(detrend=True, mean_value=np.inf),
           lambda: E.fam_plan(48, 8, 32, 1, 1), lambda: E.fam_plan(32, 8, 32, 1, 0), lambda: E.fam_plan(32, 1, 32, 1, 1),
           lambda: E.fam_plan(32, 8, 32, -1, 1), lambda: F.scd_fam(x, nchan=48), lambda: F.scd_fam(x, fs=0.0), lambda: F.scd_fam(x[:100], nchan=64),
           lambda: F.scd_fam(x, nchan=32, nblock=48), lambda: F.scd_fam(x, nchan=32, nblock=128), lambda: F.scd_fam(x, nchan=32, hop=3),
           lambda: F.scd_fam(x, nchan=32, detrend="linear"), lambda: F.scd_fam(x, nchan=32, scaling="psd"),
           lambda: F.scd_fam(np.ones((2, x.size), dtype=np.float32), nchan=32), lambda: F.scd_fam(x, nchan=32, window=np.zeros(32)),
           lambda: F.scd_fam(x, nchan=32, alpha_band=(3.0, 4.0)), lambda: F.fam_plan(100, nchan=64),
           lambda: F.fam_profile(F.FamPlane(None, None, None, None, None, 1.0), "median")]
    for i, fn in enumerate(bad):
        with pytest.raises(E.FamRefused) as exc:
            fn()
        assert _both(exc), i
        assert str(exc.value).split(":")[0] in ("fam", "fam_plan", "scd_fam", "fam_pairs", "fam_profile"), str(exc.value)
    # a sum over no blocks needs no library either
    S, Pwx, Pwy = E.fam(x, **dict(ok, nblocks=0))
    assert S.shape == (2, 8) and not S.any() and Pwx.shape == Pwy.shape == (32,) and not Pwx.any()
    assert F.FamRefused is E.FamRefused


def test_scd_fam_defaults_through_the_plan():
    d = F.fam_plan(1 << 20, nchan=256)
    assert (d["hop"], d["nblock"], d["nblocks"], d["Q"], d["npairs"]) == (64, 8192, 1, 1024, 256 * 256 // 4)
    assert d["dalpha"] == 1.0 / (8192 * 64) and d["passes"] == 1 and d["scratch"] == 8 * 256 * 8192
    d = F.fam_plan(1 << 20, fs=2.0, nchan=256, cplx=True, alpha_band=(0.0, 0.1))
    assert d["npairs"] < 256 * 256 // 8


def test_exported_declared_and_bound():
    for name in ("FamPlane", "fam_pairs", "fam_axes", "scd_fam", "fam_coherence", "fam_profile", "fam_cells", "fam_plan"):
        assert getattr(pyfft_amd, name) is getattr(F, name)
    for name in ("fam", "fam_plan", "fam_check", "FamRefused"):
        assert hasattr(E, name)
    assert issubclass(E.FamRefused, ValueError) and issubclass(E.FamRefused, NotImplementedError)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    hdr = strip("spectral_fam.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.FAM_SIGNATURES) == {"sp_fam", "sp_fam_plan"}
    assert len(_ffi.TABLES) == 6 and _ffi.FAM_SIGNATURES in _ffi.MORE_TABLES and all(t is not _ffi.FAM_SIGNATURES for t in _ffi.TABLES)
    for table in _ffi.TABLES + tuple(t for t in _ffi.MORE_TABLES if t is not _ffi.FAM_SIGNATURES):
        assert not set(_ffi.FAM_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_fam", 20), ("sp_fam_plan", 8)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.FAM_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.FAM_SIGNATURES[name][1]
    for other in ("spectral.h", "spectral_ext.h", "spectral_tfr.h", "spectral_quad.h", "spectral_cyclo.h", "spectral_uneven.h", "spectral_wbic.h"):
        assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other)))
    assert "spectral_fam.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert "SP_FAM_BLOCKS" in open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert _ffi.load_library().sp_last_passes(5) == 0
