"""Host side of the batched Hermitian eigensolver and of spectral POD.  No GPU needed.

tests/eigh_ref.py restates the kernel's ordering, scaling, skip rule, stopping rule, sort and phase convention in float64 numpy; here it
is held to numpy.linalg.eigh on every family and order that tests/test_gpu_eigh.py runs on the device, within the one tolerance used
throughout, tol(n) = 4 n 30 eps (Jacobi's backward error is of order n sweeps eps): 1.7e-12 at n = 64, 5.3e-14 at n = 2.  Then the
round-robin schedule, sp_eigh_plan, the declarations and bindings, the refusals that need no device, and spod's conventions (scaling,
doubling, weights, reconstruction, energy) against a numpy oracle with eigh_ref standing in for the device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import pyfft_amd
from pyfft_amd import _ffi, _spod_mod as SP
from pyfft_amd.windows import get_window
from oracle import cpu_ref as O
import eigh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tolerance_is_the_derived_number():
    assert R.tol(64) == 4 * 64 * 30 * np.finfo(np.float64).eps
    assert 1.6e-12 < R.tol(64) < 1.8e-12 and 5.2e-14 < R.tol(2) < 5.4e-14


@pytest.mark.parametrize("NP", [8, 16, 32, 64])
def test_schedule_is_a_tournament(NP):
    steps = R.schedule(NP)
    assert len(steps) == NP - 1
    seen = set()
    for pq in steps:
        assert pq.shape == (NP // 2, 2) and np.all(pq[:, 0] < pq[:, 1])
        assert sorted(pq.ravel().tolist()) == list(range(NP))            # the pairs of a step are disjoint and cover every index
        for p, q in pq.tolist():
            assert (p, q) not in seen
            seen.add((p, q))
    assert len(seen) == NP * (NP - 1) // 2                                # each pair once per sweep


@pytest.mark.parametrize("n", R.ORDERS)
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_reference_against_numpy(family, n):
    rng = np.random.default_rng(1000 + n)
    a = R.FAMILIES[family](rng, 2, n)
    w, V, sw = R.eigh_ref(a)
    assert w.shape == (2, n) and V.shape == (2, n, n) and sw.shape == (2,) and sw.dtype == np.int32
    t = R.tol(n)
    L = R.limits(a, w, V, sw)
    print(family, n, {k: (v / t if k in ("resid", "orth", "eig") else v) for k, v in L.items()})
    assert L["resid"] <= t and L["orth"] <= t and L["eig"] <= t, L
    assert L["descending"] and L["sweeps"] <= 30 and L["phase"] <= 4 * np.finfo(np.float64).eps, L
    if family in ("diagonal", "zero", "identity"):
        assert np.all(sw == 0)
    if family == "real_symmetric":
        assert np.max(np.abs(V.imag)) <= t


def test_reference_reads_the_lower_triangle_only():
    rng = np.random.default_rng(5)
    a = R.fam_csd(rng, 1, 9)[0]
    junk = a.copy()
    iu = np.triu_indices(9, 1)
    junk[iu] = rng.standard_normal(iu[0].size) * 1e6 + 1j
    junk[np.arange(9), np.arange(9)] += 3j
    w0, V0, s0 = R.eigh_ref(a)
    w1, V1, s1 = R.eigh_ref(junk)
    assert np.array_equal(w0, w1) and np.array_equal(V0, V1) and s0 == s1
    np.testing.assert_allclose(w0, np.linalg.eigvalsh(junk)[::-1], atol=R.tol(9) * np.abs(w0).max())      # numpy's UPLO='L' too


def test_reference_nvec_and_nan():
    rng = np.random.default_rng(6)
    a = R.fam_csd(rng, 3, 17)
    w, V, _ = R.eigh_ref(a)
    for nvec in (0, 2):
        w2, V2, _ = R.eigh_ref(a, nvec=nvec)
        assert V2.shape == (3, 17, nvec) and np.array_equal(w, w2) and np.array_equal(V[:, :, :nvec], V2)
    a[1] = np.nan
    w3, V3, sw = R.eigh_ref(a)
    assert sw[1] == 31 and sw[0] <= 30 and sw[2] <= 30
    assert np.array_equal(w3[0], w[0]) and np.array_equal(w3[2], w[2])


def plan(n, nvec, batch):
    out = (ctypes.c_int64 * 4)()
    rc = _ffi.load_library().sp_eigh_plan(n, nvec, batch, out)
    return rc, [int(v) for v in out]


def test_plan_values():
    for n, NP in ((1, 8), (8, 8), (9, 16), (33, 64), (64, 64), (16, 16), (17, 32), (32, 32)):
        for nvec in (0, n):
            rc, (got, lds, per, grid) = plan(n, nvec, 2049)
            assert rc == 0 and got == NP == R.padded_order(n)
            assert 16 * NP * (NP + 1) * (2 if nvec else 1) <= lds <= 163840          # A (and V) at the padded stride, within one CU
            assert 1 <= per <= 163840 // lds and 1 <= grid <= 2049
            assert per * (max(64, NP * NP // 4) // 64) <= 20                         # 5 waves per SIMD by the registers
    # order 64: one workgroup of 1024 threads per CU, with V by the LDS and without it by the registers; smaller orders share a CU
    assert plan(64, 64, 2049)[1][2] == 1 and plan(64, 0, 2049)[1][2] == 1 and plan(32, 32, 2049)[1][2] == 4
    assert plan(32, 0, 2049)[1][2] == 5 and plan(16, 16, 2049)[1][2] == 16
    assert plan(64, 64, 3)[1][3] == 3 and plan(64, 64, 0) == (0, [64, plan(64, 64, 1)[1][1], 1, 0])
    assert SP.spod_plan(64, 3, 2049) == dict(zip(("NP", "lds_bytes", "wg_per_cu", "grid"), plan(64, 3, 2049)[1]))


def test_plan_refusals():
    for n, nvec, batch in ((0, 0, 1), (65, 0, 1), (-1, 0, 1), (8, 9, 1), (8, -1, 1), (8, 8, -1)):
        assert plan(n, nvec, batch)[0] < 0
    assert _ffi.load_library().sp_eigh_plan(8, 8, 1, None) < 0
    with pytest.raises(NotImplementedError) as ei:
        SP.spod_plan(65)
    assert isinstance(ei.value, ValueError)
    with pytest.raises(ValueError):
        SP.spod_plan(8, 9)


def test_c_refusals_need_no_device():
    """Every refusal of sp_eigh comes before the device is touched, names sp_eigh, and batch == 0 succeeds touching nothing."""
    lib = _ffi.load_library()
    a = np.zeros((1, 4, 4), dtype=np.complex128)
    w, v, sw = np.zeros((1, 4)), np.zeros((1, 4, 4), dtype=np.complex128), np.zeros(1, dtype=np.int32)
    P = _ffi.ptr
    for args, text in (((P(a), 0, 1, 0, 30, P(w), P(v), P(sw), 0), "n = 0 outside 1 .. 64"),
                       ((P(a), 65, 1, 0, 30, P(w), P(v), P(sw), 0), "n = 65 outside 1 .. 64"),
                       ((P(a), 4, 1, 5, 30, P(w), P(v), P(sw), 0), "nvec = 5 outside 0 .. n = 4"),
                       ((P(a), 4, 1, -1, 30, P(w), P(v), P(sw), 0), "nvec = -1 outside"),
                       ((P(a), 4, -1, 4, 30, P(w), P(v), P(sw), 0), "batch = -1 must not be negative"),
                       ((P(a), 4, 1, 4, 0, P(w), P(v), P(sw), 0), "max_sweeps = 0 must be at least 1"),
                       ((None, 4, 1, 4, 30, P(w), P(v), P(sw), 0), "a, w and sweeps are required"),
                       ((P(a), 4, 1, 4, 30, None, P(v), P(sw), 0), "a, w and sweeps are required"),
                       ((P(a), 4, 1, 4, 30, P(w), P(v), None, 0), "a, w and sweeps are required"),
                       ((P(a), 4, 1, 4, 30, P(w), None, P(sw), 0), "v is required for nvec = 4")):
        assert lib.sp_eigh(*args) < 0
        msg = lib.sp_last_error().decode()
        assert msg.startswith("sp_eigh:") and text in msg, msg
    w[:] = 7.0
    assert lib.sp_eigh(None, 4, 0, 4, 30, None, None, None, 0) == 0 and np.all(w == 7.0)


def test_python_refusals_need_no_device():
    E = pyfft_amd.engine
    with pytest.raises(NotImplementedError) as ei:
        E.eigh(np.zeros((2, 65, 65)))
    assert isinstance(ei.value, ValueError) and "65" in str(ei.value)
    for bad, kw in ((np.zeros((3, 4)), {}), (np.zeros(4), {}), (np.zeros((4, 4)), dict(nvec=5)), (np.zeros((4, 4)), dict(nvec=-1)),
                    (np.zeros((4, 4)), dict(max_sweeps=0))):
        with pytest.raises(ValueError):
            E.eigh(bad, **kw)
    with pytest.raises(NotImplementedError) as ei:
        SP.spod(np.zeros((70, 1000)), nperseg=64)
    assert isinstance(ei.value, ValueError) and "70" in str(ei.value)
    for kw in (dict(nperseg=64, noverlap=64), dict(nperseg=2000), dict(nperseg=64, nmodes=0), dict(nperseg=64, nmodes=9),
               dict(nperseg=64, weights=np.ones(7)), dict(nperseg=64, weights=-np.ones(8)), dict(nperseg=64, fs=0.0),
               dict(nperseg=64, window=np.ones(63))):
        with pytest.raises(ValueError):
            SP.spod(np.zeros((8, 1000)), **kw)


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("sp_eigh", 9), ("sp_eigh_plan", 4)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt, "%s is not declared in include/spectral.h" % name
        nargs = len([a for a in mt.group(1).split(",") if a.strip()])
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs == want
        assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    for name in ("spod", "spod_energy", "spod_reconstruct", "spod_plan"):
        assert getattr(pyfft_amd, name) is getattr(SP, name)


# ---- spod's conventions against a numpy oracle, eigh_ref standing in for the device --------------------------------------------
def spod_input(nch, nfft, hop, frames):
    """x_c = (1 + 0.1 (c mod 10)) roll(common, c mod 5) + noise + 0.1 c, unit white common and noise."""
    rng = np.random.default_rng(nch * nfft)
    nsig = (frames - 1) * hop + nfft
    common = rng.standard_normal(nsig)
    return np.stack([(1 + 0.1 * (c % 10)) * np.roll(common, c % 5) + rng.standard_normal(nsig) + 0.1 * c
                     for c in range(nch)]).astype(np.float32)


def spod_oracle(x, fs, win, nfft, hop, weights=None, doubling=True):
    """(G, lam, phi) in float64: oracle.cpu_ref.csd_matrix as a density, interior bins doubled, numpy.linalg.eigh of W^1/2 G W^1/2."""
    frames = (x.shape[1] - nfft) // hop + 1
    G = O.csd_matrix(x.astype(np.float64), win, nfft, hop, frames, fs)
    if doubling:
        G[1:(nfft - 1) // 2 + 1] *= 2.0
    rw = np.ones(x.shape[0]) if weights is None else np.sqrt(np.asarray(weights, dtype=np.float64))
    lam, v = np.linalg.eigh(G * rw[None, :, None] * rw[None, None, :])
    return G, lam[:, ::-1], v[:, :, ::-1] / rw[None, :, None]


@pytest.fixture
def host_spod(monkeypatch):
    """engine.csd_matrix and engine.eigh replaced by their float64 restatements: spod's own arithmetic is what remains."""
    def csd(x, win, hop, nframes, detrend=True, scale=1.0, means=None):
        win = np.asarray(win, dtype=np.float64)
        return O.csd_matrix(np.asarray(x, dtype=np.float64), win, win.size, hop, nframes, 1.0, 1 if detrend else 0) * np.sum(win ** 2) * scale

    def eigh(A, nvec=None, max_sweeps=30, check=True):
        return R.eigh_ref(A, nvec=nvec, max_sweeps=max_sweeps)
    monkeypatch.setattr(pyfft_amd.engine, "csd_matrix", csd)
    monkeypatch.setattr(pyfft_amd.engine, "eigh", eigh)


def aligned(phi, ref):
    """|phi_m^H ref_m| per bin and mode (1 for the same mode up to a phase)."""
    return np.abs(np.sum(np.conj(phi) * ref, axis=1))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("doubling", [True, False])
def test_spod_conventions(host_spod, doubling, weighted):
    nch, nfft, hop, frames, fs = 5, 32, 16, 40, 250.0
    x = spod_input(nch, nfft, hop, frames)
    wts = 0.5 + np.arange(nch) if weighted else None
    win = np.asarray(get_window("hann", nfft), dtype=np.float64)
    G0, lam0, phi0 = spod_oracle(x, fs, win, nfft, hop, wts, doubling)
    f, lam, phi, G = SP.spod(x, fs=fs, nperseg=nfft, weights=wts, onesided_doubling=doubling, return_csd=True)
    t = R.tol(nch)
    np.testing.assert_allclose(f, np.fft.rfftfreq(nfft, 1 / fs))
    assert lam.shape == (nfft // 2 + 1, nch) and phi.shape == (nfft // 2 + 1, nch, nch)
    scale = np.abs(G0).max()
    assert np.max(np.abs(G - G0)) <= 1e-13 * scale                       # the density scaling and the doubling
    assert np.max(np.abs(lam - lam0)) <= t * np.abs(lam0).max() and np.all(np.diff(lam, axis=1) <= 0)
    assert np.min(aligned(phi[:, :, :1] * (1 if wts is None else wts[None, :, None]), phi0[:, :, :1])) >= 1 - 1e-9
    W = np.ones(nch) if wts is None else wts
    gram = np.einsum("kcm,c,kcn->kmn", np.conj(phi), W, phi)
    assert np.max(np.abs(gram - np.eye(nch)[None])) <= t                  # phi^H W phi = 1
    herm = 0.5 * (G0 + np.conj(np.swapaxes(G0, 1, 2)))
    assert np.max(np.abs(SP.spod_reconstruct(lam, phi, wts) - herm)) <= 2 * t * scale
    e = SP.spod_energy(lam)
    assert np.max(np.abs(e.sum(axis=1) - 1)) <= 1e-14 and np.all(e[:, 0] >= e[:, 1])
    # the leading modes alone, and their share of the trace
    f3, lam3, phi3 = SP.spod(x, fs=fs, nperseg=nfft, weights=wts, onesided_doubling=doubling, nmodes=3)
    assert lam3.shape[1] == 3 and phi3.shape[2] == 3 and np.array_equal(lam3, lam[:, :3]) and np.array_equal(phi3, phi[:, :, :3])
    np.testing.assert_allclose(SP.spod_energy(lam3, trace=lam.sum(axis=1)), e[:, :3], rtol=1e-14)


def test_spod_detrend_is_the_whole_record_mean(host_spod):
    x = spod_input(3, 32, 16, 20)
    win = np.asarray(get_window("hann", 32), dtype=np.float64)
    _, lam, _ = SP.spod(x, nperseg=32)
    _, lam_off, _ = SP.spod(x + 5.0, nperseg=32)
    np.testing.assert_allclose(lam_off, lam, rtol=1e-5, atol=1e-9)         # a constant offset is removed (float32 record)
    _, lam_raw, _ = SP.spod(x, nperseg=32, detrend=False)
    G = O.csd_matrix(x.astype(np.float64), win, 32, 16, 20, 1.0, 0)
    np.testing.assert_allclose(lam_raw[0], np.linalg.eigvalsh(G[0])[::-1], atol=R.tol(3) * np.abs(G[0]).max())
