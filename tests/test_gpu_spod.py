"""Spectral POD (pyfft_amd.spod) on the MI355X: the CSD matrix and its eigendecomposition, both on the device.

lam and phi are held (a) to numpy.linalg.eigh of the device's own matrix G (return_csd=True) at the eigensolver's tolerance
tol(n) = 4 n 30 eps, and (b) to the float64 oracle (oracle.cpu_ref.csd_matrix + numpy.linalg.eigh) with no new number: by Weyl
max|lam_dev - lam_ref| <= ||G_dev - G_ref||_2 + tol ||G_ref||_2 per bin, and by Davis-Kahan the angle between the leading modes obeys
sqrt(1 - |phi_dev^H phi_ref|^2) <= 2 ||G_dev - G_ref||_2 / gap + tol, gap = lam_1 - lam_2 of the oracle.  G itself is held to the oracle by
tests/test_gpu_kernels.py::test_csd_matrix.  The inputs have a leading gap of at least 0.71 lam_1 at every bin (checked on the oracle
alone); the tests assert gap >= 0.5 lam_1 as their precondition."""
import numpy as np
import pytest

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _spod_mod as SP                             # noqa: E402
from pyfft_amd.windows import get_window                          # noqa: E402
import eigh_ref as R                                              # noqa: E402
from test_host_eigh import spod_input, spod_oracle                # noqa: E402

SHAPES = [(8, 64, 32, 100), (5, 32, 16, 40), (64, 64, 32, 200), (33, 128, 64, 150)]
FS = 250.0
_cache = {}


def case(k, weighted=False):
    """The input, the oracle's (G, lam, phi) and the weights of shape k, computed once."""
    key = (k, weighted)
    if key not in _cache:
        nch, nfft, hop, frames = SHAPES[k]
        x = spod_input(nch, nfft, hop, frames)
        wts = 0.5 + 0.25 * (np.arange(nch) % 7) if weighted else None
        win = np.asarray(get_window("hann", nfft), dtype=np.float64)
        _cache[key] = (x, wts) + spod_oracle(x, FS, win, nfft, hop, wts)
        for a in _cache[key]:
            if a is not None:
                a.setflags(write=False)
    return _cache[key]


def spec2(A):
    return np.linalg.norm(A, ord=2, axis=(1, 2))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_spod_against_its_own_matrix_and_the_oracle(k, weighted):
    nch, nfft, hop, frames = SHAPES[k]
    x, wts, G0, lam0, phi0 = case(k, weighted)
    t = R.tol(nch)
    gap = lam0[:, 0] - lam0[:, 1]
    assert np.all(gap >= 0.5 * lam0[:, 0])                                   # the precondition of the Davis-Kahan bound
    f, lam, phi, G = SP.spod(x, fs=FS, nperseg=nfft, noverlap=nfft - hop, weights=wts, return_csd=True)
    nb = nfft // 2 + 1
    assert lam.shape == (nb, nch) and phi.shape == (nb, nch, nch) and G.shape == (nb, nch, nch)
    np.testing.assert_allclose(f, np.fft.rfftfreq(nfft, 1 / FS))
    rw = np.ones(nch) if wts is None else np.sqrt(wts)
    scale = lambda A: A * rw[None, :, None] * rw[None, None, :]             # noqa: E731
    # (a) the decomposition of the device's own matrix
    L = R.limits(scale(G), lam, phi * rw[None, :, None], np.zeros(nb, dtype=np.int32))
    print("shape %s weighted %s: own matrix resid %.3g tol, orth %.3g tol, eig %.3g tol" % (SHAPES[k], weighted, L["resid"] / t,
                                                                                       L["orth"] / t, L["eig"] / t))
    assert L["resid"] <= t and L["orth"] <= t and L["eig"] <= t and L["descending"] and L["phase"] <= 4 * np.finfo(float).eps, L
    # (b) the oracle: Weyl and Davis-Kahan with the distance of the two matrices, no new number
    H = R.hermitian_from_lower(scale(G))
    H0 = scale(G0)
    dG, n0 = spec2(H - H0), spec2(H0)
    weyl = np.max(np.abs(lam - lam0), axis=1)
    print("   against the oracle: ||dG||/||G|| %.3g, Weyl used %.3g of its bound" % (np.max(dG / n0), np.max(weyl / (dG + t * n0))))
    assert np.all(weyl <= dG + t * n0)
    u, v = (phi0[:, :, 0] * rw[None, :]), (phi[:, :, 0] * rw[None, :])          # unit vectors; the sine without the cancellation of
    sine = np.linalg.norm(v - u * np.sum(np.conj(u) * v, axis=1)[:, None], axis=1)   # sqrt(1 - c^2): what of v lies outside u
    print("   Davis-Kahan used %.3g of its bound" % np.max(sine / (2 * dG / gap + t)))
    assert np.all(sine <= 2 * dG / gap + t)
    e = SP.spod_energy(lam)
    assert np.max(np.abs(e.sum(axis=1) - 1)) <= 1e-13


def test_leading_modes_only():
    x = case(0)[0]
    f, lam, phi = SP.spod(x, fs=FS, nperseg=64, nmodes=3)
    f2, lam_all, phi_all, G = SP.spod(x, fs=FS, nperseg=64, return_csd=True)
    assert lam.shape == (33, 3) and phi.shape == (33, 8, 3)
    assert np.array_equal(lam, lam_all[:, :3]) and np.array_equal(phi, phi_all[:, :, :3])
    # all the modes give back the matrix that was decomposed: its lower triangle, mirrored
    assert np.max(np.abs(SP.spod_reconstruct(lam_all, phi_all) - R.hermitian_from_lower(G))) <= 2 * R.tol(8) * np.abs(G).max()
    share = SP.spod_energy(lam, trace=lam_all.sum(axis=1))
    assert np.all(share > 0) and np.all(share.sum(axis=1) <= 1 + 1e-12)


def test_too_many_channels():
    with pytest.raises(NotImplementedError) as ei:
        SP.spod(np.zeros((70, 4096), dtype=np.float32), nperseg=64)
    assert isinstance(ei.value, ValueError) and "70" in str(ei.value)


def test_device_residency():
    import torch
    x, wts, _, _, _ = case(1, True)
    want = SP.spod(x, fs=FS, nperseg=32, weights=wts, return_csd=True)
    xt = torch.as_tensor(np.array(x), device="cuda")
    f, lam, phi, G = SP.spod(xt, fs=FS, nperseg=32, weights=wts, return_csd=True)
    assert isinstance(f, np.ndarray) and lam.is_cuda and phi.is_cuda and G.is_cuda
    assert lam.dtype == torch.float64 and phi.dtype == torch.complex128 and G.dtype == torch.complex128
    for g, w_ in zip((lam, phi, G), want[1:]):
        assert np.array_equal(g.cpu().numpy(), w_)
    assert SP.spod_energy(lam).is_cuda and SP.spod_reconstruct(lam, phi).is_cuda
    np.testing.assert_allclose(SP.spod_reconstruct(lam, phi).cpu().numpy(), SP.spod_reconstruct(want[1], want[2]), rtol=0, atol=1e-12)
