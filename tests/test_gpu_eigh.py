"""The batched Hermitian eigensolver (sp_eigh, k_eigh.hip) on the MI355X.  Every matrix of every family, order and batch is held to the
same float64 limits as the numpy restatement in tests/test_host_eigh.py, with the one derived tolerance tol(n) = 4 n 30 eps:
    ||A_L V - V diag(w)||_F <= tol ||A||_F   (A_L: the Hermitian matrix of the lower triangle),   ||V^H V - I||_F <= tol,
    max|w - eigvalsh(A_L)| <= tol ||A||_2,   w descending,   the largest component of every vector real and positive,   sweeps <= 30.
A batch of 300 is more than one workgroup per CU at order 64, so the grid walks the batch; SP_EIGH_GRID makes it walk at every order."""
import os

import numpy as np
import pytest

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E                       # noqa: E402
import eigh_ref as R                                          # noqa: E402

EPS = np.finfo(np.float64).eps
BATCHES = (1, 3, 300)


def held(a, w, V, sw, what):
    n = a.shape[-1]
    t = R.tol(n)
    L = R.limits(a, w, V, sw)
    print("%s: resid %.3g tol, orth %.3g tol, eig %.3g tol, phase %.3g, sweeps %d"
          % (what, L["resid"] / t, L["orth"] / t, L["eig"] / t, L["phase"], L["sweeps"]))
    assert L["resid"] <= t and L["orth"] <= t and L["eig"] <= t, (what, L)
    assert L["descending"] and L["sweeps"] <= 30 and L["phase"] <= 4 * EPS, (what, L)
    return L


@pytest.mark.parametrize("n", R.ORDERS)
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_families(family, n):
    for batch in BATCHES:
        a = R.FAMILIES[family](np.random.default_rng(7000 + 10 * n + batch), batch, n)
        w, V, sw = E.eigh(a)
        assert w.shape == (batch, n) and w.dtype == np.float64 and V.shape == (batch, n, n) and V.dtype == np.complex128
        assert sw.shape == (batch,) and sw.dtype == np.int32
        held(a, w, V, sw, "%s n=%d batch=%d" % (family, n, batch))
        if family in ("diagonal", "zero", "identity"):
            assert np.all(sw == 0)
        if family == "real_symmetric":
            assert np.max(np.abs(V.imag)) <= R.tol(n)              # real to rounding
        if family == "identity":
            assert np.all(w == 1.0)


@pytest.mark.parametrize("n", [5, 16, 17, 64])
def test_the_grid_walks_the_batch(n):
    """Two workgroups for seven matrices: the result is that of one workgroup each, bit for bit."""
    a = R.fam_csd(np.random.default_rng(n), 7, n)
    want = E.eigh(a)
    os.environ["SP_EIGH_GRID"] = "2"
    try:
        got = E.eigh(a)
    finally:
        del os.environ["SP_EIGH_GRID"]
    held(a, *got, "grid 2, n=%d" % n)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)


@pytest.mark.parametrize("n", [3, 9, 33, 64])
def test_upper_triangle_is_not_read(n):
    rng = np.random.default_rng(40 + n)
    a = R.fam_csd(rng, 3, n)
    junk = a.copy()
    iu = np.triu_indices(n, 1)
    junk[:, iu[0], iu[1]] = 1e9 * rng.standard_normal(iu[0].size)
    junk[:, iu[0][::2], iu[1][::2]] = complex(np.nan, np.inf)
    junk[:, np.arange(n), np.arange(n)] = a[:, np.arange(n), np.arange(n)].real + 1j * np.arange(1, n + 1)    # the diagonal's imaginary part
    junk.imag[:, 0, 0] = np.inf
    for x, y in zip(E.eigh(a), E.eigh(junk)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("n", [2, 8, 17, 64])
def test_nvec_and_reruns_are_bitwise(n):
    a = R.fam_csd(np.random.default_rng(50 + n), 5, n)
    w, V, sw = E.eigh(a)
    w1, V1, sw1 = E.eigh(a)
    assert np.array_equal(w, w1) and np.array_equal(V, V1) and np.array_equal(sw, sw1)
    w0, V0, sw0 = E.eigh(a, nvec=0)
    assert V0.shape == (5, n, 0) and np.array_equal(w0, w) and np.array_equal(sw0, sw)
    w2, V2, sw2 = E.eigh(a, nvec=2)
    assert V2.shape == (5, n, 2) and np.array_equal(w2, w) and np.array_equal(sw2, sw) and np.array_equal(V2, V[:, :, :2])


def test_a_nan_matrix_reports_and_leaves_its_neighbours():
    a = R.fam_csd(np.random.default_rng(60), 5, 17)
    a[2] = np.nan
    w, V, sw = E.eigh(a, check=False)
    assert sw[2] == 31 and np.all(sw[[0, 1, 3, 4]] <= 30)
    keep = [0, 1, 3, 4]
    held(a[keep], w[keep], V[keep], sw[keep], "beside a NaN matrix")
    with pytest.raises(np.linalg.LinAlgError) as ei:
        E.eigh(a)
    assert "2" in str(ei.value)
    w5, _, sw5 = E.eigh(a, max_sweeps=5, check=False)
    assert sw5[2] == 6
    b = R.fam_csd(np.random.default_rng(61), 2, 4)
    b[1, 3, 0] = np.inf
    assert list(E.eigh(b, check=False)[2] > 30) == [False, True]


@pytest.mark.parametrize("dtype", [np.complex64, np.float32, np.float64])
def test_other_dtypes_are_cast(dtype):
    rng = np.random.default_rng(70)
    a = R.fam_real_symmetric(rng, 3, 9).real if np.dtype(dtype).kind == "f" else R.fam_csd(rng, 3, 9)
    a = a.astype(dtype)
    w, V, sw = E.eigh(a)
    held(a.astype(np.complex128), w, V, sw, str(np.dtype(dtype)))


def test_leading_axes():
    a = R.fam_csd(np.random.default_rng(80), 6, 5).reshape(2, 3, 5, 5)
    w, V, sw = E.eigh(a, nvec=3)
    assert w.shape == (2, 3, 5) and V.shape == (2, 3, 5, 3) and sw.shape == (2, 3)
    wf, Vf, _ = E.eigh(a.reshape(6, 5, 5))
    assert np.array_equal(w.reshape(6, 5), wf) and np.array_equal(V.reshape(6, 5, 3), Vf[:, :, :3])
    w0, V0, sw0 = E.eigh(np.zeros((0, 5, 5)))
    assert w0.shape == (0, 5) and V0.shape == (0, 5, 5) and sw0.shape == (0,)


def test_device_tensors_in_device_tensors_out():
    import torch
    a = R.fam_csd(np.random.default_rng(90), 4, 33)
    want = E.eigh(a)
    at = torch.as_tensor(a, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        w, V, sw = E.eigh(at, check=False)
    s.synchronize()
    assert w.is_cuda and V.is_cuda and sw.is_cuda and w.device == at.device
    assert w.dtype == torch.float64 and V.dtype == torch.complex128 and sw.dtype == torch.int32
    for g, w_ in zip((w, V, sw), want):
        assert np.array_equal(g.cpu().numpy(), w_)
    w2, V2, _ = E.eigh(at.to(torch.complex64), nvec=1)
    assert V2.shape == (4, 33, 1) and torch.allclose(w2, w, rtol=1e-5, atol=1e-6)
    bad = at.clone()
    bad[3] = float("nan")
    with pytest.raises(np.linalg.LinAlgError):
        E.eigh(bad)
    with pytest.raises(TypeError):
        E.eigh(torch.as_tensor(a))                                 # a host tensor


def test_c_refusals_with_the_device_up():
    from test_host_eigh import test_c_refusals_need_no_device
    _ffi.init()
    test_c_refusals_need_no_device()
    # device memory: NULL where a buffer is needed is refused in the same words
    import torch
    a = torch.zeros((1, 4, 4), dtype=torch.complex128, device="cuda")
    w = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
    sw = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = _ffi.lib()
    assert lib.sp_eigh(_ffi.ptr(a.data_ptr()), 4, 1, 2, 30, _ffi.ptr(w.data_ptr()), None, _ffi.ptr(sw.data_ptr()), 1) < 0
    assert "sp_eigh: v is required for nvec = 2" in lib.sp_last_error().decode()
    assert lib.sp_eigh(_ffi.ptr(a.data_ptr()), 4, 1, 0, 30, _ffi.ptr(w.data_ptr()), None, _ffi.ptr(sw.data_ptr()), 1) == 0
    torch.cuda.synchronize()
    assert int(sw[0]) == 0 and bool(torch.all(w == 0))
