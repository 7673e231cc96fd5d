"""Conditioned spectral analysis on the GPU (pyfft_amd.mimo; k_cond.hip): against the longdouble definition within the derived bound of
tests/cond_ref.py, the single-input case in closed form, bitwise agreements, the flags, the end-to-end record against float64
scipy + numpy within the measured allowance, the call history, and the bits of two existing calls."""
import os

import numpy as np
import pytest

import cond_ref as R
import guard_ref as G
import history_ref as HR
import pyfft_amd
from pyfft_amd import _ffi, engine as E, mimo as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def bits(a):
    a = np.ascontiguousarray(host(a))
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b, names=R.WANT + ("status",)):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert host(x).dtype == host(y).dtype and host(x).shape == host(y).shape and np.array_equal(bits(x), bits(y)), k


# ---- against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GPU_N)
def test_cond_against_the_definition(n):
    """every q of the table, the identity and a seeded random order, three matrices per call (scales 1, 1e-6, 1e6), every want on its own
    and all together: within the derived bound; a result beyond it is a defect of the kernel"""
    most = {k: 0.0 for k in R.WANT}
    for q in R.q_of(n):
        for kind in ("identity", "random"):
            Gm, order, refs, bounds = R.case(n, q, kind)
            Gd = dev(Gm)
            res = M.cond(Gd, q, order, want=R.WANT)
            assert not host(res.status).any()
            got = {k: host(getattr(res, k)) for k in R.WANT}
            assert got["H"].shape == (3, n - q, q) and got["Gc"].shape == (3, n - q, n - q) and got["P"].shape == (3, n, n)
            assert got["mcoh"].shape == (3, n - q) and got["piv"].shape == (3, n) and got["mcoh"].dtype == np.float64 and got["H"].dtype == np.complex128
            share = R.share_of(got, refs, bounds)
            for k in R.WANT:
                most[k] = max(most[k], share[k])
            for k in ("Gc", "P"):                                        # exactly Hermitian
                assert np.array_equal(got[k], np.conj(np.swapaxes(got[k], -1, -2)))
            for k in R.WANT:                                             # alone: the same bits, and nothing else comes back
                one = M.cond(Gd, q, order, want=(k,))
                assert np.array_equal(bits(getattr(one, k)), bits(got[k])), (k, q, kind)
                assert all(getattr(one, o) is None for o in R.WANT if o != k) and not host(one.status).any()
    print("n = %d: largest share of the derived bound %s" % (n, {k: "%.3g" % v for k, v in most.items()}))
    assert max(most.values()) <= 1.0, most


def test_a_loading_against_the_definition():
    n, q, load = 17, 8, 1e-3
    Gm = R.matrices(n, 4)
    refs = [R.ref_cond(Gm[s], q, None, load) for s in range(3)]
    res = M.cond(dev(Gm), q, loading=load, want=R.WANT)
    share = R.share_of({k: host(getattr(res, k)) for k in R.WANT}, refs, [R.bound_of(x) for x in refs])
    print("loading 1e-3, n = 17: share of the bound %s" % {k: "%.3g" % v for k, v in share.items()})
    assert max(share.values()) <= 1.0, share


def test_one_input_and_one_output_in_closed_form():
    """n = 2: H = G10 / G00 and mcoh = |G10|^2 / (G00 G11) within 4 ulp"""
    rng = np.random.default_rng(8)
    B = rng.standard_normal((200, 2, 4)) + 1j * rng.standard_normal((200, 2, 4))
    Gm = B @ np.conj(np.swapaxes(B, -1, -2))
    res = M.cond(Gm, 1)
    Hx = Gm[:, 1, 0] / Gm[:, 0, 0].real
    mx = (Gm[:, 1, 0].real ** 2 + Gm[:, 1, 0].imag ** 2) / (Gm[:, 0, 0].real * Gm[:, 1, 1].real)
    H = res.H[:, 0, 0]
    for got, want in ((H.real, Hx.real), (H.imag, Hx.imag), (res.mcoh[:, 0], mx)):
        assert np.all(np.abs(got - want) <= 4 * np.spacing(np.maximum(np.abs(want), np.abs(Hx) if want is not mx else 0)))
    assert np.array_equal(res.piv[:, 0], Gm[:, 0, 0].real)


# ---- bitwise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q", ((5, 2), (33, 16), (64, 32)))
def test_bitwise(n, q, monkeypatch):
    """twice, numpy against device tensors, SP_COND_GRID=1 with 5 matrices against the free grid, one call against one call per matrix"""
    monkeypatch.delenv("SP_COND_GRID", raising=False)
    Gm = np.concatenate((R.matrices(n, 5), R.matrices(n, 6)[:2]))
    order = R.order_of(n, 5)
    a = M.cond(dev(Gm), q, order, want=R.WANT)
    same(a, M.cond(dev(Gm), q, order, want=R.WANT))
    b = M.cond(Gm, q, order, want=R.WANT)
    assert isinstance(b.H, np.ndarray) and isinstance(b.status, np.ndarray) and a.H.is_cuda
    same(a, b)
    assert M.cond_plan(n, q, 5, R.WANT)["items_per_workgroup"] == 1
    monkeypatch.setenv("SP_COND_GRID", "1")
    plan = M.cond_plan(n, q, 5, R.WANT)
    assert plan["workgroups"] == 1 and plan["items_per_workgroup"] == 5
    same(a, M.cond(dev(Gm), q, order, want=R.WANT))
    monkeypatch.setenv("SP_COND_GRID", "2")
    same(a, M.cond(Gm, q, order, want=R.WANT))
    monkeypatch.delenv("SP_COND_GRID")
    for s in range(5):
        one = M.cond(dev(Gm[s]), q, order, want=R.WANT)
        for k in R.WANT:
            assert np.array_equal(bits(getattr(one, k)), bits(getattr(a, k)[s])), (k, s)
    # other dtypes are cast; the upper triangle and the diagonal's imaginary part are not read
    Gu = np.tril(Gm) + 1j * np.eye(n) * 3.0 + np.triu(np.full((n, n), 7.0 - 2j), 1)
    same(a, M.cond(dev(Gu), q, order, want=R.WANT))
    c64 = M.cond(dev(Gm.astype(np.complex64)), q, order, want=R.WANT)
    same(c64, M.cond(Gm.astype(np.complex64).astype(np.complex128), q, order, want=R.WANT))


@pytest.mark.parametrize("lead", range(4))
def test_calls_at_offset_pointers_with_guarded_outputs(lead):
    """G at a pitch above n^2 inside NaN, every output at a pitch inside sentinels, status inside integer guard words"""
    n, q, count = 17, 7, 3
    r = n - q
    Gm = R.matrices(n, 9)
    order = R.order_of(n, 9)
    want = M.cond(dev(Gm), q, order, want=R.WANT)
    li, lo = lead & 1, (lead >> 1) & 1
    gld = n * n + 5
    Gb, Gv = G.poisoned_input(dev(Gm.reshape(count, n * n)), li, pitch=gld)
    snap = G.snapshot(Gb)
    E._bind_stream(Gv)
    lib = _ffi.lib()
    lens = dict(H=r * q, Gc=r * r, mcoh=r, piv=n, P=n * n)
    pitch = {k: v + 3 for k, v in lens.items()}
    outs = {k: G.sentinel_output(lens[k], torch.complex128 if k in ("H", "Gc", "P") else torch.float64, lo, device="cuda", rows=count, pitch=pitch[k])
            for k in R.WANT}
    tb, ta = G.sentinel_output(count, torch.int32, lo, device="cuda")
    p = _ffi.ptr
    rc = lib.sp_cond(p(Gv.data_ptr()), gld, n, count, p(order), q, 31, 0.0, p(outs["H"][1]), pitch["H"], p(outs["Gc"][1]), pitch["Gc"],
                     p(outs["mcoh"][1]), pitch["mcoh"], p(outs["piv"][1]), pitch["piv"], p(outs["P"][1]), pitch["P"], p(ta), 1)
    assert rc == 0, lib.sp_last_error()
    torch.cuda.synchronize()
    assert G.unchanged(Gb, snap)
    for k in R.WANT:
        base = outs[k][0]
        assert G.guards_intact(base, lo, lens[k], rows=count, pitch=pitch[k]) and G.all_written(base, lo, lens[k], rows=count, pitch=pitch[k]), k
        assert np.array_equal(bits(G.interior_of(base, lo, lens[k], rows=count, pitch=pitch[k])), bits(getattr(want, k)).reshape(count, -1)), k
    assert G.guards_intact(tb, lo, count) and G.all_written(tb, lo, count) and not host(G.interior_of(tb, lo, count)).any()
    # host outputs further apart keep what lies between; unwanted outputs are NULL
    base, inner = G.sentinel_output(lens["H"], np.complex128, 1, rows=count, pitch=pitch["H"])
    st = np.full(count, -77, dtype=np.int32)
    _ffi.init()
    rc = lib.sp_cond(p(Gm), n * n, n, count, p(order), q, 1, 0.0, p(int(inner.ctypes.data)), pitch["H"], None, 0, None, 0, None, 0, None, 0, p(st), 0)
    assert rc == 0, lib.sp_last_error()
    assert G.guards_intact(base, 1, lens["H"], rows=count, pitch=pitch["H"]) and G.all_written(base, 1, lens["H"], rows=count, pitch=pitch["H"])
    assert not st.any()
    assert np.array_equal(bits(np.array(G.interior_of(base, 1, lens["H"], rows=count, pitch=pitch["H"]))), bits(want.H).reshape(count, -1))


# ---- flags -----------------------------------------------------------------------------------------------------------
def test_flags():
    n, q = 5, 3
    good = R.matrices(n, 2, spread=1.0, eps=1e-2)[0]
    # a zero matrix
    z = M.cond(dev(np.zeros((2, n, n), dtype=np.complex128)), q, want=R.WANT, check=False)
    assert host(z.status).tolist() == [1, 1]
    for k in R.WANT:
        assert not host(getattr(z, k)).any()
    # a duplicated input between two good matrices
    D = good.copy()
    D[1, :], D[:, 1] = D[0, :], D[:, 0]
    D[1, 1] = D[0, 0]
    batch = np.stack((good, D, good * 3.0))
    res = M.cond(dev(batch), q, want=R.WANT, check=False)
    assert host(res.status).tolist() == [0, 2, 0]
    for k in ("H", "Gc", "mcoh", "P"):
        assert not host(getattr(res, k))[1].any(), k
    assert host(res.piv)[1, 0] == D[0, 0].real and not host(res.piv)[1, 1:].any()
    alone = M.cond(dev(good), q, want=R.WANT)
    for k in R.WANT:
        assert np.array_equal(bits(getattr(res, k)[0]), bits(getattr(alone, k))), k
        assert np.all(np.isfinite(host(getattr(res, k))))
    for mem in (dev, np.asarray):
        with pytest.raises(np.linalg.LinAlgError, match="flat index 1"):
            M.cond(mem(batch), q)
    fixed = M.cond(dev(batch), q, loading=1e-6, want=R.WANT)
    assert not host(fixed.status).any() and np.all(np.isfinite(host(fixed.H)))
    x = R.restate_cond(D, q, loading=1e-6)
    assert np.allclose(host(fixed.H)[1], x["H"], rtol=1e-6, atol=1e-6 * np.max(np.abs(x["H"])))
    # an output that is an exact combination of the inputs: every step is exact on this matrix
    S, Hx = R.explained_output()
    e = M.cond(dev(np.stack((S, good))), 3, want=R.WANT)                 # check=True: a zero output pivot does not raise
    assert host(e.status).tolist() == [4, 0]
    assert host(e.mcoh)[0, 0] == 1.0 and 0 < host(e.mcoh)[0, 1] < 1
    assert not host(e.Gc)[0, 0].any() and not host(e.Gc)[0, :, 0].any() and host(e.Gc)[0, 1, 1].real > 0
    assert np.array_equal(host(e.H)[0], Hx) and host(e.piv)[0, 3] == 0.0 and not host(e.P)[0].any() and host(e.P)[1].any()
    # the same kind of output, inexactly: against the exact definition (H the coefficients, mcoh 1, Gc 0) within the derived bound, to
    # which the roundings of forming the matrix (inner products of 9 terms) are added.  The fourth pivot is a rounding residue of either
    # sign and of about the threshold's size, so status is 0 or 4 (q + 1) and nothing else; the outputs hold in both cases
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((4, 9)) + 1j * rng.standard_normal((4, 9))
    Hz = np.array([0.3 - 2j, 1.5, -(0.25 + 0.5j)])
    Z[3] = Hz @ Z[:3]
    S4 = Z @ np.conj(Z.T)
    f = M.cond(dev(S4), 3, want=("H", "mcoh", "Gc"))
    bH, bm, bG = R.explained_bound(S4, 3, Hz, R.cg(9) * (np.abs(Z) @ np.abs(Z).T))
    print("an explained output: status %d; share of the bound: H %.3g, mcoh %.3g, Gc %.3g"
          % (int(host(f.status)), float(np.max(np.abs(host(f.H)[0] - Hz) / bH)), abs(host(f.mcoh)[0] - 1) / float(bm), abs(host(f.Gc)[0, 0]) / float(bG)))
    assert int(host(f.status)) in (0, 4)
    assert np.all(np.abs(host(f.H)[0] - Hz) <= bH) and abs(host(f.mcoh)[0] - 1) <= bm and abs(host(f.Gc)[0, 0]) <= bG
    # a NaN in one matrix of three
    N = good.copy()
    N[2, 1] = np.nan
    res = M.cond(dev(np.stack((good, N, good * 3.0))), q, want=R.WANT, check=False)
    s = host(res.status).tolist()
    assert s[0] == 0 and s[2] == 0 and 1 <= s[1] <= q
    for k in R.WANT:
        assert np.array_equal(bits(getattr(res, k)[0]), bits(getattr(alone, k))), k
        assert np.all(np.isfinite(host(getattr(res, k))))
    third = M.cond(dev(good * 3.0), q, want=R.WANT)
    for k in R.WANT:
        assert np.array_equal(bits(getattr(res, k)[2]), bits(getattr(third, k))), k
    # a NaN between two OUTPUTS (G[4][3], q = 3) is no collinearity of the inputs: the last pivot fails on it, status is 5 > q, H, mcoh
    # and the pivots before it are those of the clean matrix, P is zeros, and the NaN is handed on in row and column 1 of Gc and
    # nowhere else (the header says so: never NaN holds for status <= q)
    N2 = good.copy()
    N2[4, 3] = N2[3, 4] = np.nan
    res = M.cond(dev(np.stack((good, N2))), q, want=R.WANT)
    assert host(res.status).tolist() == [0, 5]
    for k in ("H", "mcoh"):
        assert np.array_equal(bits(getattr(res, k)[1]), bits(getattr(alone, k))), k
    assert np.array_equal(bits(res.piv[1, :4]), bits(alone.piv[:4])) and host(res.piv)[1, 4] == 0.0 and not host(res.P)[1].any()
    gc = host(res.Gc)[1]
    assert gc[0, 0] == host(alone.Gc)[0, 0] and np.isnan(gc[1, 0]) and np.isnan(gc[0, 1]) and np.isnan(gc[1, 1])
    for k in R.WANT:
        assert np.array_equal(bits(getattr(res, k)[0]), bits(getattr(alone, k))), k


def test_refusals_leave_the_outputs_untouched():
    n, q = 6, 2
    Gd = dev(R.matrices(n, 1)).contiguous()
    E._bind_stream(Gd)
    lib = _ffi.lib()
    Hb, Ha = G.sentinel_output(8, torch.complex128, 0, device="cuda", rows=3)
    tb, ta = G.sentinel_output(3, torch.int32, 0, device="cuda")
    p = _ffi.ptr
    bad_order = np.array([0, 1, 2, 3, 4, 4], dtype=np.int32)
    for args in ((p(Gd.data_ptr()), 35, n, 3, None, q, 1, 0.0, p(Ha), 8), (p(Gd.data_ptr()), 36, n, 3, None, q, 1, 0.0, p(Ha), 7),
                 (p(Gd.data_ptr()), 36, n, 3, p(bad_order), q, 1, 0.0, p(Ha), 8), (p(Gd.data_ptr()), 36, n, 3, None, q, 1, -1.0, p(Ha), 8),
                 (p(Gd.data_ptr()), 36, n, 3, None, 7, 1, 0.0, p(Ha), 8), (p(Gd.data_ptr()), 36, n, 3, None, q, 33, 0.0, p(Ha), 8),
                 (p(Gd.data_ptr()), 36, n, 3, None, q, 1, 0.0, None, 8)):
        rc = lib.sp_cond(*args, None, 0, None, 0, None, 0, None, 0, p(ta), 1)
        assert rc == -1 and lib.sp_last_error().decode().startswith("sp_cond: ")
    torch.cuda.synchronize()
    assert G.first_unwritten(Hb, 0, 8, rows=3) == 0 and G.guards_intact(Hb, 0, 8, rows=3) and G.first_unwritten(tb, 0, 3) == 0
    with pytest.raises(M.CondRefused):
        M.cond(dev(np.ones((2, 65, 65))), 3)


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_end_to_end():
    """the record of three inputs and two outputs through mimo_frf, partial_coherence and ordered_spectra on a device tensor against the
    float64 scipy + numpy reference; the allowance is the one tests/cond_ref.py measures (twice the largest change under 32 Hermitian
    perturbations of 2e-4 per element)"""
    x, y, h = R.record(1)
    fr, Gr = R.scipy_csd(np.concatenate((x, y)))
    xd, yd = dev(x.astype(np.float32)), dev(y.astype(np.float32))
    order = np.array([4, 2, 0, 1, 3])
    f, H, mc, Gnn = M.mimo_frf(xd, yd)
    assert H.is_cuda and mc.is_cuda and Gnn.is_cuda and H.shape == (129, 2, 3) and np.allclose(f, fr)
    ref = R.outputs_of(Gr, 3, ("H", "mcoh", "Gc"))
    al = R.allowance_of(Gr, 3, ("H", "mcoh", "Gc"))
    used = {}
    for k, got in (("H", H), ("mcoh", mc), ("Gc", Gnn)):
        err = np.max(np.abs(host(got) - ref[k]).reshape(129, -1), axis=1)
        used[k] = float(np.max(err / al[k]))
    f2, pc, mall = M.partial_coherence(torch.cat((xd, yd)))
    refP = R.outputs_of(Gr, 5, ("pc", "mc"))
    alP = R.allowance_of(Gr, 5, ("pc", "mc"))
    for k, got in (("pc", pc), ("mc", mall)):
        used[k] = float(np.max(np.max(np.abs(host(got) - refP[k]).reshape(129, -1), axis=1) / alP[k]))
    f3, S = M.ordered_spectra(torch.cat((xd, yd)), order)
    refS = R.outputs_of(Gr, 5, ("piv",), order)["piv"]
    alS = R.allowance_of(Gr, 5, ("piv",), order)["piv"]
    used["piv"] = float(np.max(np.max(np.abs(host(S) - refS), axis=1) / alS))
    print("end to end: share of the measured allowance %s" % {k: "%.3g" % v for k, v in used.items()})
    assert max(used.values()) <= 1.0, used
    # what the record is for: the estimated responses are the filters', the front ends agree with one another
    Ht = R.true_response(h)
    assert np.max(np.abs(host(H) - Ht)) <= 0.1 * np.max(np.abs(Ht))
    assert np.array_equal(bits(M.multiple_coherence(xd, yd)[1]), bits(mc)) and np.array_equal(bits(M.conditioned_spectra(xd, yd)[1]), bits(Gnn))
    fb, Hb, _, _ = M.mimo_frf(xd, yd, band=(0.1, 0.2))
    sel = (fr >= 0.1) & (fr <= 0.2)
    assert np.array_equal(fb, fr[sel]) and np.array_equal(bits(Hb), bits(H[torch.as_tensor(sel, device="cuda")]))
    fh, Hh, mh, _ = M.mimo_frf(x.astype(np.float32), y.astype(np.float32))
    assert isinstance(Hh, np.ndarray) and np.array_equal(bits(Hh), bits(H)) and np.array_equal(bits(mh), bits(mc))


# ---- history and neighbours ----------------------------------------------------------------------------------------------
def test_the_same_bits_after_a_medley_of_other_calls():
    n, q = 33, 16
    Gm, order = R.matrices(n, 12), R.order_of(n, 12)
    first = M.cond(dev(Gm), q, order, want=R.WANT)
    first_host = M.cond(Gm, q, order, want=R.WANT)

    def call(run, arrays, mem):
        run(tuple(dev(a) if mem == "device" else a for a in arrays))
    for c in HR.medley():
        HR.run_call(call, c, "device")
    same(first, M.cond(dev(Gm), q, order, want=R.WANT))
    same(first_host, M.cond(Gm, q, order, want=R.WANT))
    same(first, first_host)


def test_existing_calls_are_unchanged():
    """one spod call and one ar_ls call against the bits the commit before this family gave on an MI355X (tests/golden/cond_before.npz,
    taken with that commit's library)"""
    before = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond_before.npz"))
    now = R.before_calls(pyfft_amd)
    assert sorted(before.files) == sorted(now)
    for key in before.files:
        assert before[key].dtype == now[key].dtype and np.array_equal(bits(before[key]), bits(now[key])), key
