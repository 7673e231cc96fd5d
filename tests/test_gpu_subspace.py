"""The data covariance matrix, the covariance least-squares fits and the MUSIC / eigenvector pseudospectrum on the GPU against the
float64 definitions of tests/subspace_ref.py: the smallest shapes at which each mechanism can go wrong (one snapshot, halos across
stage and tile seams, many tiles with a ragged last one, rows and frames), the derived bounds and the measured allowances, two close
tones end to end, and the invariants (bitwise repeatability, host and device calls, two passes, offset pointers inside poisoned
buffers with guarded pitched outputs, refusals and bad records that leave the outputs alone).  The calls of pyfft_amd.parametric from
before stay bit for bit what they were."""
import os

import numpy as np
import pytest

import burg_ref as B
import guard_ref as G
import subspace_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, parametric as PM, subspace as SS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def covmat_of(name, fb, x=None, **kw):
    c = R.shape_of(name)
    return E.covmat(R.signals(name) if x is None else x, c["n"], c["hop"], c["first"], c["nframes"], c["m"], fb=fb, **kw)


def cov_held(got, name, fb, detrend=True, mean_value=None):
    """every element within the derived bound of the definition; exactly Hermitian; a real diagonal -> the share of the bound used"""
    c = R.shape_of(name)
    x = R.signals(name)
    ref = R.cov_reference(name, fb, detrend, mean_value)
    got = np.asarray(got)
    assert got.shape == ref.shape == (c["rows"], c["nframes"], c["m"], c["m"]) and got.dtype == np.complex128
    assert np.all(np.isfinite(got.view(np.float64)))
    assert np.array_equal(got, np.conj(np.swapaxes(got, -1, -2))) and not np.diagonal(got, axis1=-2, axis2=-1).imag.any()
    if not c["cplx"]:
        assert not got.imag.any()
    share = 0.0
    for r in range(c["rows"]):
        for g in range(c["nframes"]):
            raw = B.segment(x[r], c["n"], c["first"], g, c["hop"], detrend=False)
            s = B.segment(x[r], c["n"], c["first"], g, c["hop"], detrend, mean_value)
            bound = R.covmat_bound(s, c["m"], R.mean_rounding(raw) if detrend and mean_value is None else 0.0)
            share = max(share, float(np.max(np.abs(got[r, g] - ref[r, g]))) / bound)
    print("covmat %s fb %d: share of the bound %.3f" % (name, fb, share))
    assert share <= 1.0, (name, fb, share)
    return share


# ---- the matrix --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", (False, True))
@pytest.mark.parametrize("name", list(R.COV_CASES))
def test_covmat_against_the_definition(name, fb):
    c = R.shape_of(name)
    cov_held(covmat_of(name, fb, detrend=False), name, fb, detrend=False)       # the bound the definition sets, with no mean in it
    cov_held(covmat_of(name, fb), name, fb)
    plan = E.sub_plan("covmat", c["n"], c["m"], c["rows"], c["nframes"], c["cplx"])
    assert plan["tiles"] == -(-c["n"] // plan["chunk"]) and plan["passes"] == 1 == E.last_passes(E.SUB_PASSES)
    if name == "long":
        assert plan["tiles"] == 49


def test_covmat_with_a_given_mean():
    cov_held(covmat_of("frames", True, mean_value=0.65), "frames", True, True, 0.65)
    cov_held(covmat_of("c333c", False, mean_value=0.6 - 0.3j), "c333c", False, True, 0.6 - 0.3j)


def test_corrmtx_cov_is_the_whole_row():
    x = R.signals("frames")
    for method, fb in (("modified", True), ("covariance", False)):
        C = SS.corrmtx_cov(x, 7, method)
        assert C.shape == (3, 7, 7) and np.array_equal(bits(C), bits(E.covmat(x, x.shape[1], 1, 0, 1, 7, fb=fb, detrend=False)[:, 0]))
        ref = R.covmat_def(x[1].astype(np.float64), 7, fb)
        assert np.max(np.abs(C[1] - ref)) <= R.covmat_bound(x[1].astype(np.float64), 7)
    assert SS.corrmtx_cov(dev(x), 7).is_cuda


# ---- the fits ----------------------------------------------------------------------------------------------------------------------
def ls_of(name, fb, x=None, **kw):
    c = B.shape_of(name)
    return E.ar_ls(B.signals(name) if x is None else x, c["n"], c["hop"], c["first"], c["nframes"], R.LS_CASES[name], fb=fb, **kw)


def ls_held(got, name, fb, what="engine.ar_ls"):
    a, e, st = (np.asarray(v) for v in got)
    assert not st.any() and np.all(np.isfinite(a.view(np.float64))) and np.all(np.isfinite(e)) and np.all(a[..., 0] == 1)
    d = R.ls_deviations((a, e[..., None], np.zeros(e.shape + (1,))), R.ls_reference(name, fb))
    shares = [v / w for v, w in zip(d, R.LS_ALLOWANCE)]
    print("%s %s fb %d: P %.2e a %.2e e %.2e, shares %.2f %.2f %.2f" % ((what, name, fb) + d + tuple(shares)))
    assert max(shares) <= 1.0, (name, fb, d, R.LS_ALLOWANCE)
    return max(shares)


@pytest.mark.parametrize("fb", (False, True))
@pytest.mark.parametrize("name", list(R.LS_CASES))
def test_ar_ls_against_lstsq(name, fb):
    c = B.shape_of(name)
    got = ls_of(name, fb)
    p = R.LS_CASES[name]
    assert got[0].shape == (c["rows"], c["nframes"], p + 1) and got[1].shape == got[2].shape == (c["rows"], c["nframes"])
    assert got[0].dtype == (np.complex128 if c["cplx"] else np.float64) and got[1].dtype == np.float64 and got[2].dtype == np.int32
    ls_held(got, name, fb)


def test_a_noiseless_tone_is_singular_and_says_so():
    n = 300
    tone = np.cos(2 * np.pi * np.arange(n) / 6.0).astype(np.float32)     # 1, 1/2, -1/2, -1 ..: exact in float32, so truly noiseless
    noisy = B.signals("w333c").real[0, :n].astype(np.float32)
    x = np.stack([noisy, tone, np.zeros(n, dtype=np.float32)])
    for fb in (False, True):
        a, e, st = E.ar_ls(x, n, 1, 0, 1, 8, fb=fb, detrend=False, check=False)
        assert st[0, 0] == 0 and 1 <= st[1, 0] <= 8 and st[2, 0] == 1
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(e)) and e[0, 0] > 0
        assert np.array_equal(a[1:, 0], np.broadcast_to(np.eye(1, 9)[0], (2, 9))) and not e[1:].any()
        with pytest.raises(np.linalg.LinAlgError, match="model .*flat index 1"):
            E.ar_ls(x, n, 1, 0, 1, 8, fb=fb, detrend=False)
        with pytest.raises(np.linalg.LinAlgError):
            E.ar_ls(dev(x), n, 1, 0, 1, 8, fb=fb, detrend=False)
    P = PM.ar_psd(a[:, 0], e[:, 0], nfft=64)[1]
    assert np.all(np.isfinite(P)) and not P[1:].any()


def test_front_ends_of_the_fits():
    x = B.signals("frames")
    for fn, pf, fb in ((PM.arcov, PM.pcov, False), (PM.armcov, PM.pmcov, True)):
        a, e = fn(x, 6)
        assert a.shape == (3, 7) and e.shape == (3,) and a.dtype == np.float64
        want = E.ar_ls(x, x.shape[1], 1, 0, 1, 6, fb=fb, detrend=False)
        assert np.array_equal(bits(a), bits(want[0][:, 0])) and np.array_equal(bits(e), bits(want[1][:, 0]))
        ref = [R.ls_lstsq(x[r].astype(np.float64), 6, fb) for r in range(3)]
        assert max(np.max(np.abs(a[r] - ref[r][0])) / np.sum(np.abs(ref[r][0])) for r in range(3)) <= R.LS_ALLOWANCE[1]
        f, P = pf(x, 6, nfft=128, fs=4.0)
        f2, P2 = PM.ar_psd(a, e, nfft=128, fs=4.0)
        assert np.array_equal(f, f2) and np.array_equal(P, P2) and P.shape == (3, 65) and P.dtype == np.float32
        Pd = pf(dev(x), 6, nfft=128, fs=4.0)[1]
        assert Pd.is_cuda and np.array_equal(Pd.cpu().numpy(), P)
    xs = x[:, :413]
    for method, one in (("cov", PM.pcov), ("mcov", PM.pmcov)):
        f, t, S = PM.ar_spectrogram(xs, 6, 100, noverlap=23, method=method, fs=2.0, nfft=64)
        nf = (413 - 100) // 77 + 1
        assert S.shape == (3, 33, nf) and np.array_equal(t, (np.arange(nf) * 77 + 50.0) / 2.0)
        for g in range(nf):
            fg, Pg = one(xs[:, g * 77:g * 77 + 100], 6, nfft=64, fs=2.0, detrend=True)
            assert np.array_equal(fg, f) and np.array_equal(S[..., g], Pg), g


# ---- the pseudospectrum --------------------------------------------------------------------------------------------------------------
_eig = {}


def eig_of(m):
    """V, w of the float64 reference for a matrix of order m (numpy's eigh, descending), computed once"""
    if m not in _eig:
        name = {2: "c64", 24: "c333c", 64: "seam64"}[m]                  # (a single snapshot, as c2 has, leaves no positive noise eigenvalue)
        c = R.shape_of(name)
        C = R.covmat_def(B.segment(R.signals(name)[0], c["n"]), m, True)
        _eig[m] = R.eigh_desc(C)
    return _eig[m]


@pytest.mark.parametrize("weighting", ("music", "ev"))
@pytest.mark.parametrize("m", (2, 24, 64))
def test_pseudospectrum_against_the_definition(m, weighting):
    w, V = eig_of(m)
    worst = 0.0
    for p in sorted({0, min(2, m - 1), m - 1}):
        for nb, start, step in ((257, 0.0, 1.0 / 512), (300, -0.5, 1.0 / 300), (5, 1e6 + 0.37, 1e-3)):
            want, st_ref = R.pseudo_def(V, w, p, nb, start, step, weighting)
            bound = R.pseudo_bound(V, w, p, nb, start, step, weighting)
            for out64 in (False, True):
                P, st = E.pseudospectrum(V[None], w[None], p, nb, start, step, weighting, out64)
                assert P.shape == (1, nb) and P.dtype == (np.float64 if out64 else np.float32) and st.shape == (1,) and st[0] == st_ref == 0
                ok = want > 0                                        # a sum of exactly zero (m = 2: v = (1, -1) / sqrt 2 at nu = 0) has no relative bound
                assert not np.any(np.isnan(P)) and ok.sum() >= nb - 1
                err = np.abs(P[0][ok] - want[ok]) / want[ok]
                lim = bound[ok] + (0.0 if out64 else 2.0 ** -23)
                assert np.all(err <= lim), (m, p, weighting, out64, float(np.max(err / lim)))
                if out64:
                    worst = max(worst, float(np.max(err / lim)))
    print("pseudospectrum m %d %s: share of the bound %.3f" % (m, weighting, worst))


def test_pseudospectrum_flags_a_weight_that_is_not_positive():
    w, V = eig_of(24)
    w2 = w.copy()
    w2[-1], w2[-3] = 0.0, -2.0
    W, VV = np.stack([w, w2, np.zeros(24)]), np.stack([V, V, V])
    P, st = E.pseudospectrum(VV, W, 2, 129, 0.0, 1.0 / 256, "ev", True)
    assert list(st) == [0, 1, 1] and np.all(np.isfinite(P)) and not P[2].any() and np.all(P[:2] > 0)
    want = R.pseudo_def(V, w2, 2, 129, 0.0, 1.0 / 256, "ev")[0]
    assert np.all(np.abs(P[1] - want) <= R.pseudo_bound(V, w2, 2, 129, 0.0, 1.0 / 256, "ev") * want)
    Pm, stm = E.pseudospectrum(VV, W, 2, 129, 0.0, 1.0 / 256, "music", True)
    assert not stm.any() and np.array_equal(Pm[0], Pm[2])
    Pd, std = E.pseudospectrum(dev(VV), dev(W), 2, 129, 0.0, 1.0 / 256, "ev", True)
    assert Pd.is_cuda and np.array_equal(bits(Pd), bits(P)) and np.array_equal(std.cpu().numpy(), st)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.E2E_CASES))
def test_two_close_tones_end_to_end(name):
    cplx, p, _ = R.E2E_CASES[name]
    x = R.tones(name)
    C, w, V, Pref = R.e2e_reference(name)
    assert w[p - 1] / w[p] >= R.MIN_GAP                                 # the condition of the allowance, on the reference
    assert np.max(np.abs(R.peaks(Pref, 2) / R.E2E_GRID - np.array(R.TONES))) <= 1.0 / R.E2E_GRID
    f, P = SS.pmusic(x, p, m=R.E2E_M, nfft=R.E2E_GRID, out64=True)
    nb, start, step = R.e2e_axis(cplx)
    assert P.shape == (nb,) and np.array_equal(f, np.arange(nb) / R.E2E_GRID if not cplx else np.fft.fftfreq(R.E2E_GRID))
    off = float(np.max(np.abs(P - Pref) / Pref))
    print("pmusic %s: %.2e of %.2e (share %.2f)" % (name, off, R.E2E_ALLOWANCE, off / R.E2E_ALLOWANCE))
    assert off <= R.E2E_ALLOWANCE
    assert np.max(np.abs(R.peaks(P, 2) / R.E2E_GRID - np.array(R.TONES))) <= 1.0 / R.E2E_GRID
    fe, Pe = SS.peig(x, p, m=R.E2E_M, nfft=R.E2E_GRID, out64=True)
    offe = float(np.max(np.abs(Pe - R.e2e_reference(name, "ev")[3]) / R.e2e_reference(name, "ev")[3]))
    assert offe <= R.E2E_ALLOWANCE and np.max(np.abs(R.peaks(Pe, 2) / R.E2E_GRID - np.array(R.TONES))) <= 1.0 / R.E2E_GRID
    Cg = SS.corrmtx_cov(x, R.E2E_M)
    wg, Vg, _ = E.eigh(Cg)
    assert np.max(np.abs(SS.esprit(Vg, p)[-2:] - np.array(R.TONES))) <= 1.0 / R.E2E_GRID
    assert SS.subspace_order(wg, R.E2E_N - R.E2E_M + 1) == SS.subspace_order(w, R.E2E_N - R.E2E_M + 1)
    fz, Pz = SS.pmusic(x, p, m=R.E2E_M, band=(0.19, 0.23), nbins=401, fs=1.0)
    assert Pz.dtype == np.float32 and np.allclose(fz, np.linspace(0.19, 0.23, 401))
    assert np.max(np.abs(fz[R.peaks(Pz, 2)] - np.array(R.TONES))) <= 2e-4


def test_white_noise_has_no_lines_and_the_spectrogram_is_the_slices():
    for cplx in (False, True):
        x = R.white(512, cplx)
        w = E.eigh(SS.corrmtx_cov(x, 24))[0]
        assert SS.subspace_order(w, 512 - 24 + 1, "mdl") == 0 and SS.subspace_order(dev(w), 512 - 24 + 1, "aic") == 0
    x = R.signals("frames")[:, :413]
    f, t, S = SS.subspace_spectrogram(x, 4, 100, noverlap=23, m=12, nfft=64, fs=2.0)
    nf = (413 - 100) // 77 + 1
    assert S.shape == (3, 33, nf) and np.array_equal(t, (np.arange(nf) * 77 + 50.0) / 2.0)
    for g in range(nf):
        fg, Pg = SS.pmusic(x[:, g * 77:g * 77 + 100], 4, m=12, nfft=64, fs=2.0, detrend=True)
        assert np.array_equal(fg, f) and np.array_equal(S[..., g], Pg), g
    Sd = SS.subspace_spectrogram(dev(np.array(x)), 4, 100, noverlap=23, m=12, nfft=64, fs=2.0, weighting="ev")[2]
    assert Sd.is_cuda and Sd.shape == (3, 33, nf)


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c333c", "seam64", "frames"))
def test_bitwise_twice_and_host_against_device(name):
    c = R.shape_of(name)
    x = R.signals(name)
    for fb in (False, True):
        one, two, on_dev = covmat_of(name, fb), covmat_of(name, fb), covmat_of(name, fb, x=dev(x))
        assert on_dev.is_cuda and on_dev.dtype == torch.complex128
        assert np.array_equal(bits(one), bits(two)) and np.array_equal(bits(one), bits(on_dev))
    p = min(c["m"] - 1, c["n"] // 2)
    args = (c["n"], c["hop"], c["first"], c["nframes"], p)
    one, two, on_dev = E.ar_ls(x, *args, fb=True), E.ar_ls(x, *args, fb=True), E.ar_ls(dev(x), *args, fb=True)
    assert on_dev[0].dtype == (torch.complex128 if c["cplx"] else torch.float64) and on_dev[2].dtype == torch.int32
    for a, b, d in zip(one, two, on_dev):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(d))


def test_two_passes(monkeypatch):
    name = "ragged"
    c = R.shape_of(name)
    x = R.signals(name)
    args = (c["n"], c["hop"], c["first"], c["nframes"])
    monkeypatch.setenv("SP_AR_SEGS", str(R.SEGS_HOOK))
    C2 = E.covmat(x, *args, c["m"])
    assert E.last_passes(E.SUB_PASSES) == 2 == E.sub_plan("covmat", c["n"], c["m"], 1, c["nframes"], True)["passes"]
    L2 = E.ar_ls(x, *args, 3, fb=True)
    assert E.last_passes(8) == 2 == E.sub_plan("ls", c["n"], 4, 1, c["nframes"], True)["passes"]
    monkeypatch.delenv("SP_AR_SEGS")
    C1 = E.covmat(x, *args, c["m"])
    assert E.last_passes(8) == 1
    L1 = E.ar_ls(x, *args, 3, fb=True)
    assert E.last_passes(8) == 1 and E.last_passes(E.AR_PASSES) == 0
    assert np.array_equal(bits(C1), bits(C2)) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(L1, L2))
    cov_held(C2, name, True)


@pytest.mark.parametrize("lead", range(4))
def test_calls_at_offset_pointers_with_guarded_outputs(lead):
    """rows of x a pitch apart inside NaN, the matrices and the models a pitch apart inside sentinels, both residues of the elements"""
    name = "frames"
    c = R.shape_of(name)
    x = R.signals(name)
    rows, nsig = x.shape
    n, m, nf = c["n"], c["m"], c["nframes"]
    segs, x_ld, C_ld, o_ld = rows * nf, nsig + 5, m * m + 3, m + 3
    lx, lo = lead & 1, (lead >> 1) & 1
    xb, xv = G.poisoned_input(dev(x), lx, pitch=x_ld)
    snap = G.snapshot(xb)
    want = E.covmat(xv, n, c["hop"], c["first"], nf, m).cpu().numpy()
    assert np.array_equal(bits(want), bits(covmat_of(name, True)))
    wa, we, ws = (v.cpu().numpy() for v in E.ar_ls(xv, n, c["hop"], c["first"], nf, m - 1, fb=True))
    E._bind_stream(xv)
    lib = _ffi.lib()
    rec = (_ffi.ptr(xv.data_ptr()), _ffi.DTYPE_F32, x_ld, nsig, rows, n, c["hop"], c["first"], nf)
    Cb, Ca = G.sentinel_output(m * m, torch.complex128, lo, device="cuda", rows=segs, pitch=C_ld)
    rc = lib.sp_covmat(*rec, m, 1, _ffi.DETREND_SEGMEAN, 0.0, 0.0, _ffi.ptr(Ca), C_ld, 1)
    assert rc == 0, lib.sp_last_error()
    ab, aa = G.sentinel_output(m, torch.float64, lo, device="cuda", rows=segs, pitch=o_ld)
    eb, ea = G.sentinel_output(segs, torch.float64, lo, device="cuda")
    sb, sa = G.sentinel_output(segs, torch.int32, lo, device="cuda")
    rc = lib.sp_ar_ls(*rec, m - 1, 1, _ffi.DETREND_SEGMEAN, 0.0, 0.0, _ffi.ptr(aa), _ffi.ptr(ea), _ffi.ptr(sa), o_ld, 1)
    assert rc == 0, lib.sp_last_error()
    torch.cuda.synchronize()
    assert G.unchanged(xb, snap)
    assert G.guards_intact(Cb, lo, m * m, rows=segs, pitch=C_ld) and G.all_written(Cb, lo, m * m, rows=segs, pitch=C_ld)
    assert np.array_equal(bits(G.interior_of(Cb, lo, m * m, rows=segs, pitch=C_ld)), bits(want.reshape(segs, m * m)))
    assert G.guards_intact(ab, lo, m, rows=segs, pitch=o_ld) and G.all_written(ab, lo, m, rows=segs, pitch=o_ld)
    assert np.array_equal(bits(G.interior_of(ab, lo, m, rows=segs, pitch=o_ld)), bits(wa.reshape(segs, m)))
    for base, w_ in ((eb, we), (sb, ws)):
        assert G.guards_intact(base, lo, segs) and G.all_written(base, lo, segs)
        assert np.array_equal(bits(G.interior_of(base, lo, segs)), bits(w_.reshape(segs)))
    # the pseudospectrum at a pitch
    wv, V = eig_of(24)
    Vd, wd = dev(np.stack([V, V])), dev(np.stack([wv, wv]))
    Pb, Pa = G.sentinel_output(100, torch.float32, lo, device="cuda", rows=2, pitch=107)
    tb, ta = G.sentinel_output(2, torch.int32, lo, device="cuda")
    rc = lib.sp_pseudospectrum(_ffi.ptr(Vd.data_ptr()), 24, _ffi.ptr(wd.data_ptr()), 24, 2, 2, 1, 100, 0.1, 0.003, 0, _ffi.ptr(Pa), 107, _ffi.ptr(ta), 1)
    assert rc == 0, lib.sp_last_error()
    torch.cuda.synchronize()
    assert G.guards_intact(Pb, lo, 100, rows=2, pitch=107) and G.all_written(Pb, lo, 100, rows=2, pitch=107) and G.guards_intact(tb, lo, 2)
    assert np.array_equal(bits(G.interior_of(Pb, lo, 100, rows=2, pitch=107)), bits(E.pseudospectrum(Vd, wd, 2, 100, 0.1, 0.003, "ev")[0]))


def test_host_matrices_further_apart_keep_what_lies_between():
    name = "frames"
    c = R.shape_of(name)
    x = np.array(R.signals(name))
    rows, nsig = x.shape
    m, nf = c["m"], c["nframes"]
    segs, C_ld = rows * nf, m * m + 5
    base, inner = G.sentinel_output(m * m, np.complex128, 1, rows=segs, pitch=C_ld)
    _ffi.init()
    rc = _ffi.lib().sp_covmat(_ffi.ptr(x), _ffi.DTYPE_F32, nsig, nsig, rows, c["n"], c["hop"], c["first"], nf, m, 1, _ffi.DETREND_SEGMEAN, 0.0, 0.0,
                              _ffi.ptr(int(inner.ctypes.data)), C_ld, 0)
    assert rc == 0, _ffi.lib().sp_last_error()
    assert G.guards_intact(base, 1, m * m, rows=segs, pitch=C_ld) and G.all_written(base, 1, m * m, rows=segs, pitch=C_ld)
    assert np.array_equal(bits(np.array(G.interior_of(base, 1, m * m, rows=segs, pitch=C_ld))), bits(covmat_of(name, True).reshape(segs, m * m)))


def test_host_pseudospectra_further_apart_keep_what_lies_between():
    """sp_pseudospectrum on host memory with P_ld > nbins, float32 and float64: the rows are staged in both directions, so the room
    between them comes back as it was, every bin is written and the bits are those of the dense call"""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((2, 9, 4)) + 1j * rng.standard_normal((2, 9, 4))
    w, V = (np.ascontiguousarray(np.stack(t)) for t in zip(*(R.eigh_desc(x.conj().T @ x) for x in X)))
    nbins, P_ld = 100, 107
    _ffi.init()
    for out64 in (False, True):
        base, inner = G.sentinel_output(nbins, np.float64 if out64 else np.float32, 1, rows=2, pitch=P_ld)
        st = np.full(2, -77, dtype=np.int32)
        rc = _ffi.lib().sp_pseudospectrum(_ffi.ptr(V), 4, _ffi.ptr(w), 4, 2, 2, 1, nbins, 0.1, 0.003, int(out64), _ffi.ptr(int(inner.ctypes.data)), P_ld,
                                          _ffi.ptr(st), 0)
        assert rc == 0, _ffi.lib().sp_last_error()
        assert G.guards_intact(base, 1, nbins, rows=2, pitch=P_ld) and G.all_written(base, 1, nbins, rows=2, pitch=P_ld) and not st.any()
        want = E.pseudospectrum(V, w, 2, nbins, 0.1, 0.003, "ev", out64=out64)[0]
        assert want.dtype == inner.dtype and np.array_equal(bits(np.array(G.interior_of(base, 1, nbins, rows=2, pitch=P_ld))), bits(want))


@pytest.mark.parametrize("entry", ("sp_covmat", "sp_ar_ls"))
def test_refusals_and_bad_records_leave_the_outputs_untouched(entry):
    name = "frames"
    c = R.shape_of(name)
    xd = dev(R.signals(name))
    rows, nsig = xd.shape
    n, m, nf = c["n"], c["m"], c["nframes"]
    E._bind_stream(xd)
    lib = _ffi.lib()
    cov = entry == "sp_covmat"

    def call(xx=xd, n_=n, hop=c["hop"], first=c["first"], nf_=nf, m_=m, ld=None, det=_ffi.DETREND_SEGMEAN, fb=1):
        sizes = [(rows * nf * m * m, torch.complex128)] if cov else [(rows * nf * m, torch.float64), (rows * nf, torch.float64), (rows * nf, torch.int32)]
        bases = [G.sentinel_output(ne, dt, 1, device="cuda") for ne, dt in sizes]
        rec = (_ffi.ptr(xx.data_ptr()), _ffi.DTYPE_F32, nsig, nsig, rows, n_, hop, first, nf_)
        if cov:
            rc = lib.sp_covmat(*rec, m_, fb, det, 0.0, 0.0, _ffi.ptr(bases[0][1]), m * m if ld is None else ld, 1)
        else:
            rc = lib.sp_ar_ls(*rec, m_ - 1, fb, det, 0.0, 0.0, *[_ffi.ptr(b[1]) for b in bases], m if ld is None else ld, 1)
        torch.cuda.synchronize()
        assert all(G.guards_intact(b[0], 1, ne) for b, (ne, _) in zip(bases, sizes))
        untouched = all(bool((G._host_words(b[0]) == np.uint32(G.SENTINEL)).all()) for b in bases)
        return rc, (lib.sp_last_error() or b"").decode(), untouched

    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    big = ("m must" if cov else "order must")
    for kw, word in ((dict(m_=1, ld=100), big), (dict(m_=65, ld=5000), big), (dict(hop=0), "hop"), (dict(first=-1), "first"), (dict(nf_=nf + 1), "reach outside"),
                     (dict(ld=m - 1), "C_ld" if cov else "out_ld"), (dict(det=2), "detrend"), (dict(n_=1), "n must"), (dict(fb=2), "fb"),
                     (dict(n_=6, m_=7), "n / 2") if not cov else (dict(n_=6, m_=7), "exceed n")):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg.startswith(entry + ": ") and word in msg and untouched, (kw, rc, msg)
    for where in ((0, c["first"]), (rows - 1, c["first"] + (nf - 1) * c["hop"] + n - 1), (1, c["first"] + 150)):
        xn = xd.clone()
        xn[where] = float("nan") if where[0] else float("inf")
        rc, msg, untouched = call(xx=xn)
        assert rc == E.AR_BAD_RECORD == -2 and msg.startswith(entry + ": ") and "not finite" in msg and untouched, (where, rc, msg)
        with pytest.raises(E.SubRefused, match="not finite"):
            (E.covmat if cov else E.ar_ls)(xn, n, c["hop"], c["first"], nf, m if cov else m - 1)
    xn = xd.clone()
    xn[0, 0], xn[2, nsig - 1] = float("nan"), float("nan")                 # outside every segment: not looked at
    rc, msg, untouched = call(xx=xn)
    assert rc == 0 and not untouched


# ---- what was there before stays bit for bit ---------------------------------------------------------------------------------------
def test_existing_calls_are_unchanged():
    """arburg, aryule and ar_spectrogram with the default method against the bits the commit before the least-squares methods gave on an
    MI355X (tests/golden/ar_before_subspace.npz), against the engine entries they have always composed, and against the float64
    definitions within the allowances of tests/burg_ref.py"""
    x = B.signals("frames")
    before = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ar_before_subspace.npz"))
    now = dict(zip(("burg_a", "burg_e", "burg_k"), PM.arburg(x, 6)))
    now.update(zip(("yule_a", "yule_e", "yule_k"), PM.aryule(x, 6)))
    now.update(zip(("spec_f", "spec_t", "spec_S"), PM.ar_spectrogram(x[:, :413], 6, 100, noverlap=23, fs=2.0, nfft=64)))
    assert sorted(before.files) == sorted(now)
    for key in before.files:
        assert before[key].dtype == now[key].dtype and np.array_equal(bits(before[key]), bits(now[key])), key
    a, e, k = PM.arburg(x, 6)
    want = E.burg(x, x.shape[1], 1, 0, 1, 6, detrend=False)
    assert np.array_equal(bits(a), bits(want[0][:, 0])) and np.array_equal(bits(e), bits(want[1][:, 0, -1])) and np.array_equal(bits(k), bits(want[2][:, 0]))
    a, e, k = PM.aryule(x, 6)
    want = E.yule(x, x.shape[1], 1, 0, 1, 6, detrend=False)
    assert np.array_equal(bits(a), bits(want[0][:, 0])) and np.array_equal(bits(e), bits(want[1][:, 0, -1]))
    xs = x[:, :413]
    f, t, S = PM.ar_spectrogram(xs, 6, 100, noverlap=23, fs=2.0, nfft=64)
    f2, t2, S2 = PM.ar_spectrogram(xs, 6, 100, noverlap=23, method="burg", fs=2.0, nfft=64)
    ab, eb, _ = E.burg(xs, 100, 77, 0, 5, 6)
    P = E.ar_psd(ab, eb[..., -1], 33, 0.0, 1.0 / 64, 0.5)
    P[..., 1:32] *= 2
    assert np.array_equal(bits(S), bits(S2)) and np.array_equal(bits(S), bits(np.swapaxes(P, -1, -2)))
    ref = B.fit_def(xs, 100, 77, 0, 5, 6, "burg")
    assert max(B.deviations((ab, eb, E.burg(xs, 100, 77, 0, 5, 6)[2]), ref)) <= B.BURG_ALLOWANCE


def test_exported():
    assert pyfft_amd.pmusic is SS.pmusic and pyfft_amd.armcov is PM.armcov and pyfft_amd.esprit is SS.esprit
