"""The cross-wavelet transform and the wavelet coherence on the GPU (k_wct_time, k_wct_scale, sp_wct_time, sp_wct_scale, engine.wct_time /
wct_scale, pyfft_amd.wavelet.xwt / wct) against the float64 reference of tests/wct_ref.py.

One case per frame length L, the smallest shapes at which each kernel form can go wrong: 256 (16 transform groups per workgroup), 1024
(one wave per group), 2048 (the first stashed size, two waves per group), 4096 and 8192 (one group of 512 threads, the largest LDS).
The scale sets start at 3.8 samples, four per octave, and fill 4 M <= L; records of 2 hop + 37 samples and one of hop - 5.

Tolerances.  eps of a case is what the float32 restatement of the same plan in wct_ref.py (complex64 transforms, the filter and the
Gaussian from float32 constants) loses against the float64 reference, as the largest error of A_t, B_t or C_t over its row's rms; it
is computed with the case and must lie between 0 and LOSS_MAX.  Measured on the CPU, real / complex records:
    L = 256: 1.6e-6 / 1.8e-6    1024: 2.7e-6 / 2.5e-6    2048: 2.2e-6 / 2.5e-6    4096: 3.3e-6 / 2.6e-6    8192: 2.9e-6 / 9.2e-6
(the larger of the one- and two-row cases; the whole-record path of the mixed cases 6.0e-5 and 4.6e-5, bound LOSS_MAX_COMPOSED).
Measured on an MI355X in those units: T at 0.33 .. 1.76 losses, Wxy at 1.0 .. 1.8, R2 at 0.4 .. 1.8 % of its bound.
The device's T, A, B and C are held to 2 eps of the row rms (the 2: a different but equally valid order of float32 operations), R2 to the
propagated bound 4 delta + delta^2 of wct_ref.r2_bound, the phase to asin(2 eps rms_C / |C|) where that is below 30 degrees.  The
reference must have no point with A or B below 0.05 of its row mean (wct_ref.assert_conditioned: a condition on the records, which is
why a case names its seed); every point is compared."""
import functools
import math

import numpy as np
import pytest

import cwt_ref as R
import guard_ref as G
import wct_ref as Q
from pyfft_amd import _ffi, engine as E, wavelet as WV

pytestmark = pytest.mark.gpu

DJ = 0.25
LOSS_MAX = 2e-5
LOSS_MAX_COMPOSED = 1e-4         # the whole-record path: complex64 transforms of 16384 points and more, as tests/test_gpu_wavelet.py
# L -> (top scale in samples, seed of the real records, seed of the complex records)
SETS = {256: (6.4, 266, 266), 1024: (25.0, 1034, 1034), 2048: (50.0, 2058, 2058), 4096: (100.0, 4106, 4106), 8192: (205.0, 8202, 8202)}
LS = sorted(SETS)
WIN = Q.scale_window(DJ)


@pytest.fixture(scope="module")
def torch():
    import torch
    _ffi.init()
    return torch


@functools.lru_cache(maxsize=None)
def plan_of(L):
    s0 = 3.8
    scales = s0 * 2 ** (np.arange(int(math.log2(SETS[L][0] / s0) * 4) + 1) / 4.0)
    plan = WV.wct_plan(1000, scales=scales)
    assert plan["L"] == L and plan["fused"].all() and 4 * plan["M"] <= L, (L, plan["L"], plan["M"])
    return plan


@functools.lru_cache(maxsize=None)
def case_of(L, cplx, short=False, rows=1):
    """-> (x, y [rows, n], plan, references (one dict per row), eps): computed once and shared, read-only."""
    plan = plan_of(L)
    n = plan["hop"] - 5 if short else 2 * plan["hop"] + 37
    pairs = [Q.make_pair(n, cplx, SETS[L][2 if cplx else 1] + 1000 * r) for r in range(rows)]
    x, y = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    refs, loss = [], 0.0
    for r in range(rows):
        ref = Q.wct_ref(x[r], y[r], plan["scales"], 6.0, DJ)
        Q.assert_conditioned(ref)
        T32 = Q.overlap_save(x[r], y[r], plan["scales"], 6.0, L, plan["Mw"], plan["Mg"], np.float32)
        loss = max(loss, *Q.component_errs(T32, ref["T"]))
        refs.append(ref)
    print("L=%d n=%d %s: the float32 restatement loses %.3g" % (L, n, "complex" if cplx else "real", loss))
    assert 0 < loss <= LOSS_MAX
    for a in (x, y):
        a.setflags(write=False)
    return x, y, plan, refs, loss


def as_dict(T, out):
    h = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v                        # noqa: E731
    return dict(T=h(T), R2=h(out[0]), phase=h(out[1]), A=h(out[2]), B=h(out[3]), C=h(out[4]))


def run(x, y, plan):
    T = E.wct_time(x, y, plan["scales"], "morlet", 6.0, plan["L"], plan["Mw"], plan["Mg"])
    return as_dict(T, E.wct_scale(T, WIN, spectra=True))


def check_T(T, ref, eps2, what):
    errs = Q.component_errs(T, ref["T"])
    print("%s T: A_t %.3g, B_t %.3g, C_t %.3g of the row rms (bound %.3g)" % ((what,) + errs + (eps2,)))
    assert np.all(np.isfinite(T)) and max(errs) <= eps2, (what, errs, eps2)


@pytest.mark.parametrize("mode", ["numpy", "device"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("L", LS)
def test_coherence_against_reference(torch, L, cplx, mode):
    rows = 2 if mode == "device" else 1
    x, y, plan, refs, eps = case_of(L, cplx, rows=rows)
    if mode == "numpy":
        got = run(x[0], y[0], plan)
        assert got["T"].dtype == np.float32 and got["T"].shape == refs[0]["T"].shape and got["C"].dtype == np.complex64
        check_T(got["T"], refs[0], 2 * eps, "L=%d" % L)
        Q.check(got, refs[0], 2 * eps, "L=%d" % L)
    else:
        n = x.shape[-1]
        _, xv = G.poisoned_input(torch.as_tensor(x, device="cuda"), 1, pitch=n + 3)          # row-strided, off alignment
        _, yv = G.poisoned_input(torch.as_tensor(y, device="cuda"), 3 if not cplx else 1, pitch=n + 5)
        got = run(xv, yv, plan)
        assert tuple(got["R2"].shape) == (rows,) + refs[0]["R2"].shape
        for r in range(rows):
            check_T(got["T"][r], refs[r], 2 * eps, "L=%d row %d" % (L, r))
            Q.check({k: v[r] for k, v in got.items()}, refs[r], 2 * eps, "L=%d row %d" % (L, r))


@pytest.mark.parametrize("L,cplx", [(256, False), (2048, True), (8192, False)])
def test_short_record(torch, L, cplx):
    """N = hop - 5: one partial frame."""
    x, y, plan, refs, eps = case_of(L, cplx, short=True)
    got = run(x[0], y[0], plan)
    check_T(got["T"], refs[0], 2 * eps, "short L=%d" % L)
    Q.check(got, refs[0], 2 * eps, "short L=%d" % L)


@pytest.mark.parametrize("L", [256, 4096])
def test_self_coherence(torch, L):
    """wct(x, x): R2 = 1 within the bound, the phase 0."""
    x, _, plan, _, _ = case_of(L, False)
    x = x[0]
    ref = Q.wct_ref(x, x, plan["scales"], 6.0, DJ)
    eps = max(Q.component_errs(Q.overlap_save(x, x, plan["scales"], 6.0, L, plan["Mw"], plan["Mg"], np.float32), ref["T"]))
    assert 0 < eps <= LOSS_MAX and np.max(np.abs(ref["R2"] - 1)) <= 1e-12
    got = run(x, x, plan)
    Q.check(got, ref, 2 * eps, "self L=%d" % L)
    bound, _ = Q.r2_bound(ref, 2 * eps)
    assert np.all(np.abs(got["R2"] - 1) <= bound + 1e-12)


WAVELETS = {"morlet": WV.Morlet(6.0), "paul": WV.Paul(4)}
XSETS = {("morlet", 256): (13.0, 1e-6), ("morlet", 2048): (104.0, 1e-6), ("morlet", 8192): (418.0, 1e-6), ("paul", 1024): (18.0, 1e-5),
         ("paul", 4096): (41.0, 1e-6)}


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("family,L", sorted(XSETS), ids=["%s-%d" % c for c in sorted(XSETS)])
def test_xwt_against_reference(torch, family, L, cplx):
    """Wxy against xwt_ref; eps is what the product of the two float32 restatements of tests/cwt_ref.py loses."""
    top, tail = XSETS[(family, L)]
    wv = WAVELETS[family]
    s0 = WV.smallest_fused_scale(wv, tail)
    scales = s0 * 2 ** (np.arange(int(math.log2(top / s0) * 4) + 1) / 4.0)
    plan = WV.cwt_plan(1000, wavelet=wv, scales=scales, tail=tail)
    assert plan["L"] == L and plan["fused"].all()
    n = 2 * plan["hop"] + 37
    x, y = Q.make_pair(n, cplx, 40 + L)
    ref = Q.xwt_ref(x, y, scales, family, wv.param)
    f32 = (R.overlap_save(x, scales, family, wv.param, L, plan["M"], np.float32)
           * np.conj(R.overlap_save(y, scales, family, wv.param, L, plan["M"], np.float32)))
    eps = Q.row_err(f32, ref)
    print("xwt %s L=%d: the float32 restatement loses %.3g" % (family, L, eps))
    assert 0 < eps <= 2e-4
    W, sc, freqs, coi = WV.xwt(x, y, wavelet=wv, scales=scales, tail=tail)
    assert W.dtype == np.complex64 and W.shape == ref.shape and coi.shape == (n,)
    np.testing.assert_allclose(freqs, 1.0 / (wv.flambda() * scales), rtol=1e-14)
    err = Q.row_err(W, ref)
    print("xwt %s L=%d: %.3g of the row rms (bound %.3g)" % (family, L, err, 2 * eps))
    assert np.all(np.isfinite(W)) and err <= 2 * eps
    Wd = WV.xwt(torch.as_tensor(x, device="cuda"), torch.as_tensor(y, device="cuda"), wavelet=wv, scales=scales, tail=tail)[0]
    assert Wd.is_cuda and np.array_equal(Wd.cpu().numpy(), W)
    if family == "morlet":
        Wx, Wy = (E.cwt(v, scales, family, wv.param, L, plan["M"])["W"] for v in (x, y))
        assert Q.row_err(W, (Wx.astype(np.complex128) * np.conj(Wy))) <= 2 * eps


def mixed_case(scales, n, seed):
    """-> (x, y, plan, ref, eps) for the public wct over a scale set that takes both paths (or the composed one alone)"""
    x, y = Q.make_pair(n, False, seed)
    plan = WV.wct_plan(n, dj=DJ, scales=scales)
    ref = Q.wct_ref(x, y, scales, 6.0, DJ)
    Q.assert_conditioned(ref)
    f, c = plan["fused"], ~plan["fused"]
    T32 = np.zeros(ref["T"].shape, dtype=np.float32)
    if f.any():
        T32[f] = Q.overlap_save(x, y, scales[f], 6.0, plan["L"], plan["Mw"], plan["Mg"], np.float32)
    T32[c] = Q.composed_f32(x, y, scales[c], 6.0, plan["n_smooth"])
    eps = max(Q.component_errs(T32, ref["T"]))
    print("both paths, n=%d: the float32 restatement loses %.3g" % (n, eps))
    assert 0 < eps <= LOSS_MAX_COMPOSED
    return x, y, plan, ref, eps


def public(x, y, scales):
    out = WV.wct(x, y, dj=DJ, scales=scales, return_spectra=True)
    h = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v                        # noqa: E731
    return dict(R2=h(out[0]), phase=h(out[1]), A=h(out[5]), B=h(out[6]), C=h(out[7])), out


def test_mixed_paths(torch):
    """Scales from 2.6 samples (where the Nyquist cut spoils the wavelet's decay) to 560 (margins above 3072): composed rows below and
    above the fused ones, smoothed across both seams in one wct_scale call."""
    n = 5000
    scales = 2.6 * 2 ** (np.arange(32) / 4.0)
    x, y, plan, ref, eps = mixed_case(scales, n, 77)
    path = list(plan["path"])
    assert path[:2] == ["composed"] * 2 and path[-2:] == ["composed"] * 2 and "fused" in path and plan["n_full"] == 16384
    got, out = public(x, y, scales)
    assert out[0].dtype == np.float32 and out[0].shape == (len(scales), n) and out[3].shape == (len(scales),) and out[4].shape == (n,)
    Q.check(got, ref, 2 * eps, "both paths")
    seam = np.nonzero(np.diff(plan["fused"].astype(int)))[0]
    rows = np.unique(np.clip(np.concatenate([seam + d for d in range(-3, 5)]), 0, len(scales) - 1))
    Q.check({k: v[rows] for k, v in got.items()}, {k: v[rows] for k, v in ref.items()}, 2 * eps, "rows at the seams")
    gd, _ = public(torch.as_tensor(x, device="cuda"), torch.as_tensor(y, device="cuda"), scales)
    for k in got:
        assert np.array_equal(gd[k], got[k]), k


def test_mixed_paths_batched_with_numpy_glue(torch, monkeypatch):
    """Two rows, and the module's torch taken away: numpy records then take the library's host path with numpy glue between the calls
    (what a caller without torch gets).  Both rows against their references across both seams; against the device mode to the same
    bounds, not bit for bit."""
    n = 3000
    scales = 2.6 * 2 ** (np.arange(30) / 4.0)
    cases = [mixed_case(scales, n, seed) for seed in (77, 79)]
    plan = cases[0][2]
    assert (~plan["fused"]).sum() >= 4 and plan["fused"].any() and not plan["fused"][0] and not plan["fused"][-1]
    x, y = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    monkeypatch.setattr(WV, "torch", None)
    got, out = public(x, y, scales)
    assert isinstance(out[0], np.ndarray) and out[0].shape == (2, len(scales), n) and out[7].dtype == np.complex64
    for r, (_, _, _, ref, eps) in enumerate(cases):
        Q.check({k: v[r] for k, v in got.items()}, ref, 2 * eps, "numpy glue row %d" % r)
    W, _, _, _ = WV.xwt(x, y, scales=scales)
    for r in range(2):
        xref = Q.xwt_ref(x[r], y[r], scales)
        f, c = plan["fused"], ~plan["fused"]
        w32 = np.zeros(xref.shape, dtype=np.complex64)
        pw = WV.cwt_plan(n, scales=scales)
        fw = pw["fused"]
        w32[fw] = (R.overlap_save(x[r], scales[fw], "morlet", 6.0, pw["L"], pw["M"], np.float32)
                   * np.conj(R.overlap_save(y[r], scales[fw], "morlet", 6.0, pw["L"], pw["M"], np.float32)))
        w32[~fw] = R.composed_f32(x[r], scales[~fw], "morlet", 6.0) * np.conj(R.composed_f32(y[r], scales[~fw], "morlet", 6.0))
        xeps = Q.row_err(w32, xref)
        err = Q.row_err(W[r], xref)
        print("numpy glue xwt row %d: %.3g of the row rms (the float32 restatement loses %.3g)" % (r, err, xeps))
        assert 0 < xeps <= 2e-4 and err <= 2 * xeps


def test_composed_only(torch):
    n = 3000
    scales = 330.0 * 2 ** (np.arange(4) / 4.0)
    x, y, plan, ref, eps = mixed_case(scales, n, 78)
    assert not plan["fused"].any() and plan["L"] is None
    got, out = public(x, y, scales)
    assert len(WV.wct(x, y, dj=DJ, scales=scales)) == 5
    Q.check(got, ref, 2 * eps, "composed alone")


@pytest.mark.parametrize("K", [1, 7, 8, 12, 16, 17, 21])
def test_scale_kernel_forms(torch, K):
    """k_wct_scale keeps up to 8 or up to 16 rows in registers and re-reads them beyond: every form against the float64 sum of the
    same T.  A sum of K float32 products by fma loses at most K 2^-24 of the sum of their magnitudes; R2 follows from the device's own
    A, B, C in float32 (two products, a sum, a product and a quotient: 6 roundings)."""
    x, y, plan, refs, eps = case_of(1024, True)
    T = E.wct_time(x[0], y[0], plan["scales"], "morlet", 6.0, 1024, plan["Mw"], plan["Mg"])
    win = (np.arange(1, K + 1) / (K * (K + 1) / 2.0)).astype(np.float32)           # not symmetric: the orientation shows
    R2, phase, A, B, C = E.wct_scale(T, win, spectra=True)
    T64, w64 = T.astype(np.float64), win.astype(np.float64)
    want = Q.smooth_scale(T64, w64)
    tol = K * 2.0 ** -24 * Q.smooth_scale(np.abs(T64), w64)
    got = np.stack([A, B, C.real, C.imag], axis=-1)
    assert np.all(np.abs(got - want) <= tol)
    r2 = (C.real.astype(np.float64) ** 2 + C.imag.astype(np.float64) ** 2) / (A.astype(np.float64) * B)
    assert np.all(np.abs(R2 - r2) <= 6 * 2.0 ** -24 * r2)
    assert np.max(np.abs(np.angle(np.exp(1j * (phase - np.arctan2(C.imag.astype(np.float64), C.real)))))) <= 1e-6


@pytest.mark.parametrize("L,cplx", [(1024, False), (8192, True)])
def test_modes_and_runs_agree_bitwise(torch, L, cplx, monkeypatch):
    x, y, plan, refs, eps = case_of(L, cplx)
    a = run(x[0], y[0], plan)
    b = run(x[0], y[0], plan)
    d = run(torch.as_tensor(x[0], device="cuda"), torch.as_tensor(y[0], device="cuda"), plan)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k]), k
    # T does not depend on how the scales are dealt to workgroups
    S = len(plan["scales"])
    for chunk in ("1", "3", str(S)):
        monkeypatch.setenv("SP_WCT_CHUNK", chunk)
        assert E.wct_plan(x.shape[-1], S, L, plan["Mw"], plan["Mg"])["chunk"] == int(chunk)
        T = E.wct_time(x[0], y[0], plan["scales"], "morlet", 6.0, L, plan["Mw"], plan["Mg"])
        assert np.array_equal(T, a["T"]), chunk
    monkeypatch.delenv("SP_WCT_CHUNK")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_nothing_written_beyond_the_outputs(torch, cplx):
    """Device-resident, through the C entries: poisoned inputs at offset pointers, sentinel-filled outputs at offset pointers (T 16 bytes
    past the guard: it must keep its alignment).  The last, partial frame writes every sample below N and nothing at or beyond it."""
    L = 1024
    x, y, plan, refs, eps = case_of(L, cplx)
    ref, sc = refs[0], np.ascontiguousarray(plan["scales"])
    S, n = len(sc), x.shape[-1]
    assert n % plan["hop"] not in (0, plan["hop"] - 1)
    xb, xv = G.poisoned_input(torch.as_tensor(x[0], device="cuda"), 1)
    yb, yv = G.poisoned_input(torch.as_tensor(y[0], device="cuda"), 1 if cplx else 3)
    snaps = G.snapshot(xb), G.snapshot(yb)
    E._bind_stream(xv)
    lib = _ffi.lib()
    Tb, Tp = G.sentinel_output(S * n * 4, torch.float32, 4, device="cuda")
    _ffi.check(lib.sp_wct_time(_ffi.ptr(xv.data_ptr()), n, _ffi.ptr(yv.data_ptr()), n, int(cplx), n, 1, _ffi.ptr(sc), S, 0, 6.0, L,
                               plan["Mw"], plan["Mg"], _ffi.ptr(Tp), None, 1))
    outs = {"R2": (S * n, torch.float32, 1), "phase": (S * n, torch.float32, 3), "A": (S * n, torch.float32, 2), "B": (S * n, torch.float32, 1),
            "C": (S * n, torch.complex64, 1)}
    held = {k: G.sentinel_output(nel, dt, lead, device="cuda") for k, (nel, dt, lead) in outs.items()}
    taps = WIN.astype(np.float32)
    _ffi.check(lib.sp_wct_scale(_ffi.ptr(Tp), n, S, 1, _ffi.ptr(taps), len(taps), *[_ffi.ptr(held[k][1]) for k in outs], 1))
    Wb, Wp = G.sentinel_output(S * n, torch.complex64, 1, device="cuda")
    pw = WV.cwt_plan(n, scales=sc)
    _ffi.check(lib.sp_wct_time(_ffi.ptr(xv.data_ptr()), n, _ffi.ptr(yv.data_ptr()), n, int(cplx), n, 1, _ffi.ptr(sc), S, 0, 6.0, pw["L"],
                               pw["M"], 0, None, _ffi.ptr(Wp), 1))
    torch.cuda.synchronize()
    assert G.unchanged(xb, snaps[0]) and G.unchanged(yb, snaps[1])
    assert G.guards_intact(Tb, 4, S * n * 4) and G.first_unwritten(Tb, 4, S * n * 4) is None
    assert G.guards_intact(Wb, 1, S * n) and G.first_unwritten(Wb, 1, S * n) is None
    for k, (nel, dt, lead) in outs.items():
        assert G.guards_intact(held[k][0], lead, nel), k
        assert G.first_unwritten(held[k][0], lead, nel) is None, k
    T = G.interior_of(Tb, 4, S * n * 4).cpu().numpy().reshape(S, n, 4)
    check_T(T, ref, 2 * eps, "T at an offset pointer")
    got = {k: G.interior_of(held[k][0], lead, nel).cpu().numpy().reshape(S, n) for k, (nel, dt, lead) in outs.items()}
    Q.check(got, ref, 2 * eps, "outputs at offset pointers")
    Wxy = G.interior_of(Wb, 1, S * n).cpu().numpy().reshape(S, n)
    xref = Q.xwt_ref(x[0], y[0], sc)
    xeps = Q.row_err(R.overlap_save(x[0], sc, "morlet", 6.0, pw["L"], pw["M"], np.float32)
                     * np.conj(R.overlap_save(y[0], sc, "morlet", 6.0, pw["L"], pw["M"], np.float32)), xref)
    assert np.all(np.isfinite(Wxy)) and 0 < xeps <= 2e-4 and Q.row_err(Wxy, xref) <= 2 * xeps
    # the alignment rule is a refusal, not a fault
    assert lib.sp_wct_time(_ffi.ptr(xv.data_ptr()), n, _ffi.ptr(yv.data_ptr()), n, int(cplx), n, 1, _ffi.ptr(sc), S, 0, 6.0, L, plan["Mw"],
                           plan["Mg"], _ffi.ptr(Tp + 4), None, 1) < 0
