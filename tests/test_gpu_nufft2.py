"""The type-2 NUFFT, the band-limited fit and regridding on the GPU (k_nufft2, sp_nufft2, pyfft_amd.nufft nufft2 / nufft_fit / regrid)
against the float64 sums of tests/nufft2_ref.py: every case of the type-1 tests with random modes, samples on and beside the tile seams
and the periodic end of the grid, a record piled into one cell and into one tile, both sides of the tile count a workgroup counts in
LDS, the row passes with their hook; a permutation of the samples permutes the outputs bit for bit; two calls and both memories agree
bitwise; the adjoint identity with nufft1; a record far from the time origin against exact phases; the modes convention; offset
pointers inside poisoned buffers with guarded, pitched outputs; refusals that leave the outputs alone; the fit against the float64
solve, clean, gapped, weighted with a ridge, cut short, with a row of zeros; regridding of a band-limited record."""
import numpy as np
import pytest
import torch            # a missing torch fails these tests, it does not skip them

import guard_ref as G
import nufft2_ref as R2
import nufft_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, nufft as NU

pytestmark = pytest.mark.gpu

USED, FIT_USED = {}, {}


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def run(name, sign, device=True, order=None):
    t, F, t_ref = R2.signals(name)
    f0, df = R2.grid_of(name)
    if order is not None:
        t = t[order]
    if device:
        return NU.nufft2(dev(t), dev(F), f0, df, sign=sign, t_ref=t_ref).cpu().numpy()
    return NU.nufft2(np.array(t), np.array(F), f0, df, sign=sign, t_ref=t_ref)


def plan_ref(M, rows, rows_force=0):
    """nufft_ref.plan_of with the interpolation kernel's own workgroup count: row groups of 4"""
    nf, w, tiles, tile, rpp, passes, _ = R.plan_of(M, rows, rows_force=rows_force)
    return nf, w, tiles, tile, rpp, passes, sum(tiles * -(-min(rpp, rows - r0) // 4) for r0 in range(0, rows, rpp)), 4


@pytest.mark.parametrize("name,sign", R2.CASES, ids=["%s%+d" % c for c in R2.CASES])
def test_shapes_against_the_direct_sums(name, sign, monkeypatch):
    s = R2.SHAPES[name]
    monkeypatch.delenv("SP_NUFFT_ROWS", raising=False)
    if name == "rows-17":
        monkeypatch.setenv("SP_NUFFT_ROWS", str(R.ROWS_HOOK))
    plan = NU.nufft_plan(s["N"], s["M"], s["rows"], type=2)
    assert tuple(plan[k] for k in ("nf", "width", "tiles", "tile", "rows_per_pass", "passes", "workgroups", "row_group")) == \
        plan_ref(s["M"], s["rows"], R.ROWS_HOOK if name == "rows-17" else 0)
    if name in ("tiles", "pile-tile"):
        assert plan["nf"] == 8192 and plan["tiles"] == 8
    if name == "long":
        assert plan["nf"] == 16384 > E.max_wg_fft()
    got = run(name, sign)
    assert got.shape == (s["rows"], s["N"]) and got.dtype == np.complex64
    assert E.last_passes(E.NUFFT_PASSES) == plan["passes"] == (9 if name == "rows-17" else 1)
    if name == "rows-17":
        assert not got[7].any()                  # a row of zeros comes back as exact zeros (of either sign: 0 x phase)
    USED[(name, sign)] = R2.assert_within(got, R2.reference(name, sign), R2.signals(name)[1], "%s %+d" % (name, sign))
    print("the device used at most %.3f of the allowance %.2e so far" % (max(USED.values()), R2.ALLOWANCE2))


def test_seams_and_piles_are_where_the_cases_say():
    """what the seam and pile cases are for, on the host: samples whose footprint starts on the first and on the last cell of a tile,
    ends on the tile's last cell, and wraps the periodic end; every sample of 'pile' in one cell, of 'pile-tile' in one tile"""
    t, _, t_ref = R2.signals("seams")
    f0, df = R2.grid_of("seams")
    nf, _, _, _, i0, dx = R._geometry(t, f0, df, R2.SHAPES["seams"]["M"], 1, t_ref)
    assert nf == 2048
    # footprints that start on the seam's cells and one on: exactly on the cell, an ulp under it (the same cell) and an ulp over (the next)
    assert {R.TILE - R.W, R.TILE - R.W + 1, R.TILE - R.W + 2, R.TILE, R.TILE + 1, R.TILE + 2} <= set(int(v) for v in i0)
    assert np.any(i0 % R.TILE == 0) and np.any((i0 + R.W - 1) % R.TILE == R.TILE - 1) and np.any((i0 + R.W - 1) % R.TILE == 0)
    assert np.any(i0 + R.W - 1 >= nf)                                             # a footprint that wraps the periodic end
    assert np.any(dx[i0 == R.TILE] < 1e-6) and np.any(dx[i0 == R.TILE + 1] > 1 - 1e-6)    # offsets at both ends of [0, 1]
    for name in ("pile", "pile-tile"):
        t, _, t_ref = R2.signals(name)
        f0, df = R2.grid_of(name)
        nf, _, _, _, i0, _ = R._geometry(t, f0, df, R2.SHAPES[name]["M"], 1, t_ref)
        if name == "pile":
            assert np.unique(i0).size == 1
        else:
            assert nf == 8192 and set(i0 // R.TILE) == set((i0 + R.W - 1) % nf // R.TILE) == {3}


@pytest.mark.parametrize("M", (1 << 20, (1 << 20) + 1))
def test_both_sides_of_the_tile_count_a_workgroup_counts_in_lds(M):
    """2048 tiles are counted per workgroup in LDS, 4096 go to the global counters directly: 64 samples and two rows keep the
    reference at 10^8 terms, summed in chunks of modes"""
    N, rows = 64, 2
    plan = NU.nufft_plan(N, M, rows, type=2)
    assert plan["tiles"] == (2048 if M == 1 << 20 else 4096)
    rng = np.random.default_rng(41)
    t = np.sort(rng.uniform(0.0, 100.0, N))
    F = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))).astype(np.complex64)
    f0, df = -3.0, 6.0 / M
    got = NU.nufft2(dev(t), dev(F), f0, df).cpu().numpy()
    ref = np.zeros((rows, N), dtype=np.complex128)
    for m0 in range(0, M, 1 << 16):
        m = np.arange(m0, min(M, m0 + (1 << 16)))
        p = (t - t[0])[:, None] * (f0 + df * m)[None, :]
        ref += F[:, m].astype(np.complex128) @ np.exp(2j * np.pi * (p - np.rint(p))).T
    R2.assert_within(got, ref, F, "M = %d" % M)
    order = rng.permutation(N)
    again = NU.nufft2(dev(t[order]), dev(F), f0, df, t_ref=float(t[0])).cpu().numpy()
    assert np.array_equal(np.ascontiguousarray(got[:, order]).view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("name", ("tails", "seams", "pile", "unsorted", "rows-17"))
def test_a_permutation_of_the_samples_permutes_the_outputs_bit_for_bit(name):
    sign = R2.SHAPES[name]["signs"][0]
    order = np.random.default_rng(99).permutation(R2.SHAPES[name]["N"])
    a, b = run(name, sign), run(name, sign, order=order)
    assert np.array_equal(np.ascontiguousarray(a[:, order]).view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", ("tails", "long", "rows-17"))
def test_two_calls_and_both_memories_agree_bitwise(name, monkeypatch):
    monkeypatch.delenv("SP_NUFFT_ROWS", raising=False)
    sign = R2.SHAPES[name]["signs"][0]
    a, b, h = run(name, sign), run(name, sign), run(name, sign, device=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), h.view(np.uint32))
    monkeypatch.setenv("SP_NUFFT_ROWS", "1")             # a row does not care which pass it is in
    assert np.array_equal(a.view(np.uint32), run(name, sign).view(np.uint32))


@pytest.mark.parametrize("name", ("tails", "tiles"))
def test_adjoint_of_nufft1(name):
    """<G, nufft1(c; -)> = <nufft2(G; +), c>: each side carries its own transform's allowance of sum|c| sum|G|"""
    t, c, t_ref = R.signals(name)
    f0, df = R.grid_of(name)
    M = R.SHAPES[name]["M"]
    c = c[0]
    G_ = R2.signals(name)[1][0]
    f1 = NU.nufft1(dev(t), dev(c), f0, df, M, sign=-1, t_ref=t_ref).cpu().numpy().astype(np.complex128)
    c2 = NU.nufft2(dev(t), dev(G_), f0, df, sign=1, t_ref=t_ref).cpu().numpy().astype(np.complex128)
    a = np.sum(np.conj(G_.astype(np.complex128)) * f1)
    b = np.sum(np.conj(c2) * c.astype(np.complex128))
    bound = (R.ALLOWANCE + R2.ALLOWANCE2) * np.sum(np.abs(c)) * np.sum(np.abs(G_))
    print("adjoint %s: |a - b| = %.3e of a bound of %.3e" % (name, abs(a - b), bound))
    assert abs(a - b) <= bound


def test_far_time_origin_against_exact_phases():
    rng = np.random.default_rng(5)
    N, M = 300, 40
    t0 = np.sort(rng.integers(0, 100 * 1024, N)) / 1024.0                 # multiples of 2^-10: exact beside 2^31
    t = t0 + 2.0 ** 31
    assert np.array_equal(t - 2.0 ** 31, t0)
    F = (rng.standard_normal((2, M)) + 1j * rng.standard_normal((2, M))).astype(np.complex64)
    f0, df = 0.0625, 0.0625                                               # dyadic: f0 + m df is exact
    ref = R2.direct2(t, F, f0, df, 1, exact=True)
    got = NU.nufft2(dev(t), dev(F), f0, df, t_ref=0.0).cpu().numpy()      # phases from the origin of t itself
    R2.assert_within(got, ref, F, "nufft2 at t + 2^31, t_ref 0")


def test_modes_convention():
    rng = np.random.default_rng(6)
    N, M = 200, 9
    x = rng.uniform(-10.0, 10.0, N)
    F = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    k = np.arange(M) - M // 2
    for sign in (1, -1):
        ref = (F.astype(np.complex128)[None, :] * np.exp(1j * sign * k[None, :] * x[:, None])).sum(axis=-1)
        got = pyfft_amd.nufft2_modes(dev(x), dev(F), sign=sign).cpu().numpy()
        assert got.shape == (N,)
        R2.assert_within(got[None], ref[None], F, "nufft2_modes sign %+d" % sign)
        assert np.array_equal(got, pyfft_amd.nufft2_modes(x, F, sign=sign))


# ---- offset pointers inside poisoned buffers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", range(8))
def test_calls_at_offset_pointers_with_guarded_outputs(lead):
    """t, F and out are 8-byte elements: both residues of each modulo 16 bytes, rows of F and out further apart than they are long"""
    name = "tails"
    t, F, t_ref = R2.signals(name)
    f0, df = R2.grid_of(name)
    rows, M = F.shape
    N, f_ld, o_ld = t.size, M + 5, t.size + 3
    lt, lf, lo = lead & 1, (lead >> 1) & 1, (lead >> 2) & 1
    tb, tv = G.poisoned_input(dev(t), lt)
    fb, fv = G.poisoned_input(dev(F), lf, pitch=f_ld)
    snaps = [G.snapshot(b) for b in (tb, fb)]
    got = E.nufft2(tv, fv, f0, df, t_ref=t_ref).cpu().numpy()
    assert np.all(np.isfinite(got.view(np.float32)))
    R2.assert_within(got, R2.reference(name, 1), F, "engine.nufft2 at lead %d" % lead)
    E._bind_stream(tv)
    ob, oa = G.sentinel_output(N, torch.complex64, lo, device="cuda", rows=rows, pitch=o_ld)
    rc = _ffi.lib().sp_nufft2(_ffi.ptr(tv.data_ptr()), _ffi.ptr(fv.data_ptr()), f_ld, N, rows, t_ref, f0, df, M, 1, _ffi.ptr(oa), o_ld, 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    torch.cuda.synchronize()
    assert all(G.unchanged(b, s) for b, s in zip((tb, fb), snaps))
    assert G.guards_intact(ob, lo, N, rows=rows, pitch=o_ld) and G.all_written(ob, lo, N, rows=rows, pitch=o_ld)     # the pad columns count as guards
    assert np.array_equal(G.interior_of(ob, lo, N, rows=rows, pitch=o_ld).cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_host_rows_further_apart_keep_their_pad_columns():
    name = "tails"
    t, F, t_ref = R2.signals(name)
    f0, df = R2.grid_of(name)
    rows, M = F.shape
    N, o_ld = t.size, t.size + 3
    tt, FF = np.array(t), np.array(F)
    ob, out = G.sentinel_output(N, np.complex64, 1, rows=rows, pitch=o_ld)
    _ffi.init()
    rc = _ffi.lib().sp_nufft2(_ffi.ptr(tt), _ffi.ptr(FF), M, N, rows, t_ref, f0, df, M, 1, _ffi.ptr(int(out.ctypes.data)), o_ld, 0)
    assert rc == 0, _ffi.lib().sp_last_error()
    assert G.guards_intact(ob, 1, N, rows=rows, pitch=o_ld) and G.all_written(ob, 1, N, rows=rows, pitch=o_ld)
    assert np.array_equal(np.array(G.interior_of(ob, 1, N, rows=rows, pitch=o_ld)).view(np.uint32), run(name, 1).view(np.uint32))


def test_refusals_leave_the_outputs_untouched():
    name = "tails"
    t, F, t_ref = R2.signals(name)
    f0, df = R2.grid_of(name)
    rows, M = F.shape
    N = t.size
    td, Fd = dev(t), dev(F)
    E._bind_stream(td)
    lib = _ffi.lib()

    def call(tt=td, ff=Fd, n=N, fld=M, old=N, m=M, tr=t_ref, a=f0, b=df, sg=1):
        ob, oa = G.sentinel_output(rows * N, torch.complex64, 1, device="cuda")
        rc = lib.sp_nufft2(_ffi.ptr(tt.data_ptr()), _ffi.ptr(ff.data_ptr()), fld, n, rows, tr, a, b, m, sg, _ffi.ptr(oa), old, 1)
        torch.cuda.synchronize()
        assert G.guards_intact(ob, 1, rows * N)
        untouched = bool((G._host_words(ob) == np.uint32(G.SENTINEL)).all())
        return rc, (lib.sp_last_error() or b"").decode(), untouched

    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    for kw, word in ((dict(n=0), "N must"), (dict(fld=M - 1), "F_ld"), (dict(old=N - 1), "out_ld"), (dict(m=0), "M must"),
                     (dict(tr=float("nan")), "t_ref"), (dict(a=float("inf")), "f0"), (dict(b=0.0), "df"), (dict(b=float("nan")), "df"),
                     (dict(sg=0), "sign")):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg.startswith("sp_nufft2: ") and word in msg and untouched, (kw, rc, msg)
    tn, Fn = td.clone(), Fd.clone()
    tn[N // 2], Fn[1, 100] = float("inf"), complex(0.0, float("nan"))
    for kw, word in ((dict(tt=tn), "t holds"), (dict(ff=Fn), "F holds")):
        rc, msg, untouched = call(**kw)
        assert rc == E.NUFFT_BAD_RECORD == -2 and msg.startswith("sp_nufft2: ") and word in msg and untouched, (rc, msg)
    bad = [lambda: E.nufft2(tn, Fd, f0, df), lambda: E.nufft2(td, Fn, f0, df), lambda: E.nufft2(td, Fd.to(torch.complex128), f0, df),
           lambda: E.nufft2(td.float(), Fd, f0, df)]
    for fn in bad:
        with pytest.raises(E.NufftRefused) as exc:
            fn()
        assert isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)
    # and the library still works
    assert np.array_equal(run(name, 1).view(np.uint32), run(name, 1).view(np.uint32))
    R2.assert_within(run(name, 1), R2.reference(name, 1), F, "after the refusals")


# ---- the fit and regridding ------------------------------------------------------------------------------------------------------
def fit_within(got, ref, what):
    used = R2.fit_deviation(got, ref) / R2.FIT_ALLOWANCE
    print("%s: ||F - fit_def|| / ||fit_def|| at %.3f of its allowance %.2e" % (what, used, R2.FIT_ALLOWANCE))
    assert used <= 1.0, (what, used)
    return used


@pytest.mark.parametrize("name", R2.FIT_CASES)
def test_fit_against_the_float64_solve(name):
    t, y, _ = R2.fit_signals(name)
    f0, df, M = R2.fit_grid()
    assert t.size == (400 if name == "clean" else 387)
    fit = NU.nufft_fit(dev(t), dev(y), f0, df, M, t_ref=0.0)
    assert isinstance(fit, NU.NufftFit) and fit.F.dtype == torch.complex64 and tuple(fit.F.shape) == (M,)
    print("%s: %d iterations (float64: %d), residual %.3e" % (name, fit.iterations, R2.FIT_ITERATIONS[name][0], float(fit.residual)))
    assert fit.converged is True and fit.iterations <= R2.FIT_ITERATIONS[name][1] == (8 if name == "clean" else 16)
    FIT_USED[name] = fit_within(fit.F.cpu().numpy(), R2.fit_def(t, y, f0, df, M), name)
    # the residual is the fit's own: the weighted rms of y - nufft2(F)
    back = NU.nufft2(dev(t), fit.F, f0, df, t_ref=0.0).cpu().numpy()
    assert abs(float(fit.residual) - np.sqrt(np.mean(np.abs(y.astype(np.complex128) - back.astype(np.complex128)) ** 2))) <= 1e-6 * np.sqrt(np.mean(np.abs(y) ** 2))
    host = NU.nufft_fit(np.array(t), np.array(y), f0, df, M, t_ref=0.0)           # numpy in, numpy out, the same bits
    assert isinstance(host.F, np.ndarray) and np.array_equal(host.F.view(np.uint32), fit.F.cpu().numpy().view(np.uint32))


def test_fit_with_weights_and_a_ridge_cut_short_and_with_a_row_of_zeros():
    t, y, _ = R2.fit_signals("gapped")
    f0, df, M = R2.fit_grid()
    w = np.random.default_rng(8).uniform(0.5, 1.5, t.size)
    fit = NU.nufft_fit(dev(t), dev(y), f0, df, M, weights=dev(w), ridge=1e-3, t_ref=0.0)
    assert fit.converged
    FIT_USED["weights"] = fit_within(fit.F.cpu().numpy(), R2.fit_def(t, y, f0, df, M, w, 1e-3), "weights and a ridge of 1e-3")
    short = NU.nufft_fit(dev(t), dev(y), f0, df, M, maxiter=2, t_ref=0.0)
    assert short.converged is False and short.iterations == 2 and np.all(np.isfinite(short.F.cpu().numpy().view(np.float32)))
    two = np.stack([y, np.zeros_like(y)])
    both = NU.nufft_fit(dev(t), dev(two), f0, df, M, t_ref=0.0)
    assert both.converged and tuple(both.F.shape) == (2, M) and tuple(both.residual.shape) == (2,)
    assert not both.F[1].cpu().numpy().any() and float(both.residual[1]) == 0.0
    fit_within(both.F[0].cpu().numpy(), R2.fit_def(t, y, f0, df, M), "beside a row of zeros")


def test_regrid_of_a_band_limited_record():
    rng = np.random.default_rng(9)
    N, period = 400, 100.0
    h = period / N
    t = (np.arange(N) + rng.uniform(-0.45, 0.45, N)) * h
    t[0], t[-1] = 0.0, period - h                           # the span closes the circle: the default period is `period`
    lines = ((0.05, 1.0, 0.3), (0.17, 0.6, -1.1), (0.31, 0.8, 2.0))       # harmonics of 1 / period below fmax
    fmax = 0.4
    signal = lambda tt: sum(a * np.cos(2 * np.pi * f * tt + ph) for f, a, ph in lines) + 0.25
    y = signal(t).astype(np.float32)
    t_new = t.min() + (t.max() - t.min()) * (np.arange(256) + 0.5) / 256          # uniform, strictly inside the span
    vals, fit = NU.regrid(dev(t), dev(y), dev(t_new), fmax, return_fit=True)
    assert vals.dtype == torch.float32 and tuple(vals.shape) == (256,) and fit.converged
    assert tuple(fit.F.shape) == (81,) and NU.regrid_grid(t.min(), t.max(), N, fmax)[:3] == (pytest.approx(period, rel=1e-14), 40, 81)
    sumF = float(fit.F.abs().sum())
    err = float(np.max(np.abs(vals.cpu().numpy() - signal(t_new))))
    print("regrid: worst value off by %.3e of sum|F| = %.3f, bound %.3e" % (err / sumF, sumF, R2.FIT_ALLOWANCE))
    assert err <= R2.FIT_ALLOWANCE * sumF
    host = NU.regrid(np.array(t), np.array(y), t_new, fmax)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host, vals.cpu().numpy())
    z = NU.regrid(dev(t), dev((y + 0j).astype(np.complex64)), dev(t_new), fmax)
    assert z.dtype == torch.complex64
    for bad in (lambda: NU.regrid(dev(t), dev(y), dev(np.append(t_new, t.max() + 1e-3)), fmax),
                lambda: NU.regrid(dev(t), dev(y), dev(np.append(t.min() - 1e-3, t_new)), fmax),
                lambda: NU.regrid(dev(t), dev(y), dev(t_new), 2.01)):              # K = 201, M = 403 > N = 400
        with pytest.raises(NU.NufftRefused):
            bad()
    with pytest.raises(NU.NufftRefused, match="more unknowns than samples"):
        NU.regrid(dev(t), dev(y), dev(t_new), 2.01)
