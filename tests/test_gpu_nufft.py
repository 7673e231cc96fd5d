"""The type-1 NUFFT and the fast Lomb-Scargle periodogram on the GPU (k_nufft, sp_nufft1, sp_lomb_sums_grid, pyfft_amd.nufft,
pyfft_amd.lomb method='fast') against the float64 direct sums of tests/nufft_ref.py: tails, several tiles, the multi-pass transform,
samples on and beside the tile seams and the periodic end of the grid, a record piled into one cell and into one tile, times in any
order, a record far from the time origin against an exact-phase reference, the row passes with their hook, the edges of M, N, f0 and
df; a permutation of the samples changes no bit; two calls and both memories agree bitwise; the Lomb sums, their finish in every form,
fast against direct, parts that add up, the spectral window; offset pointers inside poisoned buffers with guarded outputs; refusals
that leave the outputs alone."""
import numpy as np
import pytest
import torch            # a missing torch fails these tests, it does not skip them

import guard_ref as G
import lomb_ref as L
import nufft_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, lomb as LS, nufft as NU

pytestmark = pytest.mark.gpu

USED, LS_USED = {}, {}


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def run(name, sign, device=True, order=None):
    t, c, t_ref = R.signals(name)
    f0, df = R.grid_of(name)
    M = R.SHAPES[name]["M"]
    if order is not None:
        t, c = t[order], c[:, order]
    if device:
        return NU.nufft1(dev(t), dev(c), f0, df, M, sign=sign, t_ref=t_ref).cpu().numpy()
    return NU.nufft1(np.array(t), np.array(c), f0, df, M, sign=sign, t_ref=t_ref)


@pytest.mark.parametrize("name,sign", R.CASES, ids=["%s%+d" % c for c in R.CASES])
def test_shapes_against_the_direct_sums(name, sign, monkeypatch):
    s = R.SHAPES[name]
    monkeypatch.delenv("SP_NUFFT_ROWS", raising=False)
    if name == "rows-17":
        monkeypatch.setenv("SP_NUFFT_ROWS", str(R.ROWS_HOOK))
    plan = NU.nufft_plan(s["N"], s["M"], s["rows"])
    assert (plan["nf"], plan["width"], plan["tiles"], plan["tile"], plan["rows_per_pass"], plan["passes"], plan["workgroups"]) == \
        R.plan_of(s["M"], s["rows"], rows_force=R.ROWS_HOOK if name == "rows-17" else 0)
    if name in ("tiles", "pile-tile"):
        assert plan["nf"] == 8192 and plan["tiles"] == 8
    if name == "long":
        assert plan["nf"] == 16384 > E.max_wg_fft()
    got = run(name, sign)
    assert got.shape == (s["rows"], s["M"]) and got.dtype == np.complex64
    assert E.last_passes(E.NUFFT_PASSES) == plan["passes"] == (9 if name == "rows-17" else 1)
    if name == "rows-17":
        assert not got[7].any()                  # a row of zeros comes back as zeros
    USED[(name, sign)] = R.assert_within(got, R.reference(name, sign), R.signals(name)[1], "%s %+d" % (name, sign))
    print("the device used at most %.3f of the allowance %.2e so far" % (max(USED.values()), R.ALLOWANCE))


def test_pile_fills_one_cell_and_one_tile():
    """what the pile cases are for: every sample of 'pile' in one cell, every sample of 'pile-tile' inside one tile"""
    for name in ("pile", "pile-tile"):
        t, _, t_ref = R.signals(name)
        f0, df = R.grid_of(name)
        nf, _, _, _, i0, _ = R._geometry(t, f0, df, R.SHAPES[name]["M"], 1, t_ref)
        if name == "pile":
            assert np.unique(i0).size == 1
        else:
            assert nf == 8192 and set(i0 // R.TILE) == set((i0 + R.W - 1) % nf // R.TILE) == {3}


@pytest.mark.parametrize("M", (1 << 20, (1 << 20) + 1))
def test_both_sides_of_the_tile_count_a_workgroup_counts_in_lds(M):
    """2048 tiles are counted per workgroup in LDS before they reach the global counters, 4096 go to the global counters directly: the
    largest grid of the first kind and the smallest of the second, on a sample of the bins (the direct sums of all of them are a
    host's hour), and a permutation of the samples"""
    plan = NU.nufft_plan(300, M, 2)
    assert plan["tiles"] == (2048 if M == 1 << 20 else 4096)
    rng = np.random.default_rng(41)
    N = 300
    t = np.sort(rng.uniform(0.0, 100.0, N))
    c = (rng.standard_normal((2, N)) + 1j * rng.standard_normal((2, N))).astype(np.complex64)
    f0, df = -3.0, 6.0 / M
    got = NU.nufft1(dev(t), dev(c), f0, df, M).cpu().numpy()
    m = np.unique(np.concatenate([[0, 1, M // 2 - 1, M // 2, M // 2 + 1, M - 2, M - 1], rng.integers(0, M, 90)]))
    p = (t - t[0])[:, None] * (f0 + df * m)[None, :]
    ref = c.astype(np.complex128) @ L.e(p - np.rint(p))
    R.assert_within(got[:, m], ref, c, "M = %d, %d bins" % (M, m.size))
    order = rng.permutation(N)
    again = NU.nufft1(dev(t[order]), dev(c[:, order]), f0, df, M, t_ref=float(t[0])).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_far_time_origin_against_exact_phases():
    rng = np.random.default_rng(5)
    N, M = 300, 40
    t0 = np.sort(rng.integers(0, 100 * 1024, N)) / 1024.0                 # multiples of 2^-10: exact beside 2^31
    t = t0 + 2.0 ** 31
    assert np.array_equal(t - 2.0 ** 31, t0)
    c = (rng.standard_normal((2, N)) + 1j * rng.standard_normal((2, N))).astype(np.complex64)
    f0, df = 0.0625, 0.0625                                               # dyadic: f0 + m df is exact
    ref = R.direct(t, c, f0, df, M, 1, exact=True)
    got = NU.nufft1(dev(t), dev(c), f0, df, M, t_ref=0.0).cpu().numpy()   # phases from the origin of t itself
    R.assert_within(got, ref, c, "nufft1 at t + 2^31, t_ref 0")
    y = (np.sin(2 * np.pi * L.LINE_F * t0 + 0.4) + 0.01 * rng.standard_normal(N) + 0.2).astype(np.float32)
    f = f0 + df * np.arange(M)
    for nz in ("normalize", "amplitude"):
        lref = L.lomb_def(t, y.astype(np.float64), f, None, True, nz, exact=True)
        lgot = LS.ls_periodogram(dev(t), dev(y), f, normalize=nz, method="fast").cpu().numpy()
        L.assert_within(lgot[None], lref, "fast periodogram at t + 2^31, %s" % nz, R.LS_ALLOWANCE)


def test_modes_convention():
    rng = np.random.default_rng(6)
    N, M = 200, 9
    x = rng.uniform(-10.0, 10.0, N)
    c = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
    k = np.arange(M) - M // 2
    for sign in (1, -1):
        ref = (c.astype(np.complex128)[None, :] * np.exp(1j * sign * k[:, None] * x[None, :])).sum(axis=-1)
        got = pyfft_amd.nufft1_modes(dev(x), dev(c), M, sign=sign).cpu().numpy()
        assert got.shape == (M,)
        R.assert_within(got[None], ref[None], c, "nufft1_modes sign %+d" % sign)
        assert np.array_equal(got, pyfft_amd.nufft1_modes(x, c, M, sign=sign))


@pytest.mark.parametrize("name", ("tails", "tiles", "seams", "pile", "unsorted", "rows-17"))
def test_a_permutation_of_the_samples_changes_no_bit(name):
    sign = R.SHAPES[name]["signs"][0]
    order = np.random.default_rng(99).permutation(R.SHAPES[name]["N"])
    a, b = run(name, sign), run(name, sign, order=order)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_permutation_changes_no_bit_of_the_lomb_sums():
    t, y32, w, f, (f0, df) = R.ls_signals("ls-tails")
    order = np.random.default_rng(98).permutation(t.size)
    mean = y32.astype(np.float64).mean(axis=-1)
    for ww, kw in ((None, {}), (w, dict(wnorm=float(np.sum(w))))):
        kw = dict(kw, t_ref=float(t[0]), mean_value=mean)
        a = E.lomb_sums_grid(dev(t), dev(y32), f0, df, f.size, weights=None if ww is None else dev(ww), **kw)
        b = E.lomb_sums_grid(dev(t[order]), dev(y32[:, order]), f0, df, f.size, weights=None if ww is None else dev(ww[order]), **kw)
        assert torch.equal(a.common.view(torch.int64), b.common.view(torch.int64))
        assert torch.equal(a.rows.view(torch.int64), b.rows.view(torch.int64))


@pytest.mark.parametrize("name", ("tails", "long", "rows-17"))
def test_two_calls_and_both_memories_agree_bitwise(name, monkeypatch):
    monkeypatch.delenv("SP_NUFFT_ROWS", raising=False)
    sign = R.SHAPES[name]["signs"][0]
    a, b, h = run(name, sign), run(name, sign), run(name, sign, device=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), h.view(np.uint32))
    monkeypatch.setenv("SP_NUFFT_ROWS", "1")             # a row does not care which pass it is in
    assert np.array_equal(a.view(np.uint32), run(name, sign).view(np.uint32))


# ---- the Lomb-Scargle forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.LS_SHAPES))
def test_lomb_sums_grid_against_the_direct_sums_and_every_form(name, monkeypatch):
    monkeypatch.delenv("SP_NUFFT_ROWS", raising=False)
    if name == "ls-rows-17":
        monkeypatch.setenv("SP_NUFFT_ROWS", "4")
    t, y32, w, f, (f0, df) = R.ls_signals(name)
    rows, M = y32.shape[0], f.size
    for wt in (False, True):
        s = E.lomb_sums_grid(dev(t), dev(y32), f0, df, M, weights=dev(w) if wt else None)
        assert E.last_passes(E.NUFFT_PASSES) == (5 if name == "ls-rows-17" else 1)
        assert s.common.dtype == torch.float64 and tuple(s.common.shape) == (M, 4) and tuple(s.rows.shape) == (rows, M, 2)
        common, rws, totals = R.ls_sums_ref(name, wt)
        # against lomb_ref.sums_def, every cell relative to its row's sum of |strength|: w32 for A1 and A2, wy32_r for B_r
        w32, wy32, _, _ = R.lomb_strengths(t, y32, w if wt else None)
        ga, gb = R.rows_as_complex(s.common.cpu().numpy(), s.rows.cpu().numpy())
        ra, rb = R.rows_as_complex(common, rws)
        R.assert_within(ga, ra, np.stack([w32, w32]), "%s w%d A1, A2" % (name, wt))
        R.assert_within(gb, rb, wy32, "%s w%d B" % (name, wt))
        d = E.lomb_sums(dev(t), dev(y32), f, weights=dev(w) if wt else None)
        assert torch.equal(s.totals, d.totals)                              # the same preparing kernel: bitwise
        for fm, nz in [(fm, nz) for fm in (False, True) for nz in R.LS_FORMS_OF[name]]:
            got = E.lomb_finish(s, f, floating_mean=fm, normalize=nz).cpu().numpy()
            LS_USED[(name, wt, fm, nz)] = L.assert_within(got, R.ls_reference(name, (wt, fm, nz)), "%s w%d f%d %s" % (name, wt, fm, nz),
                                                          R.LS_ALLOWANCE)
    print("the device used at most %.3f of the allowance %.2e so far" % (max(LS_USED.values()), R.LS_ALLOWANCE))


def test_fast_against_direct_parts_and_the_window():
    name = "ls-tails"
    t, y32, w, f, (f0, df) = R.ls_signals(name)
    td, yd, wd = dev(t), dev(y32), dev(w)
    for fm, nz in ((True, "normalize"), (False, "amplitude"), (True, "power")):
        fast = LS.ls_periodogram(td, yd, f, weights=wd, floating_mean=fm, normalize=nz, method="fast").cpu().numpy()
        direct = LS.ls_periodogram(td, yd, f, weights=wd, floating_mean=fm, normalize=nz, method="direct").cpu().numpy()
        L.assert_within(fast, direct, "fast against direct, %s" % nz, R.LS_ALLOWANCE + L.ALLOWANCE)
        assert np.array_equal(fast, LS.ls_periodogram(np.array(t), np.array(y32), f, weights=np.array(w), floating_mean=fm, normalize=nz,
                                                      method="fast"))
    # the record cut at an odd sample: both parts with the whole's origin, mean and weight sum
    whole = E.lomb_sums_grid(td, yd, f0, df, f.size, weights=wd)
    cut, kw = 333, dict(t_ref=whole.t_ref, mean_value=whole.mean, wnorm=float(np.sum(w)))
    parts = (E.lomb_sums_grid(td[:cut], yd[:, :cut], f0, df, f.size, weights=wd[:cut], **kw)
             + E.lomb_sums_grid(td[cut:], yd[:, cut:], f0, df, f.size, weights=wd[cut:], **kw))
    assert parts.N == whole.N
    for fm, nz in ((True, "normalize"), (False, "amplitude")):
        got = E.lomb_finish(parts, f, floating_mean=fm, normalize=nz).cpu().numpy()
        L.assert_within(got, R.ls_reference(name, (True, fm, nz)), "two parts added, %s" % nz, R.LS_ALLOWANCE)
    # the spectral window, from the sums without rows
    win = LS.ls_window(td, f, weights=wd, method="fast").cpu().numpy()
    wn = w / w.sum()
    ref = np.abs((wn[None, :] * np.exp(2j * np.pi * f[:, None] * (t - t[0])[None, :])).sum(axis=-1)) ** 2
    assert win.dtype == np.float64 and np.max(np.abs(win - ref)) <= 2 * R.ALLOWANCE
    assert np.array_equal(win, LS.ls_window(np.array(t), f, weights=np.array(w), method="fast"))
    assert np.allclose(win, LS.ls_window(td, f, weights=wd).cpu().numpy(), rtol=0, atol=2 * R.ALLOWANCE + L.ALLOWANCE)


# ---- offset pointers inside poisoned buffers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", (0, 1, 2, 3))
def test_calls_at_offset_pointers_with_guarded_outputs(lead):
    name = "tails"
    t, c, t_ref = R.signals(name)
    f0, df = R.grid_of(name)
    rows, N = c.shape
    M, ld = R.SHAPES[name]["M"], N + 5
    tb, tv = G.poisoned_input(dev(t), lead % 2)
    cb, cv = G.poisoned_input(dev(c), (lead + 1) % 2, pitch=ld)
    snaps = [G.snapshot(b) for b in (tb, cb)]
    got = E.nufft1(tv, cv, f0, df, M, t_ref=t_ref).cpu().numpy()
    assert np.all(np.isfinite(got.view(np.float32)))
    R.assert_within(got, R.reference(name, 1), c, "engine.nufft1 at lead %d" % lead)
    E._bind_stream(tv)
    ob, oa = G.sentinel_output(rows * M, torch.complex64, lead % 2, device="cuda")
    rc = _ffi.lib().sp_nufft1(_ffi.ptr(tv.data_ptr()), _ffi.ptr(cv.data_ptr()), ld, N, rows, t_ref, f0, df, M, 1, _ffi.ptr(oa), 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    torch.cuda.synchronize()
    assert all(G.unchanged(b, s) for b, s in zip((tb, cb), snaps))
    assert G.guards_intact(ob, lead % 2, rows * M) and G.all_written(ob, lead % 2, rows * M)
    assert np.array_equal(G.interior_of(ob, lead % 2, rows * M).cpu().numpy().reshape(rows, M).view(np.uint32), got.view(np.uint32))
    # the Lomb entry: float32 rows at every residue
    lt, y32, w, f, (lf0, ldf) = R.ls_signals("ls-tails")
    rows, N = y32.shape
    ld = N + 5
    tb2, tv2 = G.poisoned_input(dev(lt), lead % 2)
    yb, yv = G.poisoned_input(dev(y32), lead, pitch=ld)
    wb, wv = G.poisoned_input(dev(w), (lead + 1) % 2)
    snaps = [G.snapshot(b) for b in (tb2, wb, yb)]
    mean = np.ascontiguousarray(y32.astype(np.float64).mean(axis=-1))
    sizes = (4 * f.size, rows * f.size * 2, 1 + 2 * rows)
    outs = [G.sentinel_output(n, torch.float64, lead % 2, device="cuda") for n in sizes]
    rc = _ffi.lib().sp_lomb_sums_grid(_ffi.ptr(tv2.data_ptr()), _ffi.ptr(wv.data_ptr()), _ffi.ptr(yv.data_ptr()), ld, N, rows, float(lt[0]), 0.0,
                                      lf0, ldf, f.size, _ffi.ptr(mean), *[_ffi.ptr(o[1]) for o in outs], 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    torch.cuda.synchronize()
    assert all(G.unchanged(b, s) for b, s in zip((tb2, wb, yb), snaps))
    for (b, _), n in zip(outs, sizes):
        assert G.guards_intact(b, lead % 2, n) and G.all_written(b, lead % 2, n)
    s = E.lomb_sums_grid(dev(lt), dev(y32), lf0, ldf, f.size, weights=dev(w), mean_value=mean)
    assert torch.equal(G.interior_of(outs[0][0], lead % 2, sizes[0]).view(torch.int64), s.common.reshape(-1).view(torch.int64))
    assert torch.equal(G.interior_of(outs[1][0], lead % 2, sizes[1]).view(torch.int64), s.rows.reshape(-1).view(torch.int64))


def test_refusals_leave_the_outputs_untouched():
    name = "tails"
    t, c, t_ref = R.signals(name)
    f0, df = R.grid_of(name)
    rows, N = c.shape
    M = R.SHAPES[name]["M"]
    td, cd = dev(t), dev(c)
    E._bind_stream(td)
    lib = _ffi.lib()

    def call(tt=td, cc=cd, n=N, ld=N, m=M, tr=t_ref, a=f0, b=df, sg=1):
        ob, oa = G.sentinel_output(rows * M, torch.complex64, 1, device="cuda")
        rc = lib.sp_nufft1(_ffi.ptr(tt.data_ptr()), _ffi.ptr(cc.data_ptr()), ld, n, rows, tr, a, b, m, sg, _ffi.ptr(oa), 1)
        torch.cuda.synchronize()
        assert G.guards_intact(ob, 1, rows * M)
        untouched = bool((G._host_words(ob) == np.uint32(G.SENTINEL)).all())
        return rc, (lib.sp_last_error() or b"").decode(), untouched

    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    for kw, word in ((dict(n=0), "N must"), (dict(ld=N - 1), "c_ld"), (dict(m=0), "M must"), (dict(tr=float("nan")), "t_ref"),
                     (dict(a=float("inf")), "f0"), (dict(b=0.0), "df"), (dict(b=float("nan")), "df"), (dict(sg=0), "sign")):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg.startswith("sp_nufft1: ") and word in msg and untouched, (kw, rc, msg)
    tn, cn = td.clone(), cd.clone()
    tn[N // 2], cn[1, 100] = float("nan"), complex(0.0, float("inf"))
    for kw, word in ((dict(tt=tn), "t holds"), (dict(cc=cn), "c holds")):
        rc, msg, untouched = call(**kw)
        assert rc == E.NUFFT_BAD_RECORD == -2 and msg.startswith("sp_nufft1: ") and word in msg and untouched, (rc, msg)
    lt, y32, w, f, (lf0, ldf) = R.ls_signals("ls-tails")
    ltd, yd, wd = dev(lt), dev(y32), dev(w)
    ltn, wn, yn = ltd.clone(), wd.clone(), yd.clone()
    ltn[3], wn[7], yn[1, 100] = float("inf"), -1.0, float("nan")
    bad = [lambda: E.nufft1(tn, cd, f0, df, M), lambda: E.nufft1(td, cn, f0, df, M), lambda: E.nufft1(td, cd.to(torch.complex128), f0, df, M),
           lambda: E.nufft1(td.float(), cd, f0, df, M)]
    for fn in bad:
        with pytest.raises(E.NufftRefused) as exc:
            fn()
        assert isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)
    for fn in (lambda: E.lomb_sums_grid(ltn, yd, lf0, ldf, f.size), lambda: E.lomb_sums_grid(ltd, yd, lf0, ldf, f.size, weights=wn),
               lambda: E.lomb_sums_grid(ltd, yn, lf0, ldf, f.size), lambda: LS.ls_window(ltn, f, method="fast"),
               lambda: LS.ls_periodogram(ltd, yd, f ** 2, method="fast")):
        with pytest.raises(E.LombRefused):
            fn()
    # and the library still works
    assert np.array_equal(run(name, 1).view(np.uint32), run(name, 1).view(np.uint32))
    R.assert_within(run(name, 1), R.reference(name, 1), c, "after the refusals")


def test_auto_takes_the_measured_path(monkeypatch):
    t, y32, w, f, _ = R.ls_signals("ls-tails")
    calls = []
    real_grid, real_direct = E.lomb_sums_grid, E.lomb
    monkeypatch.setattr(E, "lomb_sums_grid", lambda *a, **k: calls.append("fast") or real_grid(*a, **k))
    monkeypatch.setattr(E, "lomb", lambda *a, **k: calls.append("direct") or real_direct(*a, **k))
    LS.ls_periodogram(dev(t), dev(y32), f, method="auto")
    pairs = E.nufft_plan(t.size, f.size)["fast_min_pairs"]
    assert calls == ["fast" if t.size * f.size >= pairs else "direct"]
    assert LS.ls_plan(t.size, f.size, 3, method="auto")["path"] == calls[0]
    LS.ls_periodogram(dev(t), dev(y32), f ** 2, method="auto")          # not uniform: the direct sums
    assert calls[1] == "direct"
