"""Lomb-Scargle spectra on the GPU (k_lomb, sp_lomb, pyfft_amd.lomb) against the float64 closed form of tests/lomb_ref.py: all 24
forms of scipy's options, tails of the sample and frequency tiles, the row-group loop, the sum over sample runs with and without
its hook, the passes over a long frequency list, times in any order, records far from the time origin against an exact-phase
reference, a gapped grid and its spectral window, the un-finished sums and their additivity, bitwise repeatability, host arrays
against device tensors, offset pointers inside poisoned buffers with guarded outputs, and refusals that leave the outputs alone."""
import numpy as np
import pytest
import torch            # a missing torch fails these tests, it does not skip them

import guard_ref as G
import lomb_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, lomb as LS

pytestmark = pytest.mark.gpu

USED = {}          # case -> the share of the allowance the device used


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def dev_rows(a, pitch):
    """the float32 rows of a on the device, N + pitch apart, NaN between them"""
    rows, n = a.shape
    if not pitch:
        return dev(a.astype(np.float32))
    base = torch.full((rows * (n + pitch),), float("nan"), dtype=torch.float32, device="cuda")
    view = base.as_strided((rows, n), (n + pitch, 1))
    view.copy_(dev(a.astype(np.float32)))
    return view


def run(name, form, device=True):
    """ls_periodogram of a shape's rows: numpy [rows, M]"""
    s = R.SHAPES[name]
    t, y, w, _ = R.signals(name)
    wt, fm, pc, nz = form
    assert not pc
    f = R.freqs_of(name, form)
    if device:
        out = LS.ls_periodogram(dev(t), dev_rows(y, s["pitch"]), f, weights=dev(w) if wt else None, floating_mean=fm, normalize=nz)
        return out.cpu().numpy()
    return LS.ls_periodogram(np.array(t), y.astype(np.float32), f, weights=np.array(w) if wt else None, floating_mean=fm, normalize=nz)


@pytest.mark.parametrize("form", R.FORMS24, ids=[R.form_id(f) for f in R.FORMS24])
def test_every_form_of_scipys_options(form):
    name = "n1000-m300"
    t, y, w, _ = R.signals(name)
    wt, fm, pc, nz = form
    f = R.freqs_of(name, form)
    assert (f[0] == 0.0) == (not fm)
    got = pyfft_amd.lombscargle(np.array(t), np.array(y[0]), 2 * np.pi * f, precenter=pc, normalize=nz, weights=np.array(w) if wt else None,
                                floating_mean=fm)
    assert got.shape == (f.size,) and got.dtype == (np.complex64 if nz == "amplitude" else np.float32)
    USED[(name, form)] = R.assert_within(got[None], R.reference(name, form), "%s %s" % (name, R.form_id(form)))


OTHERS = [c for c in R.CASES if c[0] not in ("n1000-m300", "rows-max")]


@pytest.mark.parametrize("name,form", OTHERS, ids=["%s-%s" % (n, R.form_id(f)) for n, f in OTHERS])
def test_shapes_against_reference(name, form, monkeypatch):
    s = R.SHAPES[name]
    monkeypatch.delenv("SP_LOMB_SPLIT", raising=False)
    monkeypatch.delenv("SP_LOMB_FREQS", raising=False)
    E.lomb(np.arange(4.0), np.ones(4, dtype=np.float32), [0.1])          # the library is up: the plan counts the device's CUs
    if name == "split-hook":
        monkeypatch.setenv("SP_LOMB_SPLIT", str(R.SPLIT_HOOK))
        assert LS.ls_plan(s["N"], s["M"], s["rows"])["split"] == R.SPLIT_HOOK
    if name == "passes":
        monkeypatch.setenv("SP_LOMB_FREQS", str(R.FREQS_HOOK))
    plan = LS.ls_plan(s["N"], s["M"], s["rows"])
    if name == "split-plan":
        assert plan["split"] > 1, plan
    if name == "rows-17":
        assert plan["rows_per_group"] < s["rows"] and plan["workgroups"] >= 3, plan
    got = run(name, form)
    assert got.shape == (s["rows"], s["M"])
    if name == "passes":
        assert plan["passes"] == 3 and E.last_passes(E.LOMB_PASSES) == 3
    else:
        assert E.last_passes(E.LOMB_PASSES) == 1
    if name == "rows-17":
        assert not got[7].any()                  # a row of zeros
    USED[(name, form)] = R.assert_within(got, R.reference(name, form), "%s %s" % (name, R.form_id(form)))
    print("the device used at most %.3f of the allowance %.2e so far" % (max(USED.values()), R.ALLOWANCE))


def test_largest_batch_walks_the_prep_columns_and_the_group_launches(monkeypatch):
    """65535 rows: the prepared record's 65537 columns take more than one launch of the prep kernel, and the 8192 row groups more
    than one launch of the sums kernel -- the second with its products offset by the groups before it and no window sums to write"""
    name = "rows-max"
    s, form = R.SHAPES[name], R.SHAPES[name]["forms"][0]
    assert s["rows"] == E.LOMB_MAX_ROWS
    monkeypatch.delenv("SP_LOMB_SPLIT", raising=False)
    monkeypatch.delenv("SP_LOMB_FREQS", raising=False)
    t, y, w, _ = R.signals(name)
    wt, fm, pc, nz = form
    f = R.freqs_of(name, form)
    y32 = y.astype(np.float32)
    mean = y32.astype(np.float64).mean(axis=-1)                   # given: the mean pass would be a call per row
    plan = LS.ls_plan(s["N"], s["M"], s["rows"])
    assert plan["rows_per_group"] == 8 and plan["workgroups"] == 8192 and plan["passes"] == 1, plan
    got = E.lomb(dev(t), dev(y32), f, floating_mean=fm, normalize=nz, mean_value=mean)
    assert E.last_passes(E.LOMB_LAUNCHES) == 2 and E.last_passes(E.LOMB_PASSES) == 1
    got = got.cpu().numpy()
    USED[(name, form)] = R.assert_within(got, R.reference(name, form), "%s %s" % (name, R.form_id(form)))
    assert np.array_equal(got, E.lomb(np.array(t), y32, f, floating_mean=fm, normalize=nz, mean_value=mean))
    sums = E.lomb_sums(dev(t), dev(y32), f, mean_value=mean)
    assert E.last_passes(E.LOMB_LAUNCHES) == 2
    assert np.array_equal(E.lomb_finish(sums, f, floating_mean=fm, normalize=nz).cpu().numpy(), got)
    E.lomb(dev(t), dev(y32[:17]), f, mean_value=mean[:17])
    assert E.last_passes(E.LOMB_LAUNCHES) == 1


def test_passes_and_runs_change_nothing_but_the_order(monkeypatch):
    name, form = "passes", R.SHAPES["passes"]["forms"][0]
    monkeypatch.delenv("SP_LOMB_SPLIT", raising=False)
    monkeypatch.delenv("SP_LOMB_FREQS", raising=False)
    whole = run(name, form)
    monkeypatch.setenv("SP_LOMB_FREQS", str(R.FREQS_HOOK))
    cut = run(name, form)
    assert E.last_passes(E.LOMB_PASSES) == 3
    assert np.array_equal(whole, cut)            # a frequency does not care which pass it is in: the seams at 128 and 256 included
    monkeypatch.setenv("SP_LOMB_SPLIT", "3")
    runs = run(name, form)
    assert not np.array_equal(whole, runs)       # three sample runs are another order of summation ...
    R.assert_within(runs, R.reference(name, form), "passes in three runs")      # ... and as good


def _far_record():
    rng = np.random.default_rng(5)
    N, M = 300, 40
    t0 = np.sort(rng.integers(0, 100 * 1024, N)) / 1024.0                 # multiples of 2^-10: exact beside 2^31
    y = (np.sin(2 * np.pi * R.LINE_F * t0 + 0.4) + 0.01 * rng.standard_normal(N) + 0.2).astype(np.float32)
    f = np.linspace(0.05, 3.0, M)
    t = t0 + 2.0 ** 31
    assert np.array_equal(t - 2.0 ** 31, t0)
    return t, y, f


@pytest.mark.parametrize("nz", ("normalize", "amplitude"))
def test_far_time_origin_against_exact_phases(nz):
    t, y, f = _far_record()
    ref = R.lomb_def(t, y.astype(np.float64), f, None, True, nz, exact=True)
    got = pyfft_amd.lombscargle(t, y.astype(np.float64), 2 * np.pi * f, normalize=nz, floating_mean=True)
    R.assert_within(got[None], ref, "lombscargle at t + 2^31, %s" % nz)
    got = E.lomb(dev(t), dev(y), f, floating_mean=True, normalize=nz, t_ref=2.0 ** 31)
    R.assert_within(got.cpu().numpy()[None], ref, "engine.lomb with t_ref = 2^31, %s" % nz)


def test_gapped_grid_peak_and_spectral_window():
    rng = np.random.default_rng(8)
    n, fs, f0 = 1000, 10.0, 1.7
    keep = np.sort(rng.permutation(n)[:600])                              # 40 % of the samples dropped
    t = keep / fs
    y = (np.sin(2 * np.pi * f0 * t + 1.0) + 0.05 * rng.standard_normal(t.size)).astype(np.float32)
    f = LS.ls_grid(t, oversample=5)
    P = LS.ls_periodogram(dev(t), dev(y), f).cpu().numpy()
    assert abs(f[int(np.argmax(P))] - f0) <= f[1] - f[0] and P.max() > 0.9
    fw = np.linspace(0.0, 2 * fs, 801)
    win = LS.ls_window(dev(t), fw).cpu().numpy()
    ref = np.abs(np.exp(2j * np.pi * fw[:, None] * (t - t[0])[None, :]).sum(axis=-1)) ** 2 / t.size ** 2
    assert win.dtype == np.float64 and np.max(np.abs(win - ref)) <= R.ALLOWANCE
    assert abs(win[0] - 1) <= R.ALLOWANCE and abs(win[400] - 1) <= R.ALLOWANCE and abs(win[800] - 1) <= R.ALLOWANCE
    host = LS.ls_window(t, fw)
    assert isinstance(host, np.ndarray) and np.allclose(win, host, rtol=1e-13, atol=0)
    assert np.array_equal(E.lomb_sums(dev(t), None, fw).common.cpu().numpy(), E.lomb_sums(t, None, fw).common)


def test_finished_sums_are_the_periodogram_bitwise_and_parts_add_up():
    name = "tails"
    t, y, w, f = R.signals(name)
    y32 = y.astype(np.float32)
    td, yd, wd = dev(t), dev(y32), dev(w)
    for fm, nz in ((True, "normalize"), (False, "amplitude"), (True, "power")):
        s = E.lomb_sums(td, yd, f, weights=wd)
        assert s.common.dtype == torch.float64 and tuple(s.rows.shape) == (3, f.size, 2) and tuple(s.totals.shape) == (7,)
        a = E.lomb_finish(s, f, floating_mean=fm, normalize=nz).cpu().numpy()
        b = E.lomb(td, yd, f, weights=wd, floating_mean=fm, normalize=nz).cpu().numpy()
        assert np.array_equal(a, b)
        sh = E.lomb_sums(np.array(t), y32, f, weights=np.array(w))
        assert np.array_equal(E.lomb_finish(sh, f, floating_mean=fm, normalize=nz), a)
    # the record cut at an odd place: both parts with the whole's mean, origin and weight sum
    whole = E.lomb_sums(td, yd, f, weights=wd)
    cut, kw = 333, dict(t_ref=whole.t_ref, mean_value=whole.mean, wnorm=float(np.sum(w)))
    parts = E.lomb_sums(td[:cut], yd[:, :cut], f, weights=wd[:cut], **kw) + E.lomb_sums(td[cut:], yd[:, cut:], f, weights=wd[cut:], **kw)
    assert parts.N == whole.N
    for fm, nz in ((True, "normalize"), (False, "amplitude")):
        got = E.lomb_finish(parts, f, floating_mean=fm, normalize=nz).cpu().numpy()
        R.assert_within(got, R.lomb_def(t, y, f, w, fm, nz), "two parts added, %s" % nz)
    # dealt out sample by sample to two ranks, equal weights
    kw = dict(t_ref=whole.t_ref, mean_value=whole.mean, wnorm=float(t.size))
    dealt = E.lomb_sums(td[0::2], yd[:, 0::2].contiguous(), f, **kw) + E.lomb_sums(td[1::2], yd[:, 1::2].contiguous(), f, **kw)
    R.assert_within(E.lomb_finish(dealt, f).cpu().numpy(), R.lomb_def(t, y, f, None, True, "normalize"), "dealt to two ranks")


@pytest.mark.parametrize("name", ("tails", "rows-17", "split-plan"))
def test_two_calls_and_both_memories_agree_bitwise(name):
    form = R.SHAPES[name]["forms"][0]
    a, b, h = run(name, form), run(name, form), run(name, form, device=False)
    assert np.array_equal(a, b)
    assert np.array_equal(a, h)


# ---- offset pointers inside poisoned buffers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", (0, 1, 2, 3))
def test_engine_call_at_offset_pointers(lead):
    name, form = "tails", (True, True, False, "normalize")
    t, y, w, f = R.signals(name)
    tb, tv = G.poisoned_input(dev(t), lead % 2)
    wb, wv = G.poisoned_input(dev(w), (lead + 1) % 2)
    yb, yv = G.poisoned_input(dev(y.astype(np.float32)), lead, pitch=y.shape[1] + 5)
    snaps = [G.snapshot(b) for b in (tb, wb, yb)]
    got = E.lomb(tv, yv, f, weights=wv).cpu().numpy()
    assert all(G.unchanged(b, s) for b, s in zip((tb, wb, yb), snaps))
    assert np.all(np.isfinite(got))
    R.assert_within(got, R.reference(name, form), "engine.lomb at lead %d" % lead)


@pytest.mark.parametrize("lead", (0, 1, 2, 3))
def test_c_entries_at_offset_pointers_with_guarded_outputs(lead):
    name, form = "tails", (True, True, False, "normalize")
    t, y, w, f = R.signals(name)
    rows, N = y.shape
    M, ld = f.size, N + 5
    tb, tv = G.poisoned_input(dev(t), (lead + 1) % 2)
    wb, wv = G.poisoned_input(dev(w), lead % 2)
    yb, yv = G.poisoned_input(dev(y.astype(np.float32)), (lead + 2) % 4, pitch=ld)
    snaps = [G.snapshot(b) for b in (tb, wb, yb)]
    mean = np.ascontiguousarray(y.astype(np.float32).astype(np.float64).mean(axis=-1))
    fv = np.ascontiguousarray(f)
    E._bind_stream(tv)
    Pb, Pa = G.sentinel_output(rows * M, torch.float32, lead, device="cuda")
    rc = _ffi.lib().sp_lomb(_ffi.ptr(tv.data_ptr()), _ffi.ptr(wv.data_ptr()), _ffi.ptr(yv.data_ptr()), ld, N, rows, float(t[0]), _ffi.ptr(fv), M,
                            _ffi.ptr(mean), 1, 1, _ffi.ptr(Pa), 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    outs = [G.sentinel_output(n, torch.float64, lead % 2, device="cuda") for n in (4 * M, rows * M * 2, 1 + 2 * rows)]
    rc = _ffi.lib().sp_lomb_sums(_ffi.ptr(tv.data_ptr()), _ffi.ptr(wv.data_ptr()), _ffi.ptr(yv.data_ptr()), ld, N, rows, float(t[0]), 0.0,
                                 _ffi.ptr(fv), M, _ffi.ptr(mean), *[_ffi.ptr(o[1]) for o in outs], 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    Qb, Qa = G.sentinel_output(rows * M, torch.float32, (lead + 1) % 4, device="cuda")
    rc = _ffi.lib().sp_lomb_finish(*[_ffi.ptr(o[1]) for o in outs], N, rows, float(t[0]), _ffi.ptr(fv), M, _ffi.ptr(mean), 1, 1, _ffi.ptr(Qa), 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    torch.cuda.synchronize()
    assert all(G.unchanged(b, s) for b, s in zip((tb, wb, yb), snaps))
    for (b, _), n in zip(outs, (4 * M, rows * M * 2, 1 + 2 * rows)):
        assert G.guards_intact(b, lead % 2, n) and G.all_written(b, lead % 2, n)
    got = []
    for b, ol in ((Pb, lead), (Qb, (lead + 1) % 4)):
        assert G.guards_intact(b, ol, rows * M) and G.all_written(b, ol, rows * M)
        got.append(G.interior_of(b, ol, rows * M).cpu().numpy().reshape(rows, M))
    assert np.array_equal(got[0], got[1])
    R.assert_within(got[0], R.reference(name, form), "sp_lomb at lead %d" % lead)


def test_refusals_leave_the_outputs_untouched():
    name = "tails"
    t, y, w, f = R.signals(name)
    rows, N = y.shape
    M = f.size
    fv, yd = np.ascontiguousarray(f), dev(y.astype(np.float32))
    E._bind_stream(yd)
    lib = _ffi.lib()

    def call(td, wd, yy=yd, n=N, ld=N, ff=fv, t_ref=0.0, nz=1):
        Pb, Pa = G.sentinel_output(rows * M, torch.float32, 1, device="cuda")
        rc = lib.sp_lomb(_ffi.ptr(td.data_ptr()), None if wd is None else _ffi.ptr(wd.data_ptr()), _ffi.ptr(yy.data_ptr()), ld, n, rows, t_ref,
                         _ffi.ptr(ff), M, None, 1, nz, _ffi.ptr(Pa), 1)
        torch.cuda.synchronize()
        assert G.guards_intact(Pb, 1, rows * M)
        untouched = bool((G._host_words(Pb) == np.uint32(G.SENTINEL)).all())
        return rc, (lib.sp_last_error() or b"").decode(), untouched

    td, wd = dev(t), dev(w)
    rc, msg, untouched = call(td, wd)
    assert rc == 0 and not untouched
    # what the argument checks refuse: the device is not touched
    fbad = fv.copy()
    fbad[5] = np.inf
    for kw, word in ((dict(n=0), "N must"), (dict(ld=N - 1), "y_ld"), (dict(ff=fbad), "f must"), (dict(t_ref=float("nan")), "t_ref"),
                     (dict(nz=3), "normalize")):
        rc, msg, untouched = call(td, wd, **kw)
        assert rc == -1 and msg.startswith("sp_lomb: ") and word in msg and untouched, (kw, rc, msg)
    # what only the record itself shows: found by the kernel that prepares it, before anything is written
    tn, wn, wz, yn = td.clone(), wd.clone(), torch.zeros_like(wd), yd.clone()
    tn[N // 2], wn[7], yn[1, 100] = float("nan"), -1.0, float("inf")
    for args, word in (((tn, wd), "t holds"), ((td, wn), "w holds"), ((td, wz), "do not sum"), ((td, wd, yn), "y holds")):
        rc, msg, untouched = call(*args)
        assert rc == E.LOMB_BAD_RECORD == -2 and msg.startswith("sp_lomb: ") and word in msg and untouched, (rc, msg)
    for bad in (lambda: E.lomb(tn, yd, f), lambda: E.lomb(td, yd, f, weights=wn), lambda: E.lomb(td, yn, f), lambda: LS.ls_window(tn, f),
                lambda: E.lomb(td, yd.double(), f), lambda: E.lomb(td.float(), yd, f)):
        with pytest.raises(E.LombRefused) as exc:
            bad()
        assert isinstance(exc.value, ValueError) and isinstance(exc.value, NotImplementedError)
    assert np.array_equal(E.lomb(td, yd, f).cpu().numpy(), E.lomb(td, yd, f).cpu().numpy())         # and the library still works
