"""The discrete wavelet transforms on the GPU against the float64 restatements of tests/dwt_ref.py, every result within the running
bound carried beside the reference (no factor, no absolute term beyond the smallest normal float): both kernel forms forced at the
smallest shapes that can go wrong (rows shorter than the filter, whose extension wraps more than once and whose halo is longer than
the record; odd lengths; the deepest level), the tile form where it is the natural one (first, last and interior tiles), pitched rows
between NaNs and sentinels, passes, the inverses on coefficients that are nobody's transform, the MODWT with its inversion and energy
split, packets in both orders, and the invariants: the two forms, host arrays and device tensors, and two calls agree bitwise."""
import functools

import numpy as np
import pytest

import dwt_ref as R
import pyfft_amd
from pyfft_amd import _ffi, engine as E, _dwt_mod as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WAVELETS = {2: "db1", 4: "db2", 8: "db4", 20: "db10"}
NS = (1, 2, 3, 5, 8, 17, 37, 64, 1000, 1024)


def bank(L):
    return D.wavelet_filters(WAVELETS[L])


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def bits(a):
    a = np.ascontiguousarray(host(a))
    return a.view(np.uint32) if a.dtype.itemsize == 4 or a.dtype == np.complex64 else a.view(np.uint64)


def held(got, ref, bound, what):
    """every element within its bound -> the share of the bound used"""
    got = host(got).astype(np.complex128 if np.iscomplexobj(ref) else np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got.view(np.float64))), what
    share = float(np.max(np.abs(got - ref) / (bound + R.TINY))) if got.size else 0.0
    assert share <= 1.0, (what, share)
    return share


@functools.lru_cache(maxsize=None)
def ref_pyramid(n, L, mode, levels, cplx, rows=2):
    x = R.signal(n, rows, cplx, seed=L)
    dl, dh, _, _ = bank(L)
    c, b = R.wavedec(x.astype(np.complex128 if cplx else np.float64), dl, dh, mode, levels, B=0.0)
    for a in (x,) + tuple(c) + tuple(b):
        a.setflags(write=False)
    return x, np.concatenate(c, axis=-1), np.concatenate(b, axis=-1), c, b


# ---- both forms, forced -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("L", sorted(WAVELETS))
def test_both_forms_forced(L, mode):
    dl, dh, rl, rh = bank(L)
    worst = 0.0
    for n in NS:
        for levels in sorted({1, E.dwt_max_levels(n, L, mode)}):
            for cplx in (False, True):
                x, ref, bound, _, _ = ref_pyramid(n, L, mode, levels, cplx)
                row, tile = E.dwt(x, dl, dh, mode, levels, form="row"), E.dwt(x, dl, dh, mode, levels, form="tile")
                assert row.dtype == x.dtype and np.array_equal(bits(row), bits(tile)), (n, levels, cplx)
                worst = max(worst, held(row, ref, bound, ("dwt", n, levels, cplx)))
                assert E.dwt_plan("dwt", n, L, mode, levels, 2, cplx, "row")["form"] == 1 and E.dwt_plan("dwt", n, L, mode, levels, 2, cplx, "tile")["form"] == 2
    print("dwt L %d %s: share of the bound %.3f" % (L, mode, worst))


@pytest.mark.parametrize("mode", ("symmetric", "periodization", "zero"))
@pytest.mark.parametrize("L", (8, 20))
def test_tile_seams(L, mode):
    """3 tiles + 1 and an exact multiple of the tile at level 1, both parities of n, levels 1 .. 4: the first, the last and the interior tiles"""
    dl, dh, rl, rh = bank(L)
    for K in (3 * 1024 + 1, 2 * 1024):
        for n in ((2 * K - 1, 2 * K) if mode == "periodization" else (2 * K - L + 1, 2 * K - L + 2)):
            assert E.dwt_coeff_len(n, L, mode) == K
            for levels in (1, 2, 3, 4):
                x, ref, bound, _, _ = ref_pyramid(n, L, mode, levels, False, 1)
                tile = E.dwt(x, dl, dh, mode, levels, form="tile")
                held(tile, ref, bound, ("tile", n, levels))
                assert E.last_passes(E.DWT_PASSES) == 1
                if levels == 4:
                    assert np.array_equal(bits(tile), bits(E.dwt(x, dl, dh, mode, levels, form="row")))
                    back = E.idwt(tile, n, rl, rh, mode, levels, form="tile")
                    assert np.array_equal(bits(back), bits(E.idwt(tile, n, rl, rh, mode, levels, form="row")))


@pytest.mark.parametrize("cplx", (False, True))
def test_the_natural_tile_form(cplx):
    """a row past what the row form holds takes the tile form by itself: 10 tiles + 1 at level 1 (float32), and the plan says so"""
    L, mode, levels = 8, "symmetric", 3
    K = 10 * 1024 + 1
    n = 2 * K - L + 1
    dl, dh, rl, rh = bank(L)
    plan = E.dwt_plan("dwt", n, L, mode, levels, 1, cplx)
    assert plan["form"] == 2 and plan["launches"] == levels and plan["entries"][-1] == (K, plan["entries"][-2][1] + plan["entries"][-2][0])
    with pytest.raises(E.DwtRefused):
        E.dwt_plan("dwt", n, L, mode, levels, 1, cplx, form="row")
    x, ref, bound, c, b = ref_pyramid(n, L, mode, levels, cplx, 1)
    got = E.dwt(x, dl, dh, mode, levels)
    print("natural tile form: share %.3f" % held(got, ref, bound, "auto"))
    back, bb = R.waverec([host(got)[..., o:o + ln].astype(ref.dtype) for ln, o in plan["entries"]], n, rl, rh, mode, bounds=[np.zeros(1)] * (levels + 1))
    held(E.idwt(got, n, rl, rh, mode, levels), back, bb, "auto inverse")


# ---- rows, pitches, passes ---------------------------------------------------------------------------------------------------------
SENT = np.uint32(0xDEADBEEF)


@pytest.mark.parametrize("rows", (1, 3, 257))
@pytest.mark.parametrize("form", ("row", "tile"))
def test_pitched_rows_between_nans_and_sentinels(rows, form, monkeypatch):
    n, L, mode, levels, pad = 37, 8, "reflect", 3, 5
    dl, dh, rl, rh = bank(L)
    lib = _ffi.load_library()
    x = R.signal(n, rows, seed=3)
    want = E.dwt(x, dl, dh, mode, levels, form=form)
    total = want.shape[-1]
    wide = np.full((rows, n + pad), np.nan, dtype=np.float32)
    wide[:, :n] = x
    got = E.dwt(dev(wide)[:, :n], dl, dh, mode, levels, form=form)                # a row-strided view goes through as it is
    assert np.array_equal(bits(got), bits(want))
    for mem in (0, 1):
        out = np.full((rows, total + pad), SENT, dtype=np.uint32).view(np.float32)       # (the sentinel is an ordinary float32)
        xin, o = (dev(wide), dev(out)) if mem else (wide, out)
        E._enter(xin)
        rc = lib.sp_dwt(_ffi.ptr(xin.data_ptr() if mem else xin), 0, n + pad, n, rows, _ffi.ptr(dl), _ffi.ptr(dh), L, E.DWT_MODES[mode], levels,
                        _ffi.ptr(o.data_ptr() if mem else o), total + pad, E.DWT_FORMS[form], mem)
        assert rc == 0, lib.sp_last_error()
        o = host(o).view(np.uint32)
        assert np.array_equal(o[:, :total], bits(want)) and np.all(o[:, total:] == SENT), mem
        back = np.full((rows, n + pad), SENT, dtype=np.uint32).view(np.float32)
        o = o.view(np.float32)
        ci, bo = (dev(o), dev(back)) if mem else (o, back)
        rc = lib.sp_idwt(_ffi.ptr(ci.data_ptr() if mem else ci), 0, total + pad, n, rows, _ffi.ptr(rl), _ffi.ptr(rh), L, E.DWT_MODES[mode], levels,
                         _ffi.ptr(bo.data_ptr() if mem else bo), n + pad, E.DWT_FORMS[form], mem)
        assert rc == 0, lib.sp_last_error()
        bo = host(bo).view(np.uint32)
        assert np.array_equal(bo[:, :n], bits(E.idwt(want, n, rl, rh, mode, levels, form=form))) and np.all(bo[:, n:] == SENT), mem
    if form == "tile" and rows > 1:
        monkeypatch.setenv("SP_DWT_ROWS", "2")
        again = E.dwt(x, dl, dh, mode, levels, form="tile")
        assert E.last_passes(E.DWT_PASSES) == -(-rows // 2) > 1 and np.array_equal(bits(again), bits(want))
        back = E.idwt(again, n, rl, rh, mode, levels, form="tile")
        assert E.last_passes(E.DWT_PASSES) == -(-rows // 2)
        W = E.modwt(x, rl, rh, 3, form="tile")
        assert E.last_passes(E.DWT_PASSES) == -(-rows // 2)
        xb = E.imodwt(W, rl, rh, form="tile")
        assert E.last_passes(E.DWT_PASSES) == -(-rows // 2)
        monkeypatch.delenv("SP_DWT_ROWS")
        assert np.array_equal(bits(back), bits(E.idwt(want, n, rl, rh, mode, levels, form="tile"))) and E.last_passes(E.DWT_PASSES) == 1
        assert np.array_equal(bits(W), bits(E.modwt(x, rl, rh, 3, form="tile"))) and np.array_equal(bits(xb), bits(E.imodwt(W, rl, rh, form="row")))


# ---- the inverse -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("L", sorted(WAVELETS))
def test_inverse_of_arbitrary_coefficients_and_the_round_trip(L, mode):
    dl, dh, rl, rh = bank(L)
    worst = trip = 0.0
    for n in (1, 2, 3, 5, 8, 17, 37, 64, 1000):
        for levels in sorted({1, min(E.dwt_max_levels(n, L, mode), 5)}):
            for cplx in (False, True):
                lens, entries, total = E.dwt_layout(n, L, mode, levels)
                coef = R.signal(total, 2, cplx, seed=11 + L)                      # nobody's transform
                parts = [coef[..., o:o + ln].astype(np.complex128 if cplx else np.float64) for ln, o in entries]
                ref, bound = R.waverec(parts, n, rl, rh, mode, bounds=[np.zeros(1)] * (levels + 1))
                row, tile = E.idwt(coef, n, rl, rh, mode, levels, form="row"), E.idwt(coef, n, rl, rh, mode, levels, form="tile")
                assert np.array_equal(bits(row), bits(tile)), (n, levels, cplx)
                worst = max(worst, held(row, ref, bound, ("idwt", n, levels, cplx)))
                if levels == 1:
                    one = E.idwt_level(coef[..., :lens[1]], coef[..., lens[1]:], n, rl, rh, mode)
                    assert np.array_equal(bits(one), bits(row))
                    a, d = E.dwt_level(row, dl, dh, mode, form="row")
                    assert np.array_equal(bits(np.concatenate((a, d), axis=-1)), bits(E.dwt(row, dl, dh, mode, 1, form="tile")))
                x, _, _, c, b = ref_pyramid(n, L, mode, levels, cplx)
                back, bb = R.waverec(list(c), n, rl, rh, mode, bounds=list(b))      # the forward bounds carried through the inverse
                rec = D.waverec(D.wavedec(x, WAVELETS[L], mode, levels), WAVELETS[L], mode, n=n)
                trip = max(trip, held(rec, back, bb, ("round trip", n, levels, cplx)))
    print("idwt L %d %s: share of the bound %.3f, round trip %.3f" % (L, mode, worst, trip))


# ---- the MODWT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,levels", [(5, 4), (37, 1), (37, 4), (4099, 1), (4099, 2), (4099, 3), (4099, 4), (4099, 5), (4099, 6)])
def test_modwt_both_forms_inversion_and_energy(n, levels):
    for L in (2, 8, 20):
        dl, dh, rl, rh = bank(L)
        for cplx in (False, True):
            x = R.signal(n, 2, cplx, seed=5)
            ref, bound = R.modwt(x.astype(np.complex128 if cplx else np.float64), rl, rh, levels, B=0.0)
            row, tile = E.modwt(x, rl, rh, levels, form="row"), E.modwt(x, rl, rh, levels, form="tile")
            assert row.shape == (levels + 1, 2, n) and np.array_equal(bits(row), bits(tile))
            share = held(row, ref, bound, ("modwt", n, levels, L, cplx))
            # the energy split: exact for the float64 filters; the float32 taps are each off by a relative 2^-24, which moves the
            # energy a level passes on by at most 4 L 2^-24 of it; the coefficients' own errors enter through 2 |w| B + B^2
            e_got, e_x = float(np.sum(np.abs(host(row).astype(np.complex128)) ** 2)), float(np.sum(np.abs(x.astype(np.complex128)) ** 2))
            assert abs(e_got - e_x) <= float(np.sum(2 * np.abs(ref) * bound + bound ** 2)) + 4 * levels * L * R.U * e_x
            back, bb = R.imodwt(ref, rl, rh, B=bound)
            xr, xt = E.imodwt(row, rl, rh, form="row"), E.imodwt(row, rl, rh, form="tile")
            assert np.array_equal(bits(xr), bits(xt))
            held(xr, back, bb, ("imodwt", n, levels, L, cplx))
            W = R.signal(n, 2 * (levels + 1), cplx, seed=9).reshape(levels + 1, 2, n)        # nobody's transform
            back, bb = R.imodwt(W.astype(np.complex128 if cplx else np.float64), rl, rh, B=0.0)
            held(E.imodwt(W, rl, rh, form="tile"), back, bb, ("imodwt of anything", n, levels, L, cplx))
    print("modwt n %d levels %d: last share %.3f" % (n, levels, share))


# ---- packets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,level", [(64, 3), (64, 6), (96, 5)])
def test_packets_in_both_orders(n, level):
    for L in (2, 8):
        dl, dh, rl, rh = bank(L)
        for cplx in (False, True):
            x = R.signal(n, 3, cplx, seed=2)
            ref, bound = R.wpdec(x.astype(np.complex128 if cplx else np.float64), dl, dh, level, B=0.0)
            nat = D.wpdec(x, WAVELETS[L], level)
            assert nat.shape == (3, 1 << level, n >> level)
            held(nat, ref, bound, ("wpdec", n, level, L, cplx))
            frq = D.wpdec(dev(x), WAVELETS[L], level, order="freq")
            assert np.array_equal(bits(frq), bits(nat[:, R.gray(level), :]))
            back, bb = R.wprec(ref, rl, rh, B=bound)
            held(D.wprec(nat, WAVELETS[L]), back, bb, ("wprec", n, level, L, cplx))
            assert np.array_equal(bits(D.wprec(frq, WAVELETS[L], order="freq")), bits(D.wprec(nat, WAVELETS[L])))
    with pytest.raises(E.DwtRefused):
        D.wpdec(x, "db4", 7)


# ---- bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", (False, True))
def test_host_arrays_device_tensors_and_two_calls_agree_bitwise(cplx):
    n, L, mode, levels = 1000, 8, "symmetric", 4
    dl, dh, rl, rh = bank(L)
    x = R.signal(n, 3, cplx, seed=4)
    xd = dev(x)
    for form in ("row", "tile"):
        c = E.dwt(x, dl, dh, mode, levels, form)
        cd = E.dwt(xd, dl, dh, mode, levels, form)
        assert isinstance(cd, torch.Tensor) and cd.is_cuda and np.array_equal(bits(c), bits(cd)) and np.array_equal(bits(c), bits(E.dwt(x, dl, dh, mode, levels, form)))
        a, d = E.dwt_level(x, dl, dh, mode, form)
        ad, dd = E.dwt_level(xd, dl, dh, mode, form)
        pair = E.dwt_level(xd, dl, dh, mode, form, interleave=True)
        assert np.array_equal(bits(a), bits(ad)) and np.array_equal(bits(d), bits(dd))
        assert np.array_equal(bits(pair), bits(E.dwt_level(x, dl, dh, mode, form, interleave=True))) and np.array_equal(bits(pair[:, 1]), bits(d))
        b = E.idwt(c, n, rl, rh, mode, levels, form)
        assert np.array_equal(bits(b), bits(E.idwt(cd, n, rl, rh, mode, levels, form))) and np.array_equal(bits(b), bits(E.idwt(c, n, rl, rh, mode, levels, form)))
        one = E.idwt_level(a, d, n, rl, rh, mode, form)
        assert np.array_equal(bits(one), bits(E.idwt_level(ad, dd, n, rl, rh, mode, form))) and np.array_equal(bits(one), bits(E.idwt_level(pair, None, n, rl, rh, mode, form)))
        W = E.modwt(x, rl, rh, levels, form)
        Wd = E.modwt(xd, rl, rh, levels, form)
        assert np.array_equal(bits(W), bits(Wd)) and np.array_equal(bits(W), bits(E.modwt(x, rl, rh, levels, form)))
        v = E.imodwt(W, rl, rh, form)
        assert np.array_equal(bits(v), bits(E.imodwt(Wd, rl, rh, form))) and np.array_equal(bits(v), bits(E.imodwt(W, rl, rh, form)))
    lst = D.wavedec(xd, "db4", mode, levels, axis=-1)
    assert all(isinstance(p, torch.Tensor) for p in lst) and [p.shape[-1] for p in lst] == [ln for ln, _ in E.dwt_layout(n, L, mode, levels)[1]]
    assert np.array_equal(bits(torch.cat(lst, dim=-1)), bits(E.dwt(x, dl, dh, mode, levels)))
    moved = D.wavedec(np.ascontiguousarray(x.T), "db4", mode, levels, axis=0)
    assert np.array_equal(bits(np.concatenate(moved, axis=0).T), bits(E.dwt(x, dl, dh, mode, levels)))


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_wavelet_variance_and_the_multiresolution_analysis():
    """modwt_variance against float64 on a record with a known octave structure (a period of 3 samples lives at level 1, one of 24 at
    level 4), and modwt_mra adds up to x: the tolerances are 4 x the errors of the float32 restatement at this shape, measured on the
    CPU (tests/test_host_dwt.py::test_the_recorded_float32_figures re-measures them)."""
    x, level = R.octave_record(), R.OCTAVE_LEVEL
    _, _, rl, rh = D.wavelet_filters("db4")
    nu2, edof = D.modwt_variance(dev(x), "db4", level)
    want, wdof = R.modwt_variance(x.astype(np.float64), rl, rh, level)
    assert isinstance(nu2, torch.Tensor) and nu2.dtype == torch.float64 and np.array_equal(edof, wdof)
    rel = float(np.max(np.abs(host(nu2) - want) / want))
    assert int(np.argmax(want)) == 3 and want[0] > want[1] and rel <= 4 * R.F32_VARIANCE_REL, rel
    W = D.modwt(x, "db4", level)
    mra = D.modwt_mra(W, "db4")
    err = float(np.max(np.abs(mra.astype(np.float64).sum(axis=0) - x)))
    assert mra.shape == (level + 1, x.size) and err <= 4 * R.F32_MRA_SUM, err
    print("variance: %.3f of the allowance; mra sum: %.3f of the allowance" % (rel / (4 * R.F32_VARIANCE_REL), err / (4 * R.F32_MRA_SUM)))
    assert np.array_equal(bits(D.modwt_variance(x, "db4", level)[0]), bits(D.modwt_variance(x, "db4", level)[0]))
    assert pyfft_amd.modwt_variance is D.modwt_variance
