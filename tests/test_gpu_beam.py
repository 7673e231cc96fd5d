"""The array scan on the GPU (k_beam.hip; sp_beamscan; pyfft_amd.beamform) against the float64 definitions and derived bounds of
tests/beam_ref.py, its invariants (bitwise repeatability, host against device, the item loop of a capped grid, guarded outputs, refusals)
and the two end-to-end cases: a ring of unevenly placed coils and a probe rake resolving two waves half a Rayleigh width apart."""
import os

import numpy as np
import pytest

import beam_ref as R
import guard_ref as G
import subspace_ref as S
import pyfft_amd
from pyfft_amd import _ffi, beamform as BF, engine as E, subspace as SS
from pyfft_amd.windows import get_window

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WIN = np.asarray(get_window("hann", R.NPERSEG), dtype=np.float64)


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


# ---- against the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.DEF_M)
def test_beamscan_against_the_definition(m):
    """three models with three scales in one call; every method, p, loading, nk around a tile, ndim, a phase 1e6 turns out, both outputs"""
    w, V = R.eig_of(m)
    worst = {}
    for nk, ndim, far in R.GEOMS:
        pos, kv = R.geometry(m, nk, ndim, far)
        for method, p, loading in R.variants(m):
            ref = [R.beam_def(V[s], w[s], pos, kv, method, p, loading, R.SCALES[s]) for s in range(3)]
            want = np.stack([r[0] for r in ref])
            bound = np.stack([R.beam_bound(V[s], w[s], pos, kv, method, p, loading, R.SCALES[s]) for s in range(3)])
            for out64 in (False, True):
                P, st = E.beamscan(V, w, pos, kv, method, p, loading, np.array(R.SCALES), out64)
                assert P.shape == (3, nk) and P.dtype == (np.float64 if out64 else np.float32) and st.shape == (3,) and st.dtype == np.int32
                assert not st.any() and not any(r[1] for r in ref) and not np.any(np.isnan(P))
                lim = bound + (0.0 if out64 else 2.0 ** -23 * np.abs(want))
                err = np.abs(P - want)
                assert np.all(err <= lim), (m, nk, ndim, far, method, p, loading, out64, float(np.max(err / lim)))
                if out64:
                    worst[method] = max(worst.get(method, 0.0), float(np.max(err / lim)))
    print("beamscan m %d: share of the bound %s" % (m, ", ".join("%s %.3f" % kv_ for kv_ in sorted(worst.items()))))


@pytest.mark.parametrize("method", ("music", "ev"))
def test_unit_spacing_is_the_pseudospectrum(method):
    """pos = i: the steering vector of sp_pseudospectrum, within the sum of the two bounds"""
    for m in R.DEF_M:
        w, V = R.eig_of(m)
        nb, start, step = 300, -0.3, 1.0 / 256
        for p in sorted({0, min(2, m - 1), m - 1}):
            Pp, _ = E.pseudospectrum(V, w, p, nb, start, step, method, True)
            nu = start + np.arange(nb) * step
            Pb, st = E.beamscan(V, w, np.arange(m, dtype=np.float64), nu, method, p, out64=True)
            assert not st.any()
            for s in range(3):
                want = R.beam_def(V[s], w[s], np.arange(m, dtype=np.float64), nu, method, p)[0]
                lim = R.beam_bound(V[s], w[s], np.arange(m, dtype=np.float64), nu, method, p) + S.pseudo_bound(V[s], w[s], p, nb, start, step, method) * want
                assert np.all(np.abs(Pb[s] - Pp[s]) <= lim), (m, p, s, float(np.max(np.abs(Pb[s] - Pp[s]) / lim)))


def test_flags_and_zero_sums():
    w, V = R.eig_of(23)
    w2 = w[0].copy()
    w2[-1], w2[-3] = 0.0, -2.0
    W, VV = np.stack([w[0], w2, np.zeros(23)]), np.stack([V[0], V[0], V[0]])
    pos, kv = R.geometry(23, 130, 2, False)
    for method, loading, flags in (("capon", 0.0, [0, 1, 1]), ("ev", 0.0, [0, 1, 1]), ("music", 0.0, [0, 0, 0]), ("bartlett", 0.0, [0, 0, 0])):
        P, st = E.beamscan(VV, W, pos, kv, method, 2, loading, None, True)
        assert list(st) == flags and np.all(np.isfinite(P)), method
        if method != "music":
            assert not P[2].any()                                        # a zero matrix: a sum of exactly zero
        for s in (0, 1):
            want, st_ref = R.beam_def(VV[s], W[s], pos, kv, method, 2, loading)
            assert st_ref == flags[s] and np.all(np.abs(P[s] - want) <= R.beam_bound(VV[s], W[s], pos, kv, method, 2, loading)), (method, s)
        Pd, std = E.beamscan(dev(VV), dev(W), pos, kv, method, 2, loading, None, True)
        assert Pd.is_cuda and np.array_equal(bits(Pd), bits(P)) and np.array_equal(std.cpu().numpy(), st)
    P, st = E.beamscan(VV, W, pos, kv, "capon", 0, 1e-3)                  # delta = loading max(trace, 0) / m lifts the zero, not the -2
    assert list(st) == [0, 1, 1]


# ---- invariants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
def test_bitwise(method, monkeypatch):
    """twice, host against device, scale=None against ones, one call of three models against three calls, SP_BEAM_GRID=1 against the default"""
    monkeypatch.delenv("SP_BEAM_GRID", raising=False)
    for m, nk, ndim in ((23, 300, 2), (64, 65, 3)):
        w, V = R.eig_of(m)
        pos, kv = R.geometry(m, nk, ndim, False)
        for out64 in (False, True):
            args = (pos, kv, method, 2, 1e-3)
            one, two = E.beamscan(V, w, *args, None, out64), E.beamscan(V, w, *args, None, out64)
            on_dev = E.beamscan(dev(V), dev(w), *args, None, out64)
            ones = E.beamscan(V, w, *args, np.ones(3), out64)
            assert on_dev[0].is_cuda and on_dev[0].dtype == (torch.float64 if out64 else torch.float32) and on_dev[1].dtype == torch.int32
            for a, b, c, d in zip(one, two, on_dev, ones):
                assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)) and np.array_equal(bits(a), bits(d))
            for s in range(3):
                Ps, sts = E.beamscan(V[s], w[s], *args, None, out64)
                assert Ps.shape == (nk,) and sts.shape == () and np.array_equal(bits(Ps), bits(one[0][s]))
            assert E.beam_plan(m, nk, 3, method, 2, ndim)["items_per_workgroup"] == 1
            monkeypatch.setenv("SP_BEAM_GRID", "1")
            assert E.beam_plan(m, nk, 3, method, 2, ndim)["items_per_workgroup"] == 3 * -(-nk // R.TQ) > 1       # one workgroup walks every item
            walked = E.beamscan(V, w, *args, None, out64)
            monkeypatch.setenv("SP_BEAM_GRID", "4")
            four = E.beamscan(dev(V), dev(w), *args, None, out64)
            monkeypatch.delenv("SP_BEAM_GRID")
            for a, b, c in zip(one, walked, four):
                assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    # leading axes
    w, V = R.eig_of(23)
    pos, kv = R.geometry(23, 70, 1, False)
    P4, st4 = E.beamscan(np.stack([V, V])[:, :, None], np.stack([w, w])[:, :, None], pos[:, 0], kv[:, 0], method, 2, scale=np.array(R.SCALES)[None, :, None])
    P1, st1 = E.beamscan(V, w, pos, kv, method, 2, scale=np.array(R.SCALES))
    assert P4.shape == (2, 3, 1, 70) and st4.shape == (2, 3, 1) and np.array_equal(bits(P4[1, :, 0]), bits(P1))


@pytest.mark.parametrize("lead", range(4))
def test_calls_at_offset_pointers_with_guarded_outputs(lead):
    """V and w inside NaN at both residues of their elements, P at a pitch inside sentinels, status inside integer guard words"""
    m, nk, P_ld = 23, 100, 107
    w, V = R.eig_of(m)
    pos, kv = R.geometry(m, nk, 2, False)
    li, lo = lead & 1, (lead >> 1) & 1
    Vb, Vv = G.poisoned_input(dev(V.reshape(-1)), li)
    wb, wv = G.poisoned_input(dev(w.reshape(-1)), li)
    snaps = G.snapshot(Vb), G.snapshot(wb)
    E._bind_stream(Vv)
    lib = _ffi.lib()
    scale = np.array(R.SCALES)
    for method, out64 in ((1, 0), (3, 1)):
        want, wst = E.beamscan(dev(V), dev(w), pos, kv, ("bartlett", "capon", "music", "ev")[method], 2, 1e-3, scale, bool(out64))
        Pb, Pa = G.sentinel_output(nk, torch.float64 if out64 else torch.float32, lo, device="cuda", rows=3, pitch=P_ld)
        tb, ta = G.sentinel_output(3, torch.int32, lo, device="cuda")
        rc = lib.sp_beamscan(_ffi.ptr(Vv.data_ptr()), m, _ffi.ptr(wv.data_ptr()), m, 3, _ffi.ptr(pos), 2, _ffi.ptr(kv), nk, _ffi.ptr(scale), method, 2, 1e-3, out64,
                             _ffi.ptr(Pa), P_ld, _ffi.ptr(ta), 1)
        assert rc == 0, lib.sp_last_error()
        torch.cuda.synchronize()
        assert G.unchanged(Vb, snaps[0]) and G.unchanged(wb, snaps[1])
        assert G.guards_intact(Pb, lo, nk, rows=3, pitch=P_ld) and G.all_written(Pb, lo, nk, rows=3, pitch=P_ld)
        assert G.guards_intact(tb, lo, 3) and G.all_written(tb, lo, 3)
        assert np.array_equal(bits(G.interior_of(Pb, lo, nk, rows=3, pitch=P_ld)), bits(want))
        assert np.array_equal(G.interior_of(tb, lo, 3).cpu().numpy(), wst.cpu().numpy())
    # host rows further apart keep what lies between
    base, inner = G.sentinel_output(nk, np.float32, 1, rows=3, pitch=P_ld)
    st = np.full(3, -77, dtype=np.int32)
    _ffi.init()
    rc = lib.sp_beamscan(_ffi.ptr(V), m, _ffi.ptr(w), m, 3, _ffi.ptr(pos), 2, _ffi.ptr(kv), nk, None, 0, 0, 0.0, 0, _ffi.ptr(int(inner.ctypes.data)), P_ld, _ffi.ptr(st), 0)
    assert rc == 0, lib.sp_last_error()
    assert G.guards_intact(base, 1, nk, rows=3, pitch=P_ld) and G.all_written(base, 1, nk, rows=3, pitch=P_ld) and not st.any()
    assert np.array_equal(bits(np.array(G.interior_of(base, 1, nk, rows=3, pitch=P_ld))), bits(E.beamscan(V, w, pos, kv)[0]))


def test_refusals_leave_the_outputs_untouched():
    m, nk = 23, 100
    w, V = R.eig_of(m)
    Vd, wd = dev(V), dev(w)
    pos, kv = R.geometry(m, nk, 2, False)
    E._bind_stream(Vd)
    lib = _ffi.lib()

    def call(m_=m, vld=m, nm=3, ndim=2, nk_=nk, pld=nk, method=3, p=2, loading=0.0, pos_=pos, kv_=kv, scale=None):
        bases = [G.sentinel_output(3 * nk, torch.float32, 1, device="cuda"), G.sentinel_output(3, torch.int32, 1, device="cuda")]
        rc = lib.sp_beamscan(_ffi.ptr(Vd.data_ptr()), vld, _ffi.ptr(wd.data_ptr()), m_, nm, _ffi.ptr(pos_), ndim, _ffi.ptr(kv_), nk_, _ffi.ptr(scale), method, p,
                             loading, 0, _ffi.ptr(bases[0][1]), pld, _ffi.ptr(bases[1][1]), 1)
        torch.cuda.synchronize()
        assert G.guards_intact(bases[0][0], 1, 3 * nk) and G.guards_intact(bases[1][0], 1, 3)
        untouched = all(bool((G._host_words(b[0]) == np.uint32(G.SENTINEL)).all()) for b in bases)
        return rc, (lib.sp_last_error() or b"").decode(), untouched

    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    nan_kv, inf_pos = kv.copy(), pos.copy()
    nan_kv[-1, -1], inf_pos[0, 0] = np.nan, np.inf
    for kw, word in ((dict(m_=1), "m must"), (dict(m_=65, vld=65), "m must"), (dict(vld=m - 1), "V_ld"), (dict(ndim=0), "ndim"), (dict(ndim=4), "ndim"),
                     (dict(nk_=0), "nk must"), (dict(pld=nk - 1), "P_ld"), (dict(method=4), "method"), (dict(p=m), "p must"), (dict(p=-1), "p must"),
                     (dict(loading=-1.0), "loading"), (dict(loading=float("nan")), "loading"), (dict(kv_=nan_kv), "kv must"), (dict(pos_=inf_pos), "pos must"),
                     (dict(scale=np.array([1.0, np.inf, 1.0])), "scale must"), (dict(nm=-1), "nmodels")):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg.startswith("sp_beamscan: ") and word in msg and untouched, (kw, rc, msg)
    rc, msg, untouched = call(nm=0)
    assert rc == 0 and untouched


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _spectrum(case, method, x=None, **kw):
    x = R.record(case) if x is None else x
    c = R.E2E[case]
    band = (c["f"] - 0.01, c["f"] + 0.01)
    ns = 2 if method in ("music", "ev") else None
    if case == "ring":
        return BF.mode_spectrum(x, R.sensors(case), R.RING_MODES, method=method, nsources=ns, nperseg=R.NPERSEG, band=band, out64=True, **kw)
    return BF.array_spectrum(x, R.sensors(case), R.scan(case), method=method, nsources=ns, nperseg=R.NPERSEG, band=band, out64=True, **kw)


@pytest.mark.parametrize("case", list(R.E2E))
def test_end_to_end(case):
    """ring: 16 unevenly placed coils, modes 2 and -3 at one frequency, all four methods put their two largest values there.  line: 12
    probes, two waves half a Rayleigh width apart: Capon, MUSIC and EV show both within a grid step, Bartlett has no peak within a grid
    step of the second.  Values against the all-float64 chain from the raw record."""
    c = R.E2E[case]
    Gm, w, V = R.e2e_matrix(case, WIN)
    assert w[1] / w[2] >= R.MIN_GAP                                      # the condition of the allowances, on the reference
    near = R.nearest(case)
    for method in R.METHODS:
        f, P = _spectrum(case, method)
        b = int(np.argmin(np.abs(f - c["f"])))
        assert abs(f[b] - c["bin"] / R.NPERSEG) < 1e-12 and P.shape == (len(f), len(R.scan(case))) and P.dtype == np.float64
        row, ref = P[b], R.e2e_reference(case, method, WIN)
        pk_ref, pk = R.peak_bins(ref, 2), R.peak_bins(row, 2)
        if case == "ring":
            assert sorted(pk_ref) == sorted(near) and sorted(pk) == sorted(near), (method, pk, near)
            assert sorted(np.argsort(-row)[:2]) == sorted(near)          # the two largest values, not only maxima
        elif method != "bartlett":
            for n in near:
                assert min(abs(int(i) - n) for i in pk_ref) <= 1 and min(abs(int(i) - n) for i in pk) <= 1, (method, pk, near)
        else:
            every = R.peak_bins(row, len(row))
            assert min(abs(int(i) - near[1]) for i in every) > 1 and min(abs(int(i) - near[1]) for i in R.peak_bins(ref, len(ref))) > 1
        if method == "bartlett":
            off, allow = float(np.max(np.abs(row - ref)) / np.max(ref)), R.CSDM_PARITY
        else:
            off, allow = float(np.max(np.abs(row - ref) / ref)), R.e2e_allowance(case, method)
        print("%s %s: %.2e of %.2e (share %.2g)" % (case, method, off, allow, off / allow))
        assert off <= allow, (case, method, off, allow)
    kp, pp = BF.beam_peaks(_spectrum(case, "capon")[1][b], R.scan(case), 2)
    assert np.max(np.abs(np.sort(kp) - np.sort(R.truth(case)))) <= (R.scan(case)[1] - R.scan(case)[0])


def test_the_front_ends_reduce_to_one_another():
    """mode_spectrum, beam_scan and slowness_scan are array_spectrum / engine.beamscan calls bit for bit; a device x stays on the device"""
    x, ang = R.record("ring")[:, :4096], R.sensors("ring")
    modes = R.RING_MODES
    for method, ns in (("capon", None), ("music", 2)):
        f, P = BF.mode_spectrum(x, ang, modes, fs=2.0, method=method, nsources=ns, loading=1e-3, nperseg=128, band=(0.2, 0.3))
        f2, P2 = BF.array_spectrum(x, ang, modes.astype(np.float64), fs=2.0, method=method, nsources=ns, loading=1e-3, nperseg=128, band=(0.2, 0.3))
        assert np.array_equal(f, f2) and np.array_equal(bits(P), bits(P2)) and P.dtype == np.float32 and P.shape == (len(f), 16)
        assert np.all((f >= 0.2) & (f <= 0.3)) and len(f) == 7
        fd, Pd = BF.mode_spectrum(dev(x), ang, modes, fs=2.0, method=method, nsources=ns, loading=1e-3, nperseg=128, band=(0.2, 0.3))
        assert Pd.is_cuda and np.array_equal(fd, f) and np.array_equal(bits(Pd), bits(P))
        # the same matrices by hand
        win = np.asarray(get_window("hann", 128), dtype=np.float64)
        Gm = E.csd_matrix(x, win, 64, 1 + (4096 - 128) // 64, detrend=True, scale=1.0 / (2.0 * float(np.sum(win * win))))
        Gb = Gm[13:20] * 2.0
        assert np.array_equal(np.fft.rfftfreq(128, 0.5)[13:20], f)
        Ps = BF.beam_scan(Gb, ang, modes, method=method, nsources=ns, loading=1e-3)
        assert np.array_equal(bits(Ps), bits(P))
        wv, Vv, _ = E.eigh(Gb)
        Pe, _ = E.beamscan(Vv, wv, ang, -modes / (2 * np.pi), method, ns or 0, 1e-3)
        assert np.array_equal(bits(Pe), bits(P))
        # slowness: k = 2 pi f s, formed per bin by the engine from one table
        s = np.linspace(-3.0, 3.0, 41)
        Pl = BF.slowness_scan(Gb, f, ang, s, method=method, nsources=ns, loading=1e-3)
        Pe, _ = E.beamscan(Vv, wv, ang, -s, method, ns or 0, 1e-3, scale=f)
        assert Pl.shape == (7, 41) and np.array_equal(bits(Pl), bits(Pe))
        for i in (0, 6):                                                   # ... which is the scan at k = 2 pi f s within the phase's rounding
            Pk = BF.beam_scan(Gb[i], ang, 2 * np.pi * f[i] * s, method=method, nsources=ns, loading=1e-3, out64=True)
            assert np.max(np.abs(Pl[i] - Pk) / Pk) <= 1e-5
        Pld = BF.slowness_scan(dev(Gb), f, ang, s, method=method, nsources=ns, loading=1e-3)
        assert Pld.is_cuda and np.array_equal(bits(Pld), bits(Pl))


# ---- what was there before stays bit for bit ---------------------------------------------------------------------------------------
def test_existing_calls_are_unchanged():
    """one pmusic and one spod call against the bits the commit before the array scan gave on an MI355X (tests/golden/beam_before.npz,
    taken with that commit's library)"""
    before = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_before.npz"))
    x = S.signals("frames")
    now = dict(zip(("music_f", "music_P"), SS.pmusic(x, 4, m=12, nfft=64, fs=2.0)))
    now.update(zip(("spod_f", "spod_lam", "spod_phi"), pyfft_amd.spod(R.record("ring")[:, :4096], fs=2.0, nperseg=64, nmodes=2)))
    assert sorted(before.files) == sorted(now)
    for key in before.files:
        assert before[key].dtype == now[key].dtype and np.array_equal(bits(before[key]), bits(now[key])), key


def test_exported():
    assert pyfft_amd.array_spectrum is BF.array_spectrum and pyfft_amd.mode_spectrum is BF.mode_spectrum and pyfft_amd.BeamRefused is E.BeamRefused
