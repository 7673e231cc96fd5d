"""Autoregressive fits and spectra on the GPU against the float64 definitions of tests/burg_ref.py: both forms of k_burg at the smallest
shapes at which each mechanism can go wrong, the lags and Levinson kernels across tile seams, the spectrum kernel, the geometry of
rows and frames, two passes, the invariants (bitwise repeatability, host and device calls, offset pointers inside poisoned buffers
with guarded pitched outputs, refusals and bad records that leave the outputs alone) and the front ends of pyfft_amd.parametric."""
import numpy as np
import pytest

import burg_ref as R
import guard_ref as G
import pyfft_amd
from pyfft_amd import _ffi, engine as E, parametric as PM

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FITS = {"burg": E.burg, "yule": E.yule}
ALLOW = {"burg": R.BURG_ALLOWANCE, "yule": R.YULE_ALLOWANCE}


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def run(name, method, monkeypatch=None, x=None):
    c = R.shape_of(name)
    if monkeypatch is not None:
        monkeypatch.setenv("SP_BURG_FORM", str(c["form"]))
    x = R.signals(name) if x is None else x
    return FITS[method](x, c["n"], c["hop"], c["first"], c["nframes"], c["p"])


def held(got, name, method, what):
    d = R.deviations(got, R.reference(name, method))
    print("%s %s: P %.2e k %.2e a %.2e E %.2e of %.2e (share %.2f)" % ((what, name) + d + (ALLOW[method], max(d) / ALLOW[method])))
    assert all(np.all(np.isfinite(np.asarray(v).view(np.float64))) for v in got)
    assert max(d) <= ALLOW[method], (what, name, d)
    return max(d) / ALLOW[method]


# ---- the fits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_burg_against_the_definition(name, monkeypatch):
    c = R.shape_of(name)
    got = run(name, "burg", monkeypatch)
    want_form = 1 if (c["n"] > R.CROSSOVER or c["form"] == 2) else 0
    assert E.ar_plan("burg", c["n"], c["p"], c["rows"], c["nframes"], c["cplx"])["form"] == want_form
    assert got[0].shape == (c["rows"], c["nframes"], c["p"] + 1) and got[2].shape == (c["rows"], c["nframes"], c["p"])
    assert got[0].dtype == (np.complex128 if c["cplx"] else np.float64) and got[1].dtype == np.float64 and np.all(got[0][..., 0] == 1)
    share = held(got, name, "burg", "engine.burg")
    assert share <= 1.0


@pytest.mark.parametrize("name", list(R.CASES) + list(R.YULE_ONLY))
def test_yule_against_the_definition(name):
    c = R.shape_of(name)
    got = run(name, "yule")
    assert E.ar_plan("yule", c["n"], c["p"], c["rows"], c["nframes"], c["cplx"])["form"] == 2
    held(got, name, "yule", "engine.yule")


def test_both_forms_run_the_crossover_length(monkeypatch):
    """the same record of CROSSOVER samples in the wave form and in the workgroup form: both within the allowance of one reference,
    and the forms differ from each other by the order of their float64 sums alone"""
    x = R.signals("w1024")
    monkeypatch.setenv("SP_BURG_FORM", "0")
    wave = E.burg(x, R.CROSSOVER, 1, 0, 1, 16)
    monkeypatch.setenv("SP_BURG_FORM", "2")
    wg = E.burg(x, R.CROSSOVER, 1, 0, 1, 16)
    held(wave, "w1024", "burg", "wave form")
    held(wg, "w1024", "burg", "workgroup form")
    assert np.max(np.abs(wave[2] - wg[2])) <= 1e-6 and not np.array_equal(wave[2], np.zeros_like(wave[2]))


def test_a_given_mean_and_no_detrend():
    name = "frames"
    c = R.shape_of(name)
    x = R.signals(name)
    for method in ("burg", "yule"):
        for kw, ref_kw in ((dict(detrend=False), dict(detrend=False)), (dict(mean_value=0.65), dict(detrend=True, mean_value=0.65))):
            got = FITS[method](x, c["n"], c["hop"], c["first"], c["nframes"], c["p"], **kw)
            ref = R.fit_def(x, c["n"], c["hop"], c["first"], c["nframes"], c["p"], method, **ref_kw)
            d = R.deviations(got, ref)
            assert max(d) <= ALLOW[method], (method, kw, d)


def test_two_passes(monkeypatch):
    name = "ragged"
    monkeypatch.setenv("SP_AR_SEGS", str(R.SEGS_HOOK))
    for method in ("burg", "yule"):
        got = run(name, method)
        assert E.last_passes(E.AR_PASSES) == 2 == E.ar_plan(method, 64, 3, 1, 11, True)["passes"]
        monkeypatch.delenv("SP_AR_SEGS")
        one = run(name, method)
        assert E.last_passes(7) == 1
        monkeypatch.setenv("SP_AR_SEGS", str(R.SEGS_HOOK))
        assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, one))
        held(got, name, method, "two passes")


def test_zero_and_constant_records_and_noiseless_tones():
    """finite everywhere, the zero model and zeros of P where E = 0; a noiseless tone (|k| -> 1) gets no value test"""
    n, p = 300, 6
    tone = np.cos(2 * np.pi * 0.123 * np.arange(2 * n)).astype(np.float32)
    x = np.stack([np.zeros(2 * n, dtype=np.float32), np.full(2 * n, 3.5, dtype=np.float32), tone])
    for fit in (E.burg, E.yule):
        a, e, k = fit(x, n, n, 0, 2, p)
        assert all(np.all(np.isfinite(v)) for v in (a, e, k))
        assert np.array_equal(a[:2], np.broadcast_to(np.eye(1, p + 1)[0], (2, 2, p + 1))) and not e[:2].any() and not k[:2].any()
        P = E.ar_psd(a, e[..., -1], 65, 0.0, 1.0 / 128)
        assert np.all(np.isfinite(P[:2])) and not P[:2].any() and not np.any(np.isnan(P))
    ac, ec, kc = E.burg(np.zeros(64, dtype=np.complex64), 64, 1, 0, 1, 4)
    assert ac.dtype == np.complex128 and np.array_equal(ac[0], np.eye(1, 5)[0]) and not ec.any() and not kc.any()


# ---- the spectrum ------------------------------------------------------------------------------------------------------------------
def _psd_bound(a, m, start, step):
    """the rounding of the float64 spectrum, relative to P: Horner's rule over p + 1 terms is off by 2 p u sum|a| at the most (u = 2^-53),
    a unit-circle point good to 2 u moves z^j by 2 j u, so the sum by another 2 p u sum|a|; relative to |A|, and twice that on |A|^2:
    8 (p + 1) u sum|a| / |A| = (p + 1) 2^-50 sum|a| / |A|"""
    nu = start + np.arange(m) * step
    A = np.abs(np.exp(-2j * np.pi * np.outer(nu - np.floor(nu), np.arange(len(a)))) @ a)
    return (len(a) + 1) * 2.0 ** -50 * np.sum(np.abs(a)) / A              # one more term for the reference's own sum


@pytest.mark.parametrize("m,start,step", [(1, 0.11, 0.0), (257, 0.0, 1.0 / 512), (4096, -0.5, 1.0 / 4096), (257, 1e6 + 0.37, 1e-3)])
def test_ar_psd_against_the_definition(m, start, step):
    refs = [R.reference("w333c", "burg"), R.reference("g8192c", "burg")]
    for ref in refs:
        a, Ev = ref[0][0], ref[1][0, :, -1]
        want = np.stack([R.psd_def(a[s], Ev[s], m, start, step, 0.5) for s in range(a.shape[0])])
        for out64 in (False, True):
            got = E.ar_psd(a, Ev, m, start, step, 0.5, out64)
            assert got.shape == (a.shape[0], m) and got.dtype == (np.float64 if out64 else np.float32)
            bound = np.stack([_psd_bound(a[s], m, start, step) for s in range(a.shape[0])]) + (0.0 if out64 else R.PSD_ALLOWANCE32)
            assert np.all(np.abs(got - want) <= bound * want), float(np.max(np.abs(got - want) / want))
    ar, Er, _ = R.reference("frames", "yule")
    wr = np.stack([[R.psd_def(ar[r, g], Er[r, g, -1], 257, 0.0, 1.0 / 512) for g in range(5)] for r in range(3)])
    gr = E.ar_psd(ar, Er[..., -1], 257, 0.0, 1.0 / 512, out64=True)
    br = np.stack([[_psd_bound(ar[r, g], 257, 0.0, 1.0 / 512) for g in range(5)] for r in range(3)])
    assert gr.shape == (3, 5, 257) and np.all(np.abs(gr - wr) <= br * wr)


def test_ar_psd_padded_rows_and_zero_power():
    a8 = R.reference("w333c", "burg")[0][0, 0]
    a4 = R.burg_def(R.segment(R.signals("w333c")[0], 333), 4)[0]
    A = np.stack([a8, np.concatenate([a4, np.zeros(4)]), a8])
    Ev = np.array([1.5, 0.7, 0.0])
    got = E.ar_psd(A, Ev, 129, 0.0, 1.0 / 128, out64=True)
    assert np.array_equal(got[1], E.ar_psd(a4[None], Ev[1:2], 129, 0.0, 1.0 / 128, out64=True)[0])      # a model of lower order, bit for bit
    assert np.max(np.abs(got[1] - R.psd_def(a4, 0.7, 129, 0.0, 1.0 / 128)) / got[1]) <= 1e-12
    assert not got[2].any() and np.all(got[0] > 0)


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("burg", "yule"))
@pytest.mark.parametrize("name", ("w333c", "g1025", "frames"))
def test_bitwise_twice_and_host_against_device(name, method):
    c = R.shape_of(name)
    x = R.signals(name)
    one, two = run(name, method), run(name, method)
    xd = dev(x)
    on_dev = FITS[method](xd, c["n"], c["hop"], c["first"], c["nframes"], c["p"])
    assert all(v.is_cuda for v in on_dev) and on_dev[0].dtype == (torch.complex128 if c["cplx"] else torch.float64)
    for a, b, d in zip(one, two, on_dev):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(d.cpu().numpy()).view(np.uint64))
    Ph = E.ar_psd(one[0], one[1][..., -1], 100, 0.1, 0.003)
    Pd = E.ar_psd(on_dev[0], on_dev[1][..., -1], 100, 0.1, 0.003)
    assert np.array_equal(Ph.view(np.uint32), Pd.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("method", ("burg", "yule"))
@pytest.mark.parametrize("lead", range(4))
def test_calls_at_offset_pointers_with_guarded_outputs(lead, method):
    """rows of x a pitch apart inside NaN, the three outputs out_ld apart inside sentinels, both residues of the 4- and 8-byte elements"""
    name = "frames"
    c = R.shape_of(name)
    x = R.signals(name)
    rows, nsig = x.shape
    n, p, nf = c["n"], c["p"], c["nframes"]
    segs, x_ld, o_ld = rows * nf, nsig + 5, p + 4
    lx, lo = lead & 1, (lead >> 1) & 1
    xb, xv = G.poisoned_input(dev(x), lx, pitch=x_ld)
    snap = G.snapshot(xb)
    got = [v.cpu().numpy() for v in FITS[method](xv, n, c["hop"], c["first"], nf, p)]
    held(got, name, method, "offset pointers, lead %d" % lead)
    E._bind_stream(xv)
    ab, aa = G.sentinel_output(p + 1, torch.float64, lo, device="cuda", rows=segs, pitch=o_ld)
    eb, ea = G.sentinel_output(p + 1, torch.float64, lo, device="cuda", rows=segs, pitch=o_ld)
    kb, ka = G.sentinel_output(p, torch.float64, lo, device="cuda", rows=segs, pitch=o_ld)
    entry = _ffi.lib().sp_burg if method == "burg" else _ffi.lib().sp_yule
    rc = entry(_ffi.ptr(xv.data_ptr()), _ffi.DTYPE_F32, x_ld, nsig, rows, n, c["hop"], c["first"], nf, p, _ffi.DETREND_SEGMEAN, 0.0, 0.0,
               _ffi.ptr(aa), _ffi.ptr(ea), _ffi.ptr(ka), o_ld, 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    torch.cuda.synchronize()
    assert G.unchanged(xb, snap)
    for base, ne, want in ((ab, p + 1, got[0]), (eb, p + 1, got[1]), (kb, p, got[2])):
        assert G.guards_intact(base, lo, ne, rows=segs, pitch=o_ld) and G.all_written(base, lo, ne, rows=segs, pitch=o_ld)
        inner = G.interior_of(base, lo, ne, rows=segs, pitch=o_ld).cpu().numpy()
        assert np.array_equal(inner.view(np.uint64), np.ascontiguousarray(want).reshape(segs, ne).view(np.uint64))


def test_host_models_further_apart_keep_what_lies_between():
    name = "frames"
    c = R.shape_of(name)
    x = np.array(R.signals(name))
    rows, nsig = x.shape
    p, nf = c["p"], c["nframes"]
    segs, o_ld = rows * nf, p + 3
    outs = [G.sentinel_output(ne, np.float64, 1, rows=segs, pitch=o_ld) for ne in (p + 1, p + 1, p)]
    _ffi.init()
    rc = _ffi.lib().sp_burg(_ffi.ptr(x), _ffi.DTYPE_F32, nsig, nsig, rows, c["n"], c["hop"], c["first"], nf, p, _ffi.DETREND_SEGMEAN, 0.0, 0.0,
                            *[_ffi.ptr(int(o[1].ctypes.data)) for o in outs], o_ld, 0)
    assert rc == 0, _ffi.lib().sp_last_error()
    want = run(name, "burg")
    for (base, _), ne, w in zip(outs, (p + 1, p + 1, p), want):
        assert G.guards_intact(base, 1, ne, rows=segs, pitch=o_ld) and G.all_written(base, 1, ne, rows=segs, pitch=o_ld)
        assert np.array_equal(np.array(G.interior_of(base, 1, ne, rows=segs, pitch=o_ld)).view(np.uint64), np.ascontiguousarray(w).reshape(segs, ne).view(np.uint64))


def test_host_spectra_further_apart_keep_what_lies_between():
    """sp_ar_psd on host memory with P_ld > m, float32 and float64: the rows are staged in both directions, so the room between them
    comes back as it was, every bin is written and the bits are those of the dense call"""
    a, e = np.array([[1.0, -0.5, 0.25, -0.1], [1.0, 0.3, -0.2, 0.05]]), np.array([1.0, 2.5])
    m, P_ld = 100, 107
    _ffi.init()
    for out64 in (False, True):
        base, inner = G.sentinel_output(m, np.float64 if out64 else np.float32, 1, rows=2, pitch=P_ld)
        rc = _ffi.lib().sp_ar_psd(_ffi.ptr(a), 0, 4, _ffi.ptr(e), 1, 3, 2, m, 0.1, 0.003, 1.0, int(out64), _ffi.ptr(int(inner.ctypes.data)), P_ld, 0)
        assert rc == 0, _ffi.lib().sp_last_error()
        assert G.guards_intact(base, 1, m, rows=2, pitch=P_ld) and G.all_written(base, 1, m, rows=2, pitch=P_ld)
        want = E.ar_psd(a, e, m, 0.1, 0.003, out64=out64)
        assert want.dtype == inner.dtype and np.array(G.interior_of(base, 1, m, rows=2, pitch=P_ld)).tobytes() == want.tobytes()


@pytest.mark.parametrize("method", ("burg", "yule"))
def test_refusals_and_bad_records_leave_the_outputs_untouched(method):
    name = "frames"
    c = R.shape_of(name)
    xd = dev(R.signals(name))
    rows, nsig = xd.shape
    n, p, nf = c["n"], c["p"], c["nframes"]
    E._bind_stream(xd)
    lib = _ffi.lib()
    entry = lib.sp_burg if method == "burg" else lib.sp_yule

    def call(xx=xd, n_=n, hop=c["hop"], first=c["first"], nf_=nf, p_=p, old=p + 1, det=_ffi.DETREND_SEGMEAN):
        bases = [G.sentinel_output(rows * nf * (p + 1), torch.float64, 1, device="cuda") for _ in range(3)]
        rc = entry(_ffi.ptr(xx.data_ptr()), _ffi.DTYPE_F32, nsig, nsig, rows, n_, hop, first, nf_, p_, det, 0.0, 0.0,
                   *[_ffi.ptr(b[1]) for b in bases], old, 1)
        torch.cuda.synchronize()
        assert all(G.guards_intact(b[0], 1, rows * nf * (p + 1)) for b in bases)
        untouched = all(bool((G._host_words(b[0]) == np.uint32(G.SENTINEL)).all()) for b in bases)
        return rc, (lib.sp_last_error() or b"").decode(), untouched

    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    who = "sp_" + method
    for kw, word in ((dict(p_=0), "order"), (dict(p_=101, old=102), "n / 2"), (dict(hop=0), "hop"), (dict(first=-1), "first"), (dict(nf_=nf + 1), "reach outside"),
                     (dict(old=p), "out_ld"), (dict(det=2), "detrend"), (dict(n_=1), "n must")):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg.startswith(who + ": ") and word in msg and untouched, (kw, rc, msg)
    for where in ((0, c["first"]), (rows - 1, c["first"] + (nf - 1) * c["hop"] + n - 1), (1, c["first"] + 150)):
        xn = xd.clone()
        xn[where] = float("nan") if where[0] else float("inf")
        rc, msg, untouched = call(xx=xn)
        assert rc == E.AR_BAD_RECORD == -2 and msg.startswith(who + ": ") and "not finite" in msg and untouched, (where, rc, msg)
        with pytest.raises(E.ArRefused, match="not finite"):
            FITS[method](xn, n, c["hop"], c["first"], nf, p)
    xn = xd.clone()
    xn[0, 0], xn[2, nsig - 1] = float("nan"), float("nan")                 # outside every segment: not looked at
    rc, msg, untouched = call(xx=xn)
    assert rc == 0 and not untouched


# ---- the front ends ----------------------------------------------------------------------------------------------------------------
def test_pburg_is_ar_psd_of_arburg():
    x = R.signals("frames")
    a, e, k = PM.arburg(x, 6)
    assert a.shape == (3, 7) and e.shape == (3,) and k.shape == (3, 6)
    ref = R.fit_def(x, x.shape[1], 1, 0, 1, 6, "burg", detrend=False)
    assert max(R.deviations((a[:, None], PM.arburg(x, 6, evar=True)[1][:, None], k[:, None]), ref)) <= R.BURG_ALLOWANCE
    f, P = PM.pburg(x, 6, nfft=128, fs=4.0)
    f2, P2 = PM.ar_psd(a, e, nfft=128, fs=4.0)
    assert np.array_equal(f, f2) and np.array_equal(f, np.arange(65) * 4.0 / 128) and np.array_equal(P, P2) and P.shape == (3, 65) and P.dtype == np.float32
    two = PM.pburg(x, 6, nfft=128, fs=4.0, return_onesided=False)[1]
    assert two.shape == (3, 128) and np.array_equal(P[:, 0], two[:, 0]) and np.array_equal(P[:, 64], two[:, 64])      # DC and Nyquist are left alone
    assert np.array_equal(P[:, 1:64], 2 * two[:, 1:64])
    want = np.stack([R.psd_def(ref[0][r, 0], ref[1][r, 0, -1], 128, 0.0, 1.0 / 128, 0.25) for r in range(3)])
    assert np.max(np.abs(two - want) / want) <= R.BURG_ALLOWANCE + R.PSD_ALLOWANCE32
    fz, Pz = PM.pburg(x, 6, fs=4.0, band=(0.3, 0.6), m=33, out64=True)
    wz = np.stack([2 * R.psd_def(ref[0][r, 0], ref[1][r, 0, -1], 33, 0.3 / 4, 0.3 / 4 / 32, 0.25) for r in range(3)])
    assert np.allclose(fz, np.linspace(0.3, 0.6, 33)) and np.max(np.abs(Pz - wz) / wz) <= R.BURG_ALLOWANCE
    xc = R.signals("w333c")
    fc, Pc = PM.pburg(xc, 8, nfft=64)
    assert Pc.shape == (1, 64) and np.array_equal(fc, np.fft.fftfreq(64))                       # a complex record is two-sided
    Pd = PM.pburg(dev(x), 6, nfft=128, fs=4.0)[1]
    assert Pd.is_cuda and np.array_equal(Pd.cpu().numpy(), P)


@pytest.mark.parametrize("method", ("burg", "yule"))
def test_spectrogram_columns_are_the_slices_spectra(method):
    x = R.signals("frames")[:, :413]
    f, t, S = PM.ar_spectrogram(x, 6, 100, noverlap=23, method=method, fs=2.0, nfft=64)
    hop, nf = 77, (413 - 100) // 77 + 1
    assert S.shape == (3, 33, nf) and np.array_equal(t, (np.arange(nf) * hop + 50.0) / 2.0)
    one = PM.pburg if method == "burg" else PM.pyulear
    for g in range(nf):
        fg, Pg = one(x[:, g * hop:g * hop + 100], 6, nfft=64, fs=2.0, detrend=True)
        assert np.array_equal(fg, f) and np.array_equal(S[..., g], Pg), g
    Sd = PM.ar_spectrogram(dev(np.array(x)), 6, 100, noverlap=23, method=method, fs=2.0, nfft=64)[2]
    assert Sd.is_cuda and np.array_equal(Sd.cpu().numpy(), S)


def test_order_stepup_psd_equals_a_direct_fit():
    x = R.signals("w1024")
    a, ev, k = PM.arburg(x, 16, detrend=True, evar=True)
    order = PM.ar_order(ev, 1024, "mdl")
    assert order.shape == (1,) and 4 <= order[0] <= 16
    q = int(order[0])
    low = PM.ar_stepup(k, q)
    direct = PM.arburg(x, q, detrend=True)
    # the lattice is nested: the order-16 fit's first q reflection coefficients and q + 1 powers ARE the order-q fit's, bit for bit
    kq, evq = PM.arburg(x, q, detrend=True, evar=True)[2], PM.arburg(x, q, detrend=True, evar=True)[1]
    assert np.array_equal(k[:, :q], direct[2]) and np.array_equal(k[:, :q], kq) and np.array_equal(ev[:, :q + 1], evq) and ev[0, q] == direct[1][0]
    # so the host's float64 step-up differs from the kernel's by rounding alone: a step adds 2 u max|a_m| (u = 2^-53) and carries what
    # it was given times 1 + |k_m| at the most, and max|a_m| <= prod (1 + |k_i|): q 2^-52 prod_{i <= q} (1 + |k_i|)
    assert np.max(np.abs(low - direct[0])) <= q * 2.0 ** -52 * np.prod(1 + np.abs(k[0, :q]))
    P1, P2 = PM.ar_psd(low, ev[:, q], nfft=256, out64=True)[1], PM.ar_psd(direct[0], direct[1], nfft=256, out64=True)[1]
    off = float(np.max(np.abs(P1 - P2) / P2))
    print("ar_order + ar_stepup + ar_psd against the direct fit at order %d: %.2e of %.2e" % (q, off, R.BURG_ALLOWANCE))
    assert off <= R.BURG_ALLOWANCE
    kd = dev(k)
    assert np.array_equal(PM.ar_stepup(kd, q).cpu().numpy(), low) and int(PM.ar_order(dev(ev), 1024, "mdl")[0]) == q


def test_pyulear_integrates_to_the_mean_square():
    """the Yule-Walker model matches r[0]; on nfft bins the mean of the two-sided density aliases rho[l nfft], l != 0, which decays like
    R^nfft with R the largest pole radius: nfft = 4096 and R < 0.99 leave 1e-17, so what remains is the fit's float32 allowance"""
    x = R.signals("w1024")
    a, e, k = PM.aryule(x, 16, detrend=True)
    assert np.max(np.abs(np.roots(a[0]))) < 0.99
    f, P = PM.pyulear(x, 16, nfft=4096, fs=3.0, return_onesided=False, detrend=True, out64=True)
    ms = np.var(x.astype(np.float64))                                  # the mean square of the record less its mean
    assert abs(np.sum(P) * 3.0 / 4096 - ms) <= R.YULE_ALLOWANCE * ms
    f1, P1 = PM.pyulear(x, 16, nfft=4096, fs=3.0, detrend=True, out64=True)
    assert abs(np.sum(P1) * 3.0 / 4096 - ms) <= R.YULE_ALLOWANCE * ms                     # one-sided: the same integral over [0, fs / 2]


def test_exported():
    assert pyfft_amd.pburg is PM.pburg and pyfft_amd.ar_spectrogram is PM.ar_spectrogram
