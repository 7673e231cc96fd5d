"""Device-resident calls at offset pointers inside poisoned buffers (tests/guard_ref.py holds the instrument and the case table).

Group A enters pyfft_amd.engine with device tensors that are contiguous views `lead` elements into a NaN-filled allocation (and, where
the engine passes strided rows through, rows n + 3 apart): the pointer has the residue of `lead` elements modulo 16, which every
placement asserts, the view is contiguous, so engine.py's .contiguous() hands its address through unchanged, and everything next to the
samples is NaN.  Each result must be finite and within the entry's existing tolerance of the float64 reference; for biquad_filter,
sos_filter, upfirdn and ddc, where the pointer only changes how samples are staged, every placement must also give the bits of the
aligned one (the pitched cases compare lead 1 with lead 0 at the same pitch: k_ddc's oscillator follows the row pitch, see guard_ref).
The allocation of every input must come back unchanged.

Group B calls the C ABI (mem = 1) with a poisoned input and the interior of a sentinel-filled allocation as the output: the guard
words must be intact, every interior word written, the interior finite and within the same tolerance.

include/spectral.h demands no more than natural alignment of any pointer (it never mentions alignment), so no entry has a refusal
to exercise below it: every lead here is inside the contract."""
import numpy as np
import pytest
import scipy.signal as ss

import guard_ref as G
from guard_ref import wide
from pyfft_amd import _ffi, engine as E

pytestmark = pytest.mark.gpu

IDS = [c.id for c in G.INPUT_CASES]
_RESTATED = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    _ffi.init()
    return torch


def place(torch, arrays, run):
    """the arrays on the device, each at its (lead, extra pitch) -> (bases, views, snapshots)"""
    bases, views = [], []
    for a, (lead, extra) in zip(arrays, run):
        t = torch.as_tensor(a, device="cuda")
        base, view = G.poisoned_input(t, lead, pitch=a.shape[-1] + extra if extra else None)
        assert view.data_ptr() % 16 == (lead * t.element_size()) % 16
        if not extra:
            assert view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
        else:
            assert view.stride(0) == a.shape[-1] + extra and view.stride(1) == 1
        bases.append(base)
        views.append(view)
    return bases, views, [G.snapshot(b) for b in bases]


def host(v):
    if isinstance(v, (tuple, list)):
        return tuple(host(u) for u in v)
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def call(case, d, v):
    """the engine call of the case on the device views v"""
    import pyfft_amd
    import detrend_ref as R
    from pyfft_amd import filters
    p, f = case.p, case.family
    if f == "mean":
        return E.mean(v[0])
    if f == "biquad_filter":
        return E.biquad_filter(d["b"], d["a"], v[0])
    if f == "sos_filter":
        return E.sos_filter(d["sos"], v[0])
    if f == "sosfiltfilt":
        return filters.sosfiltfilt(d["sos"], v[0])
    if f == "upfirdn":
        return E.upfirdn(v[0], d["h"], p["up"], p["down"])
    if f == "ddc":
        return E.ddc(v[0], G.NU, p["q"], d["h"], n0=G.N0)
    if f == "fir_filter":
        return E.fir_filter(d["h"], v[0], nfft=p["nfft"])
    if f == "hilbert_rows":
        return E.hilbert_rows(v[0], p["n"])
    if f == "spectral_filter_rows":
        return E.spectral_filter_rows(v[0], d["H"])
    if f == "xcorr_normalised":
        return E.xcorr_normalised(v[0], v[1])
    if f in ("welch_psd", "stft_frames", "stft_cog", "frame_sum", "welch_csd"):
        det = G.DETREND_MODE[p.get("mode", "mean")]
        nfft, hop, M = p["nfft"], p["hop"], p["M"]
        if f == "frame_sum":
            return E.frame_sum(v[0], nfft, hop, M, detrend=det)
        win = d["win"]
        if f == "welch_psd":
            return E.welch_psd(v[0], win, hop, M, detrend=det, sided=E.SIDED_TWO, scale=1.0 / float(np.sum(win ** 2)))
        if f == "stft_frames":
            return E.stft_frames(v[0], win, hop, M, detrend=det, sided=E.SIDED_ONE, amp_scale=1.0 / float(np.sum(win)), want_pseg=True)
        if f == "stft_cog":
            return E.stft_cog(v[0], win, hop, M, R.FS, detrend=det)
        return E.welch_csd(v[0], v[1], win, hop, M, detrend=det, sided=E.SIDED_ONE, scale=1.0 / float(np.sum(win ** 2)))
    if f == "csd_matrix":
        return E.csd_matrix(v[0], d["win"], p["hop"], p["M"], detrend=True, scale=1.0)
    if f == "pfb":
        return E.pfb(v[0], d["h"], p["M"], p["D"], d["first"], p["nf"], 1, d["r0"])
    if f == "czt":
        return E.czt(v[0], p["m"], d["start"], d["step"])
    if f == "xcorr_frames":
        nw, maxlag, hop, _ = d["shape"]
        return E.xcorr_frames(v[0], v[1], nw, hop, p["nframes"], maxlag, frames=True)[0]
    if f == "welch_blocks":
        win = d["win"]
        nframes = (len(d["arrays"][0]) - p["nfft"]) // p["hop"] + 1
        return E.welch_blocks(v[0], win, p["hop"], nframes, p["navg"], p["step"], y=v[1], detrend=True,
                              scale=1.0 / float(np.sum(win ** 2)), doubled=True)
    if f == "multitaper":
        return pyfft_amd.multitaper_spectra(v[0], v[1], **d["kw"])[1:]
    if f == "bispectrum":
        return E.bispectrum(v[0], d["win"], d["hop"], p["M"], detrend=1)
    if f == "skf":
        nfft, hop, nk, (b0, nb), _ = d["shape"]
        return E.skf(v[0], v[1], nfft, hop, p["nframes"], b0, nb, nk, win=d["win"], segmean=True, cross=False, scale=d["scale"])
    raise KeyError(f)


def peak_err(got, ref):
    return float(np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref)))


def rowerr(y, ref):
    y = np.asarray(y, dtype=np.float64)
    return float(np.max(np.max(np.abs(y - ref), axis=-1) / np.max(np.abs(ref), axis=-1)))


def restated(case, d):
    """(rms of the reference, what a float32 numpy restatement of the same sum loses of it): the bound of tests/test_gpu_resample.py
    and tests/test_gpu_baseband.py is 4 x that loss.  Computed once per case."""
    if case.id not in _RESTATED:
        ref = G.reference(case)
        x = d["arrays"][0]
        if case.family == "upfirdn":
            from test_host_resample import upfirdn_ref
            f32 = upfirdn_ref(d["h"], x, case.p["up"], case.p["down"], dtype=np.float32)
        else:
            from test_gpu_baseband import ddc_f32
            f32 = ddc_f32(x, G.NU, case.p["q"], d["h"], G.N0)
        rms = float(np.sqrt(np.mean(np.abs(ref) ** 2)))
        loss = float(np.max(np.abs(f32.astype(ref.dtype) - ref))) / rms
        assert 0 < loss < 1e-4                                           # a guard on the restatement itself, not the bound
        _RESTATED[case.id] = (rms, loss)
    return _RESTATED[case.id]


def spec_tol(ref):
    return 2e-4 * np.abs(ref) + 1e-6 * float(np.max(np.abs(ref)))


def within(got, ref, tol, what):
    got = np.asarray(got)
    assert got.shape == np.shape(ref), (what, got.shape, np.shape(ref))
    r = float(np.max(np.abs(got - ref) / tol))
    print("%s: %.3g of the tolerance" % (what, r))
    assert r <= 1.0, "%s: error %.3g tolerances" % (what, r)


def check(case, d, got, ref, what):
    """finite, and within the entry's existing tolerance of the float64 reference"""
    import detrend_ref as R
    p, f = case.p, case.family
    for a in (got if isinstance(got, tuple) else (got,)):
        if f != "bispectrum":
            assert np.all(np.isfinite(a)), what
    if f == "mean":
        assert abs(got - ref) < 1e-9, (what, got, ref)
    elif f == "biquad_filter":
        assert got.dtype == np.float32 and got.shape == ref.shape and peak_err(got, ref) <= 3e-7, (what, peak_err(got, ref))
    elif f in ("sos_filter", "sosfiltfilt"):
        assert got.dtype == np.float32 and got.shape == ref.shape and rowerr(got, ref) <= 5e-7, (what, rowerr(got, ref))
    elif f in ("upfirdn", "ddc"):
        rms, loss = restated(case, d)
        assert got.shape == ref.shape and got.dtype == (np.float32 if f == "upfirdn" and not case.cplx else np.complex64), what
        err = float(np.max(np.abs(got.astype(ref.dtype) - ref))) / rms
        print("%s: max err / rms = %.3g (bound %.3g)" % (what, err, 4.0 * loss))
        assert err <= 4.0 * loss, what
    elif f in ("fir_filter", "hilbert_rows", "spectral_filter_rows"):
        tol = 2e-5 if p["n"] >= (1 << 21) else 1e-4
        assert got.shape == ref.shape and peak_err(got, ref) <= tol, (what, peak_err(got, ref))
    elif f == "xcorr_normalised":
        assert got.shape == ref.shape and peak_err(got, ref) <= 1e-4, (what, peak_err(got, ref))
        assert np.argmax(got) == np.argmax(ref), what
    elif f == "welch_psd":
        within(got, ref, spec_tol(ref), what)
    elif f == "stft_frames":
        assert got[0].dtype == np.complex64
        within(got[0], ref[0], 1e-4 * float(np.max(np.abs(ref[0]))), what)
        within(got[1], ref[1], 1e-4 * ref[1], what + " pseg")
    elif f == "stft_cog":
        within(got, ref, 2e-4 * R.FS, what)
    elif f == "frame_sum":
        within(got, ref, 2e-5 * float(np.max(np.abs(wide(d["arrays"][0])))) * p["M"], what)
    elif f == "welch_csd":
        (pxx, pyy, pxy), (rxx, ryy, rxy) = got, ref
        within(pxx, rxx, spec_tol(rxx), what + " pxx")
        within(pyy, ryy, 2e-4 * ryy + 1e-6 * ryy.max(axis=1, keepdims=True), what + " pyy")
        geo = np.sqrt(rxx[None, :] * ryy)
        within(pxy, rxy, 2e-4 * geo + 1e-6 * geo.max(axis=1, keepdims=True), what + " pxy")
    elif f == "csd_matrix":
        from test_gpu_kernels import _csd_per_bin_excess
        assert got.shape == ref.shape and _csd_per_bin_excess(got, ref) <= 1.0, (what, _csd_per_bin_excess(got, ref))
    elif f in ("pfb", "czt"):
        assert got.shape == ref.shape and got.dtype == np.complex64 and peak_err(got, ref) <= 1e-4, (what, peak_err(got, ref))
    elif f == "xcorr_frames":
        assert got.shape == ref.shape and peak_err(got.astype(ref.dtype), ref) <= 1e-4, (what, peak_err(got, ref))
    elif f == "welch_blocks":
        from test_gpu_welch_blocks import within as blocks_within
        blocks_within(got, ref, what)
    elif f == "multitaper":
        from test_gpu_multitaper import assert_psd, assert_cross
        assert_psd(got[0], ref[0], what + " pxx")
        assert_psd(got[1], ref[1], what + " pyy")
        assert_cross(got[2], ref[2], what + " pxy")
    elif f == "bispectrum":
        from test_gpu_bispectrum import assert_parity
        (B, b2, P), (Bo, b2o, A, Po) = got, ref
        assert_parity(B, b2, Bo, b2o, A)
        assert np.all(np.isfinite(P))
        np.testing.assert_allclose(P, Po, rtol=1e-5, atol=1e-7 * Po.max())
    elif f == "skf":
        from test_gpu_skf import within as skf_within
        skf_within(got, d["ref"], d["psd"], what)
    else:
        raise KeyError(f)


def same_bits(a, b):
    return all(u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(a if isinstance(a, tuple) else (a,),
                                                                                 b if isinstance(b, tuple) else (b,)))


# ======================================================================================================================== group A
@pytest.mark.parametrize("case", G.INPUT_CASES, ids=IDS)
def test_input_side(torch, case):
    d = G.inputs(case)
    ref = G.reference(case)
    first = None
    for run in case.places:
        what = "%s at %s" % (case.id, run)
        bases, views, snaps = place(torch, d["arrays"], run)
        got = host(call(case, d, views))
        torch.cuda.synchronize()
        for b, s in zip(bases, snaps):
            assert G.unchanged(b, s), what + ": the call wrote into its input's allocation"
        check(case, d, got, ref, what)
        if case.family in G.BITWISE:
            if first is None:
                assert all(lead == 0 for lead, _ in run)
                first = got
            else:
                assert same_bits(got, first), what + ": differs from the aligned placement's bits"


# ======================================================================================================================== group B
def case_of(name):
    return G.BY_ID[name]


LEAD_PAIRS = {(False, False): [(0, 0), (0, 1), (1, 0), (3, 3), (2, 1), (0, 3)], (False, True): [(0, 0), (0, 1), (1, 0), (3, 1), (2, 0)],
              (True, True): [(0, 0), (0, 1), (1, 0), (1, 1)], (True, False): [(0, 0), (0, 1), (1, 0), (1, 3), (0, 3)]}


def lead_pairs(in_cplx, out_cplx):
    """(input lead, output lead) pairs: both aligned first, then aligned in / misaligned out, the converse, and both misaligned; the
    output leads are {0, 1, 3} for float32 and {0, 1} for complex64"""
    return LEAD_PAIRS[in_cplx, out_cplx]


class Out:
    """an output region inside a sentinel-filled device allocation"""

    def __init__(self, nelem, dtype, lead, rows=1):
        self.args = (lead, nelem)
        self.rows = rows
        self.base, self.ptr = G.sentinel_output(nelem, dtype, lead, device="cuda", rows=rows)
        assert self.ptr % 16 == (lead * self.base.element_size()) % 16

    def result(self, what):
        """guards intact, every word written, finite -> the interior on the host"""
        assert G.guards_intact(self.base, *self.args, rows=self.rows), what
        hole = G.first_unwritten(self.base, *self.args, rows=self.rows)
        assert hole is None, "%s: element %d of the output was never written" % (what, hole)
        a = G.interior_of(self.base, *self.args, rows=self.rows).cpu().numpy()
        assert np.all(np.isfinite(a)), what
        return a


def sync_ok(torch, rc, what):
    assert rc == 0, (what, _ffi.lib().sp_last_error())
    torch.cuda.synchronize()


def run_b(torch, name, outputs, invoke, in_cplx=False, out_cplx=False, pairs=None, bitwise=False, judge=None):
    """One C entry over the lead pairs.  outputs(out_lead) -> list of Out; invoke(views, outs) -> rc; the first output is checked
    against the case's reference with the case's tolerance (judge overrides), every output for its guards."""
    case = case_of(name)
    d, ref = G.inputs(case), G.reference(case)
    first = None
    for li, lo in (lead_pairs(in_cplx, out_cplx) if pairs is None else pairs):
        what = "%s in %d out %d" % (name, li, lo)
        bases, views, snaps = place(torch, d["arrays"], ((li, 0),) * len(d["arrays"]))
        E._bind_stream(views[0])
        outs = outputs(lo)
        sync_ok(torch, invoke(views, outs), what)
        got = tuple(o.result(what) for o in outs)
        for b, s in zip(bases, snaps):
            assert G.unchanged(b, s), what
        if judge is None:
            check(case, d, got[0].reshape(np.shape(ref)), ref, what)
        else:
            judge(got, what)
        if bitwise:
            if first is None:
                assert (li, lo) == (0, 0)
                first = got
            else:
                assert same_bits(got, first), what + ": differs from the aligned call's bits"


def p_(x):
    return _ffi.ptr(x if isinstance(x, (int, np.ndarray)) or x is None else x.data_ptr())


def test_sp_biquad(torch):
    lib, name = _ffi.lib(), "biquad_filter-f32-notch-n%d" % (2 * G.TILE + 5)
    d = G.inputs(case_of(name))
    n = d["arrays"][0].size
    b, a = (np.ascontiguousarray(c, dtype=np.float64) for c in (d["b"], d["a"]))
    run_b(torch, name, lambda lo: [Out(n, torch.float32, lo)],
          lambda v, o: lib.sp_biquad(p_(b), p_(a), p_(v[0]), n, p_(o[0].ptr), 1), bitwise=True)


def test_sp_sosfilt_with_zf(torch):
    lib, name = _ffi.lib(), "sos_filter-f32-K3-bandpass"
    d = G.inputs(case_of(name))
    x = d["arrays"][0]
    R, n = x.shape
    sos = np.ascontiguousarray(d["sos"])
    K = sos.shape[0]
    zi = ss.sosfilt_zi(sos)[:, None, :] * wide(x)[:, 0][None, :, None]                     # (K, rows, 2), scipy's layout
    want, zf_want = ss.sosfilt(sos, wide(x), axis=-1, zi=zi)
    zi_dev = torch.as_tensor(np.ascontiguousarray(zi.transpose(1, 0, 2)), device="cuda")     # [R][K][2]

    def judge(got, what):
        y, zf = got[0].reshape(R, n), got[1].reshape(R, K, 2).transpose(1, 0, 2)
        assert rowerr(y, want) <= 5e-7, (what, rowerr(y, want))
        assert np.abs(zf - zf_want).max() <= 1e-6 * np.abs(zf_want).max(), what

    run_b(torch, name, lambda lo: [Out(n, torch.float32, lo, rows=R), Out(R * K * 2, torch.float64, lo % 2)],
          lambda v, o: lib.sp_sosfilt(p_(sos), K, p_(v[0]), R, n, p_(zi_dev), p_(o[0].ptr), p_(o[1].ptr), 1), bitwise=True, judge=judge)


def test_sp_sosfiltfilt(torch):
    from pyfft_amd import filters
    lib, name = _ffi.lib(), "sosfiltfilt-f32-K3-bandpass"
    d = G.inputs(case_of(name))
    R, n = d["arrays"][0].shape
    sos = np.ascontiguousarray(d["sos"])
    padlen = filters._sos_padlen(sos)
    run_b(torch, name, lambda lo: [Out(n, torch.float32, lo, rows=R)],
          lambda v, o: lib.sp_sosfiltfilt(p_(sos), sos.shape[0], p_(v[0]), R, n, E.PADTYPES["odd"], padlen, p_(o[0].ptr), 1))


@pytest.mark.parametrize("cplx", [False, True], ids=["f32", "c64"])
def test_sp_upfirdn(torch, cplx):
    lib, name = _ffi.lib(), "upfirdn-%s-3-2" % ("c64" if cplx else "f32")
    case = case_of(name)
    d = G.inputs(case)
    rows, n = d["arrays"][0].shape
    h = np.ascontiguousarray(d["h"], dtype=np.float32)
    nout = G.reference(case).shape[-1]
    assert nout % G.upfirdn_n(case)[1]                                                     # a ragged last tile
    run_b(torch, name, lambda lo: [Out(nout, torch.complex64 if cplx else torch.float32, lo, rows=rows)],
          lambda v, o: lib.sp_upfirdn(p_(v[0]), int(cplx), n, n, rows, p_(h), h.size, 3, 2, 0, nout, p_(o[0].ptr), 1),
          in_cplx=cplx, out_cplx=cplx, bitwise=True)


@pytest.mark.parametrize("cplx", [False, True], ids=["f32", "c64"])
def test_sp_ddc(torch, cplx):
    lib, name = _ffi.lib(), "ddc-%s-q8" % ("c64" if cplx else "f32")
    case = case_of(name)
    d = G.inputs(case)
    rows, n = d["arrays"][0].shape
    h = np.ascontiguousarray(d["h"], dtype=np.float32)
    nout = -(-n // 8)
    assert nout % G.ddc_n(case)[1]
    run_b(torch, name, lambda lo: [Out(nout, torch.complex64, lo, rows=rows)],
          lambda v, o: lib.sp_ddc(p_(v[0]), int(cplx), n, n, rows, G.NU, G.N0, 8, p_(h), h.size, p_(o[0].ptr), 1),
          in_cplx=cplx, out_cplx=True, bitwise=True)


def test_sp_fftfilt(torch):
    lib, name = _ffi.lib(), "fir_filter-f32-31-5000-1024"
    d = G.inputs(case_of(name))
    n = d["arrays"][0].size
    h = np.ascontiguousarray(d["h"], dtype=np.float32)
    run_b(torch, name, lambda lo: [Out(n, torch.float32, lo)],
          lambda v, o: lib.sp_fftfilt(p_(h), h.size, p_(v[0]), n, 1024, p_(o[0].ptr), 1))


@pytest.mark.parametrize("rows,n", [(2, 1000), (2, 4096), (1, 1 << 21)])
def test_sp_hilbert(torch, rows, n):
    lib, name = _ffi.lib(), "hilbert_rows-f32-%dx%d" % (rows, n)
    pairs = None
    if n == 1 << 21:
        pairs = [(0, 1), (1, 1)]          # an output that is 8-byte aligned only: the path behind the failed 16-byte test, held to 2e-5

    def outputs(lo):
        o = Out(n, torch.complex64, lo, rows=rows)
        if n == 1 << 21:
            assert o.ptr % 16 == 8
        return [o]
    run_b(torch, name, outputs, lambda v, o: lib.sp_hilbert(p_(v[0]), n, n, n, rows, p_(o[0].ptr), 1), out_cplx=True, pairs=pairs)


def test_sp_xcorr(torch):
    lib, name = _ffi.lib(), "xcorr_normalised-f32-n777"
    n = 777
    run_b(torch, name, lambda lo: [Out(2 * n - 1, torch.float32, lo)],
          lambda v, o: lib.sp_xcorr(p_(v[0]), p_(v[1]), n, p_(o[0].ptr), 1))


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_sp_fft_c2c(torch, inplace):
    lib = _ffi.lib()
    n, batch = 1000, 3
    x = G.noise(batch * n, True, 1000, 0.7).reshape(batch, n)
    ref = np.fft.fft(wide(x), axis=-1)
    tol = 4e-6 * np.sqrt(np.log2(n))                                                       # test_fft_arbitrary_length
    for li, lo in lead_pairs(True, True):
        what = "fft n %d batch %d in %d out %d %s" % (n, batch, li, lo, "in place" if inplace else "")
        out = Out(n, torch.complex64, lo, rows=batch)
        if inplace:
            G.interior_of(out.base, lo, n, rows=batch).copy_(torch.as_tensor(x, device="cuda"))
            src, bases = out.ptr, []
        else:
            bases, views, snaps = place(torch, [x], ((li, 0),))
            src = views[0].data_ptr()
        E._bind_stream(out.base)
        sync_ok(torch, lib.sp_fft_c2c(p_(src), p_(out.ptr), n, batch, -1, 1), what)
        got = out.result(what)
        assert peak_err(got, ref) <= tol, (what, peak_err(got, ref))
        if not inplace:
            assert G.unchanged(bases[0], snaps[0]), what


@pytest.mark.parametrize("cplx", [False, True], ids=["f32", "c64"])
def test_sp_stft(torch, cplx):
    lib, name = _ffi.lib(), "stft_frames-%s-256x64" % ("c64" if cplx else "f32")
    case = case_of(name)
    d, ref = G.inputs(case), G.reference(case)
    nsig = d["arrays"][0].size
    M, nb = ref[0].shape
    win = np.ascontiguousarray(d["win"], dtype=np.float32)
    amp = 1.0 / float(np.sum(d["win"]))

    def judge(got, what):
        within(got[0].reshape(M, nb), ref[0], 1e-4 * float(np.max(np.abs(ref[0]))), what)
        within(got[1], ref[1], 1e-4 * ref[1], what + " pseg")

    run_b(torch, name, lambda lo: [Out(M * nb, torch.complex64, lo), Out(M, torch.float64, lo)],
          lambda v, o: lib.sp_stft(p_(v[0]), int(cplx), nsig, p_(win), 256, 64, M, _ffi.DETREND_MEAN, 0.0, 0.0, _ffi.SIDED_ONE, amp, 0, 0,
                                   p_(o[0].ptr), p_(o[1].ptr), 1), in_cplx=cplx, out_cplx=True, judge=judge)


def test_sp_istft(torch):
    """nfft 32, hop 8 (the smallest shape of tests/test_gpu_istft.py), three records, real output cut to an odd nout"""
    from test_gpu_istft import record, spectra, scipy_inverse
    lib = _ffi.lib()
    nfft, hop, nch = 32, 8, 3
    win = ss.get_window("hann", nfft)
    x = record(40 * hop + nfft + 37, False, 7 * nfft + hop, nch=nch)
    Z = np.ascontiguousarray(spectra(x, win, nfft, hop, False, True))                       # [3, nfreq, nseg] complex64, bin-major
    nseg = Z.shape[-1]
    skip = nfft // 2
    nout = (nseg - 1) * hop + nfft - 2 * skip - 3
    assert nout % 4 == 1
    ref = scipy_inverse(Z, win, nfft, hop, False, True)[..., :nout]
    w32 = np.ascontiguousarray(win, dtype=np.float32)
    for li, lo in lead_pairs(True, False):
        what = "istft in %d out %d" % (li, lo)
        bases, views, snaps = place(torch, [Z.reshape(nch, -1)], ((li, 0),))
        out = Out(nout, torch.float32, lo, rows=nch)
        E._bind_stream(views[0])
        sync_ok(torch, lib.sp_istft(p_(views[0]), _ffi.SIDED_HALF, 1, nch, nseg, p_(w32), nfft, hop, float(np.sum(win)), skip, nout,
                                    p_(out.ptr), 1), what)
        got = out.result(what)
        assert G.unchanged(bases[0], snaps[0]), what
        assert got.shape == ref.shape and peak_err(got, ref) <= 1e-4, (what, peak_err(got, ref))


@pytest.mark.parametrize("onesided", [True, False], ids=["half", "raw"])
def test_sp_pfb_synth(torch, onesided):
    """M 16, one tap per channel, hop 8 (the smallest shape of tests/test_gpu_pfb_synth.py), 257 frames, an nout that cuts the last
    frame short"""
    from test_host_pfb_synth import pfb_synth_ref
    from test_gpu_pfb_synth import tap64, random_frames, SCALE, N0
    lib = _ffi.lib()
    M, P, hop, nf, rows = 16, 1, 8, 257, 3
    L, nb = M * P, (M // 2 + 1 if onesided else M)
    g = np.random.default_rng(91).standard_normal(L)
    X = random_frames((rows, nf, nb), 92 + nf)
    nout = (nf - 1) * hop + L - 3
    r0 = N0 % M
    ref = pfb_synth_ref(X, tap64(g, M), M, hop, 0, nout, 1, r0, onesided=onesided)
    g32 = np.ascontiguousarray(g, dtype=np.float32)
    for li, lo in lead_pairs(True, not onesided):
        what = "pfb_synth in %d out %d" % (li, lo)
        bases, views, snaps = place(torch, [X.reshape(rows, -1)], ((li, 0),))
        out = Out(nout, torch.float32 if onesided else torch.complex64, lo, rows=rows)
        E._bind_stream(views[0])
        sync_ok(torch, lib.sp_pfb_synth(p_(views[0]), _ffi.SIDED_HALF if onesided else _ffi.SIDED_RAW, 0, rows, nf, p_(g32), L, M, hop, 0,
                                        1, r0, SCALE, nout, p_(out.ptr), 1), what)
        got = out.result(what)
        assert G.unchanged(bases[0], snaps[0]), what
        assert got.shape == ref.shape and peak_err(got, ref) <= 1e-4, (what, peak_err(got, ref))
