"""Spectral correlation on the GPU (k_cyclic, sp_cyclic, pyfft_amd.cyclic) against the float64 restatement of tests/cyclic_ref.py: every
shape and form within the allowance, the nu = 0 row against the Welch kernels, additivity under `first`, the passes over a long list of
cycle frequencies, bitwise repeatability, host arrays against device tensors, offset pointers inside poisoned buffers, and the cyclic
coherence of amplitude-modulated noise with its significance level."""
import numpy as np
import pytest
import torch            # a missing torch fails these tests, it does not skip them

import cyclic_ref as R
import guard_ref as G
from pyfft_amd import _ffi, cyclic as CY, engine as E

pytestmark = pytest.mark.gpu

USED = {}          # case -> the largest share of the allowance the device used (printed by the last shape test)


def dev_rows(a, pitch):
    """the rows of a on the device, nsig + pitch apart, NaN between them"""
    rows, nsig = a.shape
    if not pitch:
        return torch.as_tensor(np.array(a), device="cuda")
    ld = nsig + pitch
    base = torch.full((rows * ld,), float("nan"), dtype=torch.complex64 if np.iscomplexobj(a) else torch.float32, device="cuda")
    view = base.as_strided((rows, nsig), (ld, 1))
    view.copy_(torch.as_tensor(np.array(a), device="cuda"))
    return view


def run(name, form, device=True, **over):
    """engine.cyclic of a shape: (S, Pp, Pm) as numpy arrays [rows, A, nb]"""
    s = R.SHAPES[name]
    x, y = R.signals(name)
    cross, conj = R.form_args(form)
    w = R.hann(s["n"])
    put = (lambda a: dev_rows(a, s["pitch"])) if device else np.array
    kw = dict(y=put(y) if cross else None, conj=conj, first=s["first"], b0=s["b0"], nb=s["nb"])
    kw.update(over)
    out = E.cyclic(put(x), w, s["hop"], s["nframes"], s["nu"], **kw)
    return tuple(o.cpu().numpy() if device and o is not None else o for o in out)


@pytest.mark.parametrize("name,form", R.CASES, ids=["%s-%s" % c for c in R.CASES])
def test_shapes_against_reference(name, form):
    s = R.SHAPES[name]
    got = run(name, form)
    assert got[0].dtype == np.complex64 and got[1].dtype == np.float32 and got[0].shape == (s["rows"], len(s["nu"]), s["nb"])
    USED[(name, form)] = R.assert_within(got, R.reference(name, form), "%s %s" % (name, form), sel=lambda a: R.band(a, s))
    if len(USED) == len(R.CASES):
        print("the device used at most %.3f of the allowance %.2e" % (max(USED.values()), R.ALLOWANCE))


@pytest.mark.parametrize("name,form", R.CASES, ids=["%s-%s" % c for c in R.CASES])
def test_frame_loop_and_clamped_tail(name, form, monkeypatch):
    """every shape and form again with several frames per group and a last group that is not full: sums carried across the frames of a
    group, the images reused from frame to frame, the window table read back in every frame, the frames past the end weighted zero"""
    s, fpg = R.SHAPES[name], R.FPG[name]
    cross, conj = R.form_args(form)
    monkeypatch.setenv("SP_CYCLIC_FPG", str(fpg))
    plan = E.cyclic_plan(s["n"], s["hop"], s["nframes"], len(s["nu"]), rows=s["rows"], cplx=s["cplx"], cross=cross, conj=conj)
    assert plan["fpg"] == fpg > 1 and s["nframes"] % fpg and s["nframes"] > fpg
    got = run(name, form)
    R.assert_within(got, R.reference(name, form), "%s %s at %d frames per group" % (name, form, fpg), sel=lambda a: R.band(a, s))
    again = run(name, form)
    for p, q in zip(got, again):
        assert np.array_equal(p, q)


def test_frames_per_group_above_one_without_the_hook(monkeypatch):
    name = "n4096-runs-of-three"
    s = R.SHAPES[name]
    monkeypatch.delenv("SP_CYCLIC_FPG", raising=False)
    E.cyclic(np.zeros(4096, dtype=np.float32), R.hann(32), 8, 1, [0.0])            # the library is up: the plan counts the device's CUs
    plan = E.cyclic_plan(s["n"], s["hop"], s["nframes"], len(s["nu"]))
    assert plan["fpg"] > 1 and s["nframes"] % plan["fpg"], plan
    R.assert_within(run(name, "auto"), R.reference(name, "auto"), "%s, %d frames per group" % (name, plan["fpg"]))


def test_any_subset_of_the_outputs():
    name, form = "n256-cplx", "conj"
    full = run(name, form)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = run(name, form, S=want[0], Pp=want[1], Pm=want[2])
        for g, f, wnt in zip(got, full, want):
            assert (g is None) == (not wnt) and (g is None or np.array_equal(g, f))


def test_nu_zero_row_is_the_welch_estimate():
    # cross, real rows: S, Pp, Pm at nu = 0 are Pxy = Y conj(X), Pyy, Pxx of welch_csd over the same frames
    name = "n1024-cross-batch-pitch"
    s = R.SHAPES[name]
    x, y = R.signals(name)
    w = R.hann(s["n"])
    got = run(name, "cross", scale=1.0 / s["nframes"])
    ref = tuple(r / s["nframes"] for r in R.reference(name, "cross"))
    bd = R.bounds(ref, lambda a: R.band(a, s))
    for r in range(s["rows"]):
        pxx, pyy, pxy = E.welch_csd(np.array(x[r]), np.array(y[r]), w, s["hop"], s["nframes"], detrend=True, sided=E.SIDED_RAW, scale=1.0)
        for i, wl in ((0, pxy[0]), (1, pyy[0]), (2, pxx)):
            err = np.abs(got[i][r, 0] - R.band(wl, s))
            assert np.all(err <= bd[i][r, 0]), (r, i, float(np.max(err / bd[i][r, 0])))
    # auto, real row: Pp = Pm = the Welch PSD
    name = "n32-real-tail"
    s = R.SHAPES[name]
    x, _ = R.signals(name)
    got = run(name, "auto", scale=1.0 / s["nframes"])
    ref = tuple(r / s["nframes"] for r in R.reference(name, "auto"))
    bd = R.bounds(ref)
    pxx = E.welch_psd(np.array(x[0]), R.hann(s["n"]), s["hop"], s["nframes"], detrend=True, sided=E.SIDED_RAW, scale=1.0)
    for i in (1, 2):
        assert np.all(np.abs(got[i][0, 0] - pxx) <= bd[i][0, 0])
    assert np.all(np.abs(got[0][0, 0] - pxx) <= bd[0][0, 0])             # S at nu = 0 of a real row is its PSD


@pytest.mark.parametrize("form", ("conj", "plain"))
def test_additive_under_first_on_the_device(form):
    name, cut = "n256-cplx", 21                       # cut after frame 20
    s = R.SHAPES[name]
    x, _ = R.signals(name)
    cross, conj = R.form_args(form)
    w, n, hop, first = R.hann(s["n"]), s["n"], s["hop"], s["first"]
    m = complex(R.row_mean(x[0]))
    xd = torch.as_tensor(np.array(x[0]), device="cuda")
    kw = dict(conj=conj, mean_value=m)
    a = E.cyclic(xd[:(cut - 1) * hop + n], w, hop, cut, s["nu"], first=first, **kw)
    b = E.cyclic(xd[cut * hop:], w, hop, s["nframes"] - cut, s["nu"], first=first + cut * hop, **kw)
    local = E.cyclic(xd[cut * hop:], w, hop, s["nframes"] - cut, s["nu"], first=first, **kw)
    ref = tuple(r[0] for r in R.reference(name, form))
    total = tuple((p + q).cpu().numpy() for p, q in zip(a, b))
    R.assert_within(total, ref, "parts added, %s" % form)
    wrong = (a[0] + local[0]).cpu().numpy()
    assert np.max(np.abs(wrong - ref[0]) / R.bounds(ref)[0]) > 100.0          # the local index does not add up


def test_many_alpha_in_three_passes(monkeypatch):
    name = "n64-many-alpha"
    monkeypatch.delenv("SP_CYCLIC_CHUNK", raising=False)
    monkeypatch.delenv("SP_CYCLIC_FPG", raising=False)
    whole = run(name, "auto")
    assert E.last_passes(E.CYC_PASSES) == 1
    monkeypatch.setenv("SP_CYCLIC_CHUNK", str(R.MANY_ALPHA_CHUNK))
    got = run(name, "auto")
    assert E.last_passes(E.CYC_PASSES) == 3
    for g, wl in zip(got, whole):
        assert np.array_equal(g, wl)
    ref = R.reference(name, "auto")
    seams = [127, 128, 255, 256]
    R.assert_within(tuple(g[:, seams] for g in got), tuple(r[:, seams] for r in ref), "rows at the seams")
    monkeypatch.delenv("SP_CYCLIC_CHUNK")
    E.cyclic(np.array(R.signals(name)[0]), R.hann(64), 16, 13, [0.1])
    assert E.last_passes(E.CYC_PASSES) == 1 and E.last_passes(0) == 0


@pytest.mark.parametrize("name,form", [("n256-cplx", "conj"), ("n256-cplx", "plain"), ("n1024-cross-batch-pitch", "cross"), ("n8192-hop1", "auto")])
def test_two_calls_and_both_memories_agree_bitwise(name, form):
    a, b = run(name, form), run(name, form)
    h = run(name, form, device=False)
    for p, q, r in zip(a, b, h):
        assert np.array_equal(p, q)
        assert np.array_equal(p, r)


# ---- offset pointers inside poisoned buffers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form,lead", [("n32-real-tail", "auto", 3), ("n256-cplx", "plain", 1)])
def test_engine_call_at_offset_pointers(name, form, lead):
    s = R.SHAPES[name]
    x, _ = R.signals(name)
    base, view = G.poisoned_input(torch.as_tensor(np.array(x), device="cuda"), lead)       # one row: NaN before and behind it
    snap = G.snapshot(base)
    cross, conj = R.form_args(form)
    out = E.cyclic(view, R.hann(s["n"]), s["hop"], s["nframes"], s["nu"], conj=conj, first=s["first"])
    got = tuple(o.cpu().numpy() for o in out)
    assert G.unchanged(base, snap)
    assert all(np.all(np.isfinite(g)) for g in got)
    R.assert_within(got, R.reference(name, form), "%s %s at lead %d" % (name, form, lead))


@pytest.mark.parametrize("name,form,lead", [("n32-real-tail", "auto", 3), ("n256-cplx", "conj", 1)])
def test_c_entry_at_offset_pointers_with_guarded_outputs(name, form, lead):
    s = R.SHAPES[name]
    x, _ = R.signals(name)
    rows, nsig = x.shape
    ld = nsig
    base, view = G.poisoned_input(torch.as_tensor(np.array(x), device="cuda"), lead)
    snap = G.snapshot(base)
    cross, conj = R.form_args(form)
    A, nb = len(s["nu"]), s["nb"]
    nelem = rows * A * nb
    outs = [G.sentinel_output(nelem, dt, ol, device="cuda") for dt, ol in ((torch.complex64, 1), (torch.float32, 3), (torch.float32, 1))]
    w = np.ascontiguousarray(R.hann(s["n"]), dtype=np.float32)
    nu = np.array(s["nu"], dtype=np.float64)
    m = complex(R.row_mean(x[0]))
    mean = np.array([[m.real, m.imag]] * rows, dtype=np.float64)
    E._bind_stream(view)
    code = _ffi.DTYPE_C64 if s["cplx"] else _ffi.DTYPE_F32
    rc = _ffi.lib().sp_cyclic(_ffi.ptr(view.data_ptr()), None, code, code, ld, nsig, rows, _ffi.ptr(w), s["n"], s["hop"], s["nframes"],
                              s["first"], _ffi.ptr(nu), A, int(conj), _ffi.ptr(mean), None, s["b0"], nb, 1.0,
                              *[_ffi.ptr(o[1]) for o in outs], 1)
    assert rc == 0, _ffi.lib().sp_last_error()
    torch.cuda.synchronize()
    assert G.unchanged(base, snap)
    got = []
    for (b, _), ol, shape in zip(outs, (1, 3, 1), ((rows, A, nb),) * 3):
        assert G.guards_intact(b, ol, nelem)
        assert G.all_written(b, ol, nelem)
        got.append(G.interior_of(b, ol, nelem).cpu().numpy().reshape(shape))
    R.assert_within(tuple(got), R.reference(name, form), "%s %s through the C entry" % (name, form))


# ---- what the estimator is for ----------------------------------------------------------------------------------------------------
def test_cyclic_coherence_of_modulated_noise_and_the_level_on_white_noise():
    white, am = R.level_rows()
    f, al, S, Pp, Pm, gam = CY.cyclic_spectra(torch.as_tensor(np.array(am), device="cuda"), R.LEVEL_NU, fs=1.0, window="hann",
                                              nperseg=R.LEVEL_N)
    assert np.array_equal(al, np.array(R.LEVEL_NU)) and np.array_equal(f, np.fft.fftfreq(R.LEVEL_N))
    ref = R.level_reference(1)
    gref = R.coherence(*ref)
    bS, bP, bM = R.bounds(ref)
    den = np.sqrt(ref[1] * ref[2])
    bound = 1.01 * (bS / den + np.abs(gref) * 0.5 * (bP / ref[1] + bM / ref[2]))       # the allowance carried through S / sqrt(Pp Pm)
    g = gam.cpu().numpy()
    assert g.dtype == np.complex128
    err = np.abs(g[0] - gref[0])
    print("gamma at the modulation rate: worst cell at %.3f of the propagated allowance; mean |gamma| %.4f" % (float(np.max(err / bound[0])), np.abs(g[0]).mean()))
    assert np.all(err <= bound[0])
    assert abs(np.abs(g[0]).mean() - 0.606) <= 0.03
    prof = CY.cyclic_profile(gam).cpu().numpy()
    assert prof.shape == (len(R.LEVEL_NU),) and int(np.argmax(prof)) == 0
    _, _, gw = CY.cyclic_coherence(np.array(white), R.LEVEL_NU[1:], fs=1.0, nperseg=R.LEVEL_N)
    lvl = CY.cyclic_level(R.LEVEL_FRAMES, R.hann(R.LEVEL_N), R.LEVEL_HOP, 0.05)
    share = float(np.mean(np.abs(gw) ** 2 > lvl))
    print("white noise: %.4f of the cells above the 5 %% level %.5f" % (share, lvl))
    assert gw.shape == (7, R.LEVEL_N) and 0.03 <= share <= 0.08
