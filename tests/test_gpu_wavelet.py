"""The continuous wavelet transform on the GPU (k_cwt, sp_cwt, sp_icwt, engine.cwt, pyfft_amd.wavelet) against the float64 reference of
tests/cwt_ref.py.  The bound is that of tests/test_gpu_baseband.py and tests/test_gpu_resample.py: per scale row, the largest error
over the row's rms is at most 4 x what a float32 numpy restatement of the same plan loses against the same reference, and the
restatement itself must lose between 0 and 1e-4.  With eps that bound, the derived outputs follow from |W - Wref| <= eps rms_s:
    gws      |sum |W|^2 - sum |Wref|^2| <= (2 eps + eps^2) sum |Wref|^2                    (Cauchy-Schwarz)
    recon    |sum_s w_s (W - Wref)|     <= eps sum_s |w_s| rms_s
    bandpow  |sum_s v_s (|W|^2 - |Wref|^2)| <= sum_s v_s (2 |Wref| eps rms_s + eps^2 rms_s^2)
Records of about 2 hop + 37 samples and one of hop - 5.  Paul-4 has no case at L = 256: its margins are 25 x the scale at tail = 1e-6
and its Nyquist step keeps scales below 8.2 samples out, so no Paul-4 scale set fits 4 M <= 256 with a restatement loss under 1e-4;
its L = 1024 case takes tail = 1e-5."""
import functools
import math
import os

import numpy as np
import pytest

import cwt_ref as R
import guard_ref as G
from pyfft_amd import _ffi, engine as E, wavelet as WV

pytestmark = pytest.mark.gpu

WAVELETS = {"morlet": WV.Morlet(6.0), "paul": WV.Paul(4)}
# (family, L) -> (top scale in samples, tail): the default plan picks L
SETS = {("morlet", 256): (13, 1e-6), ("morlet", 1024): (52, 1e-6), ("morlet", 4096): (209, 1e-6), ("morlet", 8192): (627, 1e-6),
        ("paul", 1024): (18, 1e-5), ("paul", 4096): (41, 1e-6), ("paul", 8192): (124, 1e-6)}
CASES = sorted(SETS)


@pytest.fixture(scope="module")
def torch():
    import torch
    _ffi.init()
    return torch


@functools.lru_cache(maxsize=None)
def plan_of(family, L):
    top, tail = SETS[(family, L)]
    wv = WAVELETS[family]
    s0 = WV.smallest_fused_scale(wv, tail)
    scales = s0 * 2 ** (np.arange(int(math.log2(top / s0) * 4) + 1) / 4.0)
    plan = WV.cwt_plan(1000, wavelet=wv, scales=scales, tail=tail)
    assert plan["L"] == L and plan["fused"].all(), (family, L, plan["L"], plan["M"])
    return plan


@functools.lru_cache(maxsize=None)
def case_of(family, L, cplx, short=False, rows=1):
    """-> (x [rows, n], scales, plan, reference [rows, S, n] float64, eps): computed once and shared, read-only."""
    plan = plan_of(family, L)
    n = plan["hop"] - 5 if short else 2 * plan["hop"] + 37
    x = np.stack([R.make_signal(n, cplx, 10 + r + L) for r in range(rows)])
    return (x,) + restated(x, family, L)


def restated(x, family, L):
    plan = plan_of(family, L)
    wv = WAVELETS[family]
    sc = plan["scales"]
    ref = np.stack([R.cwt_ref(row, sc, family, wv.param) for row in x])
    loss = max(R.row_err(R.overlap_save(row, sc, family, wv.param, L, plan["M"], np.float32), ref[r]) for r, row in enumerate(x))
    print("%s L=%d n=%d: the float32 restatement loses %.3g" % (family, L, x.shape[-1], loss))
    assert 0 < loss <= 1e-4
    for a in (x, ref):
        a.setflags(write=False)
    return sc, plan, ref, 4 * loss


def check_rows(W, ref, eps, what):
    err = R.row_err(W, ref)
    print("%s: %.3g of the row rms (bound %.3g)" % (what, err, eps))
    assert np.all(np.isfinite(W)) and err <= eps, what


@pytest.mark.parametrize("mode", ["numpy", "device"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("family,L", CASES, ids=["%s-%d" % c for c in CASES])
def test_w_against_reference(torch, family, L, cplx, mode):
    wv = WAVELETS[family]
    rows = 2 if mode == "device" else 1
    x, sc, plan, ref, eps = case_of(family, L, cplx, rows=rows)
    if mode == "numpy":
        W = E.cwt(x[0], sc, family, wv.param, L, plan["M"])["W"]
        assert W.dtype == np.complex64 and W.shape == ref.shape[1:]
        check_rows(W, ref[0], eps, "W")
    else:
        base, view = G.poisoned_input(torch.as_tensor(x, device="cuda"), 1, pitch=x.shape[-1] + 3)      # row-strided, off alignment
        assert view.stride(0) == x.shape[-1] + 3
        W = E.cwt(view, sc, family, wv.param, L, plan["M"])["W"]
        assert W.is_cuda and tuple(W.shape) == ref.shape
        W = W.cpu().numpy()
        for r in range(rows):
            check_rows(W[r], ref[r], eps, "W row %d" % r)


@pytest.mark.parametrize("family,L,cplx", [("morlet", 256, False), ("morlet", 4096, True), ("paul", 4096, False)])
def test_short_record(torch, family, L, cplx):
    """N = hop - 5: one partial frame."""
    x, sc, plan, ref, eps = case_of(family, L, cplx, short=True)
    out = E.cwt(x[0], sc, family, WAVELETS[family].param, L, plan["M"], gws=True)
    check_rows(out["W"], ref[0], eps, "W")
    g = np.sum(np.abs(ref[0]) ** 2, axis=-1)
    assert np.max(np.abs(out["gws"] - g) / g) <= 2 * eps + eps * eps


@pytest.mark.parametrize("family,L,cplx", [("morlet", 1024, False), ("morlet", 8192, True), ("paul", 4096, True), ("morlet", 256, True)])
def test_derived_outputs(torch, family, L, cplx, monkeypatch):
    wv = WAVELETS[family]
    x, sc, plan, ref, eps = case_of(family, L, cplx)
    x, ref, S = x[0], ref[0], len(sc)
    rng = np.random.default_rng(L)
    wr = (rng.uniform(0.2, 1.0, S) / np.sqrt(sc)).astype(np.float32)
    wb = (rng.uniform(0.2, 1.0, S) / sc).astype(np.float32)
    wb[::3] = 0
    args = (x, sc, family, wv.param, L, plan["M"])
    full = E.cwt(*args, W=True, gws=True, recon=wr, bandpow=wb)
    check_rows(full["W"], ref, eps, "W beside the other outputs")
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1))
    g = np.sum(np.abs(ref) ** 2, axis=-1)
    gerr = np.max(np.abs(full["gws"] - g) / g)
    rec_ref = np.sum(wr[:, None].astype(np.float64) * ref, axis=0)
    rec_bound = eps * np.sum(np.abs(wr) * rms)
    rerr = np.max(np.abs(full["recon"] - rec_ref))
    bp_ref = np.sum(wb[:, None].astype(np.float64) * np.abs(ref) ** 2, axis=0)
    bp_bound = np.sum(wb[:, None] * (2 * np.abs(ref) * eps * rms[:, None] + (eps * rms[:, None]) ** 2), axis=0)
    berr = np.abs(full["bandpow"] - bp_ref)
    print("gws %.3g (bound %.3g); recon %.3g (bound %.3g); bandpow %.3g of its bound" % (gerr, 2 * eps + eps * eps, rerr, rec_bound,
                                                                                         np.max(berr / bp_bound)))
    assert full["gws"].dtype == np.float64 and full["bandpow"].dtype == np.float32 and full["recon"].dtype == np.complex64
    assert gerr <= 2 * eps + eps * eps and rerr <= rec_bound and np.all(berr <= bp_bound)
    # the outputs alone (W never formed) are the same numbers, and a second run agrees bitwise
    alone = E.cwt(*args, W=False, gws=True, recon=wr, bandpow=wb)
    again = E.cwt(*args, W=False, gws=True, recon=wr, bandpow=wb)
    for k in ("gws", "recon", "bandpow"):
        assert np.array_equal(alone[k], again[k]) and np.array_equal(alone[k], full[k]), k
    assert "W" not in alone
    # W and gws do not depend on how the scales are dealt to workgroups
    seen = []
    for chunk in ("1", "3", str(S)):
        monkeypatch.setenv("SP_CWT_CHUNK", chunk)
        assert E.cwt_plan(len(x), S, L, plan["M"], gws=True)["chunk"] == int(chunk)
        seen.append(E.cwt(*args, W=True, gws=True))
    monkeypatch.delenv("SP_CWT_CHUNK")
    for o in seen:
        assert np.array_equal(o["W"], full["W"]) and np.array_equal(o["gws"], full["gws"])
    # the fused sum against sp_icwt of the materialised W: the same S products and additions in float32
    y = E.icwt_sum(full["W"], wr)
    tol = 4 * S * 2.0 ** -24 * np.sum(np.abs(wr)[:, None] * np.abs(full["W"]), axis=0)
    assert y.dtype == np.complex64 and np.all(np.abs(y - full["recon"]) <= tol)
    check = np.sum(wr[:, None].astype(np.float64) * full["W"], axis=0)
    assert np.all(np.abs(y - check) <= tol)


@pytest.mark.parametrize("L", [256, 4096])
def test_frame_seams(torch, L):
    """One sample at n = hop - 1 and one at n = hop: the last output of frame 0 and the first of frame 1."""
    plan = plan_of("morlet", L)
    hop, n = plan["hop"], 2 * plan["hop"] + 37
    x = np.zeros((1, n), dtype=np.float32)
    x[0, hop - 1], x[0, hop] = 1.0, -0.7
    sc, plan, ref, eps = restated(x, "morlet", L)
    W = E.cwt(x[0], sc, "morlet", 6.0, L, plan["M"])["W"]
    check_rows(W, ref[0], eps, "W")
    seam = slice(hop - 40, hop + 40)
    check_rows(W[:, seam], ref[0][:, seam], eps * np.sqrt(np.mean(np.abs(ref[0]) ** 2) / np.mean(np.abs(ref[0][:, seam]) ** 2)), "seam")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_nothing_written_beyond_the_record(torch, cplx):
    """Sentinel-filled outputs at offset pointers: the last, partial frame writes every sample below N and nothing at or beyond it."""
    family, L = "morlet", 1024
    x, sc, plan, ref, eps = case_of(family, L, cplx)
    x, ref, S, n = x[0], ref[0], len(sc), x.shape[-1]
    assert n % plan["hop"] not in (0, plan["hop"] - 1)
    xd = torch.as_tensor(x, device="cuda")
    wr = np.ones(S, dtype=np.float32)
    outs = {"W": (S * n, torch.complex64, 1), "gws": (S, torch.float64, 1), "recon": (n, torch.complex64, 1), "bandpow": (n, torch.float32, 3)}
    held = {k: G.sentinel_output(nel, dt, lead, device="cuda") for k, (nel, dt, lead) in outs.items()}
    E._bind_stream(xd)
    _ffi.check(_ffi.lib().sp_cwt(_ffi.ptr(xd.data_ptr()), int(cplx), n, n, 1, _ffi.ptr(np.ascontiguousarray(sc)), S, 0, 6.0, 0.0, L,
                                 plan["M"], _ffi.ptr(wr), _ffi.ptr(wr), *[_ffi.ptr(held[k][1]) for k in ("W", "gws", "recon", "bandpow")], 1))
    torch.cuda.synchronize()
    for k, (nel, dt, lead) in outs.items():
        assert G.guards_intact(held[k][0], lead, nel), k
        assert G.first_unwritten(held[k][0], lead, nel) is None, k
    W = G.interior_of(held["W"][0], 1, S * n).cpu().numpy().reshape(S, n)
    check_rows(W, ref, eps, "W at an offset pointer")


def test_composed_path(torch):
    """Scales from 2 dt on: the first ones lie where the Nyquist cut spoils the decay and take the whole-record path."""
    n, dt = 5000, 0.5
    x = R.make_signal(n, False, 77)
    scales = 2.0 * dt * 2 ** (np.arange(17) / 4.0)
    plan = WV.cwt_plan(n, dt, scales=scales)
    nc = int((~plan["fused"]).sum())
    assert list(plan["path"][:4]) == ["composed"] * 4 and plan["path"][-1] == "fused" and 0 < nc < len(scales)
    assert np.all(plan["scales"][~plan["fused"]] / dt < 3.7) and plan["n_full"] == 16384 and plan["L"] is not None
    ref = R.cwt_ref(x, scales / dt)
    c32 = R.composed_f32(x, scales[:nc] / dt, "morlet", 6.0)
    f32 = R.overlap_save(x, scales[nc:] / dt, "morlet", 6.0, plan["L"], plan["M"], np.float32)
    loss = max(R.row_err(c32, ref[:nc]), R.row_err(f32, ref[nc:]))
    print("composed path: the float32 restatement loses %.3g" % loss)
    assert 0 < loss <= 1e-4
    W, sc, freqs, coi = WV.cwt(x, dt, scales=scales)
    np.testing.assert_allclose(freqs, 1.0 / (WV.Morlet(6.0).flambda() * scales), rtol=1e-14)
    assert coi.shape == (n,) and coi[0] == pytest.approx(WV.Morlet(6.0).flambda() * 0.5 * dt / math.sqrt(2), rel=1e-12)
    check_rows(W, ref, 4 * loss, "W over both paths")
    Wd = WV.cwt(torch.as_tensor(x, device="cuda"), dt, scales=scales)[0]
    check_rows(Wd.cpu().numpy(), ref, 4 * loss, "W over both paths, device tensor")


def test_round_trip_and_filter(torch):
    """cwt -> icwt of a band-limited record under twice the float64 reference's own residual plus the float32 bound, and cwt_filter: a
    line inside the band passes, one outside goes, to the level the reference's band sum does."""
    n, dt, dj = 6000, 0.25, 1.0 / 8
    wv = WV.Morlet(6.0)
    x = R.band_limited(n, (14.0, 37.0, 95.0, 240.0))
    scales = WV.cwt_scales(n, dt, dj, s0=4.0 * dt, J=int(math.log2(600 / 4.0) / dj), wavelet=wv)
    plan = WV.cwt_plan(n, dt, scales=scales)
    assert plan["fused"].all()
    ref = R.cwt_ref(x, scales / dt)
    w = WV.recon_weights(wv, scales, dt, dj)
    f32 = R.overlap_save(x, scales / dt, "morlet", 6.0, plan["L"], plan["M"], np.float32)
    eps = 4 * R.row_err(f32, ref)
    rms_s, rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1)), float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    y_ref = np.sum(w[:, None] * ref.real, axis=0)
    r_ref = np.sqrt(np.mean((y_ref - x) ** 2)) / rms
    W, sc, _, _ = WV.cwt(x, dt, dj, scales=scales)
    y = WV.icwt(W, sc, dt, dj, wv)
    r = np.sqrt(np.mean((y - x) ** 2)) / rms
    f32_term = eps * np.sum(np.abs(w) * rms_s) / rms
    print("round trip: residual %.3g, the reference's own %.3g, float32 term %.3g" % (r, r_ref, f32_term))
    assert y.dtype == np.float32 and r <= 2 * r_ref + f32_term
    # band-pass: keep the periods 37 and 95 samples (scales x flambda), drop 14 and 240
    fl = wv.flambda()
    band = (22.0 * dt / fl, 150.0 * dt / fl)
    inb = (scales >= band[0]) & (scales <= band[1])
    yb_ref = np.sum((w * inb)[:, None] * ref.real, axis=0)
    for xin in (x, torch.as_tensor(x, device="cuda")):
        yb = WV.cwt_filter(xin, dt, dj, scales=scales, band=band)
        yb = yb.cpu().numpy() if hasattr(yb, "cpu") else yb
        berr = np.max(np.abs(yb - yb_ref))
        bound = eps * np.sum(np.abs(w * inb) * rms_s)
        print("cwt_filter: %.3g from the reference's band sum (bound %.3g)" % (berr, bound))
        assert berr <= bound
    t = np.arange(n)
    amp = lambda v, p: abs(np.sum(v * np.exp(-2j * np.pi * t / p))) / abs(np.sum(x.astype(np.float64) * np.exp(-2j * np.pi * t / p)))   # noqa: E731
    got = {p: amp(yb, p) for p in (14.0, 37.0, 95.0, 240.0)}
    want = {p: amp(yb_ref, p) for p in got}
    print("cwt_filter gains by period:", {p: "%.4f (reference %.4f)" % (got[p], want[p]) for p in got})
    for p in got:
        assert abs(got[p] - want[p]) <= 1e-3
    assert want[37.0] > 0.8 and want[95.0] > 0.8 and want[14.0] < 0.05 and want[240.0] < 0.05
    # the power outputs of the public layer: W is never materialised
    gws, sc2, bp = WV.cwt_power(x, dt, dj, scales=scales, band=band)
    g_ref = np.mean(np.abs(ref) ** 2, axis=-1)
    cd = WV.cdelta(wv, scales, dt, dj)
    v = np.where(inb, dj * dt / (cd * scales), 0.0)
    bp_ref = np.sum(v[:, None] * np.abs(ref) ** 2, axis=0)
    bp_bound = np.sum(v[:, None] * (2 * np.abs(ref) * eps * rms_s[:, None] + (eps * rms_s[:, None]) ** 2), axis=0)
    assert np.max(np.abs(gws - g_ref) / g_ref) <= 2 * eps + eps * eps
    assert np.all(np.abs(bp - bp_ref) <= bp_bound + 2.0 ** -22 * bp_ref)           # (+ the float32 rounding of the weights v)
