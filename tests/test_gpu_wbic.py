"""Wavelet bispectrum and bicoherence on the GPU against the float64 reference of tests/wbic_ref.py.

Parity is the bound the project holds k_bispec to (assert_parity of tests/test_gpu_bispectrum.py): |dB| <= 1e-4 A + 1e-6 max A,
|db2| <= 2e-4, NaN in exactly the same places; P to rtol 1e-5.  The shapes are the smallest at which each thing can go wrong.

The band of cases 1 and 5 is asked for as k = 2 .. 40 at df = 1/100.  Of these only k <= 26 (Morlet-6) and k <= 8 (Paul-4) have scales
that fuse: the rows above have scales under 3.72 (8.4) samples, where the filter's cut at Nyquist gives tails that fall off like 1 / n,
and wbic_freqs leaves them out as the contract says (forced through at L = 1024, M = 238, the overlap-save plan itself, in float64, is
1.67 times the B bound away from the whole-record transform).  Case 1b has the 39 rows k = 2 .. 40 on a grid where all of them fuse.

The seam test does not ask for bitwise agreement between pass plans: a pass starts its transform frames at its own first sample less
the margin, so the frames of a block align differently under another plan, and the results agree to rounding (a tenth of the parity
bound), not bit for bit.  Two calls under one plan do agree bitwise."""
import functools

import numpy as np
import pytest
import torch

import guard_ref as G
import wbic_ref as R
from pyfft_amd import _ffi, engine as E, wavelet as W, wbicoherence as WB
from test_gpu_bispectrum import assert_parity

pytestmark = pytest.mark.gpu

# name -> (wavelet, df, k band asked for, rows that fuse, record length in hops (+ 37), kind, keywords of wavelet_bispectrum)
CASES = {
    "1-ragged-tile": (("morlet", 6.0), 1 / 100, (2, 40), (2, 26), 2, "real", {}),
    "1b-39-rows": (("morlet", 6.0), 1 / 160, (2, 40), (2, 40), 2, "real", {}),
    "2-klo-1": (("morlet", 6.0), 1 / 100, (1, 20), (1, 20), 2, "real", {}),
    "3-cross-blocks": (("morlet", 6.0), R.QPC_DF, (R.QPC_KLO, R.QPC_KHI), (R.QPC_KLO, R.QPC_KHI), 3, "cross", dict(trim=True, block=1500)),
    "4-overlap": (("morlet", 6.0), 1 / 800, (4, 132), (4, 132), 2, "real", dict(block=2000, step=500)),
    "5-paul": (("paul", 4.0), 1 / 100, (2, 40), (2, 8), 2, "real", {}),
}


def _wavelet(spec):
    return W.Morlet(spec[1]) if spec[0] == "morlet" else W.Paul(spec[1])


@functools.lru_cache(maxsize=None)
def case(name):
    """the records of a case, what the public entry is called with, the plan it makes and the float64 reference; computed once"""
    spec, df, band, rows, hops, kind, kw = CASES[name]
    wv = _wavelet(spec)
    kw = dict(kw, dt=1.0, df=df, fmin=band[0] * df, fmax=band[1] * df, wavelet=wv)
    k_lo, k_hi, f, sc = WB.wbic_freqs(1000, 1.0, df, kw["fmin"], kw["fmax"], wv)
    assert (k_lo, k_hi) == rows
    hop = W.cwt_plan(1000, 1.0, wavelet=wv, scales=sc)["hop"]
    n = hops * hop + 37
    seed = sum(map(ord, name))
    recs = [R.noise_record(n, kind == "cross", seed + k) for k in range(3 if kind == "cross" else 1)]
    x, y, z = recs if kind == "cross" else (recs[0], None, None)
    plan = WB.wbic_plan(n, nrec=len(recs), sym=y is None, **kw)
    ref = R.wbic_ref(x, sc, k_lo, plan["n0"], plan["block"], plan["step"], plan["nblocks"], y=y, z=z, family=spec[0], param=spec[1])
    for a in recs + list(ref):
        a.setflags(write=False)
    return dict(x=x, y=y, z=z, kw=kw, plan=plan, scales=sc, k_lo=k_lo, spec=spec, ref=ref, blocks="block" in kw)


def engine_call(c, dev=False):
    conv = (lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()) if dev else (lambda a: a)
    p = c["plan"]
    x = conv(c["x"])
    y, z = conv(c["y"]), conv(c["z"])
    return E.wbic(x, c["scales"], c["k_lo"], c["spec"][0], c["spec"][1], p["L"], p["M"], p["n0"], p["block"], p["step"], p["nblocks"], y=y, z=z)


def check_parity(B, b2, P, ref, label):
    Bo, b2o, A, Po = ref
    for b in range(Bo.shape[0]):
        ok = ~np.isnan(Bo[b])
        err = np.abs(B[b][ok] - Bo[b][ok]) / R.parity_bound(A[b])[ok]
        print("%s block %d: max |dB| / bound %.3g, max |db2| %.3g" % (label, b, float(err.max()), float(np.max(np.abs(b2[b][ok] - b2o[b][ok])))))
        assert_parity(B[b], b2[b], Bo[b], b2o[b], A[b])
    np.testing.assert_allclose(P, Po, rtol=1e-5)
    valid = ~np.isnan(b2o)
    assert np.all(b2[valid] >= 0.0) and np.all(b2[valid] <= 1.0 + 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_parity(name):
    c = case(name)
    f, t, B, b2 = WB.wavelet_bispectrum(c["x"], c["y"], c["z"], **c["kw"])
    p = c["plan"]
    S = p["S"]
    np.testing.assert_allclose(f, (p["k_lo"] + np.arange(S)) * c["kw"]["df"], rtol=1e-14)
    assert B.dtype == np.complex128 and b2.dtype == np.float64
    if c["blocks"]:
        assert B.shape == b2.shape == (p["nblocks"], S, S) and p["nblocks"] > 1
        np.testing.assert_allclose(t, p["n0"] + p["step"] * np.arange(p["nblocks"]) + 0.5 * (p["block"] - 1))
    else:
        assert B.shape == b2.shape == (S, S)
        B, b2 = B[None], b2[None]
    P = engine_call(c)["P"]
    check_parity(B, b2, P, c["ref"], name)
    if c["y"] is None:                                          # the auto form is exactly symmetric
        np.testing.assert_array_equal(b2, np.swapaxes(b2, -1, -2))
        np.testing.assert_array_equal(B, np.swapaxes(B, -1, -2))


def test_shapes_walk_what_they_claim():
    p = {n: case(n)["plan"] for n in CASES}
    assert p["1-ragged-tile"]["tiles"] == 1 and p["1-ragged-tile"]["S"] == 25 and p["1-ragged-tile"]["L"] == 1024
    assert p["1b-39-rows"]["S"] == 39 and p["1b-39-rows"]["tiles"] == 1 and p["2-klo-1"]["k_lo"] == 1
    c3 = p["3-cross-blocks"]
    assert (c3["S"], c3["M"], c3["L"], c3["tiles"]) == (70, R.QPC_M, R.QPC_L, 3)     # 2 x 2 tiles, (1, 1) holds no valid pair
    assert (c3["n0"], c3["nblocks"], c3["cells"]) == (R.qpc_trim(), 5, 5) and c3["n1"] - c3["n0"] - 5 * 1500 > 0
    c4 = p["4-overlap"]
    assert c4["S"] == 129 and c4["tiles"] == 2 and c4["cell_len"] == 500 and c4["cells"] == c4["nblocks"] + 3 and c4["nblocks"] >= 3
    assert p["5-paul"]["S"] == 7


def test_seam(monkeypatch):
    c = case("3-cross-blocks")
    monkeypatch.delenv("SP_WBIC_CHUNK", raising=False)
    one = engine_call(c)
    assert one["passes"] == 1
    monkeypatch.setenv("SP_WBIC_CHUNK", "3000")
    kw = c["kw"]
    plan = WB.wbic_plan(c["x"].size, nrec=3, sym=False, **kw)
    assert plan["passes"] == 3 and plan["groups"] == 5          # two blocks to a pass: a block boundary lies inside the passes 0 and 1
    cut = engine_call(c)
    assert cut["passes"] == 3
    check_parity(cut["B"], cut["b2"], cut["P"], c["ref"], "seam")
    A = c["ref"][2]
    for b in range(A.shape[0]):
        ok = ~np.isnan(A[b])
        d = np.abs(cut["B"][b][ok] - one["B"][b][ok]) / (0.1 * R.parity_bound(A[b])[ok])
        print("block %d: three passes against one: max |dB| / (bound / 10) = %.3g" % (b, float(d.max())))
        assert np.all(d <= 1.0)
        np.testing.assert_allclose(cut["b2"][b][ok], one["b2"][b][ok], rtol=0, atol=2e-5)
    np.testing.assert_allclose(cut["P"], one["P"], rtol=1e-6)


@pytest.mark.parametrize("name", ["1-ragged-tile", "3-cross-blocks", "4-overlap"])
def test_two_calls_and_both_modes_agree_bitwise(name):
    c = case(name)
    a, b, d = engine_call(c), engine_call(c), engine_call(c, dev=True)
    for k in ("B", "b2", "P"):
        assert a[k].tobytes() == b[k].tobytes()
        assert d[k].is_cuda and a[k].tobytes() == d[k].cpu().numpy().tobytes()
    assert a["passes"] == b["passes"] == d["passes"]


def test_device_call_inside_poisoned_buffers():
    """one device-resident call at offset pointers: nothing outside a buffer is read or written, every output element is written"""
    c = case("3-cross-blocks")
    p = c["plan"]
    S, nb, n = p["S"], p["nblocks"], c["x"].size
    want = engine_call(c)
    dev = torch.device("cuda")
    ins = [G.poisoned_input(torch.from_numpy(np.array(a)).to(dev), lead) for a, lead in zip((c["x"], c["y"], c["z"]), (1, 0, 1))]
    snaps = [G.snapshot(base) for base, _ in ins]
    outs = [G.sentinel_output(nelem, dt, lead, device=dev) for nelem, dt, lead in
            ((nb * S * S, torch.complex128, 1), (nb * S * S, torch.float64, 1), (nb * S, torch.float64, 1))]
    E._bind_stream(ins[0][1])
    sc = np.ascontiguousarray(c["scales"], dtype=np.float64)
    passes = _ffi.C.c_int(0)
    code = _ffi.DTYPE_C64
    _ffi.check(_ffi.lib().sp_wbic(*[_ffi.ptr(v.data_ptr()) for _, v in ins], code, code, code, n, _ffi.ptr(sc), S, c["k_lo"],
                                  E.CWT_FAMILIES[c["spec"][0]], c["spec"][1], p["L"], p["M"], p["n0"], p["block"], p["step"], nb,
                                  *[_ffi.ptr(addr) for _, addr in outs], _ffi.C.byref(passes), 1))
    torch.cuda.synchronize()
    for (base, _), snap in zip(ins, snaps):
        assert G.unchanged(base, snap)
    for (base, _), nelem, key in zip(outs, (nb * S * S, nb * S * S, nb * S), ("B", "b2", "P")):
        assert G.guards_intact(base, 1, nelem)
        got = G.interior_of(base, 1, nelem).cpu().numpy()
        assert got.tobytes() == want[key].tobytes()             # NaN at the invalid pairs is the result there, so compare all of it
    assert passes.value == 1


def test_coupling_on_the_device():
    kw = dict(dt=1.0, df=R.QPC_DF, fmin=R.QPC_KLO * R.QPC_DF, fmax=R.QPC_KHI * R.QPC_DF)
    f, t, B, b2 = WB.wavelet_bispectrum(R.qpc_record(0), **kw)
    R.assert_qpc_whole(b2)
    Bo, b2o, A, _ = R.qpc_reference(False)
    assert_parity(B, b2, Bo[0], b2o[0], A[0])
    f, t, B, b2 = WB.wavelet_bispectrum(R.qpc_record(12000), block=6000, **kw)
    assert B.shape == (4, 70, 70)
    R.assert_qpc_switched(b2)
    Bo, b2o, A, _ = R.qpc_reference(True)
    for b in range(4):
        assert_parity(B[b], b2[b], Bo[b], b2o[b], A[b])
    sb, tot = WB.summed_bicoherence(b2), WB.total_bicoherence(b2)
    m = R.QPC_COUPLED[2] - R.QPC_KLO
    assert sb.shape == (4, 70) and tot.shape == (4,) and np.all(np.isnan(sb[:, :R.QPC_KLO])) and sb[3, m] > sb[0, m]
