"""Host side of the polyphase synthesis bank: the float64 oracle pfb_synth_ref (the defining sum of sp_pfb_synth, a loop over the
frames), the least-squares dual prototype pfb_dual held to perfect reconstruction through pfb_ref -> pfb_synth_ref at hop <= M / 2 and
to its own reported residual at hop = 3 M / 4, pfb_alias_terms against the chain it describes, the host plan with every refusal that
comes before the library loads, and the declaration and binding of sp_pfb_synth.  No GPU needed.  tests/test_gpu_pfb_synth.py imports
pfb_synth_ref from here."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import pyfft_amd
from pyfft_amd import channelizer as CH
from pyfft_amd.baseband import Unsupported
from test_host_multitaper import make_signal, no_library        # noqa: F401  (no_library: a fixture)
from test_host_channelizer import pfb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pfb_synth_ref(X, tap, M, hop, first, nout, phase_ref=0, r0=0, onesided=False):
    """The definition along the last two axes, float64.  X [..., nframes, nb] frame-major; tap = g scale / M [ntaps];
    v_m[i] = sum_k X[m][k] exp(+2 pi i k i / M); y[a] = sum_m tap[a - s_m] v_m[(a - s_m + rho_m) mod M] over the frames with
    0 <= a - s_m < ntaps, s_m = first + m hop, in ascending m; rho_m = 0 (phase_ref 0) or (r0 + m hop) mod M (phase_ref 1).
    onesided: nb = M/2 + 1, Hermitian-extended, the imaginary parts of bins 0 and M/2 ignored -> float64 [..., nout]; otherwise
    nb = M -> complex128 [..., nout]."""
    X = np.asarray(X, dtype=np.complex128)
    tap = np.asarray(tap, dtype=np.float64)
    ntaps, nframes = tap.size, X.shape[-2]
    assert ntaps % M == 0
    if onesided:
        assert X.shape[-1] == M // 2 + 1
        low = X.copy()
        low[..., 0] = low[..., 0].real
        low[..., M // 2] = low[..., M // 2].real
        X = np.concatenate([low, np.conj(low[..., M // 2 - 1:0:-1])], axis=-1)
    assert X.shape[-1] == M
    v = np.fft.ifft(X, axis=-1) * M
    y = np.zeros(X.shape[:-2] + (nout,), dtype=np.complex128)
    n = np.arange(ntaps)
    for m in range(nframes):
        s = first + m * hop
        rho = (r0 + m * hop) % M if phase_ref else 0
        a = s + n
        ok = (a >= 0) & (a < nout)
        y[..., a[ok]] += tap[n[ok]] * v[..., m, (n[ok] + rho) % M]
    return y.real.copy() if onesided else y


def brute_alias(h, g, M, hop):
    """max |T - delta| from the double loop T[q][r] = sum_j g[r + j hop] h[r + j hop + q M], and the number of q terms."""
    Lh, Lg = len(h), len(g)
    worst, nq = 0.0, 0
    for q in range(-(Lg // M) - 1, Lh // M + 2):
        if not any(0 <= n + q * M < Lh for n in range(Lg)):
            continue
        nq += 1
        for r in range(hop):
            T = 0.0
            for n in range(r, Lg, hop):
                if 0 <= n + q * M < Lh:
                    T += g[n] * h[n + q * M]
            worst = max(worst, abs(T - (1.0 if q == 0 else 0.0)))
    return worst, nq


def prototype(M, taps):
    return ss.get_window("hann", M) if taps == 1 else CH.pfb_prototype(M, taps)


def round_trip(x, h, g, M, hop, center, n0, phase):
    """(y, valid) of pfb_ref -> pfb_synth_ref in float64 under the two host plans."""
    cplx = np.iscomplexobj(x)
    nsig = x.shape[-1]
    pa = CH.pfb_plan(nsig, cplx, M, hop=hop, h=h, center=center, n0=n0)
    ref_t = 1 if phase == "time" else 0
    X = pfb_ref(x, h, M, hop, pa["first"], pa["nframes"], ref_t, pa["r0"] if ref_t else 0)
    if not cplx:
        X = X[..., :M // 2 + 1]
    ps = CH.pfb_synthesis_plan(pa["nframes"], not cplx, M, hop=hop, g=g, center=center, n0=n0, nsig=nsig)
    assert (ps["first"], ps["r0"], ps["nout"]) == (pa["first"], pa["r0"], nsig)
    y = pfb_synth_ref(X, ps["g"] / M, M, hop, ps["first"], ps["nout"], ref_t, ps["r0"] if ref_t else 0, onesided=not cplx)
    return y, ps["valid"]


@pytest.mark.parametrize("M,taps,hop", [(16, 4, 8), (16, 8, 8), (16, 4, 5), (16, 1, 8)])
def test_dual_reconstructs_at_half_the_channel_count(M, taps, hop):
    """hop <= M / 2: the dual's residual is rounding, and analysis then synthesis returns the record on `valid` (measured <= 6e-15 of
    max |x|), for both phase references, a complex record and a real one through the one-sided bins."""
    h = prototype(M, taps)
    g, residual = CH.pfb_dual(h, M, hop)
    assert g.dtype == np.float64 and g.shape == h.shape
    print("residual %.3g" % residual)
    assert residual <= 1e-12
    nsig = 40 * M + 7
    for cplx in (True, False):
        x = make_signal(nsig, cplx, 81)
        for phase in ("time", "frame"):
            y, (lo, hi) = round_trip(x, h, g, M, hop, True, 5, phase)
            assert 0 <= lo < hi <= nsig and hi - lo > nsig // 2
            err = float(np.max(np.abs(y[lo:hi] - x[lo:hi])) / np.max(np.abs(x)))
            print("cplx %d phase %s: round trip %.3g" % (cplx, phase, err))
            assert err <= 1e-12


@pytest.mark.parametrize("M,taps,hop", [(16, 4, 12), (64, 8, 48)])
def test_dual_at_three_quarters(M, taps, hop):
    """hop = 3 M / 4: the reported residual is max |T - delta| by the double loop, and the round trip stays within
    (number of q terms) * residual * max |x| on `valid`."""
    h = prototype(M, taps)
    g, residual = CH.pfb_dual(h, M, hop)
    worst, nq = brute_alias(h, g, M, hop)
    print("residual %.3g, brute force %.3g, %d terms" % (residual, worst, nq))
    assert abs(residual - worst) <= 1e-12
    assert 1e-6 < residual < 1e-2              # neither rounding nor useless
    x = make_signal(40 * M + 7, True, 82)
    for phase in ("time", "frame"):
        y, (lo, hi) = round_trip(x, h, g, M, hop, True, 5, phase)
        err = float(np.max(np.abs(y[lo:hi] - x[lo:hi])))
        print("phase %s: round trip %.3g of max |x|" % (phase, err / np.max(np.abs(x))))
        assert err <= nq * residual * np.max(np.abs(x))


def test_no_dual_at_critical_sampling():
    """hop = M: a dual of this length does not exist; pfb_dual says so through the residual (0.25 for the default prototype)."""
    _, residual = CH.pfb_dual(CH.pfb_prototype(16, 4), 16, 16)
    assert 0.1 < residual < 0.5
    g, residual = CH.pfb_dual(CH.pfb_prototype(16, 4), 16, 8, taps=6)     # a dual of another length than h
    assert g.shape == (96,) and residual <= 1e-12


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("phase", ["time", "frame"])
def test_alias_terms_describe_the_chain(center, phase):
    """A random g that is no dual: y[a] = sum_q T[q][(a - first) mod hop] x[a + q M] on `valid`, x zero outside the record."""
    M, P, hop = 16, 3, 11
    rng = np.random.default_rng(83)
    h = CH.pfb_prototype(M, P)
    g = rng.standard_normal(2 * M)                          # shorter than h
    T = CH.pfb_alias_terms(h, g, M, hop)
    q0 = (g.size - 1) // M
    assert T.dtype == np.float64 and T.shape == (q0 + (h.size - 1) // M + 1, hop)
    x = make_signal(30 * M + 3, True, 84)
    first = -(g.size // 2) if center else 0                 # the synthesis plan's first for this g; the analysis is run from there
    nf =(x.size - first + hop - 1) // hop
    ref_t = 1 if phase == "time" else 0
    r0 = (77 + first) % M if ref_t else 0
    X = pfb_ref(x, h, M, hop, first, nf, ref_t, r0)
    y = pfb_synth_ref(X, g / M, M, hop, first, x.size, ref_t, r0)
    lo, hi = max(0, first + g.size - hop), min(x.size, first + nf * hop)
    xe = np.concatenate([np.zeros(q0 * M + M), x, np.zeros(h.size + M)])
    off = q0 * M + M
    a = np.arange(lo, hi)
    want = np.zeros(a.size, dtype=np.complex128)
    for i in range(T.shape[0]):
        want += T[i][(a - first) % hop] * xe[off + a + (i - q0) * M]
    assert hi - lo > 20 * M
    assert np.max(np.abs(y[lo:hi] - want)) <= 1e-12 * np.max(np.abs(x))


def test_synth_ref_is_the_adjoint_of_the_analysis():
    """<pfb_ref(x), X> = <x, pfb_synth_ref(X)> with tap = h (scale = M): the synthesis sum is the adjoint of the analysis sum."""
    M, P, hop, nsig = 16, 3, 11, 300
    h = CH.pfb_prototype(M, P)
    rng = np.random.default_rng(85)
    x = make_signal(nsig, True, 86)
    for first, ref_t, r0 in ((0, 0, 0), (-20, 1, 7)):
        nf = 24
        X = rng.standard_normal((nf, M)) + 1j * rng.standard_normal((nf, M))
        lhs = np.vdot(X, pfb_ref(x, h, M, hop, first, nf, ref_t, r0))
        rhs = np.vdot(pfb_synth_ref(X, h, M, hop, first, nsig, ref_t, r0), x)
        assert abs(lhs - rhs) <= 1e-11 * abs(lhs)


def test_plan_geometry():
    M, P, hop, fs, n0 = 64, 4, 24, 1000.0, 12345
    L = M * P
    p = CH.pfb_synthesis_plan(50, True, M, P, hop, fs=fs, n0=n0)
    assert (p["first"], p["r0"], p["nout"], p["L"], p["P"], p["hop"], p["nb"]) == (0, n0 % M, 49 * hop + L, L, P, hop, M // 2 + 1)
    assert p["valid"] == (L - hop, 50 * hop)
    g, residual = CH.pfb_dual(CH.pfb_prototype(M, P), M, hop)
    assert np.array_equal(p["g"], g) and p["residual"] == residual and residual <= 1e-12
    np.testing.assert_allclose(p["t"], (n0 + np.arange(p["nout"])) / fs, rtol=0, atol=1e-12)
    c = CH.pfb_synthesis_plan(50, False, M, P, hop, fs=fs, center=True, n0=n0)
    assert (c["first"], c["r0"], c["nout"], c["nb"]) == (-(L // 2), (n0 - L // 2) % M, 50 * hop, M)
    assert c["valid"] == (L // 2 - hop, 50 * hop - L // 2)
    # the plans of the two directions agree on first and r0
    a = CH.pfb_plan(50 * hop, True, M, P, hop, center=True, n0=n0)
    assert (a["first"], a["r0"], a["nframes"]) == (c["first"], c["r0"], 50)
    own = CH.pfb_synthesis_plan(3, True, M, g=np.hanning(3 * M), hop=200, nsig=1000)
    assert own["residual"] is None and (own["P"], own["nout"]) == (3, 1000) and own["valid"] == (0, 600)
    few = CH.pfb_synthesis_plan(1, True, M, P, hop)         # one frame: nothing is complete
    assert few["valid"][0] >= few["valid"][1] or few["valid"] == (L - hop, hop)
    assert CH.pfb_synthesis_plan(10, True, M)["hop"] == M


def test_refusals_come_before_the_library(no_library):
    Z = np.zeros((33, 40), dtype=np.complex64)
    for M in (48, 1, 0, 16384):
        with pytest.raises(Unsupported):
            CH.pfb_synthesis_plan(40, True, M)
        with pytest.raises(Unsupported):
            CH.synthesize(Z, M)
    with pytest.raises(ValueError, match="multiple of M"):
        CH.synthesize(Z, 64, g=np.ones(100))
    with pytest.raises(ValueError, match="multiple of M"):
        CH.synthesize(Z, 64, h=np.ones(0), hop=32)
    with pytest.raises(Unsupported):
        CH.synthesize(Z, 64, taps=33)
    with pytest.raises(Unsupported):
        CH.synthesize(np.zeros((9, 40), dtype=np.complex64), 16, g=np.ones(16 * 33))
    with pytest.raises(Unsupported):
        CH.synthesize(Z, 64, g=np.ones(128) * 1j)
    with pytest.raises(Unsupported):
        CH.synthesize(Z, 64, h=np.ones(128) * 1j)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, g=np.full(128, np.nan))
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, h=np.full(128, np.inf), hop=32)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, hop=0)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, taps=0)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, hop=32, fs=0.0)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, hop=32, phase="absolute")
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, hop=32, nsig=0)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, hop=32, scale=float("inf"))
    with pytest.raises(ValueError, match="bins"):
        CH.synthesize(Z, 64, hop=32, input_onesided=False)
    with pytest.raises(ValueError, match="bins"):
        CH.synthesize(np.zeros((64, 40), dtype=np.complex64), 64, hop=32)
    with pytest.raises(ValueError):
        CH.synthesize(Z.real, 64, hop=32)
    with pytest.raises(ValueError):
        CH.synthesize(Z[0], 64, hop=32)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, hop=32, freq_axis=-1, time_axis=1)
    with pytest.raises(ValueError):
        CH.synthesize(Z, 64, hop=32, freq_axis=2)
    with pytest.raises(ValueError):
        CH.synthesize(np.zeros((33, 0), dtype=np.complex64), 64, hop=32)
    with pytest.raises(ValueError):
        CH.pfb_synthesis_plan(0, True, 64)
    with pytest.raises(ValueError):
        CH.pfb_dual(np.ones((2, 8)), 8, 4)
    with pytest.raises(ValueError):
        CH.pfb_dual(np.ones(16), 8, 0)
    with pytest.raises(ValueError):
        CH.pfb_alias_terms(np.ones(16), np.ones(0), 8, 4)
    CH.pfb_dual(CH.pfb_prototype(64, 4), 64, 32)
    CH.pfb_alias_terms(np.ones(16), np.ones(16), 8, 4)
    CH.pfb_synthesis_plan(40, True, 64, hop=32)


def test_exported():
    for name in ("pfb_alias_terms", "pfb_dual", "pfb_synthesis_plan", "synthesize"):
        assert getattr(pyfft_amd, name) is getattr(CH, name)
    assert callable(pyfft_amd.engine.pfb_synth)


def test_declared_and_bound():
    from pyfft_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "spectral.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    mt = re.search(r"int sp_pfb_synth\(([^;]*)\);", hdr)
    assert mt, "sp_pfb_synth is not declared in include/spectral.h"
    nargs = len([a for a in mt.group(1).split(",") if a.strip()])
    assert "sp_pfb_synth" in _ffi.SIGNATURES and len(_ffi.SIGNATURES["sp_pfb_synth"][1]) == nargs == 16
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "sp_pfb_synth")
