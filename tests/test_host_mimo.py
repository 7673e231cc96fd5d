"""Conditioned spectral analysis without a GPU: the identities the kernel rests on (on the reference), the float64 restatement within the
derived bound at every GPU case, the C ABI's declarations, bindings and refusals, the plan arithmetic (restated here, and under
sanitizers in tests/cond_plan_test.cpp), the significance level of the multiple coherence against a Monte Carlo run, and the end-to-end
record in float64 through scipy."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cond_ref as R
import pyfft_amd
from pyfft_amd import _ffi, mimo as M
from pyfft_amd.running import coherence_level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_entry():
    return _ffi.load_library()


@pytest.fixture(scope="module")
def e2e():
    x, y, h = R.record(1)
    f, G = R.scipy_csd(np.concatenate((x, y)))
    return x, y, h, f, G


# ---- the identities --------------------------------------------------------------------------------------------------
def test_the_three_identities_on_the_reference(e2e):
    """L_yx L_xx^-1 = G_yx G_xx^-1; L_yy L_yy^H = the Schur complement; partial coherence from the residual matrix = from the precision
    matrix, on the end-to-end record's matrices (measured: 2.4e-16 and 5.3e-15 relative for float64 numpy against the longdouble reference, 1.3e-21 inside the reference)"""
    G = e2e[4]
    worst = np.zeros(3)
    for Gb in G[1:-1:8]:
        ref = R.ref_cond(Gb, R.NX)
        A = ref["A"]
        Axx, Ayx, Ayy = A[:3, :3], A[3:, :3], A[3:, 3:]
        H = np.linalg.solve(Axx.astype(np.complex128).T, Ayx.astype(np.complex128).T).T
        worst[0] = max(worst[0], np.max(np.abs(ref["H"].astype(np.complex128) - H)) / np.max(np.abs(H)))
        schur = Ayy.astype(np.complex128) - H @ np.conj(Ayx.astype(np.complex128)).T
        worst[1] = max(worst[1], np.max(np.abs(ref["Gc"].astype(np.complex128) - schur)) / np.max(np.abs(schur)))
        # the two outputs given the three inputs: from the residual matrix, and from the precision matrix of all five
        Gc, P = ref["Gc"], ref["P"]
        a = np.abs(Gc[1, 0]) ** 2 / (np.real(Gc[0, 0]) * np.real(Gc[1, 1]))
        b = np.abs(P[4, 3]) ** 2 / (np.real(P[3, 3]) * np.real(P[4, 4]))
        worst[2] = max(worst[2], float(abs(a - b)))
    print("identities: H %.1e, Schur %.1e relative, partial coherence %.1e" % tuple(worst))
    assert worst[0] <= 1e-13 and worst[1] <= 1e-12 and worst[2] <= 1e-12


def test_the_multiple_coherence_identities_on_the_reference():
    """mcoh = 1 - Gc_ii / A_ii, and from the precision matrix 1 - 1 / (A_ii P_ii) with every other channel as an input"""
    G = R.matrices(5, 3, spread=1.0, eps=1e-2)[0]
    ref = R.ref_cond(G, 4)
    assert abs(ref["mcoh"][0] - (1 - np.real(ref["Gc"][0, 0]) / np.real(ref["A"][4, 4]))) < 1e-15
    assert abs(ref["mcoh"][0] - (1 - 1 / (np.real(ref["A"][4, 4]) * np.real(ref["P"][4, 4])))) < 1e-15
    assert np.max(np.abs(ref["P"] @ ref["A"] - np.eye(5))) < 1e-15
    assert np.max(np.abs(ref["L"] @ np.conj(ref["L"].T) - ref["A"])) < 1e-16 * np.max(np.abs(ref["A"]))
    # ordered conditioning: piv[j] = 1 / (inverse of the leading (j + 1) block)[j, j]
    for j in range(5):
        lead = R.ref_cond(G[:j + 1, :j + 1], j + 1)["P"]
        assert abs(ref["piv"][j] * np.real(lead[j, j]) - 1) < 1e-15
    # an order is the same as permuting the matrix first
    o = R.order_of(5, 0)
    a, b = R.ref_cond(G, 2, o), R.ref_cond(G[np.ix_(o, o)], 2)
    for k in R.WANT:
        assert np.array_equal(a[k], b[k])


# ---- the bound and the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GPU_N)
def test_the_restatement_stays_within_the_derived_bound(n):
    """at every GPU case; and the cases keep the bound under 1e-3 of every output's largest element, rho under 1e-3"""
    most, rel = {k: 0.0 for k in R.WANT}, {k: 0.0 for k in R.WANT}
    for q in R.q_of(n):
        for kind in ("identity", "random"):
            G, order, refs, bounds = R.case(n, q, kind)
            got = {k: [] for k in R.WANT}
            for s in range(3):
                x = R.restate_cond(G[s], q, order)
                assert x["status"] == 0
                for k in R.WANT:
                    got[k].append(x[k])
            share = R.share_of(got, refs, bounds)
            for k in R.WANT:
                most[k] = max(most[k], share[k])
                for ref, bd in zip(refs, bounds):
                    if ref[k].size and np.max(np.abs(ref[k])) > 0:
                        rel[k] = max(rel[k], float(np.max(bd[k]) / np.max(np.abs(ref[k]))))
            assert all(float(b["rho"]) < 1e-3 for b in bounds)
    print("n = %d: share of the bound %s; bound / largest element %s" % (n, {k: "%.2g" % v for k, v in most.items()}, {k: "%.1e" % v for k, v in rel.items()}))
    assert max(most.values()) <= 1.0
    assert max(rel.values()) < 1e-3


def test_the_cases_reach_the_condition_numbers_and_scales():
    conds = [np.linalg.cond(G) for n in R.GPU_N if n > 1 for G in R.matrices(n, 0)]
    assert 1e7 < max(conds) <= 1e8
    G = R.matrices(5, 0)
    assert np.max(np.abs(G[1])) < 1e-4 and np.max(np.abs(G[2])) > 1e4
    assert all(np.array_equal(g, np.conj(g.T)) for g in G)


def test_the_bound_has_no_measured_term():
    src = open(os.path.join(ROOT, "tests", "cond_ref.py")).read()
    body = src.split("def bound_of")[1].split("\n# ----")[0]
    assert "restate" not in body and "got" not in body
    # it scales with the matrix (absolute outputs) and is scale-free for the ratios
    G = R.matrices(5, 1, spread=2.0, eps=1e-3)[0]
    a, b = R.bound_of(R.ref_cond(G, 2)), R.bound_of(R.ref_cond(G * 1024.0, 2))
    assert np.allclose((b["Gc"] / a["Gc"]).astype(float), 1024.0) and np.allclose((b["H"] / a["H"]).astype(float), 1.0)
    assert np.allclose((b["mcoh"] / a["mcoh"]).astype(float), 1.0) and np.allclose((b["P"] / a["P"]).astype(float), 1 / 1024.0)


def test_the_flags_of_the_restatement():
    G = R.matrices(5, 2, spread=1.0, eps=1e-2)[0]
    # a duplicated input
    D = G.copy()
    D[1, :], D[:, 1] = D[0, :], D[:, 0]
    D[1, 1] = D[0, 0]
    x = R.restate_cond(D, 3)
    assert x["status"] == 2 and not np.any(x["H"]) and not np.any(x["Gc"]) and not np.any(x["mcoh"]) and not np.any(x["P"])
    assert x["piv"][0] == D[0, 0].real and not np.any(x["piv"][1:])
    y = R.restate_cond(D, 3, loading=1e-6)
    assert y["status"] == 0 and np.all(np.isfinite(y["H"]))
    # an output that is an exact combination of the inputs (every step of the factorisation is exact on this matrix)
    S, Hx = R.explained_output()
    x = R.restate_cond(S, 3)
    assert x["status"] == 4 and x["mcoh"][0] == 1.0 and not np.any(x["Gc"][0]) and not np.any(x["Gc"][:, 0]) and not np.any(x["P"])
    assert np.array_equal(x["H"], Hx) and x["piv"][3] == 0.0 and x["piv"][4] > 0 and 0 < x["mcoh"][1] < 1
    # NaN
    N = G.copy()
    N[0, 0] = np.nan
    x = R.restate_cond(N, 2)
    assert x["status"] == 1 and not np.any(x["H"]) and not np.any(x["piv"])
    assert R.restate_cond(np.zeros((4, 4)), 2)["status"] == 1


# ---- header, table, library --------------------------------------------------------------------------------------------
def test_exported_declared_and_bound():
    for name in ("cond", "cond_plan", "mimo_frf", "multiple_coherence", "partial_coherence", "conditioned_spectra", "ordered_spectra",
                 "multiple_coherence_level", "CondRefused", "CondResult"):
        assert getattr(pyfft_amd, name) is getattr(M, name)
    assert issubclass(M.CondRefused, ValueError) and issubclass(M.CondRefused, NotImplementedError)
    from pyfft_amd import engine
    assert not hasattr(engine, "cond") and not hasattr(engine, "cond_plan")
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)   # noqa: E731
    hdr = strip("spectral_mimo.h")
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.MIMO_SIGNATURES) == {"sp_cond", "sp_cond_plan"}
    assert len(_ffi.TABLES) == 6 and len(_ffi.MORE_TABLES) == 6 and _ffi.LATER_TABLES == (_ffi.DWT_SIGNATURES,)
    assert _ffi.ARRAY_TABLES == (_ffi.ARRAY_SIGNATURES,) and _ffi.MIMO_TABLES == (_ffi.MIMO_SIGNATURES,)
    for table in _ffi.TABLES + _ffi.MORE_TABLES + _ffi.LATER_TABLES + _ffi.ARRAY_TABLES:
        assert not set(_ffi.MIMO_SIGNATURES) & set(table)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, want in (("sp_cond", 20), ("sp_cond_plan", 5)):
        mt = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert mt and len([a for a in mt.group(1).split(",") if a.strip()]) == len(_ffi.MIMO_SIGNATURES[name][1]) == want
        assert hasattr(lib, name)
        assert getattr(_ffi.load_library(), name).argtypes == _ffi.MIMO_SIGNATURES[name][1]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "spectral_mimo.h":
            assert not declared & set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", strip(other))), other
    assert "include/spectral_mimo.h" in open(os.path.join(ROOT, "Makefile")).read()
    assert '#include "../../include/spectral_mimo.h"' in open(os.path.join(ROOT, "pyfft_amd", "csrc", "spectral.hip")).read()
    launch = open(os.path.join(ROOT, "pyfft_amd", "csrc", "launch.h")).read()
    assert "launch_cond" in launch and "SP_COND_GRID" in launch and '#include "cond_plan.h"' in launch
    kernel = open(os.path.join(ROOT, "pyfft_amd", "csrc", "k_cond.hip")).read()
    code = kernel.split("#include")[1].lower()
    assert "atomic" not in code and "hipmemset" not in code and "asm" not in code and "void k_cond(" in kernel and "lds_raise<k_cond>" in kernel


def plan_ref(n, count, want, hook=0):
    """cond_plan.h restated: pitch, threads, LDS bytes, raised, workgroups, matrices of a workgroup, offsets of W and of the diagonal"""
    pitch = n | 1
    mat = n * pitch * 16
    wantP = bool(want & 16)
    lds = mat * (2 if wantP else 1) + 64 * 8 + 16
    grid = min(count, 1 << 16)
    if hook > 0:
        grid = min(grid, hook)
    return (pitch, 64 if n <= 16 else 256 if n <= 32 else 512, lds, int(lds > 65536), grid, -(-count // grid) if grid else 0, mat if wantP else 0,
            mat * (2 if wantP else 1))


def test_plan_figures(monkeypatch):
    monkeypatch.delenv("SP_COND_GRID", raising=False)
    lib = _c_entry()
    out = np.zeros(8, dtype=np.int64)
    plan = lambda *a: (lib.sp_cond_plan(*a, _ffi.ptr(out)), tuple(int(v) for v in out))   # noqa: E731
    for n in range(1, 65):
        for want in (1, 15, 16, 31):
            for count in (0, 1, 3, 2049, 65536, 65537, 1 << 30):
                rc, got = plan(n, n // 2, count, want)
                assert rc == 0 and got == plan_ref(n, count, want), (n, want, count, got)
    assert plan(64, 32, 2049, 31)[1] == (65, 512, 133648, 1, 2049, 1, 66560, 133120)
    assert plan(45, 20, 3, 16)[1][2:4] == (65328, 0) and plan(46, 20, 3, 16)[1][2:4] == (69712, 1)
    assert plan(63, 20, 3, 15)[1][3] == 0 and plan(64, 20, 3, 15)[1][3] == 1
    assert plan(4, 2, 65536 * 4, 15)[1][4:6] == (65536, 4)
    monkeypatch.setenv("SP_COND_GRID", "1")
    assert plan(5, 2, 5, 31)[1] == plan_ref(5, 5, 31, hook=1) and plan(5, 2, 5, 31)[1][4:6] == (1, 5)
    monkeypatch.delenv("SP_COND_GRID")
    d = M.cond_plan(64, 32, 2049, M.COND_WANT)
    assert tuple(d[k] for k in M.COND_PLAN_NAMES) == plan_ref(64, 2049, 31) and d["lds_bytes"] <= 160 * 1024
    assert M.cond_plan(16, 8, 513) == pyfft_amd.cond_plan(16, 8, 513) and M.cond_plan(16, 8, 513, "P")["w_offset"] == 16 * 17 * 16
    assert lib.sp_cond_plan(8, 4, 1, 1, None) < 0
    for bad in ((0, 0, 1, 1), (65, 0, 1, 1), (8, -1, 1, 1), (8, 9, 1, 1), (8, 4, -1, 1), (8, 4, (1 << 40) + 1, 1), (8, 4, 1, 0), (8, 4, 1, 32)):
        assert lib.sp_cond_plan(*bad, _ffi.ptr(out)) < 0, bad
    for bad in ((0, 0), (65, 3), (8, -1), (8, 9), (8, 4, -1), (8, 4, 1, ("H", "Q")), (8, 4, 1, ())):
        with pytest.raises(M.CondRefused):
            M.cond_plan(*bad)


GOOD = dict(G=True, gld=36, n=6, count=2, order="perm", q=2, want=31, loading=0.0, H=True, hld=8, Gc=True, gcld=16, mcoh=True, mld=4, piv=True,
            pld=6, P=True, ppld=36, st=True)
SENT = -12345.0
NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(n=0), "n must"), (dict(n=65), "n must"), (dict(q=-1), "q must"), (dict(q=7), "q must"), (dict(count=-1), "count must"),
            (dict(count=(1 << 40) + 1), "count must"), (dict(want=0), "want must"), (dict(want=32), "want must"), (dict(gld=35), "G_ld"),
            (dict(hld=7), "H_ld"), (dict(gcld=15), "Gc_ld"), (dict(mld=3), "mcoh_ld"), (dict(pld=5), "piv_ld"), (dict(ppld=35), "P_ld"),
            (dict(loading=-1e-3), "loading"), (dict(loading=NAN), "loading"), (dict(loading=INF), "loading"), (dict(order="twice"), "order"),
            (dict(order="high"), "order"), (dict(order="negative"), "order"), (dict(G=False), "G is"), (dict(st=False), "status is"),
            (dict(H=False), "H is wanted"), (dict(Gc=False), "Gc is wanted"), (dict(mcoh=False), "mcoh is wanted"), (dict(piv=False), "piv is wanted"),
            (dict(P=False), "P is wanted")]


def _call(lib, p):
    G = np.ones(2 * 36 * 2)
    outs = [np.full(160, SENT) for _ in range(5)]
    st = np.full(2, -77, dtype=np.int32)
    order = {"perm": [5, 0, 3, 1, 2, 4], "twice": [5, 0, 3, 1, 3, 4], "high": [6, 0, 3, 1, 2, 4], "negative": [5, 0, -1, 1, 2, 4], None: None}[p["order"]]
    order = None if order is None else np.asarray(order, dtype=np.int32)
    ptr = _ffi.ptr
    H, Gc, mc, pv, P = (ptr(o) if p[k] else None for o, k in zip(outs, ("H", "Gc", "mcoh", "piv", "P")))
    rc = lib.sp_cond(ptr(G) if p["G"] else None, p["gld"], p["n"], p["count"], ptr(order), p["q"], p["want"], p["loading"], H, p["hld"], Gc, p["gcld"],
                     mc, p["mld"], pv, p["pld"], P, p["ppld"], ptr(st) if p["st"] else None, 0)
    return rc, (lib.sp_last_error() or b"").decode(), bool(all(np.all(o == SENT) for o in outs) and np.all(st == -77))


@pytest.mark.parametrize("over,word", REFUSALS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(REFUSALS)])
def test_c_refusals(over, word):
    rc, msg, untouched = _call(_c_entry(), dict(GOOD, **over))
    assert rc == -1 and msg.startswith("sp_cond: ") and word in msg and untouched, (rc, msg)


def test_nothing_to_do_returns_zero():
    lib = _c_entry()
    rc, msg, untouched = _call(lib, dict(GOOD, count=0))
    assert rc == 0 and untouched
    rc, msg, untouched = _call(lib, dict(GOOD, count=0, order=None, want=8, H=False, Gc=False, mcoh=False, P=False, G=False, st=False))
    assert rc == 0 and untouched


def test_front_ends_refuse_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_ffi, "lib", boom)
    monkeypatch.setattr(_ffi, "init", boom)
    G = np.ones((3, 6, 6), dtype=np.complex128)
    for args, kw in (((np.ones((3, 65, 65)), 2), {}), ((np.ones((3, 0, 0)), 0), {}), ((np.ones((3, 6, 5)), 2), {}), ((np.ones(6), 2), {}),
                     ((G, -1), {}), ((G, 7), {}), ((G, 2), dict(order=[0, 1, 2, 3, 4, 4])), ((G, 2), dict(order=[0, 1, 2, 3, 4])),
                     ((G, 2), dict(order=[0, 1, 2, 3, 4, 6])), ((G, 2), dict(order=[0.0, 1, 2, 3, 4, 5])), ((G, 2), dict(loading=-1.0)),
                     ((G, 2), dict(loading=NAN)), ((G, 2), dict(loading=INF)), ((G, 2), dict(want=("H", "G"))), ((G, 2), dict(want=()))):
        with pytest.raises(M.CondRefused):
            M.cond(*args, **kw)
    x = np.ones((3, 1000), dtype=np.float32)
    for fn, args, kw in ((M.mimo_frf, (x, np.ones((62, 1000), dtype=np.float32)), {}), (M.mimo_frf, (x, np.ones((2, 999), dtype=np.float32)), {}),
                         (M.mimo_frf, (x, x), dict(fs=0.0)), (M.mimo_frf, (x, x), dict(nperseg=1)), (M.mimo_frf, (x, x), dict(nperseg=2000)),
                         (M.mimo_frf, (x, x), dict(noverlap=256)), (M.mimo_frf, (x, x), dict(window=np.ones(5))), (M.mimo_frf, (x, x), dict(band=(3.0, 4.0))),
                         (M.multiple_coherence, (x, np.ones((2, 3, 4))), {}), (M.partial_coherence, (np.ones((65, 1000), dtype=np.float32),), {}),
                         (M.ordered_spectra, (x,), dict(nperseg=0)), (M.conditioned_spectra, (x, x), dict(fs=NAN))):
        with pytest.raises(M.CondRefused):
            fn(*args, **kw)


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """cond_plan.h in a stand-alone program built with g++ under ASan + UBSan, run as its own process"""
    exe = str(tmp_path / "cond_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "pyfft_amd", "csrc"), os.path.join(ROOT, "tests", "cond_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "cond_plan ok" in r.stdout


# ---- the significance level ------------------------------------------------------------------------------------------
def test_the_level_at_one_input_is_the_coherence_level():
    for nd in (2, 5, 16, 64, 1000):
        for p in (0.5, 0.9, 0.95, 0.99):
            assert M.multiple_coherence_level(nd, 1, p) == coherence_level(nd, 1.0 - p)
            from scipy.special import betaincinv
            assert abs(float(betaincinv(1, nd - 1, p)) - coherence_level(nd, 1.0 - p)) < 1e-12
    assert M.multiple_coherence_level(3, 3) == 1.0 and M.multiple_coherence_level(2, 8) == 1.0
    assert 0 < M.multiple_coherence_level(64, 3) < M.multiple_coherence_level(16, 3) < M.multiple_coherence_level(16, 8) < 1
    for bad in ((0, 1), (4, 0), (16, 3, 0.0), (16, 3, 1.0)):
        with pytest.raises(ValueError):
            M.multiple_coherence_level(*bad)
    assert "not independent" in M.multiple_coherence_level.__doc__


@pytest.mark.parametrize("nd", (16, 64))
@pytest.mark.parametrize("nin", (1, 3, 8))
def test_the_level_against_a_monte_carlo_run(nd, nin):
    """independent white channels, boxcar segments without overlap: the share of sample multiple coherences above the level lies within
    three binomial standard deviations of 1 - p"""
    p, nseg, trials = 0.95, 8, 2000
    rng = np.random.default_rng([nd, nin])
    x = rng.standard_normal((trials, nin + 1, nd, nseg))
    X = np.fft.rfft(x, axis=-1)[..., 1:nseg // 2]                   # interior bins: complex Gaussian, independent across segments
    X = np.moveaxis(X, -1, 1)                                        # [trials, bins, channels, nd]
    G = X @ np.conj(np.swapaxes(X, -1, -2)) / nd
    Gxx, gyx, gyy = G[..., :nin, :nin], G[..., nin, :nin], G[..., nin, nin].real
    sol = np.linalg.solve(np.swapaxes(Gxx, -1, -2), gyx[..., None])[..., 0]       # H: H Gxx = gyx
    mc = np.real(np.sum(sol * np.conj(gyx), axis=-1)) / gyy
    level = M.multiple_coherence_level(nd, nin, p)
    count = mc.size
    frac = float(np.mean(mc > level))
    sd = np.sqrt(p * (1 - p) / count)
    print("nd %d, nin %d: level %.4f, exceeded by %.4f of %d (1 - p = %.2f, 3 sd = %.4f)" % (nd, nin, level, frac, count, 1 - p, 3 * sd))
    assert abs(frac - (1 - p)) <= 3 * sd


# ---- the end-to-end record ---------------------------------------------------------------------------------------------
def test_the_record_of_three_inputs_and_two_outputs(e2e):
    """seed 1, 3 inputs, 2 outputs, 2^16 samples, nperseg 256, float64 through scipy.signal.csd: H within 0.1 of max |H| of the true
    responses (measured: see the printed figure), the inputs' matrix conditioned under 10"""
    x, y, h, f, G = e2e
    assert x.shape == (3, 1 << 16) and y.shape == (2, 1 << 16) and G.shape == (129, 5, 5)
    Ht = R.true_response(h)
    out = R.outputs_of(G, 3, ("H", "mcoh"))
    err = float(np.max(np.abs(out["H"] - Ht)) / np.max(np.abs(Ht)))
    kxx = max(np.linalg.cond(Gb[:3, :3]) for Gb in G)
    kall = max(np.linalg.cond(Gb) for Gb in G)
    print("record: |H - H_true| / max |H| = %.3f, cond(G_xx) <= %.1f, cond(G) <= %.1e, mcoh in %.3f .. %.3f"
          % (err, kxx, kall, out["mcoh"].min(), out["mcoh"].max()))
    assert err <= 0.1
    assert kxx <= 10


def test_the_end_to_end_allowance_is_measured(e2e):
    """twice the largest change of each output under 32 Hermitian perturbations of 2e-4 per element, printed for DESIGN.md"""
    G = e2e[4]
    al = R.allowance_of(G, 3, ("H", "mcoh", "Gc"))
    base = R.outputs_of(G, 3, ("H", "mcoh", "Gc"))
    al2 = R.allowance_of(G, 5, ("P",))
    al3 = R.allowance_of(G, 5, ("piv",), order=np.array([4, 2, 0, 1, 3]))
    rel = {k: float(np.max(al[k] / np.max(np.abs(base[k]).reshape(len(G), -1), axis=1))) for k in al}
    relP = float(np.max(al2["P"] / np.max(np.abs(R.outputs_of(G, 5, ("P",))["P"]).reshape(len(G), -1), axis=1)))
    relV = float(np.max(al3["piv"] / np.max(R.outputs_of(G, 5, ("piv",), order=np.array([4, 2, 0, 1, 3]))["piv"], axis=1)))
    print("allowance / the bin's largest element: H %.2e, mcoh %.2e, Gc %.2e, P %.2e, piv %.2e" % (rel["H"], rel["mcoh"], rel["Gc"], relP, relV))
    for v in list(rel.values()) + [relP, relV]:
        assert 0 < v < 1                  # a figure to be quoted, not a limit: the residual spectra and P are the sensitive ones
