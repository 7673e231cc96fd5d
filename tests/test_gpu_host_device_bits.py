"""Every engine call gives the same bits with numpy arrays (mem = 0, staged through the library's scratch buffers) as with the same
values in device tensors (mem = 1, the caller's own pointers).

The calls are the case table of tests/engine_trace.py (CASES: every engine function, records of 512 samples, 64-point frames) and
the cases below it here, which reach what the table does not: the long path of sp_welch_csd (a window of 4097 points, the shortest
that one workgroup does not transform), sp_welch_finish and sp_welch_apply with a given mean / state next to an odd and an even
number of bins (one- and two-sided), every subset of the four optional outputs of sp_cwt and sp_ssq, and the row means sp_cyclic,
sp_lomb and sp_lomb_sums compute by default and read back from the device (every lomb case of the table gives mean_value).  The values come from a generator seeded by the case, the same in both modes, so a
piece copied from a wrong offset reads other values.

Per case: a refusal the golden engine trace records for a mode (raised by engine.py before the library is reached; the two modes
word some of them differently, and a host array among device tensors is refused in device mode only) must come with that type and
message; otherwise both modes refuse alike (type and message) or both return arrays of the same dtype, shape and bytes, compared as
integer words -- the arrays that come back and every output array the engine allocated for the library to write.  Every output array
the engine allocates in host mode lies inside a sentinel-filled allocation (tests/guard_ref.py) with 1 KiB on either side that must
survive the call: a copy-back with too large a byte count lands there.  The device allocations start from the same sentinel, so an
element that a call leaves alone (the last column of the reflection coefficients of burg and yule, which share the pitch of the
polynomials) must be left alone in both modes.

EXEMPT names the cases whose result is not reproducible between two calls in the SAME mode, with the kernel that causes it
(float64 atomicAdd sums); they are held to their entry's tolerance in the GPU suite instead of to the bits.  OTHER_CALL and ASSEMBLED
name the two cases in which engine.py itself, not the staging, treats the modes differently."""
import json
import os
import zlib

import numpy as np
import pytest

import engine_trace as T
import guard_ref as G
from pyfft_amd import _ffi, engine as E

pytestmark = pytest.mark.gpu

GUARD_BYTES = 1024
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_trace.json")

N, NFFT, HOP, NFR, WIN = T.N, T.NFFT, T.HOP, T.NFR, T.WIN
F32, C64, F64 = T.F32, T.C64, T.F64

EXTRA = []


def extra(fn, name, build):
    EXTRA.append((name, fn, build))


# the long path of sp_welch_csd: its own successful return
LWIN, LHOP, LNFR = np.hanning(4097), 1000, 3
LN = (LNFR - 1) * LHOP + LWIN.size
extra("welch_csd", "long-4097", lambda A: T.K(A((LN,), F32), A((2, LN), F32), LWIN, LHOP, LNFR))
extra("welch_csd", "long-4097-c64-two", lambda A: T.K(A((LN,), C64), A((LN,), C64), LWIN, LHOP, LNFR, sided=E.SIDED_TWO))
# a given mean / state next to an odd number of bins (one-sided: 33 of nfft 66; two-sided: 65) and an even one (two-sided: 64)
for nfft, sided, tag in ((66, E.SIDED_ONE, "one-33"), (65, E.SIDED_TWO, "two-65"), (64, E.SIDED_TWO, "two-64")):
    extra("welch_finish", "mean-" + tag, lambda A, n=nfft, s=sided: T.K(n, A((2,), F64), 30, sided=s))
    extra("welch_apply", "state-" + tag, lambda A, n=nfft, s=sided: T.K(A((5 * n + 8,), F64), np.hanning(n), 30, sided=s))
# every subset of the four optional outputs of sp_cwt and sp_ssq (none: refused by the engine)
SSQ_H = np.hanning(NFFT)
SSQ_DH, SSQ_TH = np.gradient(SSQ_H), (np.arange(NFFT) - NFFT // 2) * SSQ_H
CWT_W = [1.0, 0.5, 0.25]
for m in range(16):
    b = [bool(m >> k & 1) for k in range(4)]
    tag = "".join(c for c, on in zip("WGRB", b) if on) or "none"
    extra("cwt", "subset-" + tag, lambda A, b=b: T.K(A((2, 400), F32), T.SCALES, "morlet", 6.0, T.CL, T.CM, W=b[0], gws=b[1],
                                                      recon=CWT_W if b[2] else None, bandpow=CWT_W if b[3] else None))
    tag = "".join(c for c, on in zip("TPIG", b) if on) or "none"
    extra("ssq", "subset-" + tag, lambda A, b=b: T.K(A((2, N), F32), SSQ_H, SSQ_DH, HOP, -NFFT // 2, NFR, th=SSQ_TH, T=b[0], P=b[1],
                                                      IF=b[2], GD=b[3], rel=1e-3))
# the row means sp_cyclic, sp_lomb and sp_lomb_sums take off by default: computed on the device, read back and judged in Python
extra("cyclic", "own-means", lambda A: T.K(A((2, N), F32), WIN, HOP, NFR, T.NU))
extra("cyclic", "own-means-y-c64", lambda A: T.K(A((2, N), C64), WIN, HOP, NFR, T.NU, y=A((2, N), C64), conj=True))
extra("lomb", "own-means", lambda A: T.K(A((N,), F64), A((2, N), F32), T.FREQ))
extra("lomb", "own-means-weights-3d", lambda A: T.K(A((N,), F64), A((2, 2, N), F32), T.FREQ, weights=T.squared(A((N,), F64)),
                                                     normalize="amplitude"))
extra("lomb_sums", "own-means", lambda A: T.K(A((N,), F64), A((2, N), F32), T.FREQ))

ALL = list(T.CASES) + EXTRA
IDS = ["%s/%s" % (c[1], c[0]) for c in ALL]

# case id -> (kernel whose float64 atomicAdd sums make two calls in one mode differ, the entry's tolerance in the GPU suite relative to
# the largest magnitude of the result).  Empty: at these shapes every case gave the same bits in two consecutive calls of either mode
# (256 frames at the most: no sum is split over workgroups that race for the order of their atomic adds).
EXEMPT = {
}
# cases in which engine.py hands the library another call in the two modes, so that staging is not all that differs
OTHER_CALL = {
    # device mode passes the rows at their pitch of n + 3, host mode packs them first, and k_ddc's oscillator follows the row pitch
    # (tests/guard_ref.py): the float32 phase of a sample is rounded from another product.  Each output is a sum of 9 float32
    # products, rounded at most twice each, and the oscillator's value once: 32 roundings of 2^-24 of the peak bound the difference
    "ddc/strided-rows": ("k_ddc (row pitch)", 32 * 2.0 ** -24),
}
# cases whose returned arrays engine.py computes from the library's output after the call, on the host with numpy and on the device
# with torch: re + 1j * im gives an imaginary -0.0 the sign +, torch.complex keeps it.  What the library wrote is compared bit by
# bit (the allocated outputs); the returned arrays as values
ASSEMBLED = {"csd_epilogue/twosided": "re + 1j * im against torch.complex(re, im)"}


class Seeded(T.Arrays):
    """The arrays of a case from a generator seeded by the case; in device mode on the GPU."""

    def __init__(self, mode, seed):
        T.Arrays.__init__(self, mode)
        self.rng = np.random.default_rng(seed)

    def __call__(self, shape, dtype="float32", host=False):
        v = self.rng.standard_normal(shape)
        if np.dtype(dtype).kind == "c":
            v = v + 1j * self.rng.standard_normal(shape)
        a = np.ascontiguousarray(np.asarray(v).astype(dtype))
        if self.dev and not host:
            import torch
            a = torch.from_numpy(a).cuda()
        self.made.append(a)
        return a


def leaves(result, found):
    """what a call returned as host numpy arrays, in order"""
    if isinstance(result, (tuple, list)):
        for v in result:
            leaves(v, found)
    elif isinstance(result, dict):
        for k in sorted(result):
            leaves(result[k], found)
    elif hasattr(result, "cpu"):
        found.append(result.cpu().numpy())
    elif result is not None:
        found.append(np.asarray(result))
    return found


def run(case, mode, guards=None):
    """one call against the built library -> ("refused", type name, message, its types as the trace lists them) or
    ("returned", [what came back as host arrays], [every output array the engine allocated for the call, as the library left it])"""
    name, fn, build = case
    A = Seeded(mode, zlib.crc32(("%s/%s" % (fn, name)).encode()))
    raw = []
    saved = E._HostMode.empty, E._DeviceMode.empty

    def guarded(self, shape, dt, like):
        shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(d) for d in shape)
        nelem, guard = int(np.prod(shape, dtype=np.int64)), GUARD_BYTES // np.dtype(dt).itemsize
        base, interior = G.sentinel_output(nelem, dt, 0, guard=guard)
        if guards is not None:
            guards.append((base, nelem, guard))
        raw.append(interior.reshape(shape))
        return raw[-1]

    def noted(self, shape, dt, like):
        raw.append(saved[1](self, shape, dt, like))
        G._words(raw[-1].reshape(-1)).fill_(G._SENTINEL_I32)     # as the host interior: an element no mode writes compares equal
        return raw[-1]
    try:
        args, kwargs = build(A)
        if fn == "welch_finish":             # the pending accumulation it finishes, in the same mode
            nfft = args[0]
            E.welch_accum(Seeded(mode, 7)((N,), C64), np.hanning(nfft), nfft // 2, (N - nfft) // (nfft // 2) + 1)
        E._HostMode.empty, E._DeviceMode.empty = guarded, noted
        try:
            result = getattr(E, fn)(*args, **kwargs)
        finally:
            E._HostMode.empty, E._DeviceMode.empty = saved
    except Exception as e:                   # noqa: BLE001 -- whatever the engine raises is the refusal under comparison
        return ("refused", type(e).__name__, str(e), [t.__name__ for t in T.REFUSAL_TYPES if isinstance(e, t)])
    return ("returned", leaves(result, []), leaves(raw, []))


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    wa, wb = np.frombuffer(a.tobytes(), np.uint8), np.frombuffer(b.tobytes(), np.uint8)
    bad = np.flatnonzero(wa != wb)
    assert bad.size == 0, "%s: %d bytes differ, the first in element %d of %d" % (what, bad.size, bad[0] // a.itemsize, a.size)


@pytest.fixture(scope="module")
def golden_refusals():
    _ffi.init()
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    return {k: v["refused"] for k, v in cases.items() if "refused" in v}


def test_the_cases_reach_what_the_table_does_not():
    assert len(T.CASES) == 628 and len({c[1] for c in T.CASES}) == 53
    # one workgroup transforms powers of two up to max_wg_fft() and, by Bluestein, other lengths n with 2 n - 1 below it
    assert LWIN.size == 4097 and 2 * 4096 - 1 <= E.max_wg_fft() < 2 * LWIN.size - 1
    assert len({i for i in IDS if i.startswith(("cwt/subset-", "ssq/subset-"))}) == 32
    assert len(EXEMPT) + len(OTHER_CALL) <= len(ALL) // 10 and set(EXEMPT) | set(OTHER_CALL) | set(ASSEMBLED) <= set(IDS)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_host_arrays_and_device_tensors_give_the_same_bits(case, golden_refusals):
    cid = "%s/%s" % (case[1], case[0])
    guards = []
    got = {"host": run(case, "host", guards), "dev": run(case, "dev")}
    for base, nelem, guard in guards:
        G.guards_intact(base, 0, nelem, guard)
    recorded = {m: golden_refusals.get("%s/%s" % (cid, m)) for m in T.MODES}
    for m in T.MODES:
        if recorded[m] is not None:
            assert got[m][0] == "refused" and got[m][2] == recorded[m]["message"] and got[m][3] == recorded[m]["types"], (m, got[m])
    if any(r is not None for r in recorded.values()):
        return
    h, d = got["host"], got["dev"]
    assert h[0] == d[0], (h[:3], d[:3])
    if h[0] == "refused":
        assert h[1:3] == d[1:3]
        return
    assert len(h[1]) == len(d[1]) >= 1 and len(h[2]) == len(d[2])
    loose = EXEMPT.get(cid) or OTHER_CALL.get(cid)
    for kind, hs, ds in (("allocated output", h[2], d[2]), ("returned array", h[1], d[1])):
        for k, (a, b) in enumerate(zip(hs, ds)):
            what = "%s %d" % (kind, k)
            if loose:
                assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
                np.testing.assert_allclose(b, a, rtol=0, atol=loose[1] * float(np.max(np.abs(a), initial=0.0)), err_msg=what)
            elif kind == "returned array" and cid in ASSEMBLED:
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), what
            else:
                assert_same_bits(a, b, what)
