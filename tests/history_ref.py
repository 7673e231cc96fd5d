"""The instrument of the call-history tests: a result of libspectral is a function of its arguments alone.

libspectral is one process-wide engine whose scratch buffers only grow and are never cleared, so what a call computes could depend on what
the process ran before it: a kernel that reads a scratch element it did not write (padding, a halo, the tail of a staged row) and gives it
a zero weight is right as long as that element is finite, and wrong for the rest of the process once one measured record with a NaN
dropout went through.  Here

    CASES             one small case per public entry of pyfft_amd.engine: the call, its sample arrays as the device sees them, its
                      float64 reference and the acceptance function its family's own test uses (no tolerance is introduced here);
    EXCLUDED          the public names of the engine that are not cases, each with its reason; PENDING those whose case is still to be
                      written (tests/test_host_history_ref.py holds the three together to the engine's public names);
    predecessors      the two calls that go before a case in a history: the case with every extent that sizes a buffer doubled, then the
                      case's exact shape, both with the sample values alone replaced by a fill: `quiet` unit noise, `nan` every sample
                      NaN, `loud` 2^60 x unit noise (finite in float32, and so are its squares: a stale value that a comparison or an
                      fmaxf would swallow as NaN arrives as a huge finite number instead);
    MEDLEY            a fixed list of nan and loud calls of other families that together reach the buffers every call shares;
    run_histories     the one driver: the case's result after each history.  The GPU test and the numpy stand-in of the host test both
                      go through it.

A helper module, not a test: nothing here is collected, and nothing here needs a GPU until a runner is called."""
import collections
import os

import numpy as np

import guard_ref as G

LOUD = 2.0 ** 60                      # the one new constant: 2^60 and its square 2^120 are finite in float32 (max 2^128)
FILLS = ("quiet", "nan", "loud")
MEMORIES = ("host", "device")
PRED_SEED = 777000                    # the predecessors' noise: never a case's seed (guard_ref's are below 200000)


class HCase(object):
    """id, family (the name in pyfft_amd.engine), arrays (the sample arrays, read-only), run(arrays) -> the engine's result,
    accept(got, what) (raises AssertionError), grown() -> (shapes of the doubled arrays, run for them), finite (the family's check
    demands finite results), refusal: None, or (exception types, the documented words) when the family refuses a non-finite record; a
    third element ("host",) marks a refusal that engine.py makes for host arrays before the library is entered (device tensors of the
    same values go through and must simply return): the nan predecessors must meet it, but it gives no `refused` history"""

    def __init__(self, id, family, arrays, run, accept, grown, finite=True, refusal=None, also=(), ref=None):
        self.id, self.family, self.arrays, self.run, self.accept, self.grown = id, family, tuple(arrays), run, accept, grown
        self.finite, self.refusal, self.also = finite, refusal, tuple(also)
        self.ref = ref                       # () -> the float64 reference the acceptance function compares with (arrays, tuple or dict)

    def __repr__(self):
        return "HCase(%s)" % self.id


Call = collections.namedtuple("Call", "run arrays family expect")          # expect: None, or (exception types, words) it must raise


def is_torch(a):
    return type(a).__module__.startswith("torch")


def fill_array(shape, dtype, fill, seed):
    """the sample array of a predecessor: the fill in every sample, both parts for complex"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64))
    if fill == "nan":
        a = np.full(n, np.nan, dtype=dtype)
        if dtype.kind == "c":
            a = a + 1j * a                                # (NaN + NaN j)
            a = a.astype(dtype)
            a.imag[:] = np.nan
    else:
        rng = np.random.default_rng(seed)
        a = rng.standard_normal(n)
        if dtype.kind == "c":
            a = a + 1j * rng.standard_normal(n)
        if fill == "loud":
            # |sample| >= 2^50 in every sample, each part for complex: the noise is kept away from zero
            if dtype.kind == "c":
                a = (np.sign(a.real) + (a.real == 0)) * (np.abs(a.real) + 1.0) + 1j * (np.sign(a.imag) + (a.imag == 0)) * (np.abs(a.imag) + 1.0)
            else:
                a = (np.sign(a) + (a == 0)) * (np.abs(a) + 1.0)
            a = a * LOUD
        else:
            assert fill == "quiet", fill
        a = a.astype(dtype)
    a = a.reshape(shape)
    a.setflags(write=False)
    return a


_FILLED = {}


def filled(shape, dtype, fill, seed):
    """fill_array, computed once per (shape, dtype, fill, seed) and shared: read-only"""
    key = (tuple(int(s) for s in shape), np.dtype(dtype).str, fill, seed)
    if key not in _FILLED:
        _FILLED[key] = fill_array(key[0], dtype, fill, seed)
    return _FILLED[key]


def predecessors(case, fill):
    """the two calls before the case in the history `fill`: the doubled extents, then the exact shape.  Only sample values differ from
    the case's own arguments: the runners are the case's (closed over its windows, taps, times, frequencies and counts)."""
    shapes2, run2 = case.grown()
    expect = case.refusal if fill == "nan" else None
    big = Call(run2, tuple(filled(s, a.dtype, fill, PRED_SEED + 1 + i) for i, (s, a) in enumerate(zip(shapes2, case.arrays))),
               case.family, expect)
    same = Call(case.run, tuple(filled(a.shape, a.dtype, fill, PRED_SEED + 11 + i) for i, a in enumerate(case.arrays)), case.family, expect)
    return [big, same]


# ======================================================================================================================================
# the medley: nan and loud calls that cover the buffers every call shares
# ======================================================================================================================================
def _engine():
    from pyfft_amd import engine
    return engine


def _m_xcorr(v):
    return _engine().xcorr_normalised(v[0], v[1])


def _m_welch_mean(v):
    return _engine().welch_psd(v[0], G.hann(1000), 250, 41, detrend=True, sided=_engine().SIDED_TWO, scale=1.0)


def _m_cog(v):
    return _engine().stft_cog(v[0], G.hann(256), 64, 61, 1000.0, detrend=True)


def _m_fft(v):
    return _engine().fft(v[0])


def _m_welch_long(v):
    return _engine().welch_psd(v[0], G.hann(16384), 8192, 6, detrend=3, sided=_engine().SIDED_TWO, scale=1.0)


def _m_csdm(v):
    return _engine().csd_matrix(v[0], G.hann(256), 128, 40, detrend=True, scale=1.0)


# (name, family, runner, [(shape, dtype)], host arrays only).  The largest case stages 8 MiB in and 16 MiB out (hilbert_rows 1 x 2^21)
# or 2 x 4 MiB in (xcorr_normalised 2^20): the first entry stages 2 x 16 MiB in (in0, in1) and 32 MiB out (out0) from host arrays in
# either memory's histories.
MEDLEY_SPEC = (
    ("staged-xcorr", "xcorr_normalised", _m_xcorr, [((1 << 22,), np.float32), ((1 << 22,), np.float32)], True),
    ("welch-mean", "welch_psd", _m_welch_mean, [((1000 + 40 * 250 + 3,), np.complex64)], False),        # work, small, onepass
    ("cog", "stft_cog", _m_cog, [((256 + 60 * 64 + 5,), np.float32)], False),                          # small, trends
    ("fft-10000", "fft", _m_fft, [((6, 10000), np.complex64)], False),                                 # blueA / blueB
    ("fft-2^20", "fft", _m_fft, [((3, 1 << 20), np.complex64)], False),                                # bigA / bigB / bigT
    ("welch-long", "welch_psd", _m_welch_long, [((16384 + 5 * 8192 + 9,), np.complex64)], False),      # longrec, trends
    ("csd-matrix", "csd_matrix", _m_csdm, [((6, 256 + 39 * 128 + 7), np.float32)], False),
)
MEDLEY_STAGED_BYTES = 2 * 4 * (1 << 22)


def medley(fills=("nan", "loud"), host_entry=True):
    """the medley's calls: every entry with the nan fill, then every entry with the loud fill.  Call.expect is None: the older families
    given NaN samples simply return.  `hostonly` entries are always called with numpy arrays (marked by family 'host:...')."""
    out = []
    for fill in fills:
        for k, (name, family, run, specs, hostonly) in enumerate(MEDLEY_SPEC):
            if hostonly and not host_entry:
                continue
            arrays = tuple(filled(s, dt, fill, PRED_SEED + 100 + 10 * k + i) for i, (s, dt) in enumerate(specs))
            out.append(Call(run, arrays, ("host:" if hostonly else "") + family, None))
    return out


def histories_of(case):
    """the histories a case is run after, in order (the same in both memories)"""
    h = ["quiet", "quiet2", "nan", "loud", "medley"]
    if (case.refusal is not None and len(case.refusal) == 2) or case.also:
        h.append("refused")
    return h


def history_calls(case, history, medley_calls=None):
    """the predecessor calls of one history"""
    if history in ("quiet", "quiet2"):
        return predecessors(case, "quiet")
    if history in ("nan", "loud"):
        return predecessors(case, history)
    if history == "medley":
        calls = medley() if medley_calls is None else medley_calls
        return [c for c in calls if c.family.replace("host:", "") != case.family]
    if history == "refused":
        calls = [c for c in predecessors(case, "nan") if c.expect is not None]
        return calls + [Call(run, arrays, case.family, expect) for run, arrays, expect in case.also]
    raise KeyError(history)


class NotRefused(AssertionError):
    pass


def run_call(call, c, memory):
    """one predecessor: its output is discarded; a call that must refuse must refuse in its documented words"""
    mem = "host" if c.family.startswith("host:") else memory
    if c.expect is None or (len(c.expect) > 2 and mem not in c.expect[2]):
        call(c.run, c.arrays, mem)
        return
    types, words = c.expect[:2]
    try:
        call(c.run, c.arrays, mem)
    except types as e:
        assert words in str(e), "refused in other words than %r: %s" % (words, e)
    else:
        raise NotRefused("a %s call that must be refused (%r) returned" % (c.family, words))


def run_histories(call, case, memory, medley_calls=None, histories=None):
    """call(run, arrays, memory) -> the result on the host.  Returns an ordered dict history -> the case's result right after the
    history's predecessor calls, for 'quiet', 'quiet2' (the baseline twice: where these two differ the family's order of additions
    varies and bits cannot be demanded), 'nan', 'loud', 'medley' and, where the family has a refusal, 'refused'."""
    out = collections.OrderedDict()
    for h in (histories_of(case) if histories is None else histories):
        for c in history_calls(case, h, medley_calls):
            run_call(call, c, memory)
        out[h] = call(case.run, case.arrays, memory)
    return out


def triples(cases=None):
    """every (case id, history, memory) the tests run: the full product, minus the 'refused' history for the families that have no
    refusal, plus the medley on another stream ('stream'), which exists for device memory only"""
    out = []
    for c in (CASES if cases is None else cases):
        for memory in MEMORIES:
            for h in histories_of(c):
                if h != "quiet2":
                    out.append((c.id, h, memory))
        out.append((c.id, "stream", "device"))
    return out


def leaves(got):
    """a result as a tuple of numpy arrays (None entries dropped, python scalars made arrays)"""
    if isinstance(got, (tuple, list)):
        return tuple(a for g in got for a in leaves(g))
    if isinstance(got, dict):
        return tuple(a for k in sorted(got) for a in leaves(got[k]))
    if got is None:
        return ()
    return (np.asarray(got),)


def same_bits(a, b):
    a, b = leaves(a), leaves(b)
    return len(a) == len(b) and all(u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes() for u, v in zip(a, b))


def all_finite(got):
    return all(np.all(np.isfinite(a)) for a in leaves(got) if a.dtype.kind in "fc")


def verdicts(case, results, bitwise=True):
    """history -> None, or what is wrong with the case's result after it: (1) not finite where the family's check demands it, (2) not
    accepted by the family's own acceptance function, (3) not the bits of the `quiet` baseline (bitwise=False: a family on the
    tolerance-only list)"""
    out = collections.OrderedDict()
    base = results["quiet"]
    for h, got in results.items():
        what = "%s after %s" % (case.id, h)
        bad = None
        if case.finite and not all_finite(got):
            bad = "not finite"
        if bad is None:
            try:
                case.accept(got, what)
            except AssertionError as e:
                bad = "not accepted: %s" % (e,)
        if bad is None and bitwise and not same_bits(got, base):
            bad = "accepted, but not the bits of the quiet baseline"
        out[h] = bad
    return out


# ======================================================================================================================================
# the case table
# ======================================================================================================================================
def _smallest(cases):
    """the first case of every family in guard_ref.INPUT_CASES (its smallest shape), in the table's order"""
    seen, out = set(), []
    for c in cases:
        if c.family not in seen:
            seen.add(c.family)
            out.append(c)
    return out


GUARD_LONG = ("hilbert_rows-f32-1x2097152", "xcorr_normalised-f32-n1048576")      # the long path: bigA / bigB / bigT


def _grow_guard(case, d):
    """(case', d') of the doubled predecessor: rows or channels, frames (the record lengthened to match), outputs m, and for the row
    transforms the next longer transform.  Windows, taps and scales stay the case's own."""
    p, f = dict(case.p), case.family
    shapes = [tuple(a.shape) for a in d["arrays"]]
    d2 = dict(d)

    def longer(extra=0):
        return [s[:-1] + (2 * s[-1] + extra,) for s in shapes]

    if f in ("mean", "biquad_filter", "fir_filter", "xcorr_normalised"):
        p["n"] = 2 * p["n"]
        shapes = longer()
    elif f in ("sos_filter", "sosfiltfilt"):
        p["rows"] = 2 * p["rows"]
        shapes = [(2 * shapes[0][0], shapes[0][1])]
    elif f in ("upfirdn", "ddc"):
        shapes = [(2 * shapes[0][0], 2 * shapes[0][1])]
    elif f in ("hilbert_rows", "spectral_filter_rows"):
        p["rows"], p["n"] = 2 * p["rows"], 2 * p["n"]
        shapes = [(2 * shapes[0][0], 2 * shapes[0][1])]
        if f == "spectral_filter_rows":
            d2["H"] = np.tile(d["H"], 2)
    elif f in ("welch_psd", "stft_frames", "stft_cog", "bispectrum"):
        p["M"] = 2 * p["M"]
        shapes = longer(d.get("hop", p.get("hop", 0)))
    elif f == "frame_sum":
        p["M"] = 2 * p["M"]
        shapes = [(2 * shapes[0][0], 2 * shapes[0][1] + p["hop"])]
    elif f == "welch_csd":
        p["M"], p["nch"] = 2 * p["M"], 2 * p["nch"]
        n2 = 2 * shapes[0][0] + p["hop"]
        shapes = [(n2,), (2 * shapes[1][0], n2)]
    elif f == "csd_matrix":
        p["M"], p["nch"] = 2 * p["M"], 2 * p["nch"]
        shapes = [(2 * shapes[0][0], 2 * shapes[0][1] + p["hop"])]
    elif f == "pfb":
        p["nf"] = 2 * p["nf"]
        shapes = [(2 * shapes[0][0], 2 * shapes[0][1] + p["D"])]
    elif f == "czt":
        p["batch"], p["m"], p["n"] = 2 * p["batch"], 2 * p["m"], 2 * p["n"]
        shapes = [(2 * shapes[0][0], 2 * shapes[0][1])]
    elif f in ("xcorr_frames", "skf"):
        p["nframes"] = 2 * p["nframes"]
        shapes = longer(d["shape"][2] if f == "xcorr_frames" else d["shape"][1])
    elif f == "welch_blocks":
        shapes = longer()                               # (the call takes its frame count from the record's length)
    elif f == "multitaper":
        shapes = longer()
    else:
        raise KeyError(f)
    case2 = case._replace(p=p)
    if f == "welch_blocks":                             # (the call reads the record's length from d["arrays"])
        d2["arrays"] = [np.empty(s, dtype=a.dtype) for s, a in zip(shapes, d["arrays"])]
    return case2, d2, shapes


def _guard_case(case):
    import test_gpu_offset_pointers as OP
    d = G.inputs(case)

    def run(v):
        return OP.call(case, d, list(v))

    def accept(got, what):
        got = tuple(np.asarray(g) for g in got) if isinstance(got, tuple) else (got if np.ndim(got) == 0 else np.asarray(got))
        OP.check(case, d, got, G.reference(case), what)
        frac = _guard_fraction(OP, case, d, got, G.reference(case))
        if frac is not None:
            print("%s: %.3g of the tolerance" % (what, frac))

    def grown():
        case2, d2, shapes = _grow_guard(case, d)
        return shapes, (lambda v: OP.call(case2, d2, list(v)))

    return HCase(case.id, case.family, d["arrays"], run, accept, grown, finite=case.family != "bispectrum", ref=lambda: G.reference(case))


def _guard_fraction(OP, case, d, got, ref):
    """the worst error as a fraction of the bound test_gpu_offset_pointers.check holds the family to, for the families whose branch
    there asserts without printing one (the bounds are restated from that function, branch by branch); None where check prints it"""
    p, f = case.p, case.family
    if f == "mean":
        return abs(got - ref) / 1e-9
    if f == "biquad_filter":
        return OP.peak_err(got, ref) / 3e-7
    if f in ("sos_filter", "sosfiltfilt"):
        return OP.rowerr(got, ref) / 5e-7
    if f in ("upfirdn", "ddc"):
        rms, loss = OP.restated(case, d)
        return float(np.max(np.abs(got.astype(ref.dtype) - ref))) / rms / (4.0 * loss)
    if f in ("fir_filter", "hilbert_rows", "spectral_filter_rows"):
        return OP.peak_err(got, ref) / (2e-5 if p["n"] >= (1 << 21) else 1e-4)
    if f in ("xcorr_normalised", "pfb", "czt"):
        return OP.peak_err(got, ref) / 1e-4
    if f == "xcorr_frames":
        return OP.peak_err(got.astype(ref.dtype), ref) / 1e-4
    if f == "csd_matrix":
        from test_gpu_kernels import _csd_per_bin_excess
        return _csd_per_bin_excess(got, ref)
    if f == "multitaper":                              # test_gpu_multitaper.assert_psd / assert_cross
        fr = [float(np.max(np.abs(g - r) / (2e-4 * np.abs(r) + 1e-6 * np.max(r)))) for g, r in zip(got[:2], ref[:2])]
        return max(fr + [float(np.max(np.abs(got[2] - ref[2]) / (2e-4 * np.abs(ref[2]) + 2e-6 * np.max(np.abs(ref[2])))))])
    if f == "bispectrum":                              # test_gpu_bispectrum.assert_parity: |dB| against 1e-4 A + 1e-6 max A, |db2| against 2e-4
        (B, b2, P), (Bo, b2o, A, Po) = got, ref
        ok = ~np.isnan(Bo)
        return max(float(np.max(np.abs(B[ok] - Bo[ok]) / (1e-4 * A[ok] + 1e-6 * np.nanmax(A)))), float(np.max(np.abs(b2[ok] - b2o[ok]))) / 2e-4)
    return None


def _fft_case(n):
    """fft against numpy: one workgroup (8), Bluestein (1000), five passes (16384), long Bluestein (10000), three passes (2^20)"""
    batch = 3 if n <= 16384 else 1
    x = G.noise(batch * n, True, 4000 + n % 9973).reshape(batch, n)
    x.setflags(write=False)
    # tests/test_gpu_kernels.py: test_fft_forward_inverse (powers of two up to 8192: 2e-6 sqrt(log2 n)), test_fft_arbitrary_length and
    # test_fft_long (4e-6 sqrt(log2 n)), of the largest |X|
    tol = (2e-6 if n == 8 else 4e-6) * max(1.0, np.sqrt(np.log2(n)))
    ref = []

    def accept(got, what):
        if not ref:
            ref.append(np.fft.fft(G.wide(x), axis=-1))
            ref.append(np.fft.ifft(G.wide(x), axis=-1))
        for got_, ref_, name in ((got[0], ref[0], "fft"), (got[1], ref[1], "ifft")):          # the same bound on both directions
            got_ = np.asarray(got_)
            assert got_.shape == ref_.shape and got_.dtype == np.complex64, what
            err = float(np.max(np.abs(got_ - ref_)) / np.max(np.abs(ref_)))
            print("%s %s: %.3g of the tolerance" % (what, name, err / tol))
            assert err <= tol, (what, name, err)

    def run(v):
        return _engine().fft(v[0]), _engine().ifft(v[0])

    return HCase("fft-c64-%dx%d" % (batch, n), "fft", [x], run, accept, lambda: ([(2 * batch, 2 * n)], run),
                 ref=lambda: (np.fft.fft(G.wide(x), axis=-1), np.fft.ifft(G.wide(x), axis=-1)))


def _welch_long_case(pipe):
    """welch_psd on the k_long_* path (nfft 16384, hop 8192, 5 frames: tests/test_gpu_long.py test_long_welch_psd_vs_oracle), and on the
    pipeline kernel with its ticket counters (nfft 4096, hop 2048, SP_WELCH_PIPE=2, 5 frames: tests/test_gpu_pipe.py)"""
    nfft, hop, M = (4096, 2048, 5) if pipe else (16384, 8192, 5)
    n = (M - 1) * hop + nfft + 17
    rng = np.random.default_rng(nfft % 9973)
    x = rng.standard_normal(n) + 0.7 * np.sin(2 * np.pi * 0.0123 * np.arange(n)) + 3.0
    x = (x + 1j * (rng.standard_normal(n) - 1.5)).astype(np.complex64)
    x.setflags(write=False)
    ref = []

    def welch(v, frames):
        from oracle import cpu_ref as O
        E = _engine()
        win = O.windows("Hanning", nwins=nfft)
        old = os.environ.get("SP_WELCH_PIPE")
        if pipe:
            os.environ["SP_WELCH_PIPE"] = "2"             # the library's existing switch, read at every call
        try:
            out = E.welch_psd(v[0], win, hop, frames, detrend=True, sided=E.SIDED_TWO, scale=1.0 / float(np.sum(win ** 2)))
            # the case is about the kernel it names: the pipeline with its ticket counters, or the multi-kernel long path
            assert E.profile_last_kernel().startswith("k_welch_pipe" if pipe else "k_long_"), E.profile_last_kernel()
            return out
        finally:
            if pipe:
                if old is None:
                    del os.environ["SP_WELCH_PIPE"]
                else:
                    os.environ["SP_WELCH_PIPE"] = old

    def reference():
        from oracle import cpu_ref as O
        if not ref:
            ref.append(O.welch_psd_stream(x, O.windows("Hanning", nwins=nfft), nfft, hop, M, 1.0, detrend_style=1))
        return ref[0]

    def accept(got, what):
        reference()
        got = np.asarray(got)
        r = float(np.max(np.abs(got - ref[0]) / (2e-4 * np.abs(ref[0]) + 1e-6 * ref[0].max())))      # rtol 2e-4, atol 1e-6 max: both tests
        print("%s: %.3g of the tolerance" % (what, r))
        assert got.shape == ref[0].shape and r <= 1.0, (what, r)

    also = ()
    if pipe:
        also = _dist_refusals()
    return HCase("welch_psd-c64-%s-%dx%d" % ("pipe" if pipe else "long", nfft, hop), "welch_psd", [x], lambda v: welch(v, M), accept,
                 lambda: ([(2 * n + hop,)], lambda v: welch(v, 2 * M)), also=also, ref=reference)


def _dist_refusals():
    """the welch_dist_submit refusals of tests/test_gpu_stream.py (test_stream_error_paths_and_empty_flush): device tensors only, so
    a host history moves the record to the device itself"""
    from pyfft_amd._ffi import SpectralError

    def submit(nfft, hop, frames, total):
        def run(v):
            import torch
            x = v[0] if is_torch(v[0]) else torch.from_numpy(np.array(v[0])).cuda()
            return _engine().welch_dist_submit(x, np.hanning(nfft), hop, frames, x.numel(), total)
        return run

    x = filled((16384 * 5,), np.complex64, "nan", PRED_SEED + 50)
    return ((submit(16384, 8192, 9, 9), (x,), ((SpectralError,), "not sharded")),
            (submit(1024, 100, 10, 10), (x,), ((SpectralError,), "hop")),
            (submit(1024, 512, 10, 5), (x,), ((SpectralError,), "frames_total")))


def _eigh_case():
    """eigh at order 17, batch 5 (tests/test_gpu_eigh.py: held); its refusal is the NaN matrix under check=True"""
    import eigh_ref as R
    a = R.fam_csd(np.random.default_rng(60), 5, 17)
    a.setflags(write=False)
    eps = np.finfo(np.float64).eps

    def run(v):
        return _engine().eigh(v[0])

    def accept(got, what):
        w, V, sw = (np.asarray(g) for g in got)
        t, L = R.tol(17), R.limits(a, w, V, sw)
        print("%s: %.3g of the tolerance" % (what, max(L["resid"], L["orth"], L["eig"]) / t))
        assert L["resid"] <= t and L["orth"] <= t and L["eig"] <= t, (what, L)
        assert L["descending"] and L["sweeps"] <= 30 and L["phase"] <= 4 * eps, (what, L)

    return HCase("eigh-c128-5x17", "eigh", [a], run, accept, lambda: ([(10, 33, 33)], run),
                 refusal=((np.linalg.LinAlgError,), "did not converge"), ref=lambda: np.linalg.eigvalsh(R.hermitian_from_lower(a)))


def _build_core():
    cases = [_guard_case(c) for c in _smallest(G.INPUT_CASES)]
    cases += [_guard_case(G.BY_ID[name]) for name in GUARD_LONG]
    cases += [_fft_case(n) for n in (8, 1000, 16384, 10000, 1 << 20)]
    cases += [_welch_long_case(False), _welch_long_case(True), _eigh_case()]
    return cases


# ======================================================================================================================================
# the entries outside guard_ref's table: each from its own reference module, at the smallest shape its GPU test runs, with that test's
# acceptance function
# ======================================================================================================================================
def beside(a, v):
    """an argument that is no sample array (times, weights, models' tables) in the memory of the samples v"""
    if a is None or not is_torch(v):
        return a
    import torch
    return torch.as_tensor(np.array(a), device=v.device)


FINITE = "finite"            # the word every refusal of a non-finite record carries, in host memory (engine.py) and device memory (spectral.hip)


def _refusal(name, *memories):
    from pyfft_amd import engine
    return ((getattr(engine, name),), FINITE) + ((memories,) if memories else ())


def _twice(t):
    """times for a record of twice the samples: the case's own, then the same again one span later"""
    t = np.asarray(t)
    return np.concatenate([t, t + (t.max() - t.min()) + 1.0])


def _uneven_cases():
    import lomb_ref as L
    import nufft_ref as N1
    import nufft2_ref as N2
    E = _engine()
    out = []

    # ---- nufft1 'tails' +1 (tests/test_gpu_nufft.py: test_shapes_against_the_direct_sums)
    t, c, t_ref = N1.signals("tails")
    f0, df = N1.grid_of("tails")
    M = N1.SHAPES["tails"]["M"]
    t2 = _twice(t)
    out.append(HCase("nufft1-tails+1", "nufft1", [c], lambda v: E.nufft1(beside(t, v[0]), v[0], f0, df, M, sign=1, t_ref=t_ref),
                     lambda got, what: N1.assert_within(np.asarray(got), N1.reference("tails", 1), c, what),
                     lambda: ([(2 * c.shape[0], 2 * c.shape[1])], lambda v: E.nufft1(beside(t2, v[0]), v[0], f0, df, 2 * M, sign=1, t_ref=t_ref)),
                     refusal=_refusal("NufftRefused"), ref=lambda: N1.reference("tails", 1)))

    # ---- nufft2 'tails' +1 (tests/test_gpu_nufft2.py: test_shapes_against_the_direct_sums)
    tb, F, tb_ref = N2.signals("tails")
    out.append(HCase("nufft2-tails+1", "nufft2", [F], lambda v: E.nufft2(beside(tb, v[0]), v[0], f0, df, sign=1, t_ref=tb_ref),
                     lambda got, what: N2.assert_within(np.asarray(got), N2.reference("tails", 1), F, what),
                     lambda: ([(2 * F.shape[0], 2 * F.shape[1])], lambda v: E.nufft2(beside(_twice(tb), v[0]), v[0], f0, df, sign=1, t_ref=tb_ref)),
                     refusal=_refusal("NufftRefused"), ref=lambda: N2.reference("tails", 1)))

    # ---- lomb 'tails', weights, floating mean, 'normalize' (tests/test_gpu_lomb.py: test_shapes_against_reference)
    form = (True, True, False, "normalize")
    lt, ly, lw, _ = L.signals("tails")
    y32 = ly.astype(np.float32)
    y32.setflags(write=False)
    f = L.freqs_of("tails", form)
    lt2, lw2, f2 = _twice(lt), np.concatenate([lw, lw]), np.concatenate([f, f + f[-1]])

    def lomb(v, t_, w_, f_):
        return E.lomb(beside(t_, v[0]), v[0], f_, weights=beside(w_, v[0]), floating_mean=True, normalize="normalize")

    out.append(HCase("lomb-tails-wf-normalize", "lomb", [y32], lambda v: lomb(v, lt, lw, f),
                     lambda got, what: L.assert_within(np.asarray(got), L.reference("tails", form), what),
                     lambda: ([(2 * y32.shape[0], 2 * y32.shape[1])], lambda v: lomb(v, lt2, lw2, f2)), refusal=_refusal("LombRefused"),
                     ref=lambda: L.reference("tails", form)))

    # ---- lomb_sums + lomb_finish (tests/test_gpu_lomb.py: test_finished_sums_are_the_periodogram_bitwise_and_parts_add_up): the sums
    # are held through their finished periodogram
    def sums(v, t_, w_, f_):
        s = E.lomb_sums(beside(t_, v[0]), v[0], f_, weights=beside(w_, v[0]))
        return s.common, s.rows, s.totals, E.lomb_finish(s, f_, floating_mean=True, normalize="normalize")

    out.append(HCase("lomb_sums-tails-w", "lomb_sums", [y32], lambda v: sums(v, lt, lw, f),
                     lambda got, what: L.assert_within(np.asarray(got[3]), L.reference("tails", form), what),
                     lambda: ([(2 * y32.shape[0], 2 * y32.shape[1])], lambda v: sums(v, lt2, lw2, f2)), refusal=_refusal("LombRefused"),
                     ref=lambda: L.reference("tails", form)))

    # ---- lomb_sums_grid 'ls-tails', weights (tests/test_gpu_nufft.py: test_lomb_sums_grid_against_the_direct_sums_and_every_form)
    gt, gy, gw, gf, (g0, gd) = N1.ls_signals("ls-tails")
    gM = gf.size

    def grid(v, t_, w_, m_):
        s = E.lomb_sums_grid(beside(t_, v[0]), v[0], g0, gd, m_, weights=beside(w_, v[0]))
        return s.common, s.rows, s.totals

    def grid_accept(got, what):
        common, rws, _ = N1.ls_sums_ref("ls-tails", True)
        w32, wy32, _, _ = N1.lomb_strengths(gt, gy, gw)
        ga, gb = N1.rows_as_complex(np.asarray(got[0]), np.asarray(got[1]))
        ra, rb = N1.rows_as_complex(common, rws)
        N1.assert_within(ga, ra, np.stack([w32, w32]), what + " A1, A2")
        N1.assert_within(gb, rb, wy32, what + " B")

    out.append(HCase("lomb_sums_grid-ls-tails-w", "lomb_sums_grid", [gy], lambda v: grid(v, gt, gw, gM), grid_accept,
                     lambda: ([(2 * gy.shape[0], 2 * gy.shape[1])], lambda v: grid(v, _twice(gt), np.concatenate([gw, gw]), 2 * gM)),
                     refusal=_refusal("LombRefused"), ref=lambda: N1.ls_sums_ref("ls-tails", True)[:2]))
    return out


def _ar_cases():
    import burg_ref as B
    import subspace_ref as S
    E = _engine()
    out = []
    name = "w64"
    c = B.shape_of(name)
    x = B.signals(name)

    def fit_case(method):
        fit = getattr(E, method)

        def accept(got, what):
            from test_gpu_parametric import held
            held(tuple(np.asarray(g) for g in got), name, method, what)

        return HCase("%s-%s" % (method, name), method, [x], lambda v: fit(v[0], c["n"], c["hop"], c["first"], c["nframes"], c["p"]), accept,
                     lambda: ([(2 * x.shape[0], 2 * x.shape[1] + 1)], lambda v: fit(v[0], c["n"], c["n"] + 1, c["first"], 2, c["p"])),
                     refusal=_refusal("ArRefused"), ref=lambda: B.reference(name, method))

    out += [fit_case("burg"), fit_case("yule")]

    # ---- covmat 'c64', forward-backward (tests/test_gpu_subspace.py: test_covmat_against_the_definition)
    sc = S.shape_of("c64")
    sx = S.signals("c64")

    def cov(v, frames, hop):
        return E.covmat(v[0], sc["n"], hop, sc["first"], frames, sc["m"], fb=True)

    def cov_accept(got, what):
        from test_gpu_subspace import cov_held
        cov_held(np.asarray(got), "c64", True)

    out.append(HCase("covmat-c64-fb", "covmat", [sx], lambda v: cov(v, sc["nframes"], sc["hop"]), cov_accept,
                     lambda: ([(2 * sx.shape[0], 2 * sx.shape[1] + 1)], lambda v: cov(v, 2, sc["n"] + 1)), refusal=_refusal("SubRefused")))
    out[-1].ref = lambda: S.cov_reference("c64", True)

    # ---- ar_ls 'w64' order 4 (tests/test_gpu_subspace.py: test_ar_ls_against_lstsq)
    def ls(v, frames, hop):
        return E.ar_ls(v[0], c["n"], hop, c["first"], frames, S.LS_CASES[name], fb=False)

    def ls_accept(got, what):
        from test_gpu_subspace import ls_held
        ls_held(tuple(np.asarray(g) for g in got), name, False, what)

    out.append(HCase("ar_ls-%s" % name, "ar_ls", [x], lambda v: ls(v, c["nframes"], c["hop"]), ls_accept,
                     lambda: ([(2 * x.shape[0], 2 * x.shape[1] + 1)], lambda v: ls(v, 2, c["n"] + 1)), refusal=_refusal("SubRefused")))
    out[-1].ref = lambda: S.ls_reference(name, False)[:2]
    return out


def _synthesis_cases():
    """istft_frames and pfb_synth at the shapes of tests/test_gpu_offset_pointers.py (test_sp_istft, test_sp_pfb_synth: the smallest of
    tests/test_gpu_istft.py and tests/test_gpu_pfb_synth.py), peak error 1e-4 as there"""
    import scipy.signal as ss
    E = _engine()
    out = []
    from test_gpu_istft import record, spectra, scipy_inverse
    nfft, hop, nch = 32, 8, 3
    win = ss.get_window("hann", nfft)
    x = record(40 * hop + nfft + 37, False, 7 * nfft + hop, nch=nch)
    Z = np.ascontiguousarray(spectra(x, win, nfft, hop, False, True))                       # [3, nfreq, nseg] complex64, bin-major
    Z.setflags(write=False)
    ref = []

    skip = nfft // 2

    def istft(v):
        nseg = int(v[0].shape[-1])
        return E.istft_frames(v[0], win, hop, sided=E.SIDED_HALF, bin_major=True, skip=skip, nout=(nseg - 1) * hop + nfft - 2 * skip - 3)

    def istft_accept(got, what):
        if not ref:
            ref.append(scipy_inverse(Z, win, nfft, hop, False, True))
        got = np.asarray(got)
        r = ref[0][..., :got.shape[-1]]
        err = float(np.max(np.abs(got - r)) / np.max(np.abs(r)))
        print("%s: %.3g of the tolerance" % (what, err / 1e-4))
        assert got.shape == r.shape and err <= 1e-4, (what, err)

    out.append(HCase("istft_frames-32x8-3ch", "istft_frames", [Z], istft, istft_accept,
                     lambda: ([(2 * nch, Z.shape[1], 2 * Z.shape[2])], istft)))
    out[-1].ref = lambda: scipy_inverse(Z, win, nfft, hop, False, True)

    from test_host_pfb_synth import pfb_synth_ref
    from test_gpu_pfb_synth import tap64, random_frames, SCALE, N0
    M, P, shop, nf, rows = 16, 1, 8, 257, 3
    L, nb = M * P, M // 2 + 1
    g = np.random.default_rng(91).standard_normal(L)
    X = random_frames((rows, nf, nb), 92 + nf)
    X.setflags(write=False)
    nout = (nf - 1) * shop + L - 3
    r0 = N0 % M
    pref = []

    def synth(v, no):
        return E.pfb_synth(v[0], g, M, shop, 0, no, 1, r0, onesided=True, scale=SCALE)

    def synth_accept(got, what):
        if not pref:
            pref.append(pfb_synth_ref(X, tap64(g, M), M, shop, 0, nout, 1, r0, onesided=True))
        got = np.asarray(got)
        err = float(np.max(np.abs(got - pref[0])) / np.max(np.abs(pref[0])))
        print("%s: %.3g of the tolerance" % (what, err / 1e-4))
        assert got.shape == pref[0].shape and err <= 1e-4, (what, err)

    out.append(HCase("pfb_synth-M16-half", "pfb_synth", [X], lambda v: synth(v, nout), synth_accept,
                     lambda: ([(2 * rows, 2 * nf, nb)], lambda v: synth(v, (2 * nf - 1) * shop + L - 3))))
    out[-1].ref = lambda: pfb_synth_ref(X, tap64(g, M), M, shop, 0, nout, 1, r0, onesided=True)
    return out


def _zoom_case():
    """zoom_welch through zoom.zoom_psd: nperseg 256, hop 128, 12 segments, 96 bins (tests/test_gpu_zoom.py: test_estimators' device
    half), check_psd of that module"""
    from pyfft_amd import zoom as ZM
    from test_host_multitaper import make_signal
    from test_host_zoom import zoom_oracle
    FS = 250.0
    nperseg, m, band = 256, 96, [0.28 * FS, 0.34 * FS]
    nsig = 12 * nperseg + 3
    kw = dict(fs=FS, window="hann", nperseg=nperseg, noverlap=128, detrend="constant")
    x = np.asarray(make_signal(nsig, False, 24)).astype(np.float32)
    x.setflags(write=False)
    ref = []

    def accept(got, what):
        from test_gpu_zoom import check_psd
        if not ref:
            ref.append(zoom_oracle(x.astype(np.float64), x.astype(np.float64), ZM.zoom_plan(nsig, False, band, m, **kw))["pxx"])
        check_psd(np.asarray(got), ref[0], what)

    return HCase("zoom_welch-256x128-m96", "zoom_welch", [x], lambda v: ZM.zoom_psd(v[0], band, m, **kw)[1], accept,
                 lambda: ([(2 * nsig + 128,)], lambda v: ZM.zoom_psd(v[0], band, 2 * m, **kw)[1]),
                 ref=lambda: zoom_oracle(x.astype(np.float64), x.astype(np.float64), ZM.zoom_plan(nsig, False, band, m, **kw))["pxx"])


def _wavelet_cases():
    """cwt and icwt_sum (tests/test_gpu_wavelet.py: test_w_against_reference, test_derived_outputs) and wct_time (tests/test_gpu_wct.py:
    test_coherence_against_reference) at L = 256, real records"""
    E = _engine()
    out = []
    import test_gpu_wavelet as TW
    x, sc, plan, ref, eps = TW.case_of("morlet", 256, False)
    param = TW.WAVELETS["morlet"].param

    def cwt(v):
        return E.cwt(v[0], sc, "morlet", param, 256, plan["M"])["W"]

    out.append(HCase("cwt-morlet-256", "cwt", [x[0]], cwt, lambda got, what: TW.check_rows(np.asarray(got), ref[0], eps, what),
                     lambda: ([(2, 2 * x.shape[-1])], cwt)))
    out[-1].ref = lambda: ref[0]

    S = len(sc)
    wr = (np.random.default_rng(256).uniform(0.2, 1.0, S) / np.sqrt(sc)).astype(np.float32)
    W = ref[0].astype(np.complex64)
    W.setflags(write=False)

    def icwt(v):
        return E.icwt_sum(v[0], wr)

    def icwt_accept(got, what):
        y = np.asarray(got)
        tol = 4 * S * 2.0 ** -24 * np.sum(np.abs(wr)[:, None] * np.abs(W), axis=0)
        check = np.sum(wr[:, None].astype(np.float64) * W, axis=0)
        print("%s: %.3g of the tolerance" % (what, float(np.max(np.abs(y - check) / tol))))
        assert y.dtype == np.complex64 and np.all(np.abs(y - check) <= tol), what

    out.append(HCase("icwt_sum-morlet-256", "icwt_sum", [W], icwt, icwt_accept, lambda: ([(S, 2 * W.shape[-1])], icwt)))
    out[-1].ref = lambda: np.sum(wr[:, None].astype(np.float64) * W, axis=0)

    import test_gpu_wct as TC
    cx, cy, cplan, refs, loss = TC.case_of(256, False)

    def wct(v):
        return E.wct_time(v[0], v[1], cplan["scales"], "morlet", 6.0, cplan["L"], cplan["Mw"], cplan["Mg"])

    out.append(HCase("wct_time-256", "wct_time", [cx[0], cy[0]], wct, lambda got, what: TC.check_T(np.asarray(got), refs[0], 2 * loss, what),
                     lambda: ([(2, 2 * cx.shape[-1]), (2, 2 * cx.shape[-1])], wct)))
    out[-1].ref = lambda: refs[0]["T"]
    return out


def _tfr_cases():
    """ssq (case 0 of ssq_ref.CASES), ssq_bands (case 2, the first with a band test), wvd ('n32-full-lag', auto), cyclic ('n32-real-tail'),
    fam ('np32-real-all'), wbic ('1-ragged-tile'): each against its module's reference with its module's acceptance function"""
    E = _engine()
    from pyfft_amd._ffi import SpectralError
    out = []
    import ssq_ref as SR
    import test_gpu_ssq as TS
    cs, x, w, c, sq = TS.case_of(0)

    def ssq(v, frames):
        return E.ssq(v[0], w[0], w[1], cs["hop"], cs["first"], frames, b0=0, nb=None, rel=SR.REL)[0]

    out.append(HCase("ssq-%s" % SR.case_id(cs), "ssq", [x], lambda v: ssq(v, SR.NFRAMES),
                     lambda got, what: TS.check_cells(np.asarray(got), sq["T"], sq["slackT"], sq["reach"], what),
                     lambda: ([(2, 2 * x.shape[-1] + cs["hop"])], lambda v: ssq(v, 2 * SR.NFRAMES))))
    out[-1].ref = lambda: sq["T"]

    cs2, x2, w2, c2, sq2 = TS.case_of(2)
    lo = sq2["b0"] + sq2["nb"] // 5
    m = np.array([[lo, lo + sq2["nb"] // 4], [lo + sq2["nb"] // 3, lo + sq2["nb"] // 2 + 7]]).astype(np.float64)
    edges = m - 0.5

    def bands(v, frames):
        return E.ssq_bands(v[0], w2[0], w2[1], cs2["hop"], cs2["first"], frames, edges, rel=SR.REL)

    def bands_accept(got, what):
        want, slack = SR.band_sums(c2, edges)
        big = np.max(c2["mag"], axis=1)
        err = np.abs(np.asarray(got) - want)
        tol = 2e-4 * np.abs(want) + 1e-6 * big + slack                       # test_band_sums_against_reference
        print("%s: %.3g of the tolerance" % (what, float(np.max(err / tol))))
        assert np.all(err <= tol), what

    out.append(HCase("ssq_bands-%s" % SR.case_id(cs2), "ssq_bands", [x2], lambda v: bands(v, SR.NFRAMES), bands_accept,
                     lambda: ([(2, 2 * x2.shape[-1] + cs2["hop"])], lambda v: bands(v, 2 * SR.NFRAMES))))
    out[-1].ref = lambda: SR.band_sums(c2, edges)[0]

    import wvd_ref as WR
    name = "n32-full-lag"
    s = WR.SHAPES[name]
    h, g = WR.windows_of(s)
    wx = WR.signals(name)[0]

    def wvd(v, times):
        return E.wvd(v[0], h, g, s["hop"], s["first"], times, s["nfft"], y=None, b0=s["b0"], nb=s["nb"])

    out.append(HCase("wvd-%s" % name, "wvd", [wx], lambda v: wvd(v, s["ntimes"]),
                     lambda got, what: WR.assert_within(np.asarray(got), WR.band(WR.reference(name, False), s), what),
                     lambda: ([(2 * wx.shape[0], 2 * wx.shape[1])], lambda v: wvd(v, 2 * s["ntimes"]))))
    out[-1].ref = lambda: WR.band(WR.reference(name, False), s)

    import cyclic_ref as CR
    cname = "n32-real-tail"
    cs_ = CR.SHAPES[cname]
    cx = CR.signals(cname)[0]
    cw = CR.hann(cs_["n"])

    def cyc(v, frames):
        return E.cyclic(v[0], cw, cs_["hop"], frames, cs_["nu"], y=None, conj=CR.form_args("auto")[1], first=cs_["first"], b0=cs_["b0"], nb=cs_["nb"])

    out.append(HCase("cyclic-%s" % cname, "cyclic", [cx], lambda v: cyc(v, cs_["nframes"]),
                     lambda got, what: CR.assert_within(tuple(None if a is None else np.asarray(a) for a in got), CR.reference(cname, "auto"), what,
                                                        sel=lambda a: CR.band(a, cs_)),
                     lambda: ([(2 * cx.shape[0], 2 * cx.shape[1] + cs_["hop"])], lambda v: cyc(v, 2 * cs_["nframes"])),
                     refusal=((SpectralError,), FINITE)))               # sp_cyclic: "mean_x and mean_y must be finite" (the record's own mean)
    out[-1].ref = lambda: tuple(a for a in CR.reference(cname, "auto") if a is not None)

    import fam_ref as FR
    fname = "np32-real-all"
    fs_ = FR.SHAPES[fname]
    fx = FR.signals(fname)[0]
    fa, fg = FR.windows(fname)
    pairs = FR.pairs_of(fname)

    def fam(v, blocks):
        return E.fam(v[0], fa, fs_["hop"], fg, blocks, pairs, y=None, conj=fs_["conj"])

    out.append(HCase("fam-%s" % fname, "fam", [fx], lambda v: fam(v, fs_["nblocks"]),
                     lambda got, what: FR.assert_within(tuple(None if a is None else np.asarray(a) for a in got), FR.reference(fname), pairs, what),
                     lambda: ([(2 * fx.shape[-1] + fs_["P"] * fs_["hop"],)] if fx.ndim == 1 else [(fx.shape[0], 2 * fx.shape[-1] + fs_["P"] * fs_["hop"])],
                              lambda v: fam(v, 2 * fs_["nblocks"])), refusal=_refusal("FamRefused")))   # "the mean of the record is not finite"
    out[-1].ref = lambda: tuple(a for a in FR.reference(fname) if a is not None)

    import test_gpu_wbic as TB
    bc = TB.case("1-ragged-tile")
    p = bc["plan"]

    def wbic(v, blocks):
        return E.wbic(v[0], bc["scales"], bc["k_lo"], bc["spec"][0], bc["spec"][1], p["L"], p["M"], p["n0"], p["block"], p["step"], blocks)

    def wbic_accept(got, what):
        got = {k: np.asarray(v) for k, v in got.items()} if isinstance(got, dict) else got
        TB.check_parity(got["B"], got["b2"], got["P"], bc["ref"], what)

    out.append(HCase("wbic-1-ragged-tile", "wbic", [bc["x"]], lambda v: wbic(v, p["nblocks"]), wbic_accept,
                     lambda: ([(2 * bc["x"].shape[-1],)], lambda v: wbic(v, p["nblocks"])), finite=False))
    out[-1].ref = lambda: bc["ref"]
    return out


def _model_cases():
    """ar_psd (tests/test_gpu_parametric.py: test_ar_psd_against_the_definition), pseudospectrum (tests/test_gpu_subspace.py:
    test_pseudospectrum_against_the_definition) and beamscan (tests/test_gpu_beam.py: test_beamscan_against_the_definition): their
    'samples' are the models they evaluate"""
    import beam_ref as BR
    import burg_ref as B
    import subspace_ref as S
    E = _engine()
    out = []
    ref = B.reference("w333c", "burg")
    a, Ev = np.ascontiguousarray(ref[0][0]), np.ascontiguousarray(ref[1][0, :, -1])
    m, start, step = 257, 0.0, 1.0 / 512

    def psd(v, bins):
        return E.ar_psd(v[0], v[1], bins, start, step, 0.5, True)

    def psd_accept(got, what):
        from test_gpu_parametric import _psd_bound
        got = np.asarray(got)
        want = np.stack([B.psd_def(a[s], Ev[s], m, start, step, 0.5) for s in range(a.shape[0])])
        bound = np.stack([_psd_bound(a[s], m, start, step) for s in range(a.shape[0])])
        print("%s: %.3g of the tolerance" % (what, float(np.max(np.abs(got - want) / (bound * want)))))
        assert got.shape == want.shape and np.all(np.abs(got - want) <= bound * want), what

    out.append(HCase("ar_psd-w333c-257", "ar_psd", [a, Ev], lambda v: psd(v, m), psd_accept,
                     lambda: ([(2 * a.shape[0], a.shape[1]), (2 * Ev.shape[0],)], lambda v: psd(v, 2 * m)), refusal=_refusal("ArRefused", "host")))
    out[-1].ref = lambda: np.stack([B.psd_def(a[s_], Ev[s_], m, start, step, 0.5) for s_ in range(a.shape[0])])

    mm = 2
    w3, V3 = BR.eig_of(mm)
    w1, V1 = np.ascontiguousarray(w3[:1]), np.ascontiguousarray(V3[:1])
    nb, pstart, pstep = 257, 0.0, 1.0 / 512

    def pseudo(v, bins):
        return E.pseudospectrum(v[0], v[1], 0, bins, pstart, pstep, "music", True)

    def pseudo_accept(got, what):
        P, st = (np.asarray(g) for g in got)
        want, st_ref = S.pseudo_def(V1[0], w1[0], 0, nb, pstart, pstep, "music")
        bound = S.pseudo_bound(V1[0], w1[0], 0, nb, pstart, pstep, "music")
        ok = want > 0
        err = np.abs(P[0][ok] - want[ok]) / want[ok]
        print("%s: %.3g of the tolerance" % (what, float(np.max(err / bound[ok]))))
        assert st[0] == st_ref == 0 and not np.any(np.isnan(P)) and np.all(err <= bound[ok]), what

    out.append(HCase("pseudospectrum-m2-music", "pseudospectrum", [V1, w1], lambda v: pseudo(v, nb), pseudo_accept,
                     lambda: ([(2, mm, mm), (2, mm)], lambda v: pseudo(v, 2 * nb)), refusal=_refusal("SubRefused", "host")))
    out[-1].ref = lambda: S.pseudo_def(V1[0], w1[0], 0, nb, pstart, pstep, "music")[0]

    nk, ndim, far = BR.GEOMS[0]
    pos, kv = BR.geometry(mm, nk, ndim, far)
    kv2 = np.concatenate([kv, kv + 0.25])

    def beam(v, k_):
        return E.beamscan(v[0], v[1], pos, k_, "bartlett", 0, 0.0, np.array(BR.SCALES), True)

    def beam_accept(got, what):
        P, st = (np.asarray(g) for g in got)
        want = np.stack([BR.beam_def(V3[s], w3[s], pos, kv, "bartlett", 0, 0.0, BR.SCALES[s])[0] for s in range(3)])
        bound = np.stack([BR.beam_bound(V3[s], w3[s], pos, kv, "bartlett", 0, 0.0, BR.SCALES[s]) for s in range(3)])
        print("%s: %.3g of the tolerance" % (what, float(np.max(np.abs(P - want) / bound))))
        assert not st.any() and not np.any(np.isnan(P)) and np.all(np.abs(P - want) <= bound), what

    out.append(HCase("beamscan-m2-bartlett", "beamscan", [V3, w3], lambda v: beam(v, kv), beam_accept,
                     lambda: ([V3.shape, w3.shape], lambda v: beam(v, kv2)), refusal=_refusal("BeamRefused", "host")))
    out[-1].ref = lambda: np.stack([BR.beam_def(V3[s_], w3[s_], pos, kv, "bartlett", 0, 0.0, BR.SCALES[s_])[0] for s_ in range(3)])
    return out


def _dwt_cases():
    """dwt, idwt, modwt, imodwt at n = 37, db4, one level, two real rows (tests/test_gpu_dwt.py: test_both_forms_forced,
    test_inverse_of_arbitrary_coefficients_and_the_round_trip, test_modwt_both_forms_inversion_and_energy), `held` of that module"""
    import dwt_ref as R
    import test_gpu_dwt as TD
    E = _engine()
    n, L, mode, levels = 37, 8, "symmetric", 1
    dl, dh, rl, rh = TD.bank(L)
    x, ref, bound, _, _ = TD.ref_pyramid(n, L, mode, levels, False)
    def dwt(v):
        return (E.dwt(v[0], dl, dh, mode, levels),) + tuple(E.dwt_level(v[0], dl, dh, mode))

    def dwt_accept(got, what):
        c, a, d = (np.asarray(g) for g in got)
        print("%s: %.3g of the tolerance" % (what, TD.held(c, ref, bound, what)))
        assert np.array_equal(TD.bits(np.concatenate((a, d), axis=-1)), TD.bits(c)), what + ": dwt_level is not dwt at one level"

    out = [HCase("dwt-db4-n37", "dwt", [x], dwt, dwt_accept, lambda: ([(4, 2 * n)], dwt))]
    out[-1].ref = lambda: ref

    lens, entries, total = E.dwt_layout(n, L, mode, levels)
    coef = R.signal(total, 2, False, seed=11 + L)
    coef.setflags(write=False)
    iref = []

    def idwt_accept(got, what):
        if not iref:
            parts = [coef[..., o:o + ln].astype(np.float64) for ln, o in entries]
            iref.append(R.waverec(parts, n, rl, rh, mode, bounds=[np.zeros(1)] * (levels + 1)))
        print("%s: %.3g of the tolerance" % (what, TD.held(np.asarray(got[0]), iref[0][0], iref[0][1], what)))
        assert np.array_equal(TD.bits(got[1]), TD.bits(got[0])), what + ": idwt_level is not idwt at one level"

    total2 = E.dwt_layout(2 * n, L, mode, levels)[2]
    def idwt(v, n_):
        k = E.dwt_layout(n_, L, mode, levels)[0][1]
        return E.idwt(v[0], n_, rl, rh, mode, levels), E.idwt_level(v[0][..., :k], v[0][..., k:], n_, rl, rh, mode)

    out.append(HCase("idwt-db4-n37", "idwt", [coef], lambda v: idwt(v, n), idwt_accept, lambda: ([(4, total2)], lambda v: idwt(v, 2 * n))))
    out[-1].ref = lambda: R.waverec([coef[..., o:o + ln].astype(np.float64) for ln, o in entries], n, rl, rh, mode, bounds=[np.zeros(1)] * (levels + 1))[0]

    mx = R.signal(n, 2, False, seed=5)
    mx.setflags(write=False)
    mref = []

    def modwt_accept(got, what):
        if not mref:
            mref.append(R.modwt(mx.astype(np.float64), rl, rh, 1, B=0.0))
        print("%s: %.3g of the tolerance" % (what, TD.held(np.asarray(got), mref[0][0], mref[0][1], what)))

    out.append(HCase("modwt-db4-n37", "modwt", [mx], lambda v: E.modwt(v[0], rl, rh, 1), modwt_accept,
                     lambda: ([(4, 2 * n)], lambda v: E.modwt(v[0], rl, rh, 2))))
    out[-1].ref = lambda: R.modwt(mx.astype(np.float64), rl, rh, 1, B=0.0)[0]

    W = R.signal(n, 4, False, seed=9).reshape(2, 2, n)
    W.setflags(write=False)
    wref = []

    def imodwt_accept(got, what):
        if not wref:
            wref.append(R.imodwt(W.astype(np.float64), rl, rh, B=0.0))
        print("%s: %.3g of the tolerance" % (what, TD.held(np.asarray(got), wref[0][0], wref[0][1], what)))

    out.append(HCase("imodwt-db4-n37", "imodwt", [W], lambda v: E.imodwt(v[0], rl, rh), imodwt_accept,
                     lambda: ([(3, 4, 2 * n)], lambda v: E.imodwt(v[0], rl, rh))))
    out[-1].ref = lambda: R.imodwt(W.astype(np.float64), rl, rh, B=0.0)[0]
    return out


def _export_case():
    """welch_export + welch_apply (the one-collective form of the sharded Welch PSD) at nfft 1024, hop 512, 9 frames, against the
    oracle with the tolerance of every Welch test (rtol 2e-4, atol 1e-6 of the largest bin: tests/test_gpu_dist.py)"""
    E = _engine()
    nfft, hop, M = 1024, 512, 9
    n = (M - 1) * hop + nfft
    x = G.noise(n, True, 5150, 0.6)
    x.setflags(write=False)
    ref = []

    def run(v, frames):
        from oracle import cpu_ref as O
        win = O.windows("Hanning", nwins=nfft)
        st = E.welch_export(v[0], win, hop, frames)
        return st, E.welch_apply(st, win, frames, sided=E.SIDED_TWO, scale=1.0 / float(np.sum(win ** 2)))

    def accept(got, what):
        from oracle import cpu_ref as O
        if not ref:
            ref.append(O.welch_psd_stream(x, O.windows("Hanning", nwins=nfft), nfft, hop, M, 1.0, detrend_style=1))
        p = np.asarray(got[1])
        r = float(np.max(np.abs(p - ref[0]) / (2e-4 * np.abs(ref[0]) + 1e-6 * ref[0].max())))
        print("%s: %.3g of the tolerance" % (what, r))
        assert p.shape == ref[0].shape and r <= 1.0, (what, r)

    def reference():
        from oracle import cpu_ref as O
        return O.welch_psd_stream(x, O.windows("Hanning", nwins=nfft), nfft, hop, M, 1.0, detrend_style=1)

    return HCase("welch_export-c64-1024x512", "welch_export", [x], lambda v: run(v, M), accept, lambda: ([(2 * n + hop,)], lambda v: run(v, 2 * M)),
                 ref=reference)


def _csd_epilogue_case():
    """csd_epilogue on two-sided spectra of 512 bins, three channels: the smallest shape of tests/test_gpu_kernels.py:
    test_csd_epilogue_on_device, whose assertions are restated here one for one (rtol 1e-12 on the element-wise outputs, 2e-6 of the
    largest correlation, 1e-5 on the energies and the correlation coefficient).  Its 'samples' are the averaged spectra."""
    E = _engine()
    nfft, nch, enbw = 512, 3, 3.7
    rng = np.random.default_rng(nfft)
    pxx = 1.0 + rng.random(nfft)
    pyy = 0.5 + rng.random((nch, nfft))
    pxy = (rng.standard_normal((nch, nfft)) + 1j * rng.standard_normal((nch, nfft))) * 0.4
    for a in (pxx, pyy, pxy):
        a.setflags(write=False)

    def back(P):
        return np.sqrt(nfft) * np.fft.ifft(np.fft.ifftshift(np.array(P, dtype=np.complex128), axes=-1), n=nfft, axis=-1)

    def reference():
        den = np.abs(pxx)[None, :] * np.abs(pyy)
        Rxx, Ryy, Rxy = back(pxx), back(pyy), back(pxy)
        Ex, Ey = Rxx[0], Ryy[:, 0]
        sh = lambda R: np.fft.fftshift(R, axes=-1)                       # noqa: E731
        return dict(Cxy=pxy / np.sqrt(den), Cxy2=np.abs(pxy) ** 2 / den, phi=np.angle(pxy), Lxx=np.sqrt(enbw * pxx),
                    Lxy=np.sqrt(enbw * np.abs(pxy)), Rxx=sh(Rxx), Ryy=sh(Ryy), Rxy=sh(Rxy), iCxy=sh(back(pxy / np.sqrt(den))), Ex=Ex, Ey=Ey,
                    corrcoef=sh(Rxy) / np.sqrt(Ex * Ey)[:, None])

    def run(v):
        return E.csd_epilogue(v[0], v[1], v[2], int(v[0].shape[-1]), False, enbw)

    def accept(got, what):
        g, r = {k: np.asarray(v) for k, v in got.items()}, reference()
        fr = {}
        for k in ("Cxy", "Cxy2", "phi", "Lxx", "Lxy"):
            fr[k] = float(np.max(np.abs(g[k] - r[k]) / (1e-12 * np.abs(r[k]))))
        sc = np.abs(r["Rxx"]).max()
        for k in ("Rxx", "Ryy", "Rxy", "iCxy"):
            fr[k] = float(np.max(np.abs(g[k] - r[k]))) / (2e-6 * max(sc, np.abs(r[k]).max()))
        for k in ("Ex", "Ey"):
            fr[k] = float(np.max(np.abs(g[k] - r[k]) / (1e-5 * np.abs(r[k]))))
        fr["corrcoef"] = float(np.max(np.abs(g["corrcoef"] - r["corrcoef"]))) / (1e-5 * np.abs(r["corrcoef"]).max())
        worst = max(fr, key=fr.get)
        print("%s: %.3g of the tolerance (%s)" % (what, fr[worst], worst))
        assert fr[worst] <= 1.0, (what, fr)

    return HCase("csd_epilogue-twosided-3x512", "csd_epilogue", [pxx, pyy, pxy], run, accept,
                 lambda: ([(2 * nfft,), (2 * nch, 2 * nfft), (2 * nch, 2 * nfft)], run), ref=reference)


def _derived_cases():
    """channel_means (tests/test_gpu_dist.py: test_channel_means_and_given_means, rtol 1e-6, atol 1e-7), ssq_sum (tests/test_gpu_ssq.py:
    test_band_sums_against_reference, 'a plain sum of the T it is given': 1e-5 of the band's sum of |T|) and wct_scale
    (tests/test_gpu_wct.py: check of wct_ref at twice the restatement's loss, on the float32 restatement's T)"""
    E = _engine()
    out = []
    x = (G.noise(7 * 5000, False, 9100).reshape(7, 5000) + np.arange(7, dtype=np.float32)[:, None]).astype(np.float32)
    x.setflags(write=False)

    def means_accept(got, what):
        want = x.astype(np.float64).mean(axis=1)
        got = np.asarray(got)
        print("%s: %.3g of the tolerance" % (what, float(np.max(np.abs(got - want) / (1e-7 + 1e-6 * np.abs(want))))))
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7, err_msg=what)

    out.append(HCase("channel_means-7x5000", "channel_means", [x], lambda v: E.channel_means(v[0]), means_accept,
                     lambda: ([(14, 10000)], lambda v: E.channel_means(v[0]))))
    out[-1].ref = lambda: x.astype(np.float64).mean(axis=1)

    out.append(_csd_epilogue_case())

    import ssq_ref as SR
    import test_gpu_ssq as TS
    cs, _, _, c, sq = TS.case_of(2)
    n, b0, nb = cs["n"], sq["b0"], sq["nb"]
    lo = b0 + nb // 5
    m = np.array([[lo, lo + nb // 4], [lo + nb // 3, lo + nb // 2 + 7]]).astype(np.float64)
    T = np.ascontiguousarray(sq["T"]).astype(np.complex64)
    T.setflags(write=False)

    def ssum(v):
        return E.ssq_sum(v[0], n, m, b0=b0)

    def ssum_accept(got, what):
        got = np.asarray(got)
        worst = 0.0
        for b in range(2):
            j0, j1 = int(m[b, 0]) - b0, int(m[b, 1]) - b0
            plain = T[:, j0:j1].astype(np.complex128).sum(axis=1)
            tol = 1e-5 * np.sum(np.abs(T[:, j0:j1]), axis=1) + 1e-30
            worst = max(worst, float(np.max(np.abs(got[b] - plain) / tol)))
        print("%s: %.3g of the tolerance" % (what, worst))
        assert got.shape == (2, T.shape[0]) and worst <= 1.0, (what, worst)

    out.append(HCase("ssq_sum-%s" % SR.case_id(cs), "ssq_sum", [T], ssum, ssum_accept, lambda: ([(2 * T.shape[0], T.shape[1])], ssum)))
    out[-1].ref = lambda: np.stack([T[:, int(m[b, 0]) - b0:int(m[b, 1]) - b0].astype(np.complex128).sum(axis=1) for b in range(2)])

    import test_gpu_wct as TC
    import wct_ref as Q
    cx, cy, cplan, refs, loss = TC.case_of(256, False)
    T32 = np.ascontiguousarray(Q.overlap_save(cx[0], cy[0], cplan["scales"], 6.0, 256, cplan["Mw"], cplan["Mg"], np.float32)).astype(np.float32)
    T32.setflags(write=False)

    def scale(v):
        return E.wct_scale(v[0], TC.WIN, spectra=True)

    def scale_accept(got, what):
        Q.check(TC.as_dict(T32, tuple(np.asarray(g) for g in got)), refs[0], 2 * loss, what)

    out.append(HCase("wct_scale-256", "wct_scale", [T32], scale, scale_accept,
                     lambda: ([T32.shape[:-2] + (2 * T32.shape[-2], 4)], scale)))          # T is [S, N, 4]
    out[-1].ref = lambda: {k: refs[0][k] for k in ("R2", "phase") if k in refs[0]}
    return out


def _build():
    cases = _build_core() + _derived_cases()
    cases += _synthesis_cases() + [_zoom_case()] + _wavelet_cases() + _tfr_cases() + _uneven_cases() + _ar_cases() + _model_cases()
    cases += _dwt_cases() + [_export_case()]
    return tuple(cases)


# the public names of pyfft_amd.engine a case's call enters, where they are not the family's own name alone
ENTRIES = {
    "sosfiltfilt": ("sos_filtfilt",),                      # filters.sosfiltfilt -> engine.sos_filtfilt
    "lomb_sums": ("lomb_sums", "lomb_finish"),
    "welch_export": ("welch_export", "welch_apply"),
    "fft": ("fft", "ifft"),
    "dwt": ("dwt", "dwt_level"),
    "idwt": ("idwt", "idwt_level"),
}

# public names of the engine that are not cases: no samples go through them, or another test of tests/test_gpu_call_history.py holds them
EXCLUDED = {
    "nbins": "host arithmetic: the number of bins of a sidedness",
    "max_wg_fft": "a constant of the build",
    "last_passes": "reads a counter of the last call",
    "profile_enable": "a switch of the profiler, no samples",
    "profile_last_ms": "reads the profiler",
    "profile_last_kernel": "reads the profiler",
    "check": "the error check of the ctypes layer (re-exported from _ffi)",
    "lib": "the ctypes handle (re-exported from _ffi)",
    "ptr": "an address helper (re-exported from _ffi)",
    "comm_unique_id": "RCCL plumbing: needs a communicator, held by tests/test_gpu_rccl.py",
    "comm_init": "RCCL plumbing",
    "comm_info": "RCCL plumbing",
    "comm_destroy": "RCCL plumbing",
    "welch_accum": "held by test_pending_accumulate_survives_other_families (its result is the pending state)",
    "welch_finish": "held by test_pending_accumulate_survives_other_families",
    "welch_dist_submit": "held by test_streamed_step_ignores_its_neighbours; its refusals are the `refused` history of the pipeline case",
    "welch_dist_flush": "held by test_streamed_step_ignores_its_neighbours",
    "ddc_tile": "host arithmetic (a size helper)",
    "upfirdn_tile": "host arithmetic (a size helper)",
    "pfb_synth_plan": "a plan: host arithmetic",
    "welch_blocks_check": "a check: raises before the library",
    "welch_blocks_plan": "a plan: host arithmetic",
    "cwt_check": "a check: raises before the library",
    "cwt_plan": "a plan: host arithmetic",
    "wct_check": "a check: raises before the library",
    "wct_taps": "a check of a tap table on the host",
    "wct_plan": "a plan: host arithmetic",
    "ssq_lds_bytes": "host arithmetic (a size helper)",
    "ssq_check": "a check: raises before the library",
    "ssq_band_check": "a check: raises before the library",
    "ssq_windows": "window tables on the host",
    "ssq_plan": "a plan: host arithmetic",
    "wvd_lds_bytes": "host arithmetic (a size helper)",
    "wvd_check": "a check: raises before the library",
    "wvd_plan": "a plan: host arithmetic",
    "cyclic_check": "a check: raises before the library",
    "cyclic_plan": "a plan: host arithmetic",
    "lomb_check": "a check: raises before the library",
    "lomb_plan": "a plan: host arithmetic",
    "nufft_check": "a check: raises before the library",
    "nufft_plan": "a plan: host arithmetic",
    "nufft2_plan": "a plan: host arithmetic",
    "wbic_check": "a check: raises before the library",
    "wbic_plan": "a plan: host arithmetic",
    "fam_check": "a check: raises before the library",
    "fam_plan": "a plan: host arithmetic",
    "ar_check": "a check: raises before the library",
    "ar_plan": "a plan: host arithmetic",
    "sub_check": "a check: raises before the library",
    "sub_plan": "a plan: host arithmetic",
    "beam_check": "a check: raises before the library",
    "beam_plan": "a plan: host arithmetic",
    "dwt_coeff_len": "host arithmetic (a size helper)",
    "dwt_max_levels": "host arithmetic (a size helper)",
    "dwt_check": "a check: raises before the library",
    "dwt_layout": "host arithmetic (a size helper)",
    "dwt_plan": "a plan: host arithmetic",
    "sos_array": "host: the section table as the library takes it",
}
# public names whose case is still to be written: none.  tests/test_host_history_ref.py fails when a name of the engine is in none of
# the three tables, so a family added later cannot skip the history tests silently.
PENDING = {}

CASES = _build()
BY_ID = collections.OrderedDict((c.id, c) for c in CASES)
assert len(BY_ID) == len(CASES)


def entries_of(case):
    return ENTRIES.get(case.family, (case.family,))
