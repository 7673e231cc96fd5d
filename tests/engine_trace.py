"""What pyfft_amd.engine hands to the C ABI, recorded without a GPU: a stand-in for libspectral.so that logs every call, and a table
of calls that drives each entry point of the engine in both calling modes (numpy arrays; torch tensors, here on the CPU) through every
branch that changes what reaches the library or what comes back.  tests/golden/make_golden_engine_trace.py wrote the trace of this
table once; tests/test_host_engine_trace.py replays it.  A plain module: nothing here is collected by pytest.

One argument of a recorded call becomes: an int or a float as it is; None (or a null pointer) null; a c_void_p ["in", k, byte offset]
when it points into the k-th array the case made, ["out", k, byte offset] when it points into the k-th array the call returned (looked
up after the call), "tmp" otherwise (the engine's own copies, windows, taps); any other ctypes object the name of its type."""
import ctypes

import numpy as np

from pyfft_amd import _ffi, engine

try:
    import torch
except Exception:                       # pragma: no cover
    torch = None

# entries whose result the engine reads: answered by the built library, which needs no GPU for them; not recorded
HOST_ARITHMETIC = ("sp_xcorr_frames_len", "sp_csd_epilogue_doubles", "sp_ddc_tile", "sp_upfirdn_tile", "sp_pfb_synth_plan", "sp_skf_plan",
                   "sp_welch_blocks_plan", "sp_cwt_plan", "sp_eigh_plan", "sp_version", "sp_max_wg_fft", "sp_wct_plan", "sp_ssq_plan",
                   "sp_wvd_plan", "sp_cyclic_plan", "sp_lomb_plan", "sp_last_passes", "sp_ar_plan", "sp_sub_plan", "sp_beamscan_plan")
REFUSAL_TYPES = (ValueError, TypeError, NotImplementedError)
MODES = ("host", "dev")

_INTS, _FLOATS = (int, np.integer), (float, np.floating)
# the signature tables whose entries the case table drives: the six of _ffi.TABLES, then one more for every family traced since
TRACED_TABLES = _ffi.TABLES + (_ffi.AR_SIGNATURES, _ffi.SUB_SIGNATURES, _ffi.ARRAY_SIGNATURES)
DECLARED = {name: sig for table in TRACED_TABLES for name, sig in table.items()}     # every entry of the traced tables


class StandIn:
    """Looks like the loaded library to the engine: every declared name is callable, checks its arguments the way ctypes would (their
    number; no float where an integer is declared) and logs them."""

    def __init__(self, events):
        self._events = events
        self._real = None

    def _delegate(self, name):
        if self._real is None:
            self._real = ctypes.CDLL(_ffi.LIB_PATH)
        fn = getattr(self._real, name)
        fn.restype, fn.argtypes = DECLARED[name]
        return fn

    def __getattr__(self, name):
        if name not in DECLARED:
            raise AttributeError(name)
        if name in HOST_ARITHMETIC:
            return self._delegate(name)
        argtypes = DECLARED[name][1]

        def record(*args):
            if len(args) != len(argtypes):
                raise TypeError("%s takes %d arguments, got %d" % (name, len(argtypes), len(args)))
            for k, (a, t) in enumerate(zip(args, argtypes)):
                if t in (ctypes.c_int, ctypes.c_int64) and not isinstance(a, _INTS):
                    raise TypeError("%s: argument %d must be an integer, got %r" % (name, k, a))
                if t is ctypes.c_double and not isinstance(a, _INTS + _FLOATS):
                    raise TypeError("%s: argument %d must be a number, got %r" % (name, k, a))
            self._events.append((name, args))
            return 0
        return record


def install(monkeypatch, events):
    """engine.lib / _ffi.lib -> a stand-in, _ffi.init and engine._bind_stream -> recorders, all logging into `events`."""
    standin = StandIn(events)
    monkeypatch.setattr(engine, "lib", lambda: standin)
    monkeypatch.setattr(_ffi, "lib", lambda: standin)
    monkeypatch.setattr(_ffi, "init", lambda device=-1: events.append(("init", device)))
    monkeypatch.setattr(engine, "_bind_stream", lambda x: events.append(("bind",)))
    return standin


def _is_tensor(a):
    return torch is not None and isinstance(a, torch.Tensor)


def _span(a):
    """(first byte, one past the last byte) of the memory an array's elements lie in"""
    if _is_tensor(a):
        if a.numel() == 0:
            return 0, 0
        reach = 1 + sum((int(d) - 1) * int(s) for d, s in zip(a.shape, a.stride()))
        return int(a.data_ptr()), int(a.data_ptr()) + reach * a.element_size()
    if a.size == 0:
        return 0, 0
    reach = a.itemsize + sum((d - 1) * abs(s) for d, s in zip(a.shape, a.strides))
    return int(a.ctypes.data), int(a.ctypes.data) + reach


def _arrays_of(result, found):
    """the arrays a call returned, in order, through tuples, lists, dicts and Nones"""
    if isinstance(result, (tuple, list)):
        for v in result:
            _arrays_of(v, found)
    elif isinstance(result, dict):
        for k in sorted(result):
            _arrays_of(result[k], found)
    elif isinstance(result, np.ndarray) or _is_tensor(result):
        found.append(result)
    return found


def _describe(result):
    if result is None:
        return None
    if isinstance(result, (tuple, list)):
        return [_describe(v) for v in result]
    if isinstance(result, dict):
        return {k: _describe(result[k]) for k in sorted(result)}
    if _is_tensor(result):
        return {"kind": "torch", "dtype": str(result.dtype).replace("torch.", ""), "shape": [int(d) for d in result.shape],
                "contiguous": bool(result.is_contiguous())}
    if isinstance(result, np.ndarray):
        return {"kind": "numpy", "dtype": str(result.dtype), "shape": [int(d) for d in result.shape],
                "contiguous": bool(result.flags["C_CONTIGUOUS"])}
    if isinstance(result, np.generic):               # an element of an output: under the stand-in its value is uninitialised memory
        return {"kind": "numpy scalar", "dtype": str(result.dtype)}
    if isinstance(result, complex):
        return {"kind": "complex", "value": [result.real, result.imag]}
    if isinstance(result, (bool, int, float, str)):
        return {"kind": type(result).__name__, "value": result}
    raise TypeError("a result the trace does not describe: %r" % (result,))


def _normalise(arg, ins, outs):
    if arg is None:
        return None
    if isinstance(arg, _INTS):
        return int(arg)
    if isinstance(arg, _FLOATS):
        return float(arg)
    if isinstance(arg, ctypes.c_void_p):
        if not arg.value:
            return None
        for tag, arrays in (("in", ins), ("out", outs)):
            for k, a in enumerate(arrays):
                lo, hi = _span(a)
                if lo <= arg.value < hi:
                    return [tag, k, arg.value - lo]
        return "tmp"
    return type(arg).__name__


class Arrays:
    """Makes the arrays of one case in the mode under test (numpy, or torch tensors on the CPU) and keeps them, in order, as the
    candidates an "in" pointer is resolved against.  Views are taken by the case from what this returns, so they resolve to their base."""

    def __init__(self, mode):
        self.dev = mode == "dev"
        self.made = []

    def __call__(self, shape, dtype="float32", host=False):
        size = int(np.prod(shape))
        v = (np.arange(size) % 7 - 3.0) / 4.0 + 0.125
        if np.dtype(dtype).kind == "c":
            v = v + 1j * ((np.arange(size) % 5 - 2.0) / 4.0)
        a = np.ascontiguousarray(v.reshape(shape).astype(dtype))
        if self.dev and not host:
            a = torch.from_numpy(a)
        self.made.append(a)
        return a


def run_case(monkeypatch, case, mode):
    """One call of the table under the stand-in -> what is kept of it (JSON-able)."""
    name, fn, build = case
    events = []
    with monkeypatch.context() as mp:
        install(mp, events)
        A = Arrays(mode)
        args, kwargs = build(A)
        kept = {}
        result = None
        try:
            result = getattr(engine, fn)(*args, **kwargs)
            kept["returned"] = _describe(result)
        except REFUSAL_TYPES as e:
            kept["refused"] = {"message": str(e), "types": [t.__name__ for t in REFUSAL_TYPES if isinstance(e, t)]}
        outs = _arrays_of(result, [])
        kept["events"] = [[ev[0]] + [_normalise(a, A.made, outs) for a in (ev[1] if ev[0].startswith("sp_") else ev[1:])]
                          for ev in events]
    return kept


def run_table(monkeypatch, only=None):
    """{case id: what was kept} over the table, both modes; case id = function/name/mode"""
    out = {}
    for case in CASES:
        for mode in MODES:
            key = "%s/%s/%s" % (case[1], case[0], mode)
            if only is None or key in only:
                out[key] = run_case(monkeypatch, case, mode)
    return out


# ------------------------------------------------------------------------------------------ the table
N, NFFT, HOP, NFR = 512, 64, 32, 15           # a record, and frames of it: (NFR - 1) * HOP + NFFT = N
WIN = np.hanning(NFFT)                        # float64: the engine's float32 copy of it is a "tmp"
WIN32 = np.hanning(32)
TAPS = np.hanning(9) / 4.0
SOS = np.array([[0.2, 0.1, 0.2, 1.0, -0.5, 0.25], [0.3, 0.0, -0.3, 1.0, 0.1, 0.5]])
CASES = []


def case(fn, name, build):
    CASES.append((name, fn, build))


def K(*args, **kwargs):
    return args, kwargs


F32, C64, F64, C128 = "float32", "complex64", "float64", "complex128"

# -- fft, mean
case("fft", "c64-rows", lambda A: K(A((4, NFFT), C64)))
case("fft", "f32-cast", lambda A: K(A((4, NFFT), F32)))
case("fft", "inverse", lambda A: K(A((NFFT,), C64), inverse=True))
case("fft", "axis0", lambda A: K(A((NFFT, 3), C64), axis=0))
case("fft", "n-longer", lambda A: K(A((2, 48), C64), n=64))
case("fft", "n-shorter", lambda A: K(A((2, 48), C64), n=32))
for dt in (F32, C64, F64):
    case("mean", dt, lambda A, dt=dt: K(A((N,), dt)))

# -- Welch PSD and its sharded halves
for dt in (F32, C64, F64):
    case("welch_psd", dt, lambda A, dt=dt: K(A((N,), dt), WIN, HOP, NFR))
case("welch_psd", "strided", lambda A: K(A((2 * N,), C64)[::2], WIN, HOP, NFR))
case("welch_psd", "mean-value", lambda A: K(A((N,), C64), WIN, HOP, NFR, mean_value=0.25 - 0.5j, scale=0.5))
case("welch_psd", "no-detrend-one", lambda A: K(A((N,), F32), WIN, HOP, NFR, detrend=False, sided=engine.SIDED_ONE))
case("welch_psd", "linear-half", lambda A: K(A((N,), F32), WIN, HOP, NFR, detrend="linear", sided=engine.SIDED_HALF))
case("welch_psd", "segmean", lambda A: K(A((N,), F32), WIN, HOP, NFR, detrend=3))
case("welch_psd", "seglinear", lambda A: K(A((N,), F32), WIN, HOP, NFR, detrend="seglinear"))
for fn in ("welch_accum", "welch_export"):
    case(fn, "c64", lambda A: K(A((N,), C64), WIN, HOP, NFR))
    case(fn, "f32-nmean", lambda A: K(A((N,), F32), WIN, HOP, NFR - 2, nmean=400))
    case(fn, "f64", lambda A: K(A((N,), F64), WIN, HOP, NFR))
case("welch_apply", "f64", lambda A: K(A((5 * NFFT + 8,), F64), WIN, 30))
case("welch_apply", "f32-one", lambda A: K(A((5 * NFFT + 8,), F32), WIN, 30, sided=engine.SIDED_ONE, scale=2.0))
case("welch_finish", "own-mean", lambda A: K(NFFT, None, 30, like=A((1,), F32)))
case("welch_finish", "mean-f64", lambda A: K(NFFT, A((2,), F64), 30, sided=engine.SIDED_ONE, scale=2.0))
case("welch_finish", "mean-f32", lambda A: K(NFFT, A((2,), F32), 30))

# -- cross spectra
case("welch_csd", "f32-3ch", lambda A: K(A((N,), F32), A((3, N), F32), WIN, HOP, NFR))
case("welch_csd", "y-1d", lambda A: K(A((N,), F32), A((N,), F32), WIN, HOP, NFR, detrend=False, sided=engine.SIDED_TWO, scale=0.5))
case("welch_csd", "c64", lambda A: K(A((N,), C64), A((2, N), C64), WIN, HOP, NFR, detrend="linear"))
case("welch_csd", "y-rows-longer", lambda A: K(A((N,), F32), A((2, N + 5), F32), WIN, HOP, NFR))
case("welch_csd", "real-x-complex-y", lambda A: K(A((N,), F32), A((2, N), C64), WIN, HOP, NFR))
case("welch_csd", "f64", lambda A: K(A((N,), F64), A((2, N), F64), WIN, HOP, NFR))
case("welch_csd", "y-f64", lambda A: K(A((N,), F32), A((2, N), F64), WIN, HOP, NFR))
case("welch_csd", "host-y", lambda A: K(A((N,), F32), A((2, N), F32, host=True), WIN, HOP, NFR))
case("welch_csd", "y-short", lambda A: K(A((N,), F32), A((2, N - 1), F32), WIN, HOP, NFR))
case("welch_csd", "x-2d", lambda A: K(A((1, N), F32), A((2, N), F32), WIN, HOP, NFR))
case("csd_matrix", "plain", lambda A: K(A((3, N), F32), WIN, HOP, NFR))
case("csd_matrix", "no-detrend", lambda A: K(A((3, N), F32), WIN, HOP, NFR, detrend=False, scale=0.5))
case("csd_matrix", "means", lambda A: K(A((3, N), F32), WIN, HOP, NFR, means=A((3,), F64)))
case("csd_matrix", "means-list", lambda A: K(A((3, N), F32), WIN, HOP, NFR, means=[0.5, 0.25, 0.0]))
case("csd_matrix", "means-wrong", lambda A: K(A((3, N), F32), WIN, HOP, NFR, means=A((2,), F64)))
case("csd_matrix", "f64", lambda A: K(A((3, N), F64), WIN, HOP, NFR))
case("csd_matrix", "transposed", lambda A: K(A((N, 3), F32).T, WIN, HOP, NFR))
case("channel_means", "plain", lambda A: K(A((3, N), F32)))
case("channel_means", "nsamples", lambda A: K(A((3, N), F32), nsamples=400))
case("channel_means", "f64", lambda A: K(A((3, N), F64)))

# -- STFT and its inverse
for dt in (F32, C64, F64):
    case("stft_frames", dt, lambda A, dt=dt: K(A((N,), dt), WIN, HOP, NFR))
case("stft_frames", "power", lambda A: K(A((N,), F32), WIN, HOP, NFR, power=True, amp_scale=0.5))
case("stft_frames", "bin-major", lambda A: K(A((N,), C64), WIN, HOP, NFR, bin_major=True, sided=engine.SIDED_TWO))
case("stft_frames", "pseg", lambda A: K(A((N,), F32), WIN, HOP, NFR, want_pseg=True))
case("stft_frames", "power-bin-major-pseg", lambda A: K(A((N,), C64), WIN, HOP, NFR, power=True, bin_major=True, want_pseg=True,
                                                          sided=engine.SIDED_RAW))
case("stft_frames", "mean-value", lambda A: K(A((N,), C64), WIN, HOP, NFR, mean_value=0.5 + 0.25j))
case("stft_frames", "segmean", lambda A: K(A((N,), F32), WIN, HOP, NFR, detrend="segmean"))
case("istft_frames", "half", lambda A: K(A((NFR, NFFT // 2 + 1), C64), WIN, HOP))
case("istft_frames", "raw-lead", lambda A: K(A((2, NFR, NFFT), C64), WIN, HOP, sided=engine.SIDED_RAW))
case("istft_frames", "bin-major", lambda A: K(A((NFFT // 2 + 1, NFR), C64), WIN, HOP, bin_major=True))
case("istft_frames", "skip-nout-scale", lambda A: K(A((NFR, NFFT // 2 + 1), C64), WIN, HOP, scale=2.0, skip=16, nout=300))
case("istft_frames", "c128", lambda A: K(A((NFR, NFFT // 2 + 1), C128), WIN, HOP))
case("istft_frames", "transposed", lambda A: K(A((NFFT // 2 + 1, NFR), C64).T, WIN, HOP))
case("istft_frames", "sided-refused", lambda A: K(A((NFR, NFFT), C64), WIN, HOP, sided=engine.SIDED_TWO))
case("istft_frames", "1d-refused", lambda A: K(A((NFFT,), C64), WIN, HOP))
case("istft_frames", "bins-refused", lambda A: K(A((NFR, NFFT), C64), WIN, HOP))

# -- bispectrum, multitaper
case("bispectrum", "auto", lambda A: K(A((N,), F32), WIN, HOP, NFR))
case("bispectrum", "y-z", lambda A: K(A((N,), F32), WIN, HOP, NFR, y=A((N,), F32), z=A((N,), F32)))
case("bispectrum", "y-only-c64", lambda A: K(A((N,), C64), WIN, HOP, NFR, y=A((N,), C64), detrend="linear"))
case("bispectrum", "z-only-mean-value", lambda A: K(A((N,), F32), WIN, HOP, NFR, z=A((N,), F32), mean_value=0.5))
case("bispectrum", "y-short", lambda A: K(A((N,), F32), WIN, HOP, NFR, y=A((N - 1,), F32)))
case("bispectrum", "y-other-dtype", lambda A: K(A((N,), F32), WIN, HOP, NFR, y=A((N,), C64)))
case("bispectrum", "segmean-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, detrend="segmean"))
case("bispectrum", "f64", lambda A: K(A((N,), F64), WIN, HOP, NFR, y=A((N,), F64)))
TAPERS = np.stack([np.hanning(NFFT), np.hamming(NFFT), np.blackman(NFFT)])
case("multitaper", "plain", lambda A: K(A((N,), F32), TAPERS, HOP, NFR))
case("multitaper", "y", lambda A: K(A((N,), F32), TAPERS, HOP, NFR, y=A((N,), F32), scale=0.5))
case("multitaper", "weights", lambda A: K(A((N,), F32), TAPERS, HOP, NFR, weights=[1.0, 0.5, 0.25]))
case("multitaper", "y-weights-c64", lambda A: K(A((N,), C64), TAPERS, HOP, NFR, y=A((N,), C64), weights=[1.0, 0.5, 0.25],
                                                 detrend="linear"))
case("multitaper", "mean-value", lambda A: K(A((N,), C64), TAPERS, HOP, NFR, mean_value=0.5 - 0.25j))
case("multitaper", "y-short", lambda A: K(A((N,), F32), TAPERS, HOP, NFR, y=A((N - 1,), F32)))
case("multitaper", "tapers-1d-refused", lambda A: K(A((N,), F32), TAPERS[0], HOP, NFR))
case("multitaper", "weights-refused", lambda A: K(A((N,), F32), TAPERS, HOP, NFR, weights=[1.0, 0.5]))
case("multitaper", "segmean-refused", lambda A: K(A((N,), F32), TAPERS, HOP, NFR, detrend="segmean"))
case("multitaper", "f64", lambda A: K(A((N,), F64), TAPERS, HOP, NFR, y=A((N,), F64)))

# -- chirp-z, zoom
RN = 200                                       # a row; the strided views keep RN of RN + 3
case("czt", "1d", lambda A: K(A((RN,), F32), 50, 0.1, 0.001))
case("czt", "rows-c64", lambda A: K(A((3, RN), C64), 50, 0.1, 0.001))
case("czt", "strided-rows", lambda A: K(A((3, RN + 3), C64)[:, :RN], 50, 0.1, 0.001))
case("czt", "strided-rows-offset", lambda A: K(A((3, RN + 3), F32)[1:, 2:RN + 2], 50, 0.1, 0.001))
case("czt", "3d", lambda A: K(A((2, 2, RN), F32), 50, 0.1, 0.001))
case("czt", "3d-strided", lambda A: K(A((2, 2, RN + 3), F32)[..., :RN], 50, 0.1, 0.001))
case("czt", "transposed", lambda A: K(A((RN, 3), F32).T, 50, 0.1, 0.001))
case("czt", "f64", lambda A: K(A((RN,), F64), 50, 0.1, 0.001))
case("czt", "0d", lambda A: K(A((), F32), 50, 0.1, 0.001))
case("zoom_welch", "plain", lambda A: K(A((N,), F32), WIN, HOP, NFR, 40, 0.1, 0.001))
case("zoom_welch", "y-c64", lambda A: K(A((N,), C64), WIN, HOP, NFR, 40, 0.1, 0.001, y=A((N,), C64), detrend="linear", scale=0.5))
case("zoom_welch", "frames", lambda A: K(A((N,), F32), WIN, HOP, NFR, 40, 0.1, 0.001, frames=True))
case("zoom_welch", "mean-value", lambda A: K(A((N,), C64), WIN, HOP, NFR, 40, 0.1, 0.001, detrend=True, mean_value=0.5 + 1j))
case("zoom_welch", "frames-y-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, 40, 0.1, 0.001, y=A((N,), F32), frames=True))
case("zoom_welch", "segmean-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, 40, 0.1, 0.001, detrend="segmean"))
case("zoom_welch", "y-short", lambda A: K(A((N,), F32), WIN, HOP, NFR, 40, 0.1, 0.001, y=A((N - 1,), F32)))
case("zoom_welch", "f64", lambda A: K(A((N,), F64), WIN, HOP, NFR, 40, 0.1, 0.001))

# -- down-converter, resampler, filter banks
case("ddc", "1d", lambda A: K(A((RN,), F32), 0.1, 4, TAPS))
case("ddc", "rows-c64-n0", lambda A: K(A((3, RN), C64), 0.1, 3, TAPS, n0=17))
case("ddc", "strided-rows", lambda A: K(A((3, RN + 3), C64)[:, :RN], 0.1, 4, TAPS))
case("ddc", "3d", lambda A: K(A((2, 2, RN), F32), 0.1, 4, TAPS))
case("ddc", "transposed", lambda A: K(A((RN, 3), F32).T, 0.1, 4, TAPS))
case("ddc", "f64", lambda A: K(A((RN,), F64), 0.1, 4, TAPS))
case("ddc", "complex-taps-refused", lambda A: K(A((RN,), F32), 0.1, 4, TAPS + 0j))
case("ddc", "taps-2d-refused", lambda A: K(A((RN,), F32), 0.1, 4, TAPS[None, :]))
case("ddc", "q-refused", lambda A: K(A((RN,), F32), 0.1, 65, TAPS))
case("ddc", "0d", lambda A: K(A((), F32), 0.1, 4, TAPS))
case("upfirdn", "1d", lambda A: K(A((RN,), F32), TAPS, 3, 2))
case("upfirdn", "rows-c64-window", lambda A: K(A((3, RN), C64), TAPS, 3, 2, m0=5, nout=100))
case("upfirdn", "strided-rows", lambda A: K(A((3, RN + 3), F32)[:, :RN], TAPS, 3, 2))
case("upfirdn", "3d", lambda A: K(A((2, 2, RN), F32), TAPS, 2, 3))
case("upfirdn", "transposed", lambda A: K(A((RN, 3), F32).T, TAPS, 3, 2))
case("upfirdn", "f64", lambda A: K(A((RN,), F64), TAPS, 3, 2))
case("upfirdn", "up-refused", lambda A: K(A((RN,), F32), TAPS, 0, 2))
case("upfirdn", "taps-empty-refused", lambda A: K(A((RN,), F32), TAPS[:0], 3, 2))
case("upfirdn", "m0-refused", lambda A: K(A((RN,), F32), TAPS, 3, 2, m0=-1))
case("upfirdn", "0d", lambda A: K(A((), F32), TAPS, 3, 2))
PM, PTAPS = 16, np.hanning(64)
case("pfb", "c64", lambda A: K(A((RN,), C64), PTAPS, PM, 8, 0, 10))
case("pfb", "f32-major1-phase", lambda A: K(A((3, RN), F32), PTAPS, PM, 8, -3, 10, phase_ref=1, r0=5, out_major=1))
case("pfb", "power", lambda A: K(A((3, RN), C64), PTAPS, PM, 8, 0, 10, power=True, scale=0.5))
case("pfb", "strided-rows", lambda A: K(A((3, RN + 3), C64)[:, :RN], PTAPS, PM, 8, 0, 10))
case("pfb", "3d", lambda A: K(A((2, 2, RN), F32), PTAPS, PM, 8, 0, 10))
case("pfb", "transposed", lambda A: K(A((RN, 3), F32).T, PTAPS, PM, 8, 0, 10))
case("pfb", "f64", lambda A: K(A((RN,), F64), PTAPS, PM, 8, 0, 10))
case("pfb", "M-refused", lambda A: K(A((RN,), F32), PTAPS, 1, 8, 0, 10))
case("pfb", "complex-taps-refused", lambda A: K(A((RN,), F32), PTAPS + 0j, PM, 8, 0, 10))
case("pfb", "0d", lambda A: K(A((), F32), PTAPS, PM, 8, 0, 10))
case("pfb_synth", "onesided", lambda A: K(A((10, PM // 2 + 1), C64), PTAPS, PM, 8, 0, 128))
case("pfb_synth", "full-lead-phase", lambda A: K(A((2, 10, PM), C64), PTAPS, PM, 8, -3, 128, phase_ref=1, r0=5, onesided=False,
                                                  scale=0.5))
case("pfb_synth", "in-major1", lambda A: K(A((PM // 2 + 1, 10), C64), PTAPS, PM, 8, 0, 128, in_major=1))
case("pfb_synth", "transposed", lambda A: K(A((PM // 2 + 1, 10), C64).T, PTAPS, PM, 8, 0, 128))
case("pfb_synth", "c128", lambda A: K(A((10, PM // 2 + 1), C128), PTAPS, PM, 8, 0, 128))
case("pfb_synth", "bins-refused", lambda A: K(A((10, PM), C64), PTAPS, PM, 8, 0, 128))
case("pfb_synth", "major-refused", lambda A: K(A((10, PM // 2 + 1), C64), PTAPS, PM, 8, 0, 128, in_major=2))

# -- frame reductions
for dt in (F32, C64, F64):
    case("stft_cog", dt, lambda A, dt=dt: K(A((N,), dt), WIN, HOP, NFR, 1000.0))
case("stft_cog", "band-mean-value", lambda A: K(A((N,), C64), WIN, HOP, NFR, 1000.0, fmin=10.0, fmax=400.0, detrend=True,
                                                 mean_value=0.5j))
case("stft_cog", "segmean", lambda A: K(A((N,), F32), WIN, HOP, NFR, 1000.0, detrend="segmean"))
case("hilbert_rows", "f32", lambda A: K(A((3, 50), F32), 64))
case("hilbert_rows", "f64", lambda A: K(A((3, 50), F64), 64))
case("hilbert_rows", "transposed", lambda A: K(A((50, 3), F32).T, 64))
case("frame_sum", "f32", lambda A: K(A((3, N), F32), NFFT, HOP, NFR))
case("frame_sum", "c64-linear", lambda A: K(A((3, N), C64), NFFT, HOP, NFR, detrend="linear"))
case("frame_sum", "f64-no-detrend", lambda A: K(A((3, N), F64), NFFT, HOP, NFR, detrend=False))
case("frame_sum", "c128", lambda A: K(A((3, N), C128), NFFT, HOP, NFR))
case("frame_sum", "transposed", lambda A: K(A((N, 3), F32).T, NFFT, HOP, NFR))
case("frame_sum", "segmean-refused", lambda A: K(A((3, N), F32), NFFT, HOP, NFR, detrend="segmean"))
HTAB = np.exp(-1j * np.arange(NFFT) / 7.0)
case("spectral_filter_rows", "f32", lambda A: K(A((3, 50), F32), HTAB))
case("spectral_filter_rows", "f64", lambda A: K(A((3, 50), F64), HTAB))
case("spectral_filter_rows", "transposed", lambda A: K(A((50, 3), F32).T, HTAB))

# -- correlations, wavenumber spectra
case("xcorr_normalised", "f32", lambda A: K(A((RN,), F32), A((RN,), F32)))
case("xcorr_normalised", "f64", lambda A: K(A((RN,), F64), A((RN,), F32)))
case("xcorr_normalised", "complex-refused", lambda A: K(A((RN,), F32), A((RN,), C64)))
case("xcorr_normalised", "length-refused", lambda A: K(A((RN,), F32), A((RN - 1,), F32)))
case("xcorr_normalised", "2d-refused", lambda A: K(A((2, RN), F32), A((2, RN), F32)))
case("xcorr_normalised", "host-x2", lambda A: K(A((RN,), F32), A((RN,), F32, host=True)))
XW, XLAG = 32, 8
case("xcorr_frames", "frames", lambda A: K(A((N,), F32), A((N,), F32), XW, 16, 31, XLAG, frames=True))
case("xcorr_frames", "avg-c64", lambda A: K(A((N,), C64), A((N,), C64), XW, 16, 31, XLAG, avg=True, segmean=False, coeff=False))
case("xcorr_frames", "peak-win-beta", lambda A: K(A((N,), F32), A((N,), F32), XW, 16, 31, XLAG, win=WIN32, beta=0.01, peak=True))
case("xcorr_frames", "all-weight", lambda A: K(A((N,), F32), A((N,), F32), XW, 16, 31, XLAG, frames=True, avg=True, peak=True,
                                                weight=np.ones(int(engine.lib().sp_xcorr_frames_len(XW, XLAG)))))
case("xcorr_frames", "f64", lambda A: K(A((N,), F64), A((N,), F64), XW, 16, 31, XLAG, avg=True))
case("xcorr_frames", "nothing-asked-refused", lambda A: K(A((N,), F32), A((N,), F32), XW, 16, 31, XLAG))
case("xcorr_frames", "win-refused", lambda A: K(A((N,), F32), A((N,), F32), XW, 16, 31, XLAG, win=WIN, avg=True))
case("xcorr_frames", "weight-refused", lambda A: K(A((N,), F32), A((N,), F32), XW, 16, 31, XLAG, weight=np.ones(3), avg=True))
case("xcorr_frames", "y-short", lambda A: K(A((N,), F32), A((N - 1,), F32), XW, 16, 31, XLAG, avg=True))
case("xcorr_frames", "y-other-dtype", lambda A: K(A((N,), F32), A((N,), C64), XW, 16, 31, XLAG, avg=True))
case("xcorr_frames", "host-y", lambda A: K(A((N,), F32), A((N,), F32, host=True), XW, 16, 31, XLAG, avg=True))
case("skf", "plain", lambda A: K(A((N,), F32), A((N,), F32), NFFT, HOP, NFR, 1, 31, 16))
case("skf", "win-cross-c64", lambda A: K(A((N,), C64), A((N,), C64), NFFT, HOP, NFR, 40, 30, 17, win=WIN, segmean=False, cross=True,
                                          scale=0.5))
case("skf", "f64", lambda A: K(A((N,), F64), A((N,), F64), NFFT, HOP, NFR, 1, 31, 16))
case("skf", "win-refused", lambda A: K(A((N,), F32), A((N,), F32), NFFT, HOP, NFR, 1, 31, 16, win=WIN32))
case("skf", "y-short", lambda A: K(A((N,), F32), A((N - 1,), F32), NFFT, HOP, NFR, 1, 31, 16))
case("skf", "host-y", lambda A: K(A((N,), F32), A((N,), F32, host=True), NFFT, HOP, NFR, 1, 31, 16))

# -- time-resolved Welch spectra
case("welch_blocks", "x-only", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4))
case("welch_blocks", "y-1d-step-doubled", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4, step=2, y=A((N,), F32), doubled=True, scale=0.5))
case("welch_blocks", "y-rows-longer-c64", lambda A: K(A((N,), C64), WIN, HOP, NFR, 4, y=A((2, N + 5), C64), detrend=False))
case("welch_blocks", "boxcar", lambda A: K(A((N,), F32), None, HOP, NFR, 4, nfft=NFFT, detrend="constant"))
case("welch_blocks", "real-x-complex-y", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4, y=A((N,), C64)))
case("welch_blocks", "complex-x-real-y", lambda A: K(A((N,), C64), WIN, HOP, NFR, 4, y=A((N,), F32)))
case("welch_blocks", "f64", lambda A: K(A((N,), F64), WIN, HOP, NFR, 4, y=A((N,), F64)))
case("welch_blocks", "host-y", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4, y=A((N,), F32, host=True)))
case("welch_blocks", "nfft-refused", lambda A: K(A((N,), F32), np.hanning(48), HOP, 10, 4))
case("welch_blocks", "no-nfft-refused", lambda A: K(A((N,), F32), None, HOP, NFR, 4))
case("welch_blocks", "y-short-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4, y=A((N - 1,), F32)))
case("welch_blocks", "y-3d-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4, y=A((1, 1, N), F32)))
case("welch_blocks", "detrend-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4, detrend="linear"))
case("welch_blocks", "scale-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, 4, scale=float("inf")))

# -- wavelets
SCALES, CL, CM = [2.0, 4.0, 8.0], 256, 32
case("cwt", "W", lambda A: K(A((400,), F32), SCALES, "morlet", 6.0, CL, CM))
case("cwt", "gws-only-paul", lambda A: K(A((400,), C64), SCALES, "paul", 4.0, CL, CM, W=False, gws=True))
case("cwt", "recon-only", lambda A: K(A((2, 400), F32), SCALES, "morlet", 6.0, CL, CM, W=False, recon=[1.0, 0.5, 0.25]))
case("cwt", "bandpow-only", lambda A: K(A((2, 400), F32), SCALES, "morlet", 6.0, CL, CM, W=False, bandpow=[1.0, 0.5, 0.25]))
case("cwt", "all", lambda A: K(A((2, 2, 400), C64), SCALES, "morlet", 6.0, CL, CM, gws=True, recon=[1.0, 0.5, 0.25],
                               bandpow=[1.0, 0.5, 0.25]))
case("cwt", "strided-rows", lambda A: K(A((3, 403), C64)[:, :400], SCALES, "morlet", 6.0, CL, CM))
case("cwt", "transposed", lambda A: K(A((400, 3), F32).T, SCALES, "morlet", 6.0, CL, CM))
case("cwt", "f64", lambda A: K(A((400,), F64), SCALES, "morlet", 6.0, CL, CM))
case("cwt", "L-refused", lambda A: K(A((400,), F32), SCALES, "morlet", 6.0, 100, 10))
case("cwt", "family-refused", lambda A: K(A((400,), F32), SCALES, "dog", 2.0, CL, CM))
case("cwt", "no-output-refused", lambda A: K(A((400,), F32), SCALES, "morlet", 6.0, CL, CM, W=False))
case("cwt", "weights-refused", lambda A: K(A((400,), F32), SCALES, "morlet", 6.0, CL, CM, recon=[1.0, 0.5]))
case("cwt", "0d", lambda A: K(A((), F32), SCALES, "morlet", 6.0, CL, CM))
case("icwt_sum", "plain", lambda A: K(A((3, 400), C64), [1.0, 0.5, 0.25]))
case("icwt_sum", "lead", lambda A: K(A((2, 3, 400), C64), [1.0, 0.5, 0.25]))
case("icwt_sum", "transposed", lambda A: K(A((400, 3), C64).T, [1.0, 0.5, 0.25]))
case("icwt_sum", "c128", lambda A: K(A((3, 400), C128), [1.0, 0.5, 0.25]))
case("icwt_sum", "no-weights-refused", lambda A: K(A((3, 400), C64), None))
case("icwt_sum", "weights-wrong-refused", lambda A: K(A((3, 400), C64), [1.0, 0.5]))
case("icwt_sum", "1d-refused", lambda A: K(A((400,), C64), [1.0]))

# -- Hermitian eigensolver (check=False: under the stand-in the sweep counts are uninitialised memory)
case("eigh", "c128", lambda A: K(A((5, 5), C128), check=False))
case("eigh", "f64-batch", lambda A: K(A((2, 3, 5, 5), F64), check=False, max_sweeps=20))
case("eigh", "c64-nvec2", lambda A: K(A((2, 5, 5), C64), nvec=2, check=False))
case("eigh", "nvec0", lambda A: K(A((5, 5), C128), nvec=0, check=False))
case("eigh", "transposed", lambda A: K(A((5, 5, 2), C128).permute(2, 1, 0) if A.dev else A((5, 5, 2), C128).transpose(2, 1, 0),
                                      check=False))
case("eigh", "order-refused", lambda A: K(A((65, 65), F32), check=False))
case("eigh", "square-refused", lambda A: K(A((4, 5), F32), check=False))
case("eigh", "nvec-refused", lambda A: K(A((5, 5), F32), nvec=6, check=False))

# -- filters
case("fir_filter", "f32", lambda A: K(TAPS, A((N,), F32)))
case("fir_filter", "f64-nfft", lambda A: K(TAPS, A((N,), F64), nfft=128))
B3, A3 = [0.2, 0.1, 0.2], [1.0, -0.5, 0.25]
case("biquad_filter", "f32", lambda A: K(B3, A3, A((N,), F32)))
case("biquad_filter", "f64-short-b", lambda A: K(B3[:2], A3, A((N,), F64)))
case("biquad_filter", "complex-refused", lambda A: K(B3, A3, A((N,), C64)))
case("biquad_filter", "2d-refused", lambda A: K(B3, A3, A((2, N), F32)))
case("biquad_filter", "unstable-refused", lambda A: K(B3, [1.0, -2.5, 1.0], A((N,), F32)))
case("sos_filter", "f32", lambda A: K(SOS, A((N,), F32)))
case("sos_filter", "rows-f64", lambda A: K(SOS, A((3, N), F64)))
case("sos_filter", "c64", lambda A: K(SOS, A((2, N), C64)))
case("sos_filter", "c128", lambda A: K(SOS, A((N,), C128)))
case("sos_filter", "zi", lambda A: K(SOS, A((3, N), F32), zi=A((2, 3, 2), F64)))
case("sos_filter", "zi-real-complex-x", lambda A: K(SOS, A((N,), C64), zi=A((2, 2), F64)))
case("sos_filter", "zi-complex", lambda A: K(SOS, A((N,), C64), zi=A((2, 2), C128)))
case("sos_filter", "zi-complex-real-x", lambda A: K(SOS, A((N,), F32), zi=A((2, 2), C128)))
case("sos_filter", "zi-host", lambda A: K(SOS, A((N,), F32), zi=A((2, 2), F64, host=True)))
case("sos_filter", "zi-refused", lambda A: K(SOS, A((N,), F32), zi=A((2, 3), F64)))
case("sos_filter", "empty-refused", lambda A: K(SOS, A((0,), F32)))
case("sos_filter", "sos-refused", lambda A: K(SOS[:, :5], A((N,), F32)))
case("sos_filtfilt", "odd", lambda A: K(SOS, A((N,), F32), padlen=15))
case("sos_filtfilt", "none-rows-f64", lambda A: K(SOS, A((3, N), F64), padtype=None, padlen=15))
case("sos_filtfilt", "even-c64", lambda A: K(SOS, A((N,), C64), padtype="even", padlen=9))
case("sos_filtfilt", "constant-default", lambda A: K(SOS, A((N,), F32), padtype="constant"))
case("sos_filtfilt", "padlen-refused", lambda A: K(SOS, A((10,), F32), padlen=10))
case("sos_filtfilt", "padtype-refused", lambda A: K(SOS, A((N,), F32), padtype="wrap"))

# -- the pwelch epilogue
NB1 = NFFT // 2
case("csd_epilogue", "onesided", lambda A: K(A((NB1,), F64), A((2, NB1), F64), A((2, NB1), C128), NFFT, True, 1.5))
case("csd_epilogue", "twosided", lambda A: K(A((NFFT,), F64), A((2, NFFT), F64), A((2, NFFT), C128), NFFT, False, 1.5))
case("csd_epilogue", "one-channel", lambda A: K(A((NB1,), F64), A((NB1,), F64), A((NB1,), C128), NFFT, True, 1.5))
case("csd_epilogue", "casts", lambda A: K(A((NB1,), F32), A((2, NB1), F32), A((2, NB1), C64), NFFT, True, 1.5))
case("csd_epilogue", "complex-powers", lambda A: K(A((NB1,), C128), A((2, NB1), C128), A((2, NB1), C128), NFFT, True, 1.5))


def squared(a):
    """a * a in a's own memory, so that a pointer to it still resolves: weights, which must not be negative"""
    a *= a
    return a


def as_tensor(A, a):
    """an array of the case as a tensor in both modes (host mode: on the same memory)"""
    return a if A.dev else torch.from_numpy(a)


# -- cross-wavelet spectra and wavelet coherence
WN = 400                                       # the wavelet record; the strided views keep WN of WN + 3 and WN + 5
case("wct_time", "coherence", lambda A: K(A((2, WN), F32), A((2, WN), F32), SCALES, "morlet", 6.0, CL, CM, 16))
case("wct_time", "xwt-paul-c64", lambda A: K(A((WN,), C64), A((WN,), C64), SCALES, "paul", 4.0, CL, CM, xwt=True))
case("wct_time", "strided-rows-two-pitches", lambda A: K(A((3, WN + 3), C64)[:, :WN], A((3, WN + 5), C64)[:, :WN], SCALES, "morlet", 6.0,
                                                           CL, CM, 16))
case("wct_time", "3d", lambda A: K(A((2, 2, WN), F32), A((2, 2, WN), F32), SCALES, "morlet", 6.0, CL, CM, 16))
case("wct_time", "f64", lambda A: K(A((WN,), F64), A((WN,), F64), SCALES, "morlet", 6.0, CL, CM, 16))
case("wct_time", "host-y", lambda A: K(A((WN,), F32), A((WN,), F32, host=True), SCALES, "morlet", 6.0, CL, CM, 16))
case("wct_time", "shape-refused", lambda A: K(A((WN,), F32), A((WN - 1,), F32), SCALES, "morlet", 6.0, CL, CM, 16))
case("wct_time", "dtype-refused", lambda A: K(A((WN,), F32), A((WN,), C64), SCALES, "morlet", 6.0, CL, CM, 16))
case("wct_time", "Mg-xwt-refused", lambda A: K(A((WN,), F32), A((WN,), F32), SCALES, "morlet", 6.0, CL, CM, 16, xwt=True))
case("wct_time", "paul-coherence-refused", lambda A: K(A((WN,), F32), A((WN,), F32), SCALES, "paul", 4.0, CL, CM, 16))
case("wct_time", "margin-refused", lambda A: K(A((WN,), F32), A((WN,), F32), SCALES, "morlet", 6.0, CL, 100, 16))
WTAPS = [0.25, 0.5, 0.25]
case("wct_scale", "r2-phase", lambda A: K(A((3, WN, 4), F32), WTAPS))
case("wct_scale", "spectra", lambda A: K(A((3, WN + 1, 4), F32), WTAPS, spectra=True))
case("wct_scale", "lead", lambda A: K(A((2, 2, 3, WN, 4), F32), WTAPS))
case("wct_scale", "strided", lambda A: K(A((3, WN, 8), F32)[..., :4], WTAPS))
case("wct_scale", "f64", lambda A: K(A((3, WN, 4), F64), WTAPS))
case("wct_scale", "last-axis-refused", lambda A: K(A((3, WN, 3), F32), WTAPS))
case("wct_scale", "2d-refused", lambda A: K(A((WN, 4), F32), WTAPS))
case("wct_scale", "taps-empty-refused", lambda A: K(A((3, WN, 4), F32), []))
case("wct_scale", "rows-0-refused", lambda A: K(A((0, 3, WN, 4), F32), WTAPS))

# -- synchrosqueezing and the reassignment fields
SSQ_H = np.hanning(NFFT)
SSQ_DH, SSQ_TH = np.gradient(SSQ_H), (np.arange(NFFT) - NFFT // 2) * SSQ_H
case("ssq", "f32-T", lambda A: K(A((2, N), F32), SSQ_H, SSQ_DH, HOP, -NFFT // 2, NFR))
case("ssq", "c64-band", lambda A: K(A((N,), C64), SSQ_H, SSQ_DH, HOP, 0, NFR, th=SSQ_TH, b0=60, nb=9, P=True, IF=True))
case("ssq", "GD-only-segmean-gamma-rel", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH, HOP, 0, NFR, th=SSQ_TH, T=False, GD=True, segmean=True,
                                                      gamma=0.5, rel=1e-3))
case("ssq", "strided-rows", lambda A: K(A((3, N + 3), F32)[:, :N], SSQ_H, SSQ_DH, HOP, 0, NFR))
case("ssq", "3d", lambda A: K(A((2, 2, N), F32), SSQ_H, SSQ_DH, HOP, 0, NFR))
case("ssq", "f64", lambda A: K(A((N,), F64), SSQ_H, SSQ_DH, HOP, 0, NFR))
case("ssq", "th-missing-refused", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH, HOP, 0, NFR, IF=True))
case("ssq", "no-output-refused", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH, HOP, 0, NFR, T=False))
case("ssq", "lds-refused", lambda A: K(A((N,), C64), SSQ_H, SSQ_DH, HOP, 0, NFR, th=SSQ_TH, P=True, IF=True))
case("ssq", "band-refused", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH, HOP, 0, NFR, b0=30, nb=9))
case("ssq", "n-refused", lambda A: K(A((N,), F32), np.hanning(48), np.hanning(48), 0, 0, NFR))         # n before hop
case("ssq", "hop-refused", lambda A: K(A((65536, 1), F32), SSQ_H, SSQ_DH, 0, 0, -1))                    # hop before nframes and rows
case("ssq", "nframes-refused", lambda A: K(A((65536, 1), F32), SSQ_H, SSQ_DH, HOP, 0, -1))              # nframes before rows
case("ssq", "rows-refused", lambda A: K(A((65536, 0), F32), SSQ_H, SSQ_DH, HOP, 0, NFR))                # rows before the empty rows
case("ssq", "empty-rows-refused", lambda A: K(A((2, 0), F32), SSQ_H, SSQ_DH, HOP, 0, NFR, gamma=-1.0))  # the empty rows before gamma
case("ssq", "gamma-refused", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH, HOP, 0, NFR, gamma=-1.0, rel=float("nan")))
case("ssq", "rel-refused", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH, HOP, 0, NFR, rel=float("nan")))
case("ssq", "dh-refused", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH[:-1], HOP, 0, NFR))
case("ssq", "0d", lambda A: K(A((), F32), SSQ_H, SSQ_DH, HOP, 0, NFR))
EDGES = [[2.0, 9.5], [9.5, 30.0]]
FRAME_EDGES = np.tile(np.array(EDGES)[:, None, :], (1, NFR, 1))
for fn, front in (("ssq_bands", lambda A, x: (x, SSQ_H, SSQ_DH, HOP, -NFFT // 2, NFR)), ("ssq_sum", lambda A, x: (x, NFFT))):
    rec = (lambda A: A((2, N), F32)) if fn == "ssq_bands" else (lambda A: A((2, NFR, NFFT // 2 + 1), C64))
    case(fn, "fixed-edges", lambda A, front=front, rec=rec: K(*front(A, rec(A)), EDGES, scale=0.5))
    case(fn, "frame-edges", lambda A, front=front, rec=rec: K(*front(A, rec(A)), FRAME_EDGES))
    case(fn, "frame-edges-tensor", lambda A, front=front, rec=rec: K(*front(A, rec(A)), as_tensor(A, A((2, NFR, 2), F32))))
    case(fn, "frame-edges-tensor-f64", lambda A, front=front, rec=rec: K(*front(A, rec(A)), as_tensor(A, A((2, NFR, 2), F64))))
    case(fn, "frame-edges-host-tensor", lambda A, front=front, rec=rec: K(*front(A, rec(A)), torch.from_numpy(A((2, NFR, 2), F32, host=True))))
    case(fn, "one-band", lambda A, front=front, rec=rec: K(*front(A, rec(A)), (2.0, 9.5)))
    case(fn, "nine-bands-refused", lambda A, front=front, rec=rec: K(*front(A, rec(A)), [[k, k + 1.0] for k in range(9)]))
    case(fn, "frame-count-refused", lambda A, front=front, rec=rec: K(*front(A, rec(A)), FRAME_EDGES[:, :-1]))
    case(fn, "tensor-frame-count-refused", lambda A, front=front, rec=rec: K(*front(A, rec(A)), as_tensor(A, A((2, NFR - 1, 2), F32))))
    case(fn, "edges-nonfinite-refused", lambda A, front=front, rec=rec: K(*front(A, rec(A)), [[2.0, float("inf")]]))
    case(fn, "scale-refused", lambda A, front=front, rec=rec: K(*front(A, rec(A)), EDGES, scale=float("nan")))
case("ssq_bands", "c64-strided-segmean", lambda A: K(A((3, N + 3), C64)[:, :N], SSQ_H, SSQ_DH, HOP, 0, NFR, EDGES, segmean=True, gamma=0.5,
                                                      rel=1e-3))
case("ssq_bands", "f64", lambda A: K(A((N,), F64), SSQ_H, SSQ_DH, HOP, 0, NFR, EDGES))
case("ssq_bands", "hop-refused", lambda A: K(A((N,), F32), SSQ_H, SSQ_DH, 0, 0, NFR, EDGES))
case("ssq_sum", "half", lambda A: K(A((2, 2, NFR, NFFT // 2 + 1), C64), NFFT, EDGES, half=True))
case("ssq_sum", "b0", lambda A: K(A((NFR, 20), C64), NFFT, FRAME_EDGES, b0=3, scale=2.0))
case("ssq_sum", "strided", lambda A: K(A((NFR, 40), C64)[:, :20], NFFT, EDGES, b0=3))
case("ssq_sum", "f64", lambda A: K(A((NFR, 20), F64), NFFT, EDGES))
case("ssq_sum", "1d-refused", lambda A: K(A((20,), C64), NFFT, EDGES))
case("ssq_sum", "n-refused", lambda A: K(A((NFR, 20), C64), 48, EDGES))
case("ssq_sum", "band-refused", lambda A: K(A((NFR, 20), C64), NFFT, EDGES, b0=NFFT))

# -- the smoothed pseudo Wigner-Ville distribution
WVD_H, WVD_G, NT = np.hanning(31), np.hanning(9), 16
case("wvd", "auto", lambda A: K(A((2, N), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT))
case("wvd", "cross", lambda A: K(A((2, N), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, y=A((2, N), C64)))
case("wvd", "cross-y-other-pitch", lambda A: K(A((2, N + 3), C64)[:, :N], WVD_H, WVD_G, HOP, 0, NT, NFFT, y=A((2, N + 5), C64)[:, :N]))
case("wvd", "cross-same-pitch", lambda A: K(A((2, N + 3), C64)[:, :N], WVD_H, WVD_G, HOP, 0, NT, NFFT, y=A((2, N + 3), C64)[:, :N]))
case("wvd", "band-first-scale", lambda A: K(A((N,), C64), WVD_H, WVD_G, HOP, -7, NT, NFFT, b0=60, nb=9, scale=0.5))
case("wvd", "strided-rows", lambda A: K(A((3, N + 3), C64)[:, :N], WVD_H, WVD_G, HOP, 0, NT, NFFT))
case("wvd", "3d-cross", lambda A: K(A((2, 2, N), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, y=A((2, 2, N), C64)))
case("wvd", "c128", lambda A: K(A((N,), C128), WVD_H, WVD_G, HOP, 0, NT, NFFT))
case("wvd", "f32-refused", lambda A: K(A((N,), F32), WVD_H, WVD_G, HOP, 0, NT, NFFT))
case("wvd", "nh-even-refused", lambda A: K(A((N,), C64), np.hanning(32), WVD_G, HOP, 0, NT, NFFT))
case("wvd", "ng-257-refused", lambda A: K(A((N,), C64), WVD_H, np.hanning(257), HOP, 0, NT, NFFT))
case("wvd", "lds-refused", lambda A: K(A((N,), C64), WVD_H, WVD_G, 100000, 0, 2, NFFT))
case("wvd", "y-shape-refused", lambda A: K(A((2, N), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, y=A((2, N - 1), C64)))
case("wvd", "y-dtype-refused", lambda A: K(A((2, N), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, y=A((2, N), F32)))
case("wvd", "host-y", lambda A: K(A((2, N), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, y=A((2, N), C64, host=True)))
case("wvd", "g-missing-refused", lambda A: K(A((N,), C64), WVD_H, None, HOP, 0, NT, NFFT))
case("wvd", "nfft-refused", lambda A: K(A((N,), C64), WVD_H, WVD_G, 0, 0, NT, 48))                       # nfft before hop
case("wvd", "hop-refused", lambda A: K(A((65536, 1), C64), WVD_H, WVD_G, 0, 0, -1, NFFT))                 # hop before ntimes and rows
case("wvd", "ntimes-refused", lambda A: K(A((65536, 1), C64), WVD_H, WVD_G, HOP, 0, -1, NFFT))            # ntimes before rows
case("wvd", "rows-refused", lambda A: K(A((65536, 0), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT))              # rows before the empty rows
case("wvd", "empty-rows-refused", lambda A: K(A((2, 0), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, nb=0))      # the empty rows before nb
case("wvd", "nb-refused", lambda A: K(A((N,), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, nb=NFFT + 1, b0=NFFT))
case("wvd", "b0-refused", lambda A: K(A((N,), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, b0=NFFT, scale=float("inf")))
case("wvd", "scale-refused", lambda A: K(A((N,), C64), WVD_H, WVD_G, HOP, 0, NT, NFFT, scale=float("inf")))

# -- spectral correlation (the row means it computes itself are read from a zeroed buffer under the stand-in: they replay alike)
NU = [0.0, 0.1, -0.25, 0.5]
case("cyclic", "f32-own-means", lambda A: K(A((2, N), F32), WIN, HOP, NFR, NU))
case("cyclic", "c64-conj", lambda A: K(A((N,), C64), WIN, HOP, NFR, NU, conj=True, mean_value=0.25 - 0.5j))
case("cyclic", "y-own-means", lambda A: K(A((2, N), F32), WIN, HOP, NFR, NU, y=A((2, N), F32)))
case("cyclic", "y-other-pitch", lambda A: K(A((2, N + 3), C64)[:, :N], WIN, HOP, NFR, NU, y=A((2, N + 5), C64)[:, :N], mean_value=0.5))
case("cyclic", "strided-rows-own-means", lambda A: K(A((3, N + 3), F32)[:, :N], WIN, HOP, NFR, NU))
case("cyclic", "no-detrend", lambda A: K(A((2, N), F32), WIN, HOP, NFR, NU, detrend=False))
case("cyclic", "mean-value-band-first-scale", lambda A: K(A((N,), F32), WIN, HOP, NFR - 1, NU, mean_value=0.5, first=7, b0=60, nb=9,
                                                           scale=0.5))
case("cyclic", "nu-scalar", lambda A: K(A((N,), F32), WIN, HOP, NFR, 0.1, mean_value=0.5))
case("cyclic", "nframes-0", lambda A: K(A((2, N), F32), WIN, HOP, 0, NU))
case("cyclic", "S-Pm", lambda A: K(A((N,), F32), WIN, HOP, NFR, NU, mean_value=0.5, Pp=False))
case("cyclic", "Pp-only", lambda A: K(A((N,), F32), WIN, HOP, NFR, NU, mean_value=0.5, S=False, Pm=False))
case("cyclic", "3d-own-means", lambda A: K(A((2, 2, N), F32), WIN, HOP, NFR, NU))
case("cyclic", "3d-y", lambda A: K(A((2, 2, N), C64), WIN, HOP, NFR, NU, y=A((2, 2, N), C64), mean_value=0.5j))
case("cyclic", "f64", lambda A: K(A((N,), F64), WIN, HOP, NFR, NU, mean_value=0.5))
case("cyclic", "no-output-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, NU, S=False, Pp=False, Pm=False))
case("cyclic", "nu-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, [0.0, 1.5]))
case("cyclic", "nu-2d-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, [NU]))
case("cyclic", "reach-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR + 1, NU))
case("cyclic", "y-shape-refused", lambda A: K(A((2, N), F32), WIN, HOP, NFR, NU, y=A((N,), F32)))
case("cyclic", "y-dtype-refused", lambda A: K(A((2, N), F32), WIN, HOP, NFR, NU, y=A((2, N), C64)))
case("cyclic", "host-y", lambda A: K(A((2, N), F32), WIN, HOP, NFR, NU, y=A((2, N), F32, host=True)))
case("cyclic", "n-refused", lambda A: K(A((N,), F32), np.hanning(48), 0, NFR, NU))                       # n before hop
case("cyclic", "hop-refused", lambda A: K(A((65536, 1), F32), WIN, 0, -1, NU))                            # hop before nframes and rows
case("cyclic", "nframes-refused", lambda A: K(A((65536, 1), F32), WIN, HOP, -1, []))                      # nframes before A
case("cyclic", "A-refused", lambda A: K(A((65536, 1), F32), WIN, HOP, NFR, []))                           # A before rows
case("cyclic", "rows-refused", lambda A: K(A((65536, 0), F32), WIN, HOP, NFR, NU))                        # rows before the empty rows
case("cyclic", "empty-rows-refused", lambda A: K(A((2, 0), F32), WIN, HOP, NFR, [1.5]))                   # the empty rows before nu
case("cyclic", "band-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, NU, b0=NFFT, scale=float("inf")))
case("cyclic", "scale-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, NU, scale=float("inf"), first=1 << 63))
case("cyclic", "first-refused", lambda A: K(A((N,), F32), WIN, HOP, NFR, NU, first=1 << 63))

# -- Lomb-Scargle spectra (every case gives mean_value: the default is read back from the library and judged in Python)
FREQ = np.linspace(0.01, 0.5, 40)
NF = FREQ.size
case("lomb", "plain", lambda A: K(A((N,), F64), A((2, N), F32), FREQ, mean_value=0.25))
case("lomb", "weights-power-row-means", lambda A: K(A((N,), F64), A((2, N), F32), FREQ, weights=squared(A((N,), F64)), normalize="power",
                                                     mean_value=[0.25, -0.5]))
case("lomb", "amplitude-fixed-mean-t-ref", lambda A: K(A((N,), F64), A((N,), F32), FREQ, floating_mean=False, normalize="amplitude", t_ref=0.5,
                                                        mean_value=0.25))
case("lomb", "normalize-bool", lambda A: K(A((N,), F64), A((N,), F32), FREQ, normalize=False, mean_value=0.25))
case("lomb", "3d-row-means", lambda A: K(A((N,), F64), A((2, 2, N), F32), FREQ, mean_value=np.array([0.25, -0.5, 0.0, 1.0])))
case("lomb", "strided-rows", lambda A: K(A((N,), F64), A((3, N + 3), F32)[:, :N], FREQ, mean_value=0.25))
case("lomb", "rows-0", lambda A: K(A((N,), F64), A((0, N), F32), FREQ, mean_value=0.25))
case("lomb", "f-tensor", lambda A: K(A((N,), F64), A((N,), F32), torch.from_numpy(FREQ.copy()), mean_value=0.25))
case("lomb", "t-f32", lambda A: K(A((N,), F32), A((N,), F32), FREQ, mean_value=0.25))
case("lomb", "y-f64", lambda A: K(A((N,), F64), A((N,), F64), FREQ, mean_value=0.25))
case("lomb", "weights-f32", lambda A: K(A((N,), F64), A((N,), F32), FREQ, weights=squared(A((N,), F32)), mean_value=0.25))
case("lomb", "host-y", lambda A: K(A((N,), F64), A((N,), F32, host=True), FREQ, mean_value=0.25))
case("lomb", "host-weights", lambda A: K(A((N,), F64), A((N,), F32), FREQ, weights=squared(A((N,), F64, host=True)), mean_value=0.25))
case("lomb", "normalize-refused", lambda A: K(A((N,), F64), A((N,), F32), FREQ, normalize="psd", mean_value=0.25))
case("lomb", "y-none-refused", lambda A: K(A((N,), F64), None, FREQ, mean_value=0.25))
case("lomb", "y-length-refused", lambda A: K(A((N,), F64), A((N - 1,), F32), FREQ, mean_value=0.25))
case("lomb", "t-2d-refused", lambda A: K(A((2, N), F64), A((2, N), F32), FREQ, mean_value=0.25))
case("lomb", "weights-shape-refused", lambda A: K(A((N,), F64), A((N,), F32), FREQ, weights=squared(A((N - 1,), F64)), mean_value=0.25))
case("lomb", "mean-count-refused", lambda A: K(A((N,), F64), A((2, N), F32), FREQ, mean_value=[0.25, 0.5, 0.75]))
case("lomb", "mean-nonfinite-refused", lambda A: K(A((N,), F64), A((2, N), F32), FREQ, mean_value=float("nan")))
case("lomb", "f-empty-refused", lambda A: K(A((N,), F64), A((N,), F32), FREQ[:0], mean_value=0.25))
case("lomb", "f-nonfinite-refused", lambda A: K(A((N,), F64), A((N,), F32), [0.1, float("inf")], mean_value=0.25))
case("lomb", "t-ref-refused", lambda A: K(A((N,), F64), A((N,), F32), FREQ, t_ref=float("inf"), mean_value=0.25))
case("lomb", "t-empty-refused", lambda A: K(A((0,), F64), A((0,), F32), FREQ, mean_value=0.25))
case("lomb_sums", "plain", lambda A: K(A((N,), F64), A((2, N), F32), FREQ, mean_value=0.25))
case("lomb_sums", "y-none", lambda A: K(A((N,), F64), None, FREQ, mean_value=0.0))
case("lomb_sums", "weights-wnorm-t-ref", lambda A: K(A((N,), F64), A((N,), F32), FREQ, weights=squared(A((N,), F64)), t_ref=0.5,
                                                      mean_value=0.25, wnorm=2.0))
case("lomb_sums", "3d-row-means", lambda A: K(A((N,), F64), A((2, 2, N), F32), FREQ, mean_value=np.array([0.25, -0.5, 0.0, 1.0])))
case("lomb_sums", "strided-rows", lambda A: K(A((N,), F64), A((3, N + 3), F32)[:, :N], FREQ, mean_value=0.25))
case("lomb_sums", "rows-0", lambda A: K(A((N,), F64), A((0, N), F32), FREQ, mean_value=0.25))
case("lomb_sums", "t-f32", lambda A: K(A((N,), F32), A((N,), F32), FREQ, mean_value=0.25))
case("lomb_sums", "wnorm-refused", lambda A: K(A((N,), F64), A((N,), F32), FREQ, mean_value=0.25, wnorm=0.0))
case("lomb_sums", "host-y", lambda A: K(A((N,), F64), A((N,), F32, host=True), FREQ, mean_value=0.25))
case("lomb_sums", "y-length-refused", lambda A: K(A((N,), F64), A((N - 1,), F32), FREQ, mean_value=0.25))


def sums(A, lead=(2,), dt=F64, mean=None, nf=NF):
    """a LombSums as lomb_sums leaves it for rows of the shape `lead`"""
    rows = int(np.prod(lead))
    mean = np.linspace(0.25, 0.5, rows) if mean is None else np.asarray(mean, dtype=np.float64)
    return engine.LombSums(A((nf, 4), dt), A(tuple(lead) + (nf, 2), dt), A((1 + 2 * rows,), dt), mean, 0.5, N)


for nz in ("power", "normalize", "amplitude"):
    case("lomb_finish", nz, lambda A, nz=nz: K(sums(A), FREQ, normalize=nz))
case("lomb_finish", "fixed-mean-int", lambda A: K(sums(A), FREQ, floating_mean=False, normalize=2))
case("lomb_finish", "lead", lambda A: K(sums(A, (2, 2)), FREQ))
case("lomb_finish", "rows-0", lambda A: K(sums(A, (0,)), FREQ))
case("lomb_finish", "f32-sums", lambda A: K(sums(A, dt=F32), FREQ))
case("lomb_finish", "strided-sums", lambda A: K(engine.LombSums(A((NF, 8), F64)[:, :4], A((2, NF, 4), F64)[..., :2], A((10,), F64)[::2],
                                                                np.array([0.25, 0.5]), 0.5, N), FREQ))
case("lomb_finish", "other-f-refused", lambda A: K(sums(A), FREQ[:-1]))
case("lomb_finish", "totals-refused", lambda A: K(sums(A)._replace(totals=A((4,), F64)), FREQ))
case("lomb_finish", "no-rows-refused", lambda A: K(sums(A)._replace(rows=None), FREQ))
case("lomb_finish", "not-sums-refused", lambda A: K((A((NF, 4), F64), A((2, NF, 2), F64), A((5,), F64)), FREQ))
case("lomb_finish", "normalize-refused", lambda A: K(sums(A), FREQ, normalize="psd"))
case("lomb_finish", "mean-nonfinite-refused", lambda A: K(sums(A, mean=[0.25, float("nan")]), FREQ))
case("lomb_finish", "N-refused", lambda A: K(sums(A)._replace(N=0), FREQ))


# -- the framed record of the autoregressive fits and the covariance entries
AR_P = 4                                       # the order of a fit, or the m of covmat


def framed(fn, name, rec, n=NFFT, hop=HOP, first=0, nframes=NFR, P=AR_P, **kw):
    """a case of an entry that takes a framed record: rec(A) makes the record, P is the order (for covmat its m)"""
    if fn == "ar_ls":                              # the stand-in writes no status: check=True would judge uninitialised memory
        kw.setdefault("check", False)
    case(fn, name, lambda A: K(rec(A), n, hop, first, nframes, P, **kw))


def with_nan(a):
    a[..., 5] = float("nan")
    return a


for fn in ("burg", "yule", "covmat", "ar_ls"):
    low, high = {"covmat": (1, 65), "ar_ls": (0, 64)}.get(fn, (0, 257))
    framed(fn, "f32-1d", lambda A: A((N,), F32))
    framed(fn, "c64-rows", lambda A: A((2, N), C64))
    framed(fn, "3d", lambda A: A((2, 2, N), F32))
    framed(fn, "strided-rows", lambda A: A((3, N + 3), F32)[:, :N])
    framed(fn, "transposed", lambda A: A((N, 3), C64).T)
    framed(fn, "f64", lambda A: A((N,), F64))
    framed(fn, "no-detrend", lambda A: A((N,), F32), detrend=False)
    framed(fn, "detrend-none", lambda A: A((N,), F32), detrend=None)
    framed(fn, "mean-real", lambda A: A((2, N), F32), mean_value=0.25)
    framed(fn, "mean-complex", lambda A: A((N,), C64), mean_value=0.25 - 0.5j)
    framed(fn, "nframes-0", lambda A: A((2, N), F32), nframes=0)
    framed(fn, "rows-0", lambda A: A((0, N), F32))
    framed(fn, "first", lambda A: A((N,), F32), first=7, nframes=NFR - 1)
    framed(fn, "0d", lambda A: A((1,), F32).reshape(()))
    framed(fn, "P-low-refused", lambda A: A((N,), F32), P=low)
    framed(fn, "P-high-refused", lambda A: A((N,), F32), P=high)
    framed(fn, "n-refused", lambda A: A((N,), F32), n=1, hop=0)                                        # n before hop
    if fn == "burg":
        framed(fn, "n-16385-refused", lambda A: A((N,), F32), n=16385)
    if fn == "covmat":
        framed(fn, "m-above-n-refused", lambda A: A((N,), F32), n=3)
        framed(fn, "fb-false", lambda A: A((N,), C64), fb=False)
    else:
        framed(fn, "order-above-half-refused", lambda A: A((N,), F32), P=33)
    if fn == "ar_ls":
        framed(fn, "fb-true", lambda A: A((N,), C64), fb=True)
        framed(fn, "nframes-0-checked", lambda A: A((2, N), F32), nframes=0, check=True)
    framed(fn, "hop-refused", lambda A: A((N,), F32), hop=0, nframes=-1)                               # hop before nframes
    framed(fn, "nframes-refused", lambda A: A((65536, 0), F32), nframes=-1)                            # nframes before the segments
    framed(fn, "segments-refused", lambda A: A((65536, 0), F32), nframes=(1 << 31) - 1, first=-1)      # the segments before first
    framed(fn, "first-refused", lambda A: A((N,), F32), first=-1, nframes=NFR + 1)                     # first before the reach
    framed(fn, "reach-refused", lambda A: A((N,), F32), nframes=NFR + 1, mean_value=float("nan"))      # the reach before the mean
    framed(fn, "mean-nonfinite-refused", lambda A: with_nan(A((N,), F32)), mean_value=float("nan"))     # the mean before the samples
    framed(fn, "mean-complex-real-x-refused", lambda A: with_nan(A((N,), F32)), mean_value=0.5j)       # ... and its kind
    framed(fn, "detrend-linear-refused", lambda A: A((N,), F32), detrend="linear", P=low)              # detrend before the order
    framed(fn, "mean-detrend-off-refused", lambda A: A((N,), F32), detrend=False, mean_value=0.25)
    framed(fn, "nan-sample", lambda A: with_nan(A((2, N), F32)))                                        # refused in host mode only
    framed(fn, "nan-sample-c64", lambda A: with_nan(A((N,), C64)))

# -- spectra of all-pole models; pseudospectra and array scans of eigen-models
PM_, PSTART, PSTEP = 50, 0.1, 0.001            # the bins of a spectrum: the m, start, step of the czt cases


def model(A, lead=(), dt=F64, nco=AR_P + 1, edt=F64, host=False):
    """-> (a, e) of ar_psd: polynomials of nco coefficients and their error powers, which must not be negative"""
    return A(tuple(lead) + (nco,), dt), squared(A(tuple(lead) or (1,), edt, host=host)).reshape(tuple(lead))


def eig(A, lead=(), m=4, dt=C128, wdt=F64, host=False):
    """-> (V, w) as eigh leaves them: V[..., m, m] and w[..., m], which must not be negative"""
    return A(tuple(lead) + (m, m), dt), squared(A(tuple(lead) + (m,), wdt, host=host))


for lead in ((), (3,), (2, 3)):
    case("ar_psd", "lead-%d" % len(lead), lambda A, lead=lead: K(*model(A, lead), PM_, PSTART, PSTEP))
    case("pseudospectrum", "lead-%d" % len(lead), lambda A, lead=lead: K(*eig(A, lead), 1, PM_, PSTART, PSTEP))
case("ar_psd", "c128-scale", lambda A: K(*model(A, (3,), C128), PM_, PSTART, PSTEP, scale=0.5))
case("ar_psd", "out64", lambda A: K(*model(A, (3,)), PM_, PSTART, PSTEP, out64=True))
case("ar_psd", "c128-out64", lambda A: K(*model(A, (3,), C128), PM_, PSTART, PSTEP, out64=True))
case("ar_psd", "order-0", lambda A: K(*model(A, (3,), nco=1), PM_, PSTART, PSTEP))
case("ar_psd", "models-0", lambda A: K(*model(A, (0,)), PM_, PSTART, PSTEP))
case("ar_psd", "a-f32", lambda A: K(*model(A, (3,), F32), PM_, PSTART, PSTEP))                        # device mode refuses, host mode casts
case("ar_psd", "a-c64", lambda A: K(*model(A, (3,), C64), PM_, PSTART, PSTEP))
case("ar_psd", "e-f32", lambda A: K(*model(A, (3,), edt=F32), PM_, PSTART, PSTEP))
case("ar_psd", "host-e", lambda A: K(*model(A, (3,), host=True), PM_, PSTART, PSTEP))
case("ar_psd", "e-shape-refused", lambda A: K(A((3, 5), F64), squared(A((2,), F64)), PM_, PSTART, PSTEP))
case("ar_psd", "0d-refused", lambda A: K(A((1,), F64).reshape(()), A((1,), F64).reshape(()), PM_, PSTART, PSTEP))
case("ar_psd", "order-refused", lambda A: K(*model(A, (3,), nco=258), 0, PSTART, PSTEP))                    # the order before m
case("ar_psd", "m-refused", lambda A: K(*model(A, (3,)), 0, float("nan"), PSTEP))                           # m before start
case("ar_psd", "start-refused", lambda A: K(*model(A, (4096,), nco=1), (1 << 31) - 1, float("nan"), PSTEP))    # start before the launch
case("ar_psd", "step-refused", lambda A: K(*model(A, (3,)), PM_, PSTART, float("inf")))
case("ar_psd", "scale-refused", lambda A: K(*model(A, (3,)), PM_, PSTART, PSTEP, scale=float("nan")))
case("ar_psd", "launch-refused", lambda A: K(*model(A, (4096,), nco=1), (1 << 31) - 1, PSTART, PSTEP))
case("ar_psd", "nan-a", lambda A: K(with_nan(A((3, 8), F64)), squared(A((3,), F64)), PM_, PSTART, PSTEP))      # refused in host mode only
case("ar_psd", "nan-e", lambda A: K(A((8, 5), F64), with_nan(A((8,), F64)), PM_, PSTART, PSTEP))

case("pseudospectrum", "ev", lambda A: K(*eig(A, (3,)), 1, PM_, PSTART, PSTEP, weighting="ev"))
case("pseudospectrum", "out64-p0", lambda A: K(*eig(A, (3,)), 0, PM_, PSTART, PSTEP, out64=True))
case("pseudospectrum", "ev-out64-p-most", lambda A: K(*eig(A, (3,)), 3, PM_, PSTART, PSTEP, weighting="ev", out64=True))
case("pseudospectrum", "models-0", lambda A: K(*eig(A, (0,)), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "V-real", lambda A: K(*eig(A, (3,), dt=F64), 1, PM_, PSTART, PSTEP))            # device mode refuses, host mode casts
case("pseudospectrum", "V-c64", lambda A: K(*eig(A, (3,), dt=C64), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "w-f32", lambda A: K(*eig(A, (3,), wdt=F32), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "host-w", lambda A: K(*eig(A, (3,), host=True), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "weighting-refused", lambda A: K(*eig(A), 1, PM_, PSTART, PSTEP, weighting="capon"))
case("pseudospectrum", "V-not-square-refused", lambda A: K(A((4, 5), C128), squared(A((4,), F64)), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "V-1d-refused", lambda A: K(A((4,), C128), squared(A((4,), F64)), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "w-shape-refused", lambda A: K(A((3, 4, 4), C128), squared(A((3, 5), F64)), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "m-low-refused", lambda A: K(*eig(A, m=1), -1, PM_, PSTART, PSTEP))              # m before p
case("pseudospectrum", "m-high-refused", lambda A: K(*eig(A, m=65), 1, PM_, PSTART, PSTEP))
case("pseudospectrum", "p-low-refused", lambda A: K(*eig(A), -1, 0, PSTART, PSTEP))                     # p before nbins
case("pseudospectrum", "p-high-refused", lambda A: K(*eig(A), 4, PM_, PSTART, PSTEP))
case("pseudospectrum", "nbins-refused", lambda A: K(*eig(A), 1, 0, float("nan"), PSTEP))                # nbins before start
case("pseudospectrum", "start-refused", lambda A: K(*eig(A, (4096,), m=2), 1, (1 << 31) - 1, float("nan"), PSTEP))   # start before the launch
case("pseudospectrum", "step-refused", lambda A: K(*eig(A), 1, PM_, PSTART, float("inf")))
case("pseudospectrum", "launch-refused", lambda A: K(*eig(A, (4096,), m=2), 1, (1 << 31) - 1, PSTART, PSTEP))
case("pseudospectrum", "nan-V", lambda A: K(with_nan(A((3, 8, 8), C128)), squared(A((3, 8), F64)), 1, PM_, PSTART, PSTEP))   # host mode only
case("pseudospectrum", "nan-w", lambda A: K(A((3, 8, 8), C128), with_nan(A((3, 8), F64)), 1, PM_, PSTART, PSTEP))

BM, BNK = 4, 33
BPOS, BKV = np.arange(BM) * 0.5, np.linspace(-0.5, 0.5, BNK)
BPOS2 = np.stack([BPOS, BPOS[::-1] * 0.25], axis=1)
BKV2 = np.stack([BKV, BKV * BKV], axis=1)
for method in ("bartlett", "capon", "music", "ev"):
    case("beamscan", method, lambda A, method=method: K(*eig(A, (3,)), BPOS, BKV, method=method, p=1))
case("beamscan", "defaults-lead-0", lambda A: K(*eig(A), BPOS, BKV))
case("beamscan", "lead-2-pos-2d", lambda A: K(*eig(A, (2, 3)), BPOS2, BKV2, method="music", p=1))
case("beamscan", "capon-loading-out64", lambda A: K(*eig(A, (3,)), BPOS2, BKV2, method="capon", loading=0.01, out64=True))
case("beamscan", "scale-scalar", lambda A: K(*eig(A, (3,)), BPOS, BKV, scale=0.5))
case("beamscan", "scale-per-model", lambda A: K(*eig(A, (2, 3)), BPOS, BKV, scale=np.linspace(0.5, 1.5, 6).reshape(2, 3)))
case("beamscan", "scale-row", lambda A: K(*eig(A, (2, 3)), BPOS, BKV, scale=[0.5, 1.0, 1.5]))
case("beamscan", "tables-tensors", lambda A: K(*eig(A, (3,)), as_tensor(A, A((BM, 2), F64)), as_tensor(A, A((BNK, 2), F32)),
                                               scale=as_tensor(A, A((3,), F64))))
case("beamscan", "tables-lists", lambda A: K(*eig(A, (3,)), list(BPOS), list(BKV), method="ev", p=3))
case("beamscan", "models-0", lambda A: K(*eig(A, (0,)), BPOS, BKV))
case("beamscan", "V-real", lambda A: K(*eig(A, (3,), dt=F64), BPOS, BKV))                              # device mode refuses, host mode casts
case("beamscan", "w-f32", lambda A: K(*eig(A, (3,), wdt=F32), BPOS, BKV))
case("beamscan", "host-w", lambda A: K(*eig(A, (3,), host=True), BPOS, BKV))
case("beamscan", "V-not-square-refused", lambda A: K(A((4, 5), C128), squared(A((4,), F64)), BPOS, BKV))
case("beamscan", "w-shape-refused", lambda A: K(A((3, 4, 4), C128), squared(A((3, 5), F64)), BPOS, BKV))
case("beamscan", "pos-3d-refused", lambda A: K(*eig(A), BPOS2[None], BKV2))
case("beamscan", "pos-width-refused", lambda A: K(*eig(A), np.zeros((BM, 4)), np.zeros((BNK, 4))))
case("beamscan", "pos-nonfinite-refused", lambda A: K(*eig(A), BPOS + float("inf"), BKV2))             # pos before kv
case("beamscan", "kv-width-refused", lambda A: K(*eig(A), BPOS, BKV2))
case("beamscan", "kv-nonfinite-refused", lambda A: K(*eig(A), BPOS, BKV + float("nan"), method="esprit"))   # kv before the method
case("beamscan", "method-refused", lambda A: K(*eig(A, m=1), BPOS, BKV, method="esprit"))              # the method before m
case("beamscan", "m-low-refused", lambda A: K(*eig(A, m=1), BPOS[:1], BKV[:0]))                          # m before nk
case("beamscan", "m-high-refused", lambda A: K(*eig(A, m=65), BPOS, BKV))
case("beamscan", "nk-refused", lambda A: K(*eig(A), BPOS, BKV[:0], method="music", p=4))                # nk before p
case("beamscan", "p-low-refused", lambda A: K(*eig(A), BPOS, BKV, method="music", p=-1, loading=-1.0))  # p before the loading
case("beamscan", "p-high-refused", lambda A: K(*eig(A), BPOS, BKV, method="ev", p=4))
case("beamscan", "p-unjudged", lambda A: K(*eig(A, (3,)), BPOS, BKV, method="capon", p=9))              # p is the eigen methods' alone
case("beamscan", "loading-refused", lambda A: K(*eig(A), BPOS[:3], BKV, loading=-1.0))                  # the loading before pos's length
case("beamscan", "loading-nonfinite-refused", lambda A: K(*eig(A), BPOS, BKV, loading=float("inf")))
case("beamscan", "pos-length-refused", lambda A: K(*eig(A), BPOS[:3], BKV, scale=float("nan")))         # pos's length before the scale
case("beamscan", "scale-nonfinite-refused", lambda A: K(*eig(A, (3,)), BPOS, BKV, scale=[1.0, float("nan"), 1.0]))
case("beamscan", "nan-V", lambda A: K(with_nan(A((3, 8, 8), C128)), squared(A((3, 8), F64)), np.arange(8.0), BKV))   # refused in host mode only
case("beamscan", "nan-w", lambda A: K(A((3, 8, 8), C128), with_nan(A((3, 8), F64)), np.arange(8.0), BKV))

FUNCTIONS = ("fft", "mean","welch_psd", "welch_accum", "welch_export", "welch_apply", "welch_finish", "welch_csd", "csd_matrix",
             "channel_means", "stft_frames", "istft_frames", "bispectrum", "multitaper", "czt", "zoom_welch", "ddc", "upfirdn", "pfb",
             "pfb_synth", "stft_cog", "hilbert_rows", "frame_sum", "spectral_filter_rows", "xcorr_normalised", "xcorr_frames", "skf",
             "welch_blocks", "cwt", "icwt_sum", "eigh", "fir_filter", "biquad_filter", "sos_filter", "sos_filtfilt", "csd_epilogue",
             "wct_time", "wct_scale", "ssq", "ssq_bands", "ssq_sum", "wvd", "cyclic", "lomb", "lomb_sums", "lomb_finish", "burg", "yule", "covmat",
             "ar_ls", "ar_psd", "pseudospectrum", "beamscan")
