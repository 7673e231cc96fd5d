"""Array-level entry points over the C ABI (libspectral.so).

Two calling modes, chosen once per call from the type of the sample array by `_mode(x)`, or by `_enter(x)`, which binds the stream first:
  * numpy arrays  -> `_HOST` (`mem=0`): the library stages host buffers through its own device scratch and returns
                     numpy results (synchronous).  This is what the drop-in modules use.
  * torch CUDA tensors -> `_DEV` (`mem=1`): device pointers are passed straight through, work is enqueued on
                     torch's current stream, results are torch tensors on the same device (asynchronous).
                     PyTorch is only the allocator / stream owner here.
The mode object holds what the two differ in (casting the samples, allocating results, taking addresses, the prologue of the call and the
trailing `mem`), so every entry point below assembles the argument list of its sp_* entry once; where the modes differ in substance
the function says so with an `if md.dev:`.  There is no CPU implementation behind these functions.
"""
import collections
import math
import operator

import numpy as np

from . import _ffi
from ._ffi import SIDED_ONE, SIDED_TWO, SIDED_RAW, SIDED_HALF, check, lib, ptr

try:                                    # torch is optional plumbing (device memory + streams)
    import torch
except Exception:                       # pragma: no cover
    torch = None


def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _bind_stream(x):
    """mem=1 prologue: make the library launch on torch's current stream for x's device."""
    if not x.is_cuda:
        raise TypeError("torch tensors passed to pyfft_amd.engine must live on the GPU")
    _ffi.init(x.device.index if x.device.index is not None else torch.cuda.current_device())
    check(lib().sp_set_stream(torch.cuda.current_stream(x.device).cuda_stream))


def _torch_samples(x):
    if x.dtype not in (torch.float32, torch.complex64):
        raise TypeError("device path takes float32 or complex64 samples, got %s" % x.dtype)
    return x.contiguous()


def _torch_checked(x):
    """_torch_samples without the copy: the strided-rows rule decides about that (the streamed step keeps the one above as it was)"""
    if x.dtype not in (torch.float32, torch.complex64):
        raise TypeError("device path takes float32 or complex64 samples, got %s" % x.dtype)
    return x


def _tcode(x):
    return _ffi.DTYPE_C64 if x.dtype == torch.complex64 else _ffi.DTYPE_F32


def _win32(win):
    return np.ascontiguousarray(np.asarray(win), dtype=np.float32)


def nbins(nfft, sided):
    """Nnyquist bins for the reference's one-sided crop (fft_analysis.py:2471-2484), else nfft."""
    if sided == SIDED_ONE:
        return (nfft + 1) // 2 if nfft % 2 else nfft // 2
    if sided == SIDED_HALF:
        return nfft // 2 + 1
    return nfft


def _detrend_args(detrend, mean_value):
    """detrend: False/0/None none, True/1/'mean' mean of the whole record, 2/'linear' its least-squares line, 3/'segmean' every
    segment's own mean, 4/'seglinear' every segment's own least-squares line (the matplotlib.mlab convention; modes 3 and 4 of
    the C ABI, on welch_psd, welch_csd, stft_frames and stft_cog); an explicit mean_value (with detrend truthy and none of
    2, 3, 4) is subtracted as a constant instead of being computed."""
    if detrend in (None, False, 0, "none"):
        return _ffi.DETREND_CONST, 0j
    if detrend in (2, "linear"):
        return _ffi.DETREND_LINEAR, 0j
    if detrend in (3, "segmean"):
        return _ffi.DETREND_SEGMEAN, 0j
    if detrend in (4, "seglinear"):
        return _ffi.DETREND_SEGLINEAR, 0j
    if mean_value is not None:
        return _ffi.DETREND_CONST, complex(mean_value)
    return _ffi.DETREND_MEAN, 0j


def _ncode(x):
    return _ffi.DTYPE_C64 if x.dtype == np.complex64 else _ffi.DTYPE_F32


class _HostMode:
    """numpy arrays in host memory, `mem=0`: what the two calling modes differ in and nothing else (see the module docstring).  dtype
    names are strings ("float64"); `like` is an array of the call, which only the device mode looks at.  Every call pays for these, so
    they are the functions themselves wherever the signatures allow it, and the instances hold no state."""
    dev, mem = False, 0
    ALIKE = "length and dtype"              # what a second signal must share with the first, for the refusals

    checked = staticmethod(_ffi.as_samples)             # samples as float32 / complex64: contiguous here, as they came on the device
    samples = staticmethod(_ffi.as_samples)             # ... and contiguous in both
    addr = staticmethod(ptr)                            # the address of an array, or None
    code = staticmethod(_ncode)                         # the dtype code of samples
    count = staticmethod(operator.attrgetter("size"))   # the number of elements

    def bind(self, x):
        pass

    def cast(self, x, dt):
        return np.ascontiguousarray(x, dtype=dt)

    def rows(self, x):
        """checked samples -> (contiguous rows, their pitch)"""
        return x, int(x.shape[-1])

    def empty(self, shape, dt, like):
        return np.empty(shape, dt)

    def alike(self, a, b):
        return a.dtype == b.dtype and a.size == b.size

    def init(self):
        _ffi.init()

    def call(self, entry, *args):
        """_ffi.init() immediately before the library call that needs the device, `mem` behind its arguments"""
        _ffi.init()
        check(entry(*args, 0))


class _DeviceMode:
    """torch tensors in device memory, `mem=1`, on torch's current stream: bind(), then as _HostMode"""
    dev, mem = True, 1
    ALIKE = "length, dtype and device"

    checked = staticmethod(_torch_checked)
    samples = staticmethod(_torch_samples)
    code = staticmethod(_tcode)
    count = staticmethod(operator.methodcaller("numel"))

    def bind(self, x):
        _bind_stream(x)

    def addr(self, a):
        return None if a is None else ptr(a.data_ptr())

    def cast(self, x, dt):
        return x.to(getattr(torch, dt)).contiguous()

    def rows(self, x):
        n = int(x.shape[-1])
        if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= n and x.shape[0] >= 1:
            return x, int(x.stride(0))                        # a row-strided view goes through as it is
        return x.contiguous(), n

    def empty(self, shape, dt, like):
        return torch.empty(shape, dtype=getattr(torch, dt), device=like.device)

    def alike(self, a, b):
        return a.dtype == b.dtype and a.numel() == b.numel() and a.device == b.device

    def init(self):
        pass                                # bind() brought the library up on the tensor's device

    def call(self, entry, *args):
        check(entry(*args, 1))


_HOST, _DEV = _HostMode(), _DeviceMode()


def _mode(x):
    """the calling mode of a call, from its sample array"""
    return _DEV if _is_torch(x) else _HOST


def _enter(x):
    """_mode(x) with the stream bound first when x is a device tensor: most entries bind before they look at their arguments"""
    if torch is not None and isinstance(x, torch.Tensor):
        _bind_stream(x)
        return _DEV
    return _HOST


# ---- what the row-batched entries share ------------------------------------------------------------------------------
def _lead_rows(shape, trailing=1):
    """the leading axes of a shape (all but its last `trailing`) as ints, and the number of rows they hold"""
    lead = tuple(map(int, shape[:-trailing]))
    rows = 1
    for d in lead:
        rows *= d
    return lead, rows


def _plan(entry, names, Refused, who, *args):
    """the answer of a sp_*_plan entry (host arithmetic) as a dict of ints under `names`, `fits` as a bool"""
    out = np.zeros(len(names), dtype=np.int64)
    if entry(*args, ptr(out)) != 0:
        raise Refused("%s: the shape is refused" % who)
    d = dict(zip(names, (int(v) for v in out)))
    if "fits" in d:
        d["fits"] = bool(d["fits"])
    return d


def _second_record(who, Refused, md, x, y):
    """a second record beside the checked x: None, or y checked to be of x's kind, shape, dtype (and device)"""
    if y is None:
        return None
    if _mode(y) is not md:
        raise TypeError("%s: x and y must both be numpy arrays or both device tensors" % who)
    y = md.checked(y)
    if tuple(y.shape) != tuple(x.shape) or not md.alike(x, y):
        raise Refused("%s: y must share x's shape, %s" % (who, md.ALIKE))
    return y


def _paired_rows(md, x, y, nsig):
    """-> (the rows of x, the rows of y or None, the pitch of both): where the two pitches differ both are packed"""
    xs, xld = md.rows(x)
    if y is None:
        return xs, None, xld
    ys, yld = md.rows(y)
    if yld != xld:
        return md.samples(xs), md.samples(ys), nsig
    return xs, ys, xld


def _row_means(v, rows, nsig, out):
    """out[r] = the mean of row r of v, by the existing mean pass (sp_mean) row by row"""
    v = v.reshape(rows, nsig)
    for r in range(rows):
        out[r] = mean(v[r])


def _range_check(Refused, who, length=None, hop=None, count=None, rows=None, nsig=None, x_ld=None, scale=None):
    """The range refusals the row-batched entries share, in this order; what is left None is not judged.  length = (its name, n, the
    least, the most), count = (its name, a number of frames or columns), rows = (rows, the most)."""
    if length is not None and (length[1] < length[2] or length[1] > length[3] or length[1] & (length[1] - 1)):
        raise Refused("%s: %s = %d must be a power of two from %d to %d" % ((who,) + length))
    if hop is not None and hop < 1:
        raise Refused("%s: hop = %d must be at least 1" % (who, hop))
    if count is not None and count[1] < 0:
        raise Refused("%s: %s = %d must not be negative" % ((who,) + count))
    if rows is not None and (rows[0] < 0 or rows[0] > rows[1]):
        raise Refused("%s: %d rows are outside 0 .. %d" % ((who,) + rows))
    if nsig is not None and nsig < 1:
        raise Refused("%s: the rows must hold at least one sample" % who)
    if x_ld is not None and x_ld < nsig:
        raise Refused("%s: x_ld = %d is below nsig = %d" % (who, x_ld, nsig))
    if scale is not None and not math.isfinite(scale):
        raise Refused("%s: scale must be finite" % who)


def _frames_check(Refused, who, n, hop, first, nframes, rows, nsig, x_ld, mean):
    """The refusals about the frames of a record that `ar_check` and `sub_check` end in, in this order."""
    _range_check(Refused, who, hop=hop, count=("nframes", nframes), rows=(rows, (1 << 31) - 1))
    if nframes > (1 << 31) - 1 or rows * nframes > 1 << 40:
        raise Refused("%s: %d rows of %d frames are more segments than 2^40" % (who, rows, nframes))
    if first < 0:
        raise Refused("%s: first = %d must not be negative" % (who, first))
    if nsig is not None and nframes > 0 and first + (nframes - 1) * hop + n > nsig:
        raise Refused("%s: %d frames of %d at hop %d from %d on reach outside the %d samples of a row" % (who, nframes, n, hop, first, nsig))
    if x_ld is not None:
        _range_check(Refused, who, nsig=nsig, x_ld=x_ld)
    if not (math.isfinite(mean.real) and math.isfinite(mean.imag)):
        raise Refused("%s: mean_value must be finite" % who)


def _framed_record(who, Refused, x, detrend, mean_value, judge):
    """The record of the fits (`burg`, `yule`) and of the covariance entries (`covmat`, `ar_ls`) -> (md, rows of x, their pitch, nsig,
    rows, lead, cplx, the detrend code, the constant).  judge(rows, nsig, mean) holds the entry's own refusals about the shape."""
    md = _enter(x)
    x = md.checked(x)
    if x.ndim < 1:
        raise Refused("%s: x needs at least one axis" % who)
    code, mean = _ar_detrend(who, detrend, mean_value, Refused)
    lead, rows = _lead_rows(x.shape)
    nsig = int(x.shape[-1])
    judge(rows, nsig, mean)
    cplx = md.code(x) == _ffi.DTYPE_C64
    if not cplx and mean.imag != 0.0:
        raise Refused("%s: a real record takes a real mean_value" % who)
    if not md.dev and not np.all(np.isfinite(x)):
        raise Refused("%s: x must be finite" % who)
    if md.dev and x.ndim != 2:
        x = x.reshape(rows, nsig)
    xs, xld = md.rows(x)
    return md, xs, xld, nsig, rows, lead, cplx, code, mean


def _eigen_models(who, Refused, V, w):
    """The eigendecompositions `pseudospectrum` and `beamscan` take, V[..., m, m] complex128 and w[..., m] float64 as `eigh` returns
    them -> (md, V, w, V's shape, m), both contiguous"""
    md = _enter(V)
    if _mode(w) is not md:
        raise TypeError("%s: V and w must both be numpy arrays or both device tensors" % who)
    if md.dev:
        if V.dtype != torch.complex128 or w.dtype != torch.float64:
            raise Refused("%s: on the device V is a complex128 tensor and w float64" % who)
        V, w = V.contiguous(), w.contiguous()
    else:
        V = np.ascontiguousarray(np.asarray(V), dtype=np.complex128)
        w = np.ascontiguousarray(np.asarray(w), dtype=np.float64)
    shape = tuple(V.shape)
    if len(shape) < 2 or shape[-1] != shape[-2] or tuple(w.shape) != shape[:-1]:
        raise Refused("%s: V must be [..., m, m] and w [..., m]" % who)
    return md, V, w, shape, int(shape[-1])


def max_wg_fft():
    return int(lib().sp_max_wg_fft())


def last_passes(which=0):
    """Passes the last call's loops made: which=0 its outermost frame-chunk loop, which=1 the most slice passes of one batch of
    long transforms inside it, which=2 (CYC_PASSES) the passes of `cyclic` over its list of cycle frequencies, which=3 (LOMB_PASSES)
    the passes of `lomb` and `lomb_sums` over their frequencies, which=4 (LOMB_LAUNCHES) the most launches the row groups of one such
    pass were dealt to, which=5 (FAM_PASSES) the passes of `fam` over its blocks, which=6 (NUFFT_PASSES) the passes of `nufft1`, `nufft2`
    and `lomb_sums_grid` over their rows; 0 where the call had no such loop (sp_last_passes).
    which=7 (AR_PASSES): the passes of `burg` and `yule` over their segments; which=8 (SUB_PASSES): those of `covmat` and `ar_ls`;
    which=9 (DWT_PASSES): the passes of the tile form of `dwt`, `idwt`, `modwt`, `imodwt` and the single-level entries over their rows."""
    return int(lib().sp_last_passes(int(which)))


# ------------------------------------------------------------------------------------------ A7
def fft(x, n=None, axis=-1, inverse=False):
    """np.fft.fft / ifft semantics (forward unnormalised, inverse 1/n) on the GPU, complex64 math."""
    md = _enter(x)
    if md.dev:
        if axis not in (-1, x.dim() - 1) or (n is not None and n != x.shape[-1]):
            raise NotImplementedError("device-tensor fft: last axis, n == length")
        a = x
    else:                                   # any axis and any n: moved, cropped or padded on the host
        a = np.moveaxis(np.asarray(x), axis, -1)
        if n is not None and n != a.shape[-1]:
            if n < a.shape[-1]:
                a = a[..., :n]
            else:
                pad = [(0, 0)] * (a.ndim - 1) + [(0, n - a.shape[-1])]
                a = np.pad(a, pad)
    a = md.cast(a, "complex64")
    out = md.empty(a.shape, "complex64", a)
    nn = a.shape[-1]
    md.call(lib().sp_fft_c2c, md.addr(a), md.addr(out), nn, md.count(a) // nn if nn else 0, 1 if inverse else -1)
    return out if md.dev else np.moveaxis(out, -1, axis)


def ifft(x, n=None, axis=-1):
    return fft(x, n=n, axis=axis, inverse=True)


# ------------------------------------------------------------------------------------------ A13
def mean(x):
    """Mean of a float32/complex64 vector accumulated in double on the device (python float / complex)."""
    out = (_ffi.C.c_double * 2)()
    md = _enter(x)
    xs = md.samples(x)
    md.call(lib().sp_mean, md.addr(xs), md.code(xs), md.count(xs), out)
    return complex(out[0], out[1]) if md.code(xs) == _ffi.DTYPE_C64 else float(out[0])


def profile_enable(on=True):
    _ffi.init()
    check(lib().sp_profile_enable(1 if on else 0))


def profile_last_ms():
    ms = _ffi.C.c_double(0.0)
    check(lib().sp_profile_last_ms(_ffi.C.byref(ms)))
    return ms.value


def profile_last_kernel():
    return (lib().sp_profile_last_kernel() or b"").decode()


# ------------------------------------------------------------------------------------------ A3+A4
def welch_psd(x, win, hop, nframes, detrend=True, sided=SIDED_TWO, scale=1.0, mean_value=None):
    """Fused Welch PSD: scale/nframes * sum_g |FFT(win*(x_g - mean))|^2, float64 [nbins].
    detrend=True subtracts the mean of the whole of x (computed on the device) unless mean_value is given."""
    w = _win32(win)
    nfft = w.size
    nb = nbins(nfft, sided)
    want, mv = _detrend_args(detrend, mean_value)
    md = _enter(x)
    xs = md.samples(x)
    out = md.empty(nb, "float64", xs)
    md.call(lib().sp_welch_psd, md.addr(xs), md.code(xs), md.count(xs), ptr(w), nfft, int(hop), int(nframes), want, mv.real, mv.imag,
            sided, float(scale), md.addr(out))
    return out


def welch_accum(x, win, hop, nframes, nmean=None):
    """First half of the sharded Welch PSD (see include/spectral.h: sp_welch_accum): accumulates this shard's frames
    against a local mean estimate.  Returns sum(x[0:nmean]) as a (2,) float64 (torch tensor on the device for device
    input, numpy otherwise) for the cross-shard all-reduce."""
    w = _win32(win)
    md = _enter(x)
    xs = md.samples(x)
    nm = md.count(xs) if nmean is None else int(nmean)
    out = md.empty(2, "float64", xs)
    md.call(lib().sp_welch_accum, md.addr(xs), md.code(xs), md.count(xs), ptr(w), w.size, int(hop), int(nframes), nm, md.addr(out))
    return out


def welch_export(x, win, hop, nframes, nmean=None):
    """One-collective form of the sharded Welch PSD (include/spectral.h: sp_welch_export): this shard's additive state,
    float64[5*nfft + 8] (torch tensor on the device for device input).  Sum the states of all shards, then welch_apply."""
    w = _win32(win)
    n = 5 * w.size + 8
    md = _enter(x)
    xs = md.samples(x)
    nm = md.count(xs) if nmean is None else int(nmean)
    out = md.empty(n, "float64", xs)
    md.call(lib().sp_welch_export, md.addr(xs), md.code(xs), md.count(xs), ptr(w), w.size, int(hop), int(nframes), nm, md.addr(out))
    return out


def welch_apply(state, win, frames_total, sided=SIDED_TWO, scale=1.0):
    """PSD of the whole stream (global-mean detrend) from the summed shard states: float64[nbins]."""
    w = _win32(win)
    nb = nbins(w.size, sided)
    md = _enter(state)
    st = md.cast(state, "float64")
    out = md.empty(nb, "float64", st)
    md.call(lib().sp_welch_apply, md.addr(st), ptr(w), w.size, int(frames_total), sided, float(scale), md.addr(out))
    return out


# ---- multi-GPU inside the library (include/spectral.h: sp_comm_*, sp_welch_dist_*) ------------------------------------
def comm_unique_id():
    """rank 0: the RCCL unique id (bytes) every rank passes to comm_init"""
    buf = (_ffi.C.c_char * 128)()
    check(lib().sp_comm_unique_id(_ffi.C.cast(buf, _ffi.C.c_void_p)))
    return bytes(buf.raw)


def comm_init(uid, world, rank, device=None):
    """join the library's own RCCL communicator (collective over all ranks; one process per GPU)"""
    _ffi.init(-1 if device is None else int(device))
    buf = (_ffi.C.c_char * 128).from_buffer_copy(uid)
    check(lib().sp_comm_init(_ffi.C.cast(buf, _ffi.C.c_void_p), int(world), int(rank)))


def comm_info():
    out = (_ffi.C.c_int * 2)()
    check(lib().sp_comm_info(out))
    return int(out[0]), int(out[1])


def comm_destroy():
    check(lib().sp_comm_destroy())


def welch_dist_submit(x, win, hop, nframes, nmean, frames_total, sided=SIDED_TWO, scale=1.0):
    """One step of the streaming Welch PSD (sp_welch_dist_submit): the main kernel on torch's current stream, the epilogue (and
    with a communicator the RCCL all-reduce of the shard's state) on the library's own stream beside the NEXT step's main kernel.
    x: device tensor (this rank's shard).  Returns (out, ndone): `out` = the tensor that will hold THIS step's PSD of the whole
    stream (float64 [nbins], device), `ndone` = how many earlier steps' tensors became valid with this call.  Keep x and out
    alive until reported (NativeWelchPipeline does the bookkeeping)."""
    w = _win32(win)
    _bind_stream(x)
    xs = _torch_samples(x)
    out = torch.empty(nbins(w.size, sided), dtype=torch.float64, device=xs.device)
    nd = _ffi.C.c_int(0)
    check(lib().sp_welch_dist_submit(ptr(xs.data_ptr()), _tcode(xs), xs.numel(), ptr(w), w.size, int(hop), int(nframes),
                                     int(nmean), int(frames_total), sided, float(scale), ptr(out.data_ptr()), _ffi.C.byref(nd)))
    return out, xs, nd.value


def welch_dist_flush():
    """finish every step in flight; returns how many outputs became valid"""
    nd = _ffi.C.c_int(0)
    check(lib().sp_welch_dist_flush(_ffi.C.byref(nd)))
    return nd.value


def welch_finish(nfft, mean, frames_total, sided=SIDED_TWO, scale=1.0, like=None):
    """Second half: apply the (global) mean -- (2,) float64 [re, im], same kind of array welch_accum returned, or None
    for the shard's own mean -- and return scale/frames_total * sum_{local frames} |X|^2 as float64 [nbins]."""
    nb = nbins(nfft, sided)
    like = mean if _is_torch(mean) else like
    md = _mode(like)
    out = md.empty(nb, "float64", like)
    if mean is not None:
        mean = md.cast(mean, "float64")
    # no prologue of its own: welch_accum's call brought the library up and bound the stream
    check(lib().sp_welch_finish(md.addr(mean), int(frames_total), sided, float(scale), md.addr(out), md.mem))
    return out


# ------------------------------------------------------------------------------------------ A5
def welch_csd(x, y, win, hop, nframes, detrend=True, sided=SIDED_ONE, scale=1.0):
    """Reference signal x[nsig] against channels y[nch, nsig] (channel-major).
    Returns (Pxx[nb], Pyy[nch, nb], Pxy[nch, nb] complex128 = Y conj(X)), all float64 based."""
    w = _win32(win)
    nfft = w.size
    nb = nbins(nfft, sided)
    md = _enter(x)
    xs = md.samples(x)
    if md.dev:                               # the tensors must agree as they come
        if not _is_torch(y):
            raise TypeError("welch_csd: x is a device tensor, y must be one too")
        ys = _torch_samples(y)
        if ys.dim() == 1:
            ys = ys[None, :]
        if ys.dtype != xs.dtype:
            raise TypeError("welch_csd: x is %s but y is %s (both float32 or both complex64)" % (xs.dtype, ys.dtype))
        if ys.device != xs.device:
            raise ValueError("welch_csd: x and y live on different devices")
        if xs.dim() != 1 or ys.dim() != 2 or ys.shape[1] < xs.numel():
            raise ValueError("welch_csd: x[nsig] against y[nch, >= nsig]")
    else:                                   # y is cast to x's dtype; a real x beside a complex y is promoted
        ys = np.asarray(y)
        if ys.ndim == 1:
            ys = ys[None, :]
        ys = np.ascontiguousarray(ys, dtype=xs.dtype)
        if np.iscomplexobj(y) and xs.dtype != np.complex64:
            xs = xs.astype(np.complex64)
            ys = np.ascontiguousarray(y, dtype=np.complex64).reshape(ys.shape)
    nch, ld = ys.shape
    pxx = md.empty(nb, "float64", xs)
    pyy = md.empty((nch, nb), "float64", xs)
    pxy = md.empty((nch, nb), "complex128", xs)
    md.call(lib().sp_welch_csd, md.addr(xs), md.addr(ys), md.code(xs), md.count(xs), nch, ld, ptr(w), nfft, int(hop), int(nframes),
            _detrend_args(detrend, None)[0], None, None, sided, float(scale), md.addr(pxx), md.addr(pyy), md.addr(pxy))
    return pxx, pyy, pxy


def csd_matrix(x, win, hop, nframes, detrend=True, scale=1.0, means=None):
    """Full cross-spectral-density matrix of real channels x[nch, nsig]:
    G[k, i, j] = scale/nframes * sum_g X_i[g,k] conj(X_j[g,k]),  k = 0..nfft/2 (rfft bins, no doubling), complex128.
    means (nch values): remove these constants instead of each channel's own mean (a frame shard of a longer record
    passes the means of the WHOLE record, see dist.csd_matrix_sharded)."""
    w = _win32(win)
    nfft = w.size
    nb = nfft // 2 + 1
    want = _detrend_args(detrend, None)[0]
    mh = None
    if means is not None:
        mh = np.ascontiguousarray(means.detach().cpu().numpy() if _is_torch(means) else means, dtype=np.float64).ravel()
    md = _enter(x)
    xs = md.cast(x, "float32")
    nch, ld = xs.shape
    out = md.empty((nb, nch, nch), "complex128", xs)
    md.init()
    if mh is not None:
        if mh.size != nch:
            raise ValueError("means must have one value per channel")
        check(lib().sp_csd_matrix_means(md.addr(xs), nch, ld, ld, ptr(w), nfft, int(hop), int(nframes), ptr(mh), float(scale),
                                        md.addr(out), md.mem))
    else:
        check(lib().sp_csd_matrix(md.addr(xs), nch, ld, ld, ptr(w), nfft, int(hop), int(nframes), want, float(scale), md.addr(out),
                                  md.mem))
    return out


def channel_means(x, nsamples=None):
    """Mean of the first `nsamples` samples of every row of x[nch, nsig] (float32 channels), float64[nch]."""
    md = _enter(x)
    xs = md.cast(x, "float32")
    nch, ld = xs.shape
    n = ld if nsamples is None else int(nsamples)
    out = md.empty(nch, "float64", xs)
    md.call(lib().sp_channel_means, md.addr(xs), nch, n, ld, md.addr(out))
    return out


# ------------------------------------------------------------------------------------------ A8/A9
def stft_frames(x, win, hop, nframes, detrend=True, sided=SIDED_ONE, amp_scale=1.0, power=False, bin_major=False,
                want_pseg=False, mean_value=None):
    """Per-frame spectra.  complex64 [nframes, nbins] (or float32 power); bin_major -> [nbins, nframes].
    Returns (out, pseg or None); pseg[g] = trapz(|win*(x_g-mean)|^2), unit sample spacing, float64."""
    w = _win32(win)
    nfft = w.size
    nb = nbins(nfft, sided)
    want, mv = _detrend_args(detrend, mean_value)
    shape = (nb, int(nframes)) if bin_major else (int(nframes), nb)
    md = _enter(x)
    xs = md.samples(x)
    out = md.empty(shape, "float32" if power else "complex64", xs)
    pseg = md.empty(int(nframes), "float64", xs) if want_pseg else None
    md.call(lib().sp_stft, md.addr(xs), md.code(xs), md.count(xs), ptr(w), nfft, int(hop), int(nframes), want, mv.real, mv.imag, sided,
            float(amp_scale), 1 if power else 0, 1 if bin_major else 0, md.addr(out), md.addr(pseg))
    return out, pseg


# ------------------------------------------------------------------------------------------ inverse STFT
def istft_frames(Z, win, hop, sided=SIDED_HALF, scale=None, bin_major=False, skip=0, nout=None):
    """Overlap-add synthesis of the frames Z (sp_istft): y[n] = scale * sum_g win[n - g hop] ifft(Z_g)[n - g hop] / sum_g
    win[n - g hop]^2 over the L = (M - 1) hop + nfft samples the M frames reach, returned as y[skip : skip + nout] (nout=None:
    up to L).  Z: complex64 [..., M, nb], or [..., nb, M] with bin_major; nb = nfft // 2 + 1 for sided=SIDED_HALF (float32
    output) or nfft for SIDED_RAW (fftfreq order, complex64 output); the leading axes are independent records.  scale=None:
    sum(win), the inverse of stft_frames(amp_scale=1 / sum(win)).  numpy in -> numpy out; device tensor in -> device tensor
    on the caller's stream."""
    w = _win32(win)
    nfft = w.size
    if sided not in (SIDED_HALF, SIDED_RAW):
        raise ValueError("istft_frames: sided must be SIDED_HALF or SIDED_RAW")
    nb = nbins(nfft, sided)
    if Z.ndim < 2:
        raise ValueError("istft_frames: Z must be at least two-dimensional")
    M = int(Z.shape[-1] if bin_major else Z.shape[-2])
    if int(Z.shape[-2] if bin_major else Z.shape[-1]) != nb:
        raise ValueError("istft_frames: Z has %d bins, the window needs %d" % (Z.shape[-2] if bin_major else Z.shape[-1], nb))
    hop, skip = int(hop), int(skip)
    total = (M - 1) * hop + nfft
    nout = total - skip if nout is None else int(nout)
    sc = float(np.sum(np.asarray(win, dtype=np.float64))) if scale is None else float(scale)
    lead, nch = _lead_rows(Z.shape, 2)
    md = _enter(Z)
    if md.dev and Z.dtype != torch.complex64:            # (host spectra are cast)
        raise TypeError("device path takes complex64 spectra, got %s" % Z.dtype)
    zs = md.cast(Z, "complex64")
    y = md.empty(lead + (max(nout, 0),), "complex64" if sided == SIDED_RAW else "float32", zs)
    md.call(lib().sp_istft, md.addr(zs), sided, 1 if bin_major else 0, nch, M, ptr(w), nfft, hop, sc, skip, nout, md.addr(y))
    return y


# ------------------------------------------------------------------------------------------ bispectrum
def bispectrum(x, win, hop, nframes, y=None, z=None, detrend=True, mean_value=None):
    """Bispectrum of the frames win * (x[g*hop : g*hop+nfft] - trend): (B complex128 [nb, nb], b2 float64 [nb, nb], Pzz float64
    [nb]), sp_bispectrum's conventions (real input: bins 0 .. nfft/2; complex: two-sided, fftshift-ed; NaN outside the valid
    region).  y = z = None: the auto bispectrum; otherwise y and z (None = x) match x's length and dtype.  detrend: as
    stft_frames, whole-record modes only.  numpy in -> numpy out; device tensors in -> device tensors on x's stream."""
    w = _win32(win)
    nfft = w.size
    want, mv = _detrend_args(detrend, mean_value)
    if want not in (_ffi.DETREND_CONST, _ffi.DETREND_MEAN, _ffi.DETREND_LINEAR):
        raise ValueError("bispectrum: detrend must be none, mean or linear over the whole record")
    md = _enter(x)
    xs = md.samples(x)
    ys, zs = [None if v is None else md.samples(v) for v in (y, z)]
    for v in (ys, zs):
        if v is not None and not md.alike(v, xs):
            raise ValueError("bispectrum: y and z must match x's %s" % md.ALIKE)
    nb = nfft if md.code(xs) == _ffi.DTYPE_C64 else nfft // 2 + 1
    B = md.empty((nb, nb), "complex128", xs)
    b2 = md.empty((nb, nb), "float64", xs)
    pzz = md.empty(nb, "float64", xs)
    md.call(lib().sp_bispectrum, md.addr(xs), md.addr(ys), md.addr(zs), md.code(xs), md.count(xs), ptr(w), nfft, int(hop), int(nframes),
            want, mv.real, mv.imag, md.addr(B), md.addr(b2), md.addr(pzz))
    return B, b2, pzz


# ------------------------------------------------------------------------------------------ multitaper
def multitaper(x, tapers, hop, nframes, y=None, detrend=True, mean_value=None, weights=None, scale=1.0):
    """Multitaper spectra of the frames tapers[k] * (x[g*hop : g*hop+nfft] - trend) in one pass (sp_multitaper):
    (pxx, pyy, pxy, skx, sky), float64 / complex128 in raw bin order with nothing doubled (real input: bins 0 .. nfft/2; complex:
    natural FFT order); pyy, pxy (= sum conj(X) Y), sky are None without y, skx and sky are None without weights.
    weights=None: plain sums over the K tapers (fold sqrt(c_k) into the rows); weights=[K]: the eigenspectra skx / sky [K, nb] too, and
    the spectra as their c-weighted sums, c = weights / sum(weights).  detrend: whole-record modes, as bispectrum; mean_value applies
    to x and y.  numpy in -> numpy out; device tensors in -> device tensors on x's stream."""
    tp = np.ascontiguousarray(np.asarray(tapers), dtype=np.float32)
    if tp.ndim != 2:
        raise ValueError("multitaper: tapers must be a [K, nfft] array")
    K, nfft = tp.shape
    want, mv = _detrend_args(detrend, mean_value)
    if want not in (_ffi.DETREND_CONST, _ffi.DETREND_MEAN, _ffi.DETREND_LINEAR):
        raise ValueError("multitaper: detrend must be none, mean or linear over the whole record")
    mean = np.array([mv.real, mv.imag], dtype=np.float64)
    wt = None if weights is None else np.ascontiguousarray(np.asarray(weights), dtype=np.float64)
    if wt is not None and wt.shape != (K,):
        raise ValueError("multitaper: weights must hold one number per taper")
    cross, eigen = y is not None, wt is not None
    md = _enter(x)
    xs = md.samples(x)
    ys = md.samples(y) if cross else None
    if cross and not md.alike(ys, xs):
        raise ValueError("multitaper: y must match x's %s" % md.ALIKE)
    nb = nfft if md.code(xs) == _ffi.DTYPE_C64 else nfft // 2 + 1
    pxx = md.empty(nb, "float64", xs)
    pyy, pxy = (md.empty(nb, "float64", xs), md.empty(nb, "complex128", xs)) if cross else (None, None)
    skx = md.empty((K, nb), "float64", xs) if eigen else None
    sky = md.empty((K, nb), "float64", xs) if eigen and cross else None
    md.call(lib().sp_multitaper, md.addr(xs), md.addr(ys), md.code(xs), md.count(xs), ptr(tp), K, nfft, int(hop), int(nframes), want,
            ptr(mean), ptr(mean), ptr(wt), float(scale), md.addr(pxx), md.addr(pyy), md.addr(pxy), md.addr(skx), md.addr(sky))
    return pxx, pyy, pxy, skx, sky


# ------------------------------------------------------------------------------------------ chirp-z / zoom
def czt(x, m, start, step):
    """Chirp-z transform on an arc along the last axis (sp_czt): X[..., k] = sum_j x[..., j] exp(-2 pi i (start + k step) j), k < m,
    start and step in cycles per sample.  complex64 [..., m]; numpy in -> numpy out, device tensor in -> device tensor on x's
    stream (rows of a 2-D tensor may be strided)."""
    m, start, step = int(m), float(start), float(step)
    md = _enter(x)
    x = md.checked(x)
    if x.ndim < 1:
        raise ValueError("czt: x must have at least one axis")
    xs, ld = md.rows(x)
    n = int(x.shape[-1])
    out = md.empty(tuple(x.shape[:-1]) + (max(m, 0),), "complex64", x)
    md.call(lib().sp_czt, md.addr(xs), md.code(xs), n, ld, md.count(xs) // n if n else 0, m, start, step, md.addr(out))
    return out


def zoom_welch(x, win, hop, nframes, m, start, step, y=None, detrend=False, mean_value=None, scale=1.0, frames=False):
    """The frames win * (x[g*hop : g*hop+nfft] - trend) transformed on the arc start + k step, k < m (sp_zoom_welch).
    frames=False: (pxx, pyy, pxy) = scale / nframes * sums over the frames of |X|^2, |Y|^2, conj(X) Y, float64 / complex128 [m], nothing
    doubled (pyy, pxy None without y); frames=True: complex64 [nframes, m] = scale * X_g.  detrend: whole-record modes, as
    multitaper.  numpy in -> numpy out; device tensors in -> device tensors on x's stream."""
    w = _win32(win)
    nfft, m = w.size, int(m)
    want, mv = _detrend_args(detrend, mean_value)
    if want not in (_ffi.DETREND_CONST, _ffi.DETREND_MEAN, _ffi.DETREND_LINEAR):
        raise ValueError("zoom_welch: detrend must be none, mean or linear over the whole record")
    if frames and y is not None:
        raise ValueError("zoom_welch: frames=True takes one signal")
    mean = np.array([mv.real, mv.imag], dtype=np.float64)
    cross = y is not None
    md = _enter(x)
    xs = md.samples(x)
    ys = md.samples(y) if cross else None
    if cross and not md.alike(ys, xs):
        raise ValueError("zoom_welch: y must match x's %s" % md.ALIKE)
    mm = max(m, 0)
    fr = md.empty((max(int(nframes), 0), mm), "complex64", xs) if frames else None
    pxx = None if frames else md.empty(mm, "float64", xs)
    pyy, pxy = (md.empty(mm, "float64", xs), md.empty(mm, "complex128", xs)) if cross else (None, None)
    md.call(lib().sp_zoom_welch, md.addr(xs), md.addr(ys), md.code(xs), md.count(xs), ptr(w), nfft, int(hop), int(nframes), want,
            ptr(mean), ptr(mean), m, float(start), float(step), float(scale), md.addr(pxx), md.addr(pyy), md.addr(pxy), md.addr(fr))
    return fr if frames else (pxx, pyy, pxy)


# ------------------------------------------------------------------------------------------ down-converter
def ddc_tile(q):
    """Outputs one workgroup of sp_ddc produces at the decimation q (it consumes q times as many samples).  Host only."""
    k = int(lib().sp_ddc_tile(int(q)))
    if k <= 0:
        raise ValueError("ddc_tile: q = %r is outside 1 .. 64" % (q,))
    return k


def ddc(x, nu, q, h, n0=0):
    """Mix, low-pass and decimate along the last axis (sp_ddc): y[..., k] = sum_j h[j] v[..., k q + (T - 1) / 2 - j] with
    v[..., n] = x[..., n] exp(-2 pi i nu (n0 + n)), nu in cycles per sample, h real with an odd length T, k < ceil(n / q).  complex64
    [..., ceil(n / q)]; numpy in -> numpy out, device tensor in -> device tensor on x's stream (rows of a 2-D tensor may be strided)."""
    nu, q, n0 = float(nu), int(q), int(n0)
    if np.iscomplexobj(h):
        raise ValueError("ddc: the taps must be real")
    taps = np.ascontiguousarray(np.asarray(h), dtype=np.float32)
    if taps.ndim != 1:
        raise ValueError("ddc: the taps must be one-dimensional")
    if not 1 <= q <= 64:
        raise ValueError("ddc: q = %d is outside 1 .. 64" % q)
    md = _enter(x)
    x = md.checked(x)
    if x.ndim < 1:
        raise ValueError("ddc: x must have at least one axis")
    xs, ld = md.rows(x)
    n = int(x.shape[-1])
    out = md.empty(tuple(x.shape[:-1]) + (-(-n // q),), "complex64", x)
    md.call(lib().sp_ddc, md.addr(xs), md.code(xs), n, ld, md.count(xs) // n if n else 0, nu, n0, q, ptr(taps), taps.size, md.addr(out))
    return out


# ------------------------------------------------------------------------------------------ rational resampler
def upfirdn_tile(up, down, ntaps, cplx):
    """Outputs one workgroup of sp_upfirdn produces for this shape (cplx: complex64 rows).  Host only."""
    k = int(lib().sp_upfirdn_tile(int(up), int(down), int(ntaps), 1 if cplx else 0))
    if k <= 0:
        raise ValueError("upfirdn_tile: up = %r, down = %r must lie in 1 .. 256 and ntaps = %r in 1 .. 8191" % (up, down, ntaps))
    return k


def upfirdn(x, h, up, down, m0=0, nout=None):
    """Zero-stuff by up, filter with the real taps h and keep every down-th sample along the last axis (sp_upfirdn):
    y[..., m] = sum_j h[j] xu[..., m down - j], xu[..., i up] = x[..., i]; returned are the outputs m0 .. m0 + nout - 1 (nout=None: up to
    the full length ceil(((n - 1) up + T) / down); beyond it the outputs are zero).  The dtype of x is kept: float32 rows stay real.
    up / down must be reduced.  numpy in -> numpy out, device tensor in -> device tensor on x's stream (rows of a 2-D tensor may be
    strided)."""
    up, down, m0 = int(up), int(down), int(m0)
    if np.iscomplexobj(h):
        raise ValueError("upfirdn: the taps must be real")
    taps = np.ascontiguousarray(np.asarray(h), dtype=np.float32)
    if taps.ndim != 1 or taps.size < 1:
        raise ValueError("upfirdn: the taps must be one-dimensional and not empty")
    if not (1 <= up <= 256 and 1 <= down <= 256):
        raise ValueError("upfirdn: up = %d and down = %d must lie in 1 .. 256" % (up, down))
    if taps.size > 8191:
        raise ValueError("upfirdn: %d taps are beyond the 8191 one launch takes" % taps.size)
    md = _enter(x)
    x = md.checked(x)
    if x.ndim < 1 or x.shape[-1] < 1:
        raise ValueError("upfirdn: x must have at least one axis, and at least one sample along it")
    n = int(x.shape[-1])
    full = -(-((n - 1) * up + taps.size) // down)
    nout = max(full - m0, 0) if nout is None else int(nout)
    if m0 < 0 or nout < 0:
        raise ValueError("upfirdn: m0 = %d and nout = %d must not be negative" % (m0, nout))
    xs, ld = md.rows(x)
    cplx = md.code(xs) == _ffi.DTYPE_C64
    out = md.empty(tuple(x.shape[:-1]) + (nout,), "complex64" if cplx else "float32", x)
    md.call(lib().sp_upfirdn, md.addr(xs), md.code(xs), n, ld, md.count(xs) // n, ptr(taps), taps.size, up, down, m0, nout, md.addr(out))
    return out


def pfb(x, h, M, hop, first, nframes, phase_ref=0, r0=0, power=False, out_major=0, scale=1.0):
    """Polyphase filter bank along the last axis (sp_pfb): frame m holds the len(h) = P M samples from first + m hop on (zero outside the
    row), folded to M under the real taps h and transformed: X[..., m, k] = sum_n h[n] x[..., first + m hop + n] exp(-2 pi i k (n + rho_m) / M),
    rho_m = 0 (phase_ref 0) or (r0 + m hop) mod M (phase_ref 1).  Complex input: nb = M bins in FFT order; real input: the bins 0 .. M/2.
    power=False: complex64 [..., nframes, nb] (out_major 0) or [..., nb, nframes] (out_major 1); power=True: float64 [..., nb] =
    scale / nframes sum_m |X|^2.  numpy in -> numpy out, device tensor in -> device tensor on x's stream (rows of a 2-D tensor may be
    strided)."""
    M, hop, first, nframes, r0 = int(M), int(hop), int(first), int(nframes), int(r0)
    if np.iscomplexobj(h):
        raise ValueError("pfb: the taps must be real")
    taps = np.ascontiguousarray(np.asarray(h), dtype=np.float32)
    if taps.ndim != 1:
        raise ValueError("pfb: the taps must be one-dimensional")
    if M < 2 or nframes < 1:
        raise ValueError("pfb: need M >= 2 and nframes >= 1")
    kind, major = (1 if power else 0), int(out_major)

    def oshape(lead, nb):
        if power:
            return tuple(lead) + (nb,)
        return tuple(lead) + ((nb, nframes) if major == 1 else (nframes, nb))
    md = _enter(x)
    x = md.checked(x)
    if x.ndim < 1 or x.shape[-1] < 1:
        raise ValueError("pfb: x must have at least one axis, with at least one sample")
    xs, ld = md.rows(x)
    n = int(x.shape[-1])
    nb = M if md.code(xs) == _ffi.DTYPE_C64 else M // 2 + 1
    out = md.empty(oshape(x.shape[:-1], nb), "float64" if power else "complex64", x)
    md.call(lib().sp_pfb, md.addr(xs), md.code(xs), n, ld, md.count(xs) // n, ptr(taps), taps.size, M, hop, first, nframes,
            int(phase_ref), r0, kind, major, float(scale), md.addr(out))
    return out


def pfb_synth(X, g, M, hop, first, nout, phase_ref=0, r0=0, onesided=True, in_major=0, scale=1.0):
    """Polyphase synthesis bank (sp_pfb_synth), the adjoint of pfb's fold: y[..., a] = sum_m tap[a - s_m] v_m[(a - s_m + rho_m) mod M]
    over the frames with 0 <= a - s_m < len(g), s_m = first + m hop, v_m = the unnormalised inverse M-point transform of frame m,
    tap = float32(g scale / M), rho_m = 0 (phase_ref 0) or (r0 + m hop) mod M (phase_ref 1); a < nout, zero where no frame reaches.
    X: complex64 [..., nframes, nb] (in_major 0) or [..., nb, nframes] (in_major 1, what channelize returns); nb = M // 2 + 1 for
    onesided=True (float32 output) or M (FFT order, complex64 output).  numpy in -> numpy out, device tensor in -> device tensor on
    X's stream (the C entry takes dense rows: a strided view is made contiguous first)."""
    M, hop, first, nout, r0, major = int(M), int(hop), int(first), int(nout), int(r0), int(in_major)
    if np.iscomplexobj(g):
        raise ValueError("pfb_synth: the taps must be real")
    taps = np.ascontiguousarray(np.asarray(g), dtype=np.float32)
    if taps.ndim != 1:
        raise ValueError("pfb_synth: the taps must be one-dimensional")
    if major not in (0, 1):
        raise ValueError("pfb_synth: in_major must be 0 or 1")
    if X.ndim < 2:
        raise ValueError("pfb_synth: X must be at least two-dimensional")
    if M < 2 or nout < 1:
        raise ValueError("pfb_synth: need M >= 2 and nout >= 1")
    nb = M // 2 + 1 if onesided else M
    nframes = int(X.shape[-1] if major else X.shape[-2])
    if int(X.shape[-2] if major else X.shape[-1]) != nb:
        raise ValueError("pfb_synth: X has %d bins, M = %d needs %d" % (X.shape[-2] if major else X.shape[-1], M, nb))
    if nframes < 1:
        raise ValueError("pfb_synth: there are no frames")
    sided = SIDED_HALF if onesided else SIDED_RAW
    lead, batch = _lead_rows(X.shape, 2)
    md = _enter(X)
    if md.dev and X.dtype != torch.complex64:           # (host frames are cast)
        raise TypeError("device path takes complex64 frames, got %s" % X.dtype)
    xs = md.cast(X, "complex64")
    y = md.empty(lead + (nout,), "float32" if onesided else "complex64", xs)
    md.call(lib().sp_pfb_synth, md.addr(xs), sided, major, batch, nframes, ptr(taps), taps.size, M, hop, first, int(phase_ref), r0,
            float(scale), nout, md.addr(y))
    return y


def pfb_synth_plan(M, ntaps, hop, nframes, onesided=True, batch=1):
    """What pfb_synth does by default at this shape (sp_pfb_synth_plan): a dict with fused (bool), groups (the transform groups of a
    workgroup whose ring fits the LDS), fpw (groups per workgroup), fpg (frames per run of the fused path) and halo."""
    out = (_ffi.C.c_int64 * 5)()
    _ffi.init()
    check(lib().sp_pfb_synth_plan(SIDED_HALF if onesided else SIDED_RAW, int(batch), int(nframes), int(ntaps), int(M), int(hop), out))
    return dict(fused=bool(out[0]), groups=int(out[1]), fpw=int(out[2]), fpg=int(out[3]), halo=int(out[4]))


# ------------------------------------------------------------------------------------------ N3
def stft_cog(x, win, hop, nframes, fs, fmin=0.0, fmax=None, detrend=False, mean_value=None):
    """Centre of gravity (power-weighted mean frequency, Doppler.py:43-58) of every frame's two-sided spectrum, reduced
    inside the transform kernel.  float64 [nframes]; band fmin <= |f| <= fmax (default: every bin)."""
    w = _win32(win)
    nfft = w.size
    want, mv = _detrend_args(detrend, mean_value)
    fmax = float(fs) if fmax is None else float(fmax)
    md = _enter(x)
    xs = md.samples(x)
    out = md.empty(int(nframes), "float64", xs)
    md.call(lib().sp_stft_cog, md.addr(xs), md.code(xs), md.count(xs), ptr(w), nfft, int(hop), int(nframes), want, mv.real, mv.imag,
            float(fs), float(fmin), fmax, md.addr(out))
    return out


# ------------------------------------------------------------------------------------------ A10
def hilbert_rows(x2d, nfft):
    """Analytic signal of each row of a real [batch, n_in] array, transform length nfft -> complex64 [batch, nfft]."""
    md = _enter(x2d)
    xs = md.cast(x2d, "float32")
    batch, n_in = xs.shape
    out = md.empty((batch, nfft), "complex64", xs)
    md.call(lib().sp_hilbert, md.addr(xs), n_in, n_in, int(nfft), batch, md.addr(out))
    return out


# ------------------------------------------------------------------------------------------ A5 (nT-model)
def frame_sum(y2d, nfft, hop, nframes, detrend=True):
    """c[ch][n] = sum_g detrended(y[ch][g*hop + n]), n < nfft, for each row of [nch, nsig]; complex128 (float64 for real
    input) [nch, nfft].  sum_g FFT(win*frame_g) = FFT(win*c): the mean spectrum without writing the frames' spectra."""
    want, _ = _detrend_args(detrend, None)
    if want not in (_ffi.DETREND_CONST, _ffi.DETREND_MEAN, _ffi.DETREND_LINEAR):
        raise ValueError("frame_sum: detrend must be none, mean or linear")
    md = _enter(y2d)
    cplx = y2d.is_complex() if md.dev else np.iscomplexobj(y2d)
    ys = md.cast(y2d, "complex64" if cplx else "float32")
    nch, nsig = ys.shape
    out = md.empty((nch, int(nfft), 2), "float64", ys)
    md.call(lib().sp_frame_sum, md.addr(ys), md.code(ys), nsig, nch, nsig, int(nfft), int(hop), int(nframes), want, md.addr(out))
    if md.dev:                              # (re, im) pairs -> a complex view, or the real parts as a view
        return torch.view_as_complex(out) if cplx else out[..., 0]
    return out.view(np.complex128)[..., 0] if cplx else out[..., 0].copy()


# ------------------------------------------------------------------------------------------ N4
def spectral_filter_rows(x2d, H):
    """IFFT(H * FFT(row)) for each real row of [batch, n]; H complex [n] (host table).  complex64 [batch, n]."""
    Hc = np.ascontiguousarray(H, dtype=np.complex64)
    nfft = Hc.size
    md = _enter(x2d)
    xs = md.cast(x2d, "float32")
    batch, n_in = xs.shape
    out = md.empty((batch, nfft), "complex64", xs)
    md.call(lib().sp_spectral_filter, md.addr(xs), n_in, n_in, nfft, batch, ptr(Hc), md.addr(out))
    return out


# ------------------------------------------------------------------------------------------ A11
def xcorr_normalised(x1, x2):
    """co[2n-1] = correlate(x1-m1, x2-m2, 'full') / (n std1 std2), float32."""
    md = _enter(x1)
    if md.dev:                              # the tensors are judged as they come, the host arrays after the cast
        if not _is_torch(x2) or x2.device != x1.device:
            raise ValueError("xcorr: both signals must be tensors on the same device")
        if x1.dim() != 1 or x2.shape != x1.shape:
            raise ValueError("xcorr: two 1-D signals of equal length")
        if x1.is_complex() or x2.is_complex():
            raise TypeError("xcorr: real signals")
    elif np.iscomplexobj(x1) or np.iscomplexobj(x2):
        raise TypeError("xcorr: real signals")
    a, b = md.cast(x1, "float32"), md.cast(x2, "float32")
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("xcorr: two 1-D signals of equal length")
    n = md.count(a)
    out = md.empty(2 * n - 1, "float32", a)
    md.call(lib().sp_xcorr, md.addr(a), md.addr(b), n, md.addr(out))
    return out


def xcorr_frames(x, y, nw, hop, nframes, maxlag, win=None, segmean=True, coeff=True, beta=0.0, weight=None, frames=False, avg=False,
                 peak=False):
    """Short-time cross-correlation (sp_xcorr_frames): frame g pairs x[g*hop : g*hop+nw] with the same stretch of y and yields the
    lags -maxlag .. maxlag of their correlation, c[l] = sum_n a[n+l] conj(b[n]).  segmean: every window's own mean removed; win: an
    optional taper [nw]; coeff: divided by sqrt(sum |a|^2 sum |b|^2); beta > 0: the regularised PHAT weighting; weight: an optional
    table of L = sp_xcorr_frames_len(nw, maxlag) real weights on the cross spectrum in FFT order.
    -> (frames, avg, peak), None for the ones not asked for: frames [nframes, 2 maxlag + 1] float32 / complex64, avg float64 /
    complex128 [2 maxlag + 1] (the mean over the frames), peak float32 [nframes, 2] = (lag of the top, its height), parabola-refined.
    numpy in -> numpy out; device tensors in -> device tensors on x's stream."""
    nw, hop, nframes, maxlag = int(nw), int(hop), int(nframes), int(maxlag)
    w = None if win is None else _win32(win)
    wt = None if weight is None else _win32(weight)
    if w is not None and w.shape != (nw,):
        raise ValueError("xcorr_frames: win must hold nw = %d values" % nw)
    if wt is not None and wt.shape != (int(lib().sp_xcorr_frames_len(nw, maxlag)),):
        raise ValueError("xcorr_frames: weight must hold sp_xcorr_frames_len(nw, maxlag) values")
    if not (frames or avg or peak):
        raise ValueError("xcorr_frames: ask for at least one of frames, avg, peak")
    md = _enter(x)
    xs, ys = md.samples(x), md.samples(y) if _is_torch(y) or not md.dev else None
    if ys is None or not md.alike(ys, xs):
        raise ValueError("xcorr_frames: y must %s x's %s" % ("be a tensor of" if md.dev else "match", md.ALIKE))
    cplx = md.code(xs) == _ffi.DTYPE_C64
    nl, m = 2 * max(maxlag, 0) + 1, max(nframes, 0)
    fr = md.empty((m, nl), "complex64" if cplx else "float32", xs) if frames else None
    av = md.empty((nl,), "complex128" if cplx else "float64", xs) if avg else None
    pk = md.empty((m, 2), "float32", xs) if peak else None
    md.call(lib().sp_xcorr_frames, md.addr(xs), md.addr(ys), md.code(xs), md.count(xs), ptr(w), nw, hop, nframes, maxlag,
            _ffi.DETREND_SEGMEAN if segmean else _ffi.DETREND_CONST, _ffi.XC_COEFF if coeff else _ffi.XC_RAW, float(beta), ptr(wt),
            md.addr(fr), md.addr(av), md.addr(pk))
    return fr, av, pk


def skf(x, y, nfft, hop, nframes, b0, nb, nk, win=None, segmean=True, cross=False, scale=1.0):
    """Two-point wavenumber-frequency histogram (sp_skf): frame g pairs x[g*hop : g*hop+nfft] with the same stretch of y; every frame
    and every bin f of the band (nb bins from b0 on, modulo nfft for complex records) adds p = (|X|^2 + |Y|^2) / 2 (cross: |X| |Y|) to
    cell j = floor((arg(X conj Y) / 2 pi + 1/2) nk) mod nk.  -> S float64 [nb, nk] = scale / nframes * the sums, nothing doubled.
    segmean: every frame's own mean removed; win: an optional taper [nfft].  numpy in -> numpy out; device tensors in -> a device
    tensor on x's stream."""
    nfft, hop, nframes, b0, nb, nk = int(nfft), int(hop), int(nframes), int(b0), int(nb), int(nk)
    w = None if win is None else _win32(win)
    if w is not None and w.shape != (nfft,):
        raise ValueError("skf: win must hold nfft = %d values" % nfft)
    md = _enter(x)
    xs, ys = md.samples(x), md.samples(y) if _is_torch(y) or not md.dev else None
    if ys is None or not md.alike(ys, xs):
        raise ValueError("skf: y must %s x's %s" % ("be a tensor of" if md.dev else "match", md.ALIKE))
    out = md.empty((max(nb, 0), max(nk, 0)), "float64", xs)
    md.call(lib().sp_skf, md.addr(xs), md.addr(ys), md.code(xs), md.count(xs), ptr(w), nfft, hop, nframes,
            _ffi.DETREND_SEGMEAN if segmean else _ffi.DETREND_NONE, _ffi.SKF_CROSS if cross else _ffi.SKF_MEAN, b0, nb, nk,
            float(scale), md.addr(out))
    return out


WELCH_BLOCKS_MIN_NFFT, WELCH_BLOCKS_MAX_NFFT = 32, 8192


class WelchBlocksRefused(ValueError, NotImplementedError):
    """A shape welch_blocks does not take: outside the limits, and a path that is not built (segments that are no power of two or
    longer than one workgroup transform, detrend modes other than the segment's own mean, zero padding)."""


def welch_blocks_check(who, nsig, nfft, hop, nframes, navg, step, detrend, nch=None, y_ld=None):
    """Every refusal of sp_welch_blocks, before the library is touched -> the detrend code."""
    _range_check(WelchBlocksRefused, who, length=("nfft", nfft, WELCH_BLOCKS_MIN_NFFT, WELCH_BLOCKS_MAX_NFFT))
    if hop < 1 or hop > nfft:
        raise WelchBlocksRefused("%s: hop = %d must lie in 1 .. nfft = %d" % (who, hop, nfft))
    if navg < 1:
        raise WelchBlocksRefused("%s: navg = %d must be at least 1" % (who, navg))
    if step < 1:
        raise WelchBlocksRefused("%s: step = %d must be at least 1" % (who, step))
    if nframes < navg:
        raise WelchBlocksRefused("%s: nframes = %d must be at least navg = %d" % (who, nframes, navg))
    if nsig < (nframes - 1) * hop + nfft:
        raise WelchBlocksRefused("%s: the record (%d samples) is shorter than %d frames of %d with hop %d"
                                 % (who, nsig, nframes, nfft, hop))
    if nch is not None and (nch < 1 or nch > 65535):
        raise WelchBlocksRefused("%s: nch = %d outside 1 .. 65535" % (who, nch))
    if y_ld is not None and y_ld < nsig:
        raise WelchBlocksRefused("%s: the rows of y (%d samples) are shorter than x (%d)" % (who, y_ld, nsig))
    if detrend is True or (isinstance(detrend, str) and detrend in ("constant", "segmean")):
        return _ffi.DETREND_SEGMEAN
    if detrend is None or detrend is False or (isinstance(detrend, str) and detrend == "none"):
        return _ffi.DETREND_NONE
    raise WelchBlocksRefused("%s: detrend must be 'constant' (every segment's own mean) or False, got %r" % (who, detrend))


def welch_blocks(x, win, hop, nframes, navg, step=None, y=None, detrend=True, scale=1.0, doubled=False, nfft=None):
    """Time-resolved Welch spectra (sp_welch_blocks): block b holds the frames b*step .. b*step + navg - 1 of the nframes frames
    x[g*hop : g*hop + nfft] (every frame's own mean removed when detrend is True / 'constant', tapered by win[nfft]; win=None: boxcar,
    then nfft is required), nblocks = (nframes - navg) // step + 1, step = navg by default.
    -> (Pxx, Pyy, Pxy): Pxx float32 [nblocks, nb] = scale / navg * sum |X|^2; with y (x's dtype; [nsig] or [nch, >= nsig]) Pyy float32
    and Pxy complex64 = scale / navg * sum conj(X) Y, [nblocks, nb] or [nch, nblocks, nb], else None.  float32 records: nb = nfft/2 + 1,
    the bins 1 .. nfft/2 - 1 doubled when `doubled`; complex64 records: nb = nfft in FFT order.  Every frame is transformed once
    whatever the overlap of the blocks.  numpy in -> numpy out; device tensors in -> device tensors on x's stream."""
    w = None if win is None else _win32(win)
    if w is None and nfft is None:
        raise ValueError("welch_blocks: nfft is required when win is None")
    nfft = int(w.size if nfft is None else nfft)
    if w is not None and w.shape != (nfft,):
        raise ValueError("welch_blocks: win must hold nfft = %d values" % nfft)
    hop, nframes, navg = int(hop), int(nframes), int(navg)
    step = navg if step is None else int(step)
    md = _mode(x)
    xs = md.samples(x)
    if md.dev:                              # the tensors must agree as they come
        ys = None
        if y is not None:
            if not _is_torch(y):
                raise TypeError("welch_blocks: x is a device tensor, y must be one too")
            ys = md.samples(y)
            if ys.dtype != xs.dtype or ys.device != xs.device:
                raise ValueError("welch_blocks: y must have x's dtype and device")
    else:                                   # y is cast to x's dtype; a real x beside a complex y is promoted
        ys = None if y is None else np.asarray(y)
        if ys is not None and (np.iscomplexobj(ys) or xs.dtype == np.complex64):
            xs = np.ascontiguousarray(xs, dtype=np.complex64)
        if ys is not None:
            ys = np.ascontiguousarray(ys, dtype=xs.dtype)
    cplx = md.code(xs) == _ffi.DTYPE_C64
    if xs.ndim != 1 or (ys is not None and ys.ndim not in (1, 2)):
        raise ValueError("welch_blocks: x[nsig] against y[nsig] or y[nch, >= nsig]")
    nsig = int(xs.shape[0])
    squeeze = ys is not None and ys.ndim == 1
    if squeeze:
        ys = ys[None, :]
    nch, ld = (None, None) if ys is None else (int(ys.shape[0]), int(ys.shape[1]))
    code = welch_blocks_check("welch_blocks", nsig, nfft, hop, nframes, navg, step, detrend, nch, ld)
    scale = float(scale)
    _range_check(ValueError, "welch_blocks", scale=scale)
    nblocks, nb = (nframes - navg) // step + 1, nfft if cplx else nfft // 2 + 1
    md.bind(xs)
    pxx = md.empty((nblocks, nb), "float32", xs)
    pyy = None if ys is None else md.empty((nch, nblocks, nb), "float32", xs)
    pxy = None if ys is None else md.empty((nch, nblocks, nb), "complex64", xs)
    md.call(lib().sp_welch_blocks, md.addr(xs), md.addr(ys), md.code(xs), nsig, nch or 0, ld or 0, ptr(w), nfft, hop, nframes, navg,
            step, code, scale, 1 if doubled else 0, md.addr(pxx), md.addr(pyy), md.addr(pxy))
    if squeeze:
        pyy, pxy = pyy[0], pxy[0]
    return pxx, pyy, pxy


def welch_blocks_plan(nfft, hop, nframes, navg, step=None, nch=1, cplx=False):
    """sp_welch_blocks_plan as a dict (host only; nch = 0: no y): nblocks, nb, q (frames of a run), runs, transforms, scratch (bytes of
    run sums), workgroups, lds_bytes."""
    nfft, hop, nframes, navg, nch = int(nfft), int(hop), int(nframes), int(navg), int(nch)
    step = navg if step is None else int(step)
    welch_blocks_check("welch_blocks_plan", (nframes - 1) * hop + nfft, nfft, hop, nframes, navg, step, False, nch if nch else None)
    return _plan(lib().sp_welch_blocks_plan, ("nblocks", "nb", "q", "runs", "transforms", "scratch", "workgroups", "lds_bytes"),
                 WelchBlocksRefused, "welch_blocks_plan", 1 if cplx else 0, nfft, hop, nframes, navg, step, nch)


CWT_MIN_L, CWT_MAX_L, CWT_MAX_ROWS = 256, 8192, 65535
CWT_FAMILIES = {"morlet": _ffi.CWT_MORLET, "paul": _ffi.CWT_PAUL}


class CwtRefused(ValueError, NotImplementedError):
    """A shape the fused wavelet transform does not take: outside the limits, and a path that is not built (frames that are no power
    of two or longer than one workgroup transform, margins that leave less than a quarter of a frame, wavelets that are not analytic)."""


def cwt_check(who, nsig, scales, family, param, L, M, rows=1):
    """Every refusal of sp_cwt's shape, before the library is touched -> (scales float64, family code, param)."""
    L, M = int(L), int(M)
    _range_check(CwtRefused, who, length=("L", L, CWT_MIN_L, CWT_MAX_L))
    if M < 0 or 2 * M >= L:
        raise CwtRefused("%s: M = %d must lie in 0 .. L / 2 - 1 = %d" % (who, M, L // 2 - 1))
    if L - 2 * M < L // 4:
        raise CwtRefused("%s: M = %d leaves hop = L - 2 M = %d below L / 4 = %d" % (who, M, L - 2 * M, L // 4))
    sc = np.ascontiguousarray(np.asarray(scales, dtype=np.float64))
    if sc.ndim != 1 or sc.size < 1:
        raise CwtRefused("%s: scales must be one-dimensional and hold at least one scale" % who)
    if not np.all(np.isfinite(sc)) or not np.all(sc > 0) or np.any(sc > 1e9):
        raise CwtRefused("%s: every scale must be positive and finite" % who)
    if not isinstance(family, str) or family.lower() not in CWT_FAMILIES:
        raise CwtRefused("%s: family %r is not built: 'morlet' or 'paul' (analytic wavelets)" % (who, family))
    param = float(param)
    code = CWT_FAMILIES[family.lower()]
    if not np.isfinite(param) or not (0.0 < param <= 64.0) or (code == _ffi.CWT_PAUL and param < 1.0):
        raise CwtRefused("%s: the %s parameter %r is outside (0, 64] (Morlet's w0) or [1, 64] (Paul's m)" % (who, family, param))
    if nsig < 1:
        raise CwtRefused("%s: the record must hold at least one sample" % who)
    if rows < 1 or rows > CWT_MAX_ROWS:
        raise CwtRefused("%s: %d rows are outside 1 .. %d" % (who, rows, CWT_MAX_ROWS))
    return sc, code, param


def _cwt_weights(who, w, S, name):
    if w is None:
        return None
    w = np.ascontiguousarray(np.asarray(w), dtype=np.float32)
    if w.shape != (S,) or not np.all(np.isfinite(w)):
        raise CwtRefused("%s: %s must hold one finite weight per scale (%d)" % (who, name, S))
    return w


def cwt(x, scales, family, param, L, M, W=True, gws=False, recon=None, bandpow=None):
    """Continuous wavelet transform along the last axis by overlap-save (sp_cwt): scales in samples, family 'morlet' (param = w0) or
    'paul' (param = m), frames of L samples with margin M on either side (hop = L - 2 M).  Outputs, any combination, as a dict:
    'W' complex64 [..., S, N] (W=True), 'gws' float64 [..., S] = sum_n |W|^2 (gws=True), 'recon' complex64 [..., N] = sum_s recon[s] W
    and 'bandpow' float32 [..., N] = sum_s bandpow[s] |W|^2 (weights, one per scale; neither forms W).  float32 records run as x + 0i.
    numpy in -> numpy out; device tensor in -> device tensors on x's stream (rows of a 2-D tensor may be strided)."""
    md = _mode(x)
    x = md.checked(x)
    if x.ndim < 1:
        raise CwtRefused("cwt: x must have at least one axis")
    n = int(x.shape[-1])
    lead, rows = _lead_rows(x.shape)
    sc, code, param = cwt_check("cwt", n, scales, family, param, L, M, rows)
    S = sc.size
    wr, wb = _cwt_weights("cwt", recon, S, "recon"), _cwt_weights("cwt", bandpow, S, "bandpow")
    if not W and not gws and wr is None and wb is None:
        raise CwtRefused("cwt: an output is required: W, gws, recon or bandpow")
    shapes = {"W": (lead + (S, n), "complex64"), "gws": (lead + (S,), "float64"), "recon": (lead + (n,), "complex64"),
              "bandpow": (lead + (n,), "float32")}
    want = {"W": bool(W), "gws": bool(gws), "recon": wr is not None, "bandpow": wb is not None}
    md.bind(x)
    xs, ld = md.rows(x)
    out = {k: md.empty(sh, dt, x) for k, (sh, dt) in shapes.items() if want[k]}
    md.call(lib().sp_cwt, md.addr(xs), md.code(xs), n, ld, rows, ptr(sc), S, code, param, 0.0, int(L), int(M), ptr(wr), ptr(wb),
            md.addr(out.get("W")), md.addr(out.get("gws")), md.addr(out.get("recon")), md.addr(out.get("bandpow")))
    return out


def cwt_plan(nsig, nscales, L, M, rows=1, W=True, gws=False, recon=False, bandpow=False):
    """sp_cwt_plan as a dict (host only): hop, frames (per row), chunk (scales per workgroup), workgroups, scratch (bytes)."""
    cwt_check("cwt_plan", int(nsig), np.ones(max(int(nscales), 0)), "morlet", 6.0, L, M, int(rows))
    bits = (1 if W else 0) | (2 if gws else 0) | (4 if recon else 0) | (8 if bandpow else 0)
    if not bits:
        raise CwtRefused("cwt_plan: an output is required: W, gws, recon or bandpow")
    return _plan(lib().sp_cwt_plan, ("hop", "frames", "chunk", "workgroups", "scratch"), CwtRefused, "cwt_plan", int(nsig), int(nscales),
                 int(rows), int(L), int(M), bits)


def icwt_sum(W, weights):
    """out[..., n] = sum_s weights[s] W[..., s, n] (sp_icwt): the sum behind the wavelet reconstruction, from a materialised W (complex64
    [..., S, N]).  numpy in -> numpy out; device tensor in -> device tensor on W's stream."""
    md = _mode(W)
    if md.dev:
        if W.dtype != torch.complex64:
            raise TypeError("icwt_sum: W must be complex64, got %s" % W.dtype)
    else:                                   # (cast before the shape is judged: a list of rows will do)
        W = md.cast(np.asarray(W), "complex64")
    if W.ndim < 2 or W.shape[-1] < 1 or W.shape[-2] < 1:
        raise CwtRefused("icwt_sum: W must be [..., S, N] with S, N >= 1")
    S, n = int(W.shape[-2]), int(W.shape[-1])
    w = _cwt_weights("icwt_sum", weights, S, "weights")
    if w is None:
        raise CwtRefused("icwt_sum: weights are required")
    lead, rows = _lead_rows(W.shape, 2)
    if rows < 1 or rows > CWT_MAX_ROWS:
        raise CwtRefused("icwt_sum: %d rows are outside 1 .. %d" % (rows, CWT_MAX_ROWS))
    md.bind(W)
    Wc = md.cast(W, "complex64")
    out = md.empty(lead + (n,), "complex64", W)
    md.call(lib().sp_icwt, md.addr(Wc), n, S, rows, ptr(w), md.addr(out))
    return out


WCT_MAX_SCALES, WCT_MAX_TAPS = 65535, 4096


class WctRefused(ValueError, NotImplementedError):
    """A shape the cross-wavelet and coherence kernels do not take: outside the limits, and a path that is not built (the refusals of
    the fused wavelet transform, with the margin Mw + Mg; the smoothing operator of any wavelet but Morlet)."""


def wct_check(who, nsig, scales, family, param, L, Mw, Mg, rows=1, xwt=False):
    """Every refusal of sp_wct_time's shape, before the library is touched -> (scales float64, family code, param)."""
    L, Mw, Mg = int(L), int(Mw), int(Mg)
    if Mw < 0 or Mg < 0:
        raise WctRefused("%s: Mw = %d and Mg = %d must not be negative" % (who, Mw, Mg))
    if xwt and Mg != 0:
        raise WctRefused("%s: Mg = %d must be 0 for the cross-wavelet transform (nothing is smoothed)" % (who, Mg))
    try:
        sc, code, param = cwt_check(who, nsig, scales, family, param, L, Mw + Mg, rows)
    except CwtRefused as e:
        raise WctRefused(str(e).replace("M =", "M = Mw + Mg =")) from None
    if sc.size > WCT_MAX_SCALES:
        raise WctRefused("%s: %d scales are outside 1 .. %d" % (who, sc.size, WCT_MAX_SCALES))
    if not xwt and code != _ffi.CWT_MORLET:
        raise WctRefused("%s: the coherence is built for Morlet wavelets only (the smoothing operator is Morlet's), not %r" % (who, family))
    return sc, code, param


def wct_time(x, y, scales, family, param, L, Mw, Mg=0, xwt=False):
    """The time half of the wavelet coherence along the last axis by overlap-save (sp_wct_time): scales in samples, frames of L samples
    with the margin Mw + Mg on either side.  -> T float32 [..., S, N, 4] = (A_t, B_t, Re C_t, Im C_t): |Wx|^2 / s', |Wy|^2 / s' and
    Wx conj(Wy) / s' smoothed along n by the Gaussian of standard deviation s' (family 'morlet' only); or, with xwt=True (Mg = 0;
    'morlet' or 'paul'), Wxy = Wx conj(Wy) complex64 [..., S, N].  x and y: equal shapes and dtypes.  numpy in -> numpy out; device
    tensor in -> device tensor on x's stream (rows of a 2-D tensor may be strided)."""
    md = _mode(x)
    if _mode(y) is not md:
        raise TypeError("wct_time: x and y must both be numpy arrays or both be device tensors")
    x, y = md.checked(x), md.checked(y)
    if tuple(x.shape) != tuple(y.shape) or x.dtype != y.dtype or (md.dev and x.device != y.device):
        raise WctRefused("wct_time: x and y must share their shape and dtype%s" % (" and device" if md.dev else ""))
    if x.ndim < 1:
        raise WctRefused("wct_time: x must have at least one axis")
    lead, rows = _lead_rows(x.shape)
    n = int(x.shape[-1])
    sc, code, param = wct_check("wct_time", n, scales, family, param, L, Mw, Mg, rows, xwt)
    md.bind(x)
    xs, xld = md.rows(x)
    ys, yld = md.rows(y)
    if xwt:
        out = md.empty(lead + (sc.size, n), "complex64", x)
    else:
        out = md.empty(lead + (sc.size, n, 4), "float32", x)
    md.call(lib().sp_wct_time, md.addr(xs), xld, md.addr(ys), yld, md.code(xs), n, rows, ptr(sc), sc.size, code, param, int(L), int(Mw),
            int(Mg), None if xwt else md.addr(out), md.addr(out) if xwt else None)
    return out


def wct_taps(who, taps):
    taps = np.ascontiguousarray(np.asarray(taps), dtype=np.float32)
    if taps.ndim != 1 or not (1 <= taps.size <= WCT_MAX_TAPS) or not np.all(np.isfinite(taps)):
        raise WctRefused("%s: taps must hold 1 .. %d finite weights" % (who, WCT_MAX_TAPS))
    return taps


def wct_scale(T, taps, spectra=False):
    """The scale half of the wavelet coherence (sp_wct_scale): T float32 [..., S, N, 4] as wct_time leaves it, summed over neighbouring
    scale rows with `taps` (scipy.signal.convolve2d(., taps[:, None], 'same'), rows outside the set zero) -> (R2, phase) float32
    [..., S, N], R2 = |C|^2 / (A B) and phase = atan2(Im C, Re C), both 0 where A B == 0; with spectra=True (R2, phase, A, B, C), the
    smoothed spectra float32, float32 and complex64.  numpy in -> numpy out; device tensor in -> device tensors on T's stream."""
    md = _mode(T)
    if md.dev:
        if T.dtype != torch.float32:
            raise TypeError("wct_scale: T must be float32, got %s" % T.dtype)
    else:
        T = md.cast(np.asarray(T), "float32")
    if T.ndim < 3 or T.shape[-1] != 4 or T.shape[-2] < 1 or not (1 <= T.shape[-3] <= WCT_MAX_SCALES):
        raise WctRefused("wct_scale: T must be [..., S, N, 4] with N >= 1 and S in 1 .. %d" % WCT_MAX_SCALES)
    taps = wct_taps("wct_scale", taps)
    S, n = int(T.shape[-3]), int(T.shape[-2])
    lead, rows = _lead_rows(T.shape, 3)
    if rows < 1 or rows > CWT_MAX_ROWS:
        raise WctRefused("wct_scale: %d rows are outside 1 .. %d" % (rows, CWT_MAX_ROWS))
    md.bind(T)
    Tc = md.cast(T, "float32")
    shape = lead + (S, n)
    out = [md.empty(shape, "float32", T), md.empty(shape, "float32", T)]
    if spectra:
        out += [md.empty(shape, "float32", T), md.empty(shape, "float32", T), md.empty(shape, "complex64", T)]
    md.call(lib().sp_wct_scale, md.addr(Tc), n, S, rows, ptr(taps), taps.size, *([md.addr(o) for o in out] + [None] * (5 - len(out))))
    return tuple(out)


def wct_plan(nsig, nscales, L, Mw, Mg=0, rows=1, xwt=False):
    """sp_wct_plan as a dict (host only): hop, frames (per row), chunk (scales per workgroup), workgroups, lds_bytes."""
    wct_check("wct_plan", int(nsig), np.ones(max(int(nscales), 0)), "morlet", 6.0, L, Mw, Mg, int(rows), xwt)
    return _plan(lib().sp_wct_plan, ("hop", "frames", "chunk", "workgroups", "lds_bytes"), WctRefused, "wct_plan", int(nsig), int(nscales),
                 int(rows), int(L), int(Mw), int(Mg), 1 if xwt else 0)


SSQ_MIN_N, SSQ_MAX_N, SSQ_MAX_ROWS, SSQ_MAX_BANDS, SSQ_LDS_MAX = 32, 8192, 65535, 8, 160 * 1024


class SsqRefused(ValueError, NotImplementedError):
    """A shape the synchrosqueezing kernel does not take: outside the limits, and what is not built (segments that are no power of two
    or longer than one workgroup transform, a band and output set whose accumulators do not fit the LDS of a workgroup)."""


def ssq_lds_bytes(cplx, n, nb, T=True, P=False, fields=False):
    """The LDS of a workgroup: an image of n + 16 complex per transform and 16 (T) + 8 (P) bytes per bin of the band, per group."""
    return max(1, 4096 // n) * (((2 if cplx else 1) + (1 if fields else 0)) * (n + 16) * 8 + nb * ((16 if T else 0) + (8 if P else 0)))


def ssq_check(who, cplx, n, hop, nframes, rows, gamma=0.0, rel=0.0, nsig=None, x_ld=None):
    """The refusals sp_ssq, sp_ssq_bands and sp_ssq_plan share, before the library is touched."""
    _range_check(SsqRefused, who, ("n", n, SSQ_MIN_N, SSQ_MAX_N), hop, ("nframes", nframes), (rows, SSQ_MAX_ROWS), nsig, x_ld)
    for name, v in (("gamma", gamma), ("rel", rel)):
        if not math.isfinite(v) or v < 0:
            raise SsqRefused("%s: %s = %r must be finite and not negative" % (who, name, v))


def ssq_band_check(who, cplx, n, b0, nb, T, P, fields):
    nbins = n if cplx else n // 2 + 1
    if nb < 1 or b0 < 0 or (b0 >= n or nb > n if cplx else b0 + nb > nbins):
        raise SsqRefused("%s: nb = %d bins from b0 = %d lie outside the %d bins of the spectrum" % (who, nb, b0, nbins))
    lds = ssq_lds_bytes(cplx, n, nb, T, P, fields)
    if lds > SSQ_LDS_MAX:
        raise SsqRefused("%s: the LDS of a workgroup, %d bytes, does not fit %d (n %d, nb %d): take a narrower band or fewer outputs"
                         % (who, lds, SSQ_LDS_MAX, n, nb))


def ssq_windows(who, n, h, dh, th=None):
    tabs = [None if w is None else _win32(w) for w in (h, dh, th)]
    for name, w in zip(("h", "dh", "th"), tabs):
        if w is not None and (w.shape != (n,) or not np.all(np.isfinite(w))):
            raise SsqRefused("%s: %s must hold n = %d finite values" % (who, name, n))
    if tabs[0] is None or tabs[1] is None:
        raise SsqRefused("%s: h and dh are required" % who)
    return tabs


def _ssq_front(who, x, n, hop, nframes, gamma, rel):
    md = _mode(x)
    x = md.checked(x)
    if x.ndim < 1:
        raise SsqRefused("%s: x must have at least one axis" % who)
    lead, rows = _lead_rows(x.shape)
    nsig = int(x.shape[-1])
    cplx = md.code(x) == _ffi.DTYPE_C64
    ssq_check(who, cplx, n, hop, nframes, rows, gamma, rel, nsig)
    md.bind(x)
    xs, xld = md.rows(x)
    return md, xs, xld, lead, rows, nsig, cplx


def ssq(x, h, dh, hop, first, nframes, th=None, b0=0, nb=None, T=True, P=False, IF=False, GD=False, segmean=False, gamma=0.0, rel=0.0):
    """The synchrosqueezed STFT and the reassignment fields along the last axis (sp_ssq): frame g = the n = len(h) samples from
    first + g*hop on (zero outside the row) under the windows h, dh (dh/dj) and th ((j - n/2) h, needed for IF / GD).
    -> (T, P, IF, GD), None for what was not asked: T complex64 [..., nframes, nb] = the sums of (-1)^k X_h over the used cells whose
    rint(khat) is the bin, P float32 the same sums of |X_h|^2, IF = khat (bins) and GD = that (samples from the frame's centre) float32
    at the source bins, NaN where |X_h| <= max(gamma, rel * the frame's largest).  The band: nb bins from b0 on (modulo n for complex
    rows; real rows have the bins 0 .. n/2).  numpy in -> numpy out; device tensor in -> device tensors on x's stream."""
    n, hop, first, nframes, b0 = int(np.asarray(h).shape[-1]), int(hop), int(first), int(nframes), int(b0)
    gamma, rel = float(gamma), float(rel)
    md, xs, xld, lead, rows, nsig, cplx = _ssq_front("ssq", x, n, hop, nframes, gamma, rel)
    nb = (n if cplx else n // 2 + 1) - b0 if nb is None else int(nb)
    fields = bool(IF or GD)
    if not (T or P or fields):
        raise SsqRefused("ssq: an output is required: T, P, IF or GD")
    if fields and th is None:
        raise SsqRefused("ssq: th is required with IF or GD")
    ssq_band_check("ssq", cplx, n, b0, nb, bool(T), bool(P), fields)
    hw, dw, tw = ssq_windows("ssq", n, h, dh, th if fields else None)
    shape = lead + (nframes, nb)
    out = [md.empty(shape, dt, xs) if want else None
           for want, dt in ((T, "complex64"), (P, "float32"), (IF, "float32"), (GD, "float32"))]
    md.call(lib().sp_ssq, md.addr(xs), xld, md.code(xs), nsig, rows, ptr(hw), ptr(dw), ptr(tw), n, hop, first, nframes,
            1 if segmean else 0, gamma, rel, b0, nb, *[md.addr(o) for o in out])
    return tuple(out)


def _ssq_edges(who, md, edges, nframes, like):
    """-> (nbands, host float64 [nbands, 2] or None, per-frame float32 [nbands, nframes, 2] in the call's memory or None)"""
    if _is_torch(edges):
        e = edges
        if e.dim() != 3 or e.shape[0] < 1 or e.shape[0] > SSQ_MAX_BANDS or e.shape[1] != nframes or e.shape[2] != 2:
            raise SsqRefused("%s: per-frame edges must be [nbands <= %d, nframes = %d, 2]" % (who, SSQ_MAX_BANDS, nframes))
        if not md.dev:
            return int(e.shape[0]), None, np.ascontiguousarray(e.detach().cpu().numpy(), dtype=np.float32)
        return int(e.shape[0]), None, e.to(device=like.device, dtype=torch.float32).contiguous()
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1 and e.shape == (2,):
        e = e[None, :]
    if e.ndim not in (2, 3) or e.shape[-1] != 2 or e.shape[0] < 1 or e.shape[0] > SSQ_MAX_BANDS or (e.ndim == 3 and e.shape[1] != nframes):
        raise SsqRefused("%s: edges must be [nbands, 2] or [nbands, nframes = %d, 2] with nbands in 1 .. %d" % (who, nframes, SSQ_MAX_BANDS))
    if not np.all(np.isfinite(e)):
        raise SsqRefused("%s: edges must be finite" % who)
    if e.ndim == 2:
        return int(e.shape[0]), np.ascontiguousarray(e), None
    e32 = np.ascontiguousarray(e, dtype=np.float32)
    if md.dev:
        return int(e.shape[0]), None, torch.from_numpy(e32).to(like.device)
    return int(e.shape[0]), None, e32


def ssq_bands(x, h, dh, hop, first, nframes, edges, scale=1.0, segmean=False, gamma=0.0, rel=0.0):
    """Modes without forming T (sp_ssq_bands): out complex64 [..., nbands, nframes], out[b, g] = scale * the sum of (-1)^k X_h over the
    used cells of frame g with lo[b, g] <= khat < hi[b, g] (the un-rounded khat, edges in bins).  edges: [nbands, 2] or, per frame,
    [nbands, nframes, 2]; nbands <= 8.  With first = -n/2 and hop = 1 and scale = 1 / (n h[n/2]) this is the band's analytic waveform;
    with hop > 1 its samples at the frame centres, carrier included."""
    n, hop, first, nframes = int(np.asarray(h).shape[-1]), int(hop), int(first), int(nframes)
    gamma, rel, scale = float(gamma), float(rel), float(scale)
    md, xs, xld, lead, rows, nsig, cplx = _ssq_front("ssq_bands", x, n, hop, nframes, gamma, rel)
    _range_check(SsqRefused, "ssq_bands", scale=scale)
    nbands, ec, et = _ssq_edges("ssq_bands", md, edges, nframes, xs)
    hw, dw, _ = ssq_windows("ssq_bands", n, h, dh)
    out = md.empty(lead + (nbands, nframes), "complex64", xs)
    md.call(lib().sp_ssq_bands, md.addr(xs), xld, md.code(xs), nsig, rows, ptr(hw), ptr(dw), n, hop, first, nframes, 1 if segmean else 0,
            gamma, rel, nbands, ptr(ec), md.addr(et), scale, md.addr(out))
    return out


def ssq_sum(T, n, edges, b0=0, half=False, scale=1.0):
    """Band sums over an existing T [..., nframes, nb] whose first bin is b0 of an n-point transform (sp_ssq_sum): out complex64
    [..., nbands, nframes], out[b, g] = scale * sum over lo <= m < hi of w_m T[g, m - b0], w = 1/2 at the bins 0 and n/2 when `half`."""
    n, b0, scale = int(n), int(b0), float(scale)
    md = _mode(T)
    if md.dev:
        if T.dtype != torch.complex64:
            raise TypeError("ssq_sum: T must be complex64, got %s" % T.dtype)
    else:
        T = np.asarray(T)
    if T.ndim < 2:
        raise SsqRefused("ssq_sum: T must be [..., nframes, nb]")
    nframes, nb = int(T.shape[-2]), int(T.shape[-1])
    lead, rows = _lead_rows(T.shape, 2)
    ssq_check("ssq_sum", True, n, 1, nframes, rows)
    if nb < 1 or b0 < 0 or b0 >= n or nb > n:
        raise SsqRefused("ssq_sum: nb = %d bins from b0 = %d lie outside the %d bins of the spectrum" % (nb, b0, n))
    _range_check(SsqRefused, "ssq_sum", scale=scale)
    md.bind(T)
    Tc = md.cast(T, "complex64")
    nbands, ec, et = _ssq_edges("ssq_sum", md, edges, nframes, Tc)
    out = md.empty(lead + (nbands, nframes), "complex64", Tc)
    md.call(lib().sp_ssq_sum, md.addr(Tc), nframes, nb, rows, n, b0, nbands, ptr(ec), md.addr(et), 1 if half else 0, scale, md.addr(out))
    return out


def ssq_plan(n, nframes, rows=1, cplx=False, nb=None, T=True, P=False, fields=False, bands=False):
    """sp_ssq_plan as a dict (host only): fpr (frames per run), workgroups, lds_bytes, transforms (per frame), fits."""
    n, nframes, rows = int(n), int(nframes), int(rows)
    ssq_check("ssq_plan", cplx, n, 1, nframes, rows)
    nb = (n if cplx else n // 2 + 1) if nb is None else int(nb)
    what = 8 if bands else (1 if T else 0) | (2 if P else 0) | (4 if fields else 0)
    if what == 0:
        raise SsqRefused("ssq_plan: an output is required")
    if not bands and (nb < 1 or nb > (n if cplx else n // 2 + 1)):
        raise SsqRefused("ssq_plan: nb = %d lies outside the %d bins of the spectrum" % (nb, n if cplx else n // 2 + 1))
    return _plan(lib().sp_ssq_plan, ("fpr", "workgroups", "lds_bytes", "transforms", "fits"), SsqRefused, "ssq_plan", 1 if cplx else 0, n,
                 nframes, rows, nb, what)


WVD_MIN_N, WVD_MAX_N, WVD_MAX_NG, WVD_MAX_ROWS, WVD_LDS_MAX = 32, 8192, 255, 65535, 160 * 1024


class WvdRefused(ValueError, NotImplementedError):
    """A shape the Wigner-Ville kernel does not take: outside the limits, and what is not built (transforms that are no power of two
    or longer than one workgroup's, time windows beyond 255 taps, real rows, a run whose staged samples do not fit the LDS)."""


def wvd_lds_bytes(cross, nfft, nh, ng, hop, cpr, ntimes):
    """The LDS of a workgroup: max(1, 4096 / nfft) images of nfft + 16 complex, and 8 bytes per staged sample: (c - 1) hop + nh + ng - 1
    of them, c = the columns per run (auto: rounded up to even), at most ntimes."""
    c = cpr if cross else cpr + (cpr & 1)
    c = min(c, max(ntimes, 1))
    return max(1, 4096 // nfft) * (nfft + 16) * 8 + 8 * ((c - 1) * hop + nh + ng - 1)


def wvd_check(who, nfft, nh, ng, hop, ntimes, rows, nb, b0=0, scale=1.0, nsig=None, x_ld=None):
    """The refusals of sp_wvd and sp_wvd_plan, before the library is touched."""
    _range_check(WvdRefused, who, ("nfft", nfft, WVD_MIN_N, WVD_MAX_N))
    if nh < 1 or not nh & 1 or nh > nfft - 1:
        raise WvdRefused("%s: nh = %d must be odd and lie in 1 .. nfft - 1 = %d" % (who, nh, nfft - 1))
    if ng < 1 or not ng & 1 or ng > WVD_MAX_NG:
        raise WvdRefused("%s: ng = %d must be odd and lie in 1 .. %d" % (who, ng, WVD_MAX_NG))
    _range_check(WvdRefused, who, None, hop, ("ntimes", ntimes), (rows, WVD_MAX_ROWS), nsig, x_ld)
    if nb < 1 or nb > nfft:
        raise WvdRefused("%s: nb = %d must lie in 1 .. nfft = %d" % (who, nb, nfft))
    if b0 < 0 or b0 >= nfft:
        raise WvdRefused("%s: b0 = %d lies outside 0 .. nfft - 1 = %d" % (who, b0, nfft - 1))
    _range_check(WvdRefused, who, scale=scale)


def _wvd_window(who, name, w):
    if w is None:
        raise WvdRefused("%s: %s is required" % (who, name))
    w = _win32(w)
    if w.ndim != 1 or not np.all(np.isfinite(w)):
        raise WvdRefused("%s: %s must be one axis of finite values" % (who, name))
    return w


def _wvd_plan_raw(who, cross, nfft, nh, ng, hop, ntimes, rows, nb):
    return _plan(lib().sp_wvd_plan, ("cpr", "workgroups", "lds_bytes", "transforms", "fits"), WvdRefused, who, 1 if cross else 0, nfft, nh,
                 ng, hop, ntimes, rows, nb)


def wvd(x, h, g, hop, first, ntimes, nfft, y=None, b0=0, nb=None, scale=1.0):
    """The smoothed pseudo Wigner-Ville distribution along the last axis (sp_wvd): column j sits at n = first + j*hop,
    K[j, tau] = h[tau] * sum_mu g[mu] x[n + mu + tau] conj(y[n + mu - tau]) with the rows zero outside themselves, h and g odd, centred
    tables, and W[j] = scale * FFT_nfft(K[j]) at the nb bins from b0 on (modulo nfft); bin k stands for k fs / (2 nfft).
    y None: float32 [..., ntimes, nb] (the distribution of x with itself is real); else the cross distribution, complex64.
    x (and y) must be complex; a real record is made analytic first (pyfft_amd.wigner does).  numpy in -> numpy out; device tensor
    in -> a device tensor on x's stream."""
    nfft, hop, first, ntimes, b0, scale = int(nfft), int(hop), int(first), int(ntimes), int(b0), float(scale)
    md = _mode(x)
    x = md.checked(x)
    if x.ndim < 1:
        raise WvdRefused("wvd: x must have at least one axis")
    if md.code(x) != _ffi.DTYPE_C64:
        raise WvdRefused("wvd: float32 rows are not taken directly: make the record analytic first (pyfft_amd.wigner.spwvd does)")
    lead, rows = _lead_rows(x.shape)
    nsig = int(x.shape[-1])
    hw, gw = _wvd_window("wvd", "h", h), _wvd_window("wvd", "g", g)
    nb = nfft if nb is None else int(nb)
    wvd_check("wvd", nfft, int(hw.size), int(gw.size), hop, ntimes, rows, nb, b0, scale, nsig)
    y = _second_record("wvd", WvdRefused, md, x, y)
    cross = y is not None
    md.bind(x)
    xs, ys, xld = _paired_rows(md, x, y, nsig)
    plan = _wvd_plan_raw("wvd", cross, nfft, int(hw.size), int(gw.size), hop, ntimes, rows, nb)
    if not plan["fits"]:
        raise WvdRefused("wvd: the LDS of a workgroup, %d bytes, does not fit %d (nfft %d, nh %d, ng %d, hop %d, %d columns per run)"
                         % (plan["lds_bytes"], WVD_LDS_MAX, nfft, hw.size, gw.size, hop, plan["cpr"]))
    out = md.empty(lead + (ntimes, nb), "complex64" if cross else "float32", xs)
    md.call(lib().sp_wvd, md.addr(xs), md.addr(ys), xld, nsig, rows, ptr(hw), int(hw.size), ptr(gw), int(gw.size), nfft, hop, first,
            ntimes, b0, nb, scale, md.addr(out))
    return out


def wvd_plan(nfft, nh, ng, hop, ntimes, rows=1, cross=False, nb=None):
    """sp_wvd_plan as a dict (host only): cpr (columns per run), workgroups, lds_bytes, transforms (per run), fits."""
    nfft, nh, ng, hop, ntimes, rows = int(nfft), int(nh), int(ng), int(hop), int(ntimes), int(rows)
    nb = nfft if nb is None else int(nb)
    wvd_check("wvd_plan", nfft, nh, ng, hop, ntimes, rows, nb)
    return _wvd_plan_raw("wvd_plan", cross, nfft, nh, ng, hop, ntimes, rows, nb)


CYC_MIN_N, CYC_MAX_N, CYC_MAX_A, CYC_MAX_ROWS, CYC_PASSES = 32, 8192, 65535, 65535, 2


class CyclicRefused(ValueError, NotImplementedError):
    """A shape the cyclic-periodogram kernel does not take: outside the limits, and what is not built (segments that are no power of
    two or longer than one workgroup's transform)."""


def cyclic_check(who, n, hop, nframes, A, rows, nsig=None, x_ld=None, nu=None, b0=0, nb=None, scale=1.0, first=0):
    """The refusals of sp_cyclic and sp_cyclic_plan, before the library is touched."""
    _range_check(CyclicRefused, who, ("n", n, CYC_MIN_N, CYC_MAX_N), hop, ("nframes", nframes))
    if A < 1 or A > CYC_MAX_A:
        raise CyclicRefused("%s: %d cycle frequencies are outside 1 .. %d" % (who, A, CYC_MAX_A))
    _range_check(CyclicRefused, who, rows=(rows, CYC_MAX_ROWS), nsig=nsig)
    if nsig is not None and nframes > 0 and (nframes - 1) * hop + n > nsig:
        raise CyclicRefused("%s: %d frames of %d at hop %d reach outside the %d samples of a row" % (who, nframes, n, hop, nsig))
    if x_ld is not None:
        _range_check(CyclicRefused, who, nsig=nsig, x_ld=x_ld)
    if nu is not None and not (np.all(np.isfinite(nu)) and np.all(np.abs(nu) <= 1.0)):
        raise CyclicRefused("%s: every nu must be finite and lie in -1 .. 1 cycles per sample" % who)
    nb = n if nb is None else nb
    if nb < 1 or nb > n or b0 < 0 or b0 >= n:
        raise CyclicRefused("%s: the band of nb = %d bins from b0 = %d lies outside the n = %d bins" % (who, nb, b0, n))
    _range_check(CyclicRefused, who, scale=scale)
    if abs(first) > 1 << 62:
        raise CyclicRefused("%s: first = %d lies beyond +-2^62" % (who, first))


def cyclic(x, win, hop, nframes, nu, y=None, conj=False, first=0, detrend=True, mean_value=None, b0=0, nb=None, scale=1.0, S=True,
           Pp=True, Pm=True):
    """Spectral correlation along the last axis by the averaged cyclic periodogram (sp_cyclic): for every nu (cycles per sample) the
    frames g < nframes of win.size samples at g*hop, Z+ = DFT(win (y - m_y) e(-nu/2 t)), Z- = DFT(win (x' - m_x') e(+nu/2 t)) with
    t = first + the sample's index and x' = conj(x) when conj, and S = scale sum_g Z+ conj(Z-), Pp = scale sum_g |Z+|^2,
    Pm = scale sum_g |Z-|^2 at the nb bins from b0 on (modulo n, two-sided fft order).  y None: y = x.  Returns (S, Pp, Pm):
    complex64, float32, float32 [..., A, nb], None for the ones not asked for.  detrend: True removes each row's mean (computed on the
    device), mean_value a given constant, False nothing.  numpy in -> numpy out; device tensors in -> device tensors on x's stream."""
    hop, nframes, first, b0, scale = int(hop), int(nframes), int(first), int(b0), float(scale)
    w = _win32(win)
    n = int(w.size)
    nuv = np.atleast_1d(np.ascontiguousarray(np.asarray(nu), dtype=np.float64))
    md = _mode(x)
    x = md.checked(x)
    if x.ndim < 1 or w.ndim != 1 or nuv.ndim != 1:
        raise CyclicRefused("cyclic: x needs at least one axis, win and nu exactly one")
    if not np.all(np.isfinite(w)):
        raise CyclicRefused("cyclic: the window must be finite")
    lead, rows = _lead_rows(x.shape)
    nsig, A = int(x.shape[-1]), int(nuv.size)
    nb = n if nb is None else int(nb)
    cyclic_check("cyclic", n, hop, nframes, A, rows, nsig, None, nuv, b0, nb, scale, first)
    if not (S or Pp or Pm):
        raise CyclicRefused("cyclic: no output is asked for")
    y = _second_record("cyclic", CyclicRefused, md, x, y)
    cross = y is not None
    md.bind(x)
    if md.dev and x.ndim != 2:              # the leading axes of a tensor as one: its rows keep their pitch where they have one
        x, y = x.reshape(rows, nsig), y.reshape(rows, nsig) if cross else None
    xs, ys, xld = _paired_rows(md, x, y, nsig)
    outs = [md.empty(lead + (A, nb), dt, xs) if want else None for want, dt in ((S, "complex64"), (Pp, "float32"), (Pm, "float32"))]
    if nframes == 0:                        # a sum over no frames: the library launches nothing and leaves the outputs as they are
        for o in outs:
            if o is not None:
                o[...] = 0
        return tuple(outs)
    means = []
    for v in (xs, ys) if cross else (xs,):
        m = np.zeros(max(rows, 1), dtype=np.complex128)             # (re, im) pairs of float64
        if detrend not in (None, False, 0, "none"):
            if mean_value is not None:
                m[:] = complex(mean_value)
            else:
                _row_means(v, rows, nsig, m)
        means.append(m)
    md.call(lib().sp_cyclic, md.addr(xs), md.addr(ys), md.code(xs), md.code(ys) if cross else md.code(xs), xld, nsig, rows, ptr(w), n, hop,
            nframes, first, ptr(nuv), A, 1 if conj else 0, ptr(means[0]), ptr(means[1]) if cross else None, b0, nb, scale,
            md.addr(outs[0]), md.addr(outs[1]), md.addr(outs[2]))
    return tuple(outs)


def cyclic_plan(n, hop, nframes, A, rows=1, cplx=False, cross=False, conj=False):
    """sp_cyclic_plan as a dict (host only): fpg (frames per group), workgroups (over all passes), alpha_per_pass, passes,
    transforms (per frame and cycle frequency: 1 in the mirrored form, else 2)."""
    n, hop, nframes, A, rows = int(n), int(hop), int(nframes), int(A), int(rows)
    cyclic_check("cyclic_plan", n, hop, nframes, A, rows)
    return _plan(lib().sp_cyclic_plan, ("fpg", "workgroups", "alpha_per_pass", "passes", "transforms"), CyclicRefused, "cyclic_plan",
                 _ffi.DTYPE_C64 if cplx else _ffi.DTYPE_F32, 1 if cross else 0, 1 if conj else 0, n, hop, nframes, A, rows)


LOMB_SUB, LOMB_MAX_M, LOMB_MAX_ROWS, LOMB_PASSES, LOMB_LAUNCHES, LOMB_BAD_RECORD = 256, 1 << 24, 65535, 3, 4, -2
LOMB_NORMALIZE = {"power": 0, "normalize": 1, "amplitude": 2}


class LombRefused(ValueError, NotImplementedError):
    """A record or a frequency list the Lomb-Scargle kernels do not take: outside the limits, values a record must not hold, and what
    is not built (float64 or complex values on the device, rows with times of their own)."""


class LombSums(collections.namedtuple("LombSums", "common rows totals mean t_ref N")):
    """The float64 sums of `lomb_sums`: common [M, 4] = C, S, C2, S2; rows [..., M, 2] = YC', YS' (None without rows); totals
    [1 + 2 rows] = W, then (Y', YY') row by row; and what they were taken with.  The sums of the parts of one record, all taken with
    the same mean, t_ref and wnorm, add up to the whole's: a + b."""
    __slots__ = ()

    def __add__(self, other):
        if not isinstance(other, LombSums):
            return NotImplemented
        if self.t_ref != other.t_ref or not np.array_equal(self.mean, other.mean):
            raise LombRefused("LombSums: the parts were taken with different t_ref or mean")
        rows = None if self.rows is None else self.rows + other.rows
        return LombSums(self.common + other.common, rows, self.totals + other.totals, self.mean, self.t_ref, self.N + other.N)


def _lomb_normalize(who, normalize):
    if isinstance(normalize, (bool, np.bool_)):
        return 1 if normalize else 0
    if isinstance(normalize, str) and normalize in LOMB_NORMALIZE:
        return LOMB_NORMALIZE[normalize]
    if isinstance(normalize, (int, np.integer)) and 0 <= int(normalize) <= 2:
        return int(normalize)
    raise LombRefused("%s: normalize must be 'power' (0, False), 'normalize' (1, True) or 'amplitude' (2), not %r" % (who, normalize))


def lomb_check(who, N, M, rows, y_ld=None, f=None, t_ref=0.0, mean=None):
    """The refusals of sp_lomb, sp_lomb_sums, sp_lomb_finish and sp_lomb_plan, before the library is touched."""
    if N < 1 or N >= 1 << 31:
        raise LombRefused("%s: N = %d samples are outside 1 .. 2^31 - 1" % (who, N))
    if M < 1 or M > LOMB_MAX_M:
        raise LombRefused("%s: M = %d frequencies are outside 1 .. 2^24" % (who, M))
    _range_check(LombRefused, who, rows=(rows, LOMB_MAX_ROWS))
    if y_ld is not None and rows > 0 and y_ld < N:
        raise LombRefused("%s: y_ld = %d is below N = %d" % (who, y_ld, N))
    if f is not None and not np.all(np.isfinite(f)):
        raise LombRefused("%s: every frequency must be finite" % who)
    if not np.isfinite(t_ref):
        raise LombRefused("%s: t_ref must be finite" % who)
    if mean is not None and not np.all(np.isfinite(mean)):
        raise LombRefused("%s: every mean must be finite" % who)


def _lomb_record(who, t, y, f, weights, t_ref, mean_value):
    """The arguments lomb and lomb_sums share, checked: (md, t, w, y rows or None, pitch, lead, N, rows, f, t_ref, mean [rows])."""
    md = _mode(t)
    if y is not None and _mode(y) is not md or weights is not None and _mode(weights) is not md:
        raise TypeError("%s: t, y and weights must all be numpy arrays or all device tensors" % who)
    if _is_torch(f):
        f = f.detach().cpu().numpy()
    fv = np.ascontiguousarray(np.asarray(f), dtype=np.float64)
    if md.dev:
        if t.dtype != torch.float64 or (weights is not None and weights.dtype != torch.float64):
            raise LombRefused("%s: times and weights on the device are float64 tensors" % who)
        if y is not None and y.dtype != torch.float32:
            raise LombRefused("%s: values on the device are float32 tensors, not %s" % (who, y.dtype))
        tv, wv = t.contiguous(), None if weights is None else weights.contiguous()
        tdim, N = tv.dim(), int(tv.shape[-1]) if tv.dim() else 0
    else:
        tv = np.ascontiguousarray(np.asarray(t), dtype=np.float64)
        wv = None if weights is None else np.ascontiguousarray(np.asarray(weights), dtype=np.float64)
        y = None if y is None else np.ascontiguousarray(np.asarray(y), dtype=np.float32)
        tdim, N = tv.ndim, int(tv.shape[-1]) if tv.ndim else 0
    if tdim != 1 or fv.ndim != 1 or (wv is not None and tuple(wv.shape) != tuple(tv.shape)):
        raise LombRefused("%s: t and f need exactly one axis, and weights the shape of t" % who)
    if y is not None and (len(y.shape) < 1 or int(y.shape[-1]) != N):
        raise LombRefused("%s: the last axis of y must have the %d samples of t" % (who, N))
    lead, rows = ((), 0) if y is None else _lead_rows(y.shape)
    if mean_value is not None and (np.size(mean_value) not in (1, rows) or not np.all(np.isfinite(mean_value))):
        raise LombRefused("%s: mean_value must be one finite value, or one per row" % who)
    if N >= 1 and t_ref is None:
        t_ref = float(tv[0])
    lomb_check(who, N, int(fv.size), rows, None, fv, 0.0 if t_ref is None else float(t_ref))
    t_ref = float(t_ref)
    if not md.dev:                          # a record on the device is checked by the kernel that prepares it
        if not np.all(np.isfinite(tv)) or (y is not None and not np.all(np.isfinite(y))):
            raise LombRefused("%s: t and y must be finite" % who)
        if wv is not None and not (np.all(np.isfinite(wv)) and np.all(wv >= 0) and np.sum(wv) > 0):
            raise LombRefused("%s: the weights must be finite, not negative and sum to a positive value" % who)
    md.bind(tv)
    ys, ld = None, N
    if rows:
        ys, ld = md.rows(y.reshape(rows, N) if len(y.shape) != 2 else y)
    mv = np.zeros(rows, dtype=np.float64)
    if mean_value is not None:
        mv[:] = np.asarray(mean_value, dtype=np.float64).reshape(-1) if np.ndim(mean_value) else float(mean_value)
    elif rows:
        _row_means(ys, rows, N, mv)
    lomb_check(who, N, int(fv.size), rows, ld, None, t_ref, mv)
    return md, tv, wv, ys, ld, lead, N, rows, fv, t_ref, mv


def _lomb_call(md, entry, *args):
    """md.call, with the return code of a record the device refused (SP_LOMB_BAD_RECORD) raised as LombRefused"""
    md.init()
    rc = entry(*args, md.mem)
    if rc == LOMB_BAD_RECORD:
        raise LombRefused((lib().sp_last_error() or b"the record was refused").decode())
    check(rc)


def lomb(t, y, f, weights=None, floating_mean=True, normalize="normalize", t_ref=None, mean_value=None):
    """The generalised Lomb-Scargle periodogram of rows y[..., N] sampled at the times t[N] (float64, any order, shared by the rows),
    at the frequencies f[M] in cycles per unit of t (sp_lomb): scipy.signal.lombscargle's definition.  weights: float64 [N], not
    negative.  normalize: 'power', 'normalize' or 'amplitude' (complex).  t_ref: the origin the phases are taken from inside the
    kernel (default t[0]); the result does not depend on it beyond rounding.  mean_value: the offset taken off each row before its
    float32 products are formed and put back in float64 (default: each row's mean, computed on the device).  Returns P [..., M],
    float32 or complex64.  numpy in -> numpy out; device tensors in (t, weights float64, y float32) -> a device tensor on t's stream."""
    nz = _lomb_normalize("lomb", normalize)
    if y is None:
        raise LombRefused("lomb: y is required (lomb_sums takes the window's sums without rows)")
    md, tv, wv, ys, ld, lead, N, rows, fv, t_ref, mv = _lomb_record("lomb", t, y, f, weights, t_ref, mean_value)
    M = int(fv.size)
    P = md.empty(lead + (M,), "complex64" if nz == 2 else "float32", tv)
    if rows:
        _lomb_call(md, lib().sp_lomb, md.addr(tv), md.addr(wv), md.addr(ys), ld, N, rows, t_ref, ptr(fv), M, ptr(mv), 1 if floating_mean else 0,
                   nz, md.addr(P))
    return P


def lomb_sums(t, y, f, weights=None, t_ref=None, mean_value=None, wnorm=None):
    """The float64 sums behind `lomb`, un-finished (sp_lomb_sums), as a LombSums; y None: the sums of the spectral window alone.
    wnorm: what the weights are divided by in place of their own sum -- give every part of a record the whole's weight sum (the
    whole's N for equal weights), the same t_ref and the same mean_value, and the parts' sums add up to the whole's."""
    wn = 0.0 if wnorm is None else float(wnorm)
    if not np.isfinite(wn) or (wnorm is not None and wn <= 0):
        raise LombRefused("lomb_sums: wnorm must be positive and finite")
    md, tv, wv, ys, ld, lead, N, rows, fv, t_ref, mv = _lomb_record("lomb_sums", t, y, f, weights, t_ref, mean_value)
    M = int(fv.size)
    common = md.empty((M, 4), "float64", tv)
    sums = md.empty(lead + (M, 2), "float64", tv) if rows else None
    totals = md.empty((1 + 2 * rows,), "float64", tv)
    _lomb_call(md, lib().sp_lomb_sums, md.addr(tv), md.addr(wv), md.addr(ys), ld, N, rows, t_ref, wn, ptr(fv), M, ptr(mv), md.addr(common),
               md.addr(sums), md.addr(totals))
    return LombSums(common, sums, totals, mv, t_ref, N)


def lomb_finish(sums, f, floating_mean=True, normalize="normalize"):
    """P from a LombSums (sp_lomb_finish): lomb_finish(lomb_sums(t, y, f), f, ...) is bitwise lomb(t, y, f, ...)."""
    nz = _lomb_normalize("lomb_finish", normalize)
    if not isinstance(sums, LombSums) or sums.rows is None:
        raise LombRefused("lomb_finish: the sums of lomb_sums with rows are required")
    md = _mode(sums.rows)
    fv = np.ascontiguousarray(np.asarray(f), dtype=np.float64)
    lead, rows = _lead_rows(sums.rows.shape, 2)
    M = int(fv.size)
    if fv.ndim != 1 or tuple(sums.common.shape) != (M, 4) or int(sums.rows.shape[-2]) != M or md.count(sums.totals) != 1 + 2 * rows:
        raise LombRefused("lomb_finish: the sums do not belong to these %d frequencies" % M)
    mv = np.ascontiguousarray(sums.mean, dtype=np.float64)
    lomb_check("lomb_finish", int(sums.N), M, rows, None, fv, float(sums.t_ref), mv)
    md.bind(sums.rows)
    cm, rw, tt = (md.cast(a, "float64") for a in (sums.common, sums.rows, sums.totals))
    P = md.empty(lead + (M,), "complex64" if nz == 2 else "float32", rw)
    if rows:
        md.call(lib().sp_lomb_finish, md.addr(cm), md.addr(rw), md.addr(tt), int(sums.N), rows, float(sums.t_ref), ptr(fv), M, ptr(mv),
                1 if floating_mean else 0, nz, md.addr(P))
    return P


def lomb_plan(N, M, rows=1):
    """sp_lomb_plan as a dict (host only): rows_per_group, freqs_per_pass, passes, split (sample runs), workgroups."""
    N, M, rows = int(N), int(M), int(rows)
    lomb_check("lomb_plan", N, M, rows)
    return _plan(lib().sp_lomb_plan, ("rows_per_group", "freqs_per_pass", "passes", "split", "workgroups"), LombRefused, "lomb_plan", N, M,
                 rows)


NUFFT_W, NUFFT_TILE, NUFFT_MAX_M, NUFFT_MAX_ROWS, NUFFT_PASSES, NUFFT_BAD_RECORD = 8, 1024, 1 << 24, 65535, 6, -2


class NufftRefused(ValueError, NotImplementedError):
    """A record or a frequency grid the type-1 and type-2 NUFFT do not take: outside the limits, values a record must not hold, and what is
    not built (float64 strengths on the device, rows with times of their own, type 3, more than one dimension)."""


def nufft_check(who, N, M, rows, c_ld=None, t_ref=0.0, f0=0.0, df=1.0, sign=1, Refused=NufftRefused):
    """The refusals of sp_nufft1, sp_lomb_sums_grid and sp_nufft1_plan, before the library is touched."""
    if N < 1 or N >= 1 << 31:
        raise Refused("%s: N = %d samples are outside 1 .. 2^31 - 1" % (who, N))
    if M < 1 or M > NUFFT_MAX_M:
        raise Refused("%s: M = %d frequencies are outside 1 .. 2^24" % (who, M))
    _range_check(Refused, who, rows=(rows, NUFFT_MAX_ROWS))
    if c_ld is not None and rows > 0 and c_ld < N:
        raise Refused("%s: the rows' pitch %d is below N = %d" % (who, c_ld, N))
    if not (np.isfinite(t_ref) and np.isfinite(f0) and np.isfinite(df)) or df == 0 or not np.isfinite(2.0 * (f0 + M * df)):
        raise Refused("%s: t_ref, f0 and df must be finite, df not zero, and f0 + M df within float64" % who)
    if sign not in (1, -1):
        raise Refused("%s: sign must be +1 or -1, not %r" % (who, sign))


def _bad_record_call(md, Refused, entry, *args):
    """md.call, with the return code of a record the device refused (-2) raised as `Refused`"""
    md.init()
    rc = entry(*args, md.mem)
    if rc == NUFFT_BAD_RECORD:
        raise Refused((lib().sp_last_error() or b"the record was refused").decode())
    check(rc)


def nufft1(t, c, f0, df, M, sign=1, t_ref=None):
    """The type-1 NUFFT (sp_nufft1): F[..., m] = sum_j c[..., j] exp(2 pi i sign (f0 + m df) (t_j - t_ref)), m = 0 .. M - 1, of
    complex strengths c[..., N] at the times t[N] (float64, any order, duplicates allowed, shared by the rows).  t_ref: the origin the
    phases are taken from (default t[0]; pass 0.0 for phases from the origin of t itself).  Returns complex64 [..., M]; a permutation
    of the samples changes no bit of it.  numpy in -> numpy out; device tensors in (t float64, c complex64) -> a device tensor."""
    who = "nufft1"
    md = _mode(t)
    if _mode(c) is not md:
        raise TypeError("%s: t and c must both be numpy arrays or both device tensors" % who)
    if md.dev:
        if t.dtype != torch.float64 or c.dtype != torch.complex64:
            raise NufftRefused("%s: on the device times are float64 and strengths complex64 tensors" % who)
        tv = t.contiguous()
        tdim, N = tv.dim(), int(tv.shape[-1]) if tv.dim() else 0
    else:
        tv = np.ascontiguousarray(np.asarray(t), dtype=np.float64)
        c = np.ascontiguousarray(np.asarray(c), dtype=np.complex64)
        tdim, N = tv.ndim, int(tv.shape[-1]) if tv.ndim else 0
    if tdim != 1 or len(c.shape) < 1 or int(c.shape[-1]) != N:
        raise NufftRefused("%s: t needs exactly one axis, and the last axis of c its %d samples" % (who, N))
    f0, df, M, sign = float(f0), float(df), int(M), int(sign) if sign in (1, -1) else sign
    lead, rows = _lead_rows(c.shape)
    if N >= 1 and t_ref is None:
        t_ref = float(tv[0])
    nufft_check(who, N, M, rows, None, 0.0 if t_ref is None else float(t_ref), f0, df, sign)
    t_ref = float(t_ref)
    if not md.dev and not (np.all(np.isfinite(tv)) and np.all(np.isfinite(c))):
        raise NufftRefused("%s: t and c must be finite" % who)
    md.bind(tv)
    out = md.empty(lead + (M,), "complex64", tv)
    if rows:
        cs, ld = md.rows(c.reshape(rows, N) if len(c.shape) != 2 else c)
        nufft_check(who, N, M, rows, ld, t_ref, f0, df, sign)
        _bad_record_call(md, NufftRefused, lib().sp_nufft1, md.addr(tv), md.addr(cs), ld, N, rows, t_ref, f0, df, M, sign, md.addr(out))
    return out


def nufft2(t, F, f0, df, sign=1, t_ref=None):
    """The type-2 NUFFT (sp_nufft2): c[..., j] = sum_m F[..., m] exp(2 pi i sign (f0 + m df) (t_j - t_ref)), j = 0 .. N - 1, of the
    modes F[..., M] (complex, M taken from it) at the times t[N] (float64, any order, duplicates allowed, shared by the rows): the
    adjoint of `nufft1` with the other sign.  t_ref: the origin the phases are taken from (default t[0]; 0.0 for the origin of t
    itself).  Returns complex64 [..., N]; an output depends on its own sample alone, so a permutation of the samples permutes it bit
    for bit.  numpy in -> numpy out; device tensors in (t float64, F complex64) -> a device tensor."""
    who = "nufft2"
    md = _mode(t)
    if _mode(F) is not md:
        raise TypeError("%s: t and F must both be numpy arrays or both device tensors" % who)
    if md.dev:
        if t.dtype != torch.float64 or F.dtype != torch.complex64:
            raise NufftRefused("%s: on the device times are float64 and modes complex64 tensors" % who)
        tv = t.contiguous()
        tdim, N = tv.dim(), int(tv.shape[-1]) if tv.dim() else 0
    else:
        tv = np.ascontiguousarray(np.asarray(t), dtype=np.float64)
        F = np.ascontiguousarray(np.asarray(F), dtype=np.complex64)
        tdim, N = tv.ndim, int(tv.shape[-1]) if tv.ndim else 0
    if tdim != 1 or len(F.shape) < 1:
        raise NufftRefused("%s: t needs exactly one axis, and F at least one: its last holds the modes" % who)
    M = int(F.shape[-1])
    f0, df, sign = float(f0), float(df), int(sign) if sign in (1, -1) else sign
    lead, rows = _lead_rows(F.shape)
    if N >= 1 and t_ref is None:
        t_ref = float(tv[0])
    nufft_check(who, N, M, rows, None, 0.0 if t_ref is None else float(t_ref), f0, df, sign)
    t_ref = float(t_ref)
    if not md.dev and not (np.all(np.isfinite(tv)) and np.all(np.isfinite(F))):
        raise NufftRefused("%s: t and F must be finite" % who)
    md.bind(tv)
    out = md.empty(lead + (N,), "complex64", tv)
    if rows:
        Fs, ld = md.rows(F.reshape(rows, M) if len(F.shape) != 2 else F)
        if ld < M:
            raise NufftRefused("%s: the rows' pitch %d is below M = %d" % (who, ld, M))
        _bad_record_call(md, NufftRefused, lib().sp_nufft2, md.addr(tv), md.addr(Fs), ld, N, rows, t_ref, f0, df, M, sign, md.addr(out), N)
    return out


def nufft2_plan(N, M, rows=1):
    """sp_nufft2_plan as a dict (host only): nf (fine-grid cells), width (kernel cells), tiles, tile (cells of one), rows_per_pass,
    passes, workgroups (of the interpolation kernel), row_group (rows a workgroup stages)."""
    N, M, rows = int(N), int(M), int(rows)
    nufft_check("nufft2_plan", N, M, rows)
    return _plan(lib().sp_nufft2_plan, ("nf", "width", "tiles", "tile", "rows_per_pass", "passes", "workgroups", "row_group"),
                 NufftRefused, "nufft2_plan", N, M, rows)


def lomb_sums_grid(t, y, f0, df, M, weights=None, t_ref=None, mean_value=None, wnorm=None):
    """`lomb_sums` at the frequencies f0 + m df, m = 0 .. M - 1, by three type-1 NUFFTs (sp_lomb_sums_grid): O(N + M log M) in place of
    O(N M).  The LombSums differ from lomb_sums' by rounding only, go to `lomb_finish` unchanged and add up like them; the totals
    are bitwise lomb_sums'.  A permutation of the samples changes no bit of common and rows, given equal weights or a wnorm and a
    mean_value."""
    who = "lomb_sums_grid"
    wn = 0.0 if wnorm is None else float(wnorm)
    if not np.isfinite(wn) or (wnorm is not None and wn <= 0):
        raise LombRefused("%s: wnorm must be positive and finite" % who)
    f0, df, M = float(f0), float(df), int(M)
    nufft_check(who, 1, M, 0, None, 0.0, f0, df, 1, LombRefused)           # the grid, before the record is looked at
    md, tv, wv, ys, ld, lead, N, rows, _, t_ref, mv = _lomb_record(who, t, y, np.array([f0, df]), weights, t_ref, mean_value)
    nufft_check(who, N, M, rows, ld, t_ref, f0, df, 1, LombRefused)
    common = md.empty((M, 4), "float64", tv)
    sums = md.empty(lead + (M, 2), "float64", tv) if rows else None
    totals = md.empty((1 + 2 * rows,), "float64", tv)
    _bad_record_call(md, LombRefused, lib().sp_lomb_sums_grid, md.addr(tv), md.addr(wv), md.addr(ys), ld, N, rows, t_ref, wn, f0, df, M, ptr(mv),
                     md.addr(common), md.addr(sums), md.addr(totals))
    return LombSums(common, sums, totals, mv, t_ref, N)


def nufft_plan(N, M, rows=1):
    """sp_nufft1_plan as a dict (host only): nf (fine-grid cells), width (kernel cells), tiles, tile (cells of one), rows_per_pass,
    passes, workgroups (of the spread kernel), fast_min_pairs (the N M from which ls_periodogram's method='auto' takes the fast path)."""
    N, M, rows = int(N), int(M), int(rows)
    nufft_check("nufft_plan", N, M, rows)
    return _plan(lib().sp_nufft1_plan, ("nf", "width", "tiles", "tile", "rows_per_pass", "passes", "workgroups", "fast_min_pairs"),
                 NufftRefused, "nufft_plan", N, M, rows)


WBIC_MAX_S, WBIC_MAX_M, WBIC_TILE, WBIC_GROUP = 512, 3072, 64, 2048
WBIC_OUT_BYTES, WBIC_ACC_BYTES = 1 << 30, 2 << 30


class WbicRefused(ValueError, NotImplementedError):
    """A shape the wavelet bispectrum does not take: outside the limits, and what is not built (scales whose margin is above 3072 samples
    -- there is no composed path here --, leading axes, blocks that neither tile nor overlap in whole steps, wavelets that are not analytic)."""


def wbic_check(who, nsig, scales, k_lo, family, param, L, M, n0, block, step, nblocks, nrec=1, sym=True):
    """Every refusal of sp_wbic's shape, before the library is touched -> (scales float64, family code, param)."""
    nsig, k_lo, L, M, n0, block, step, nblocks = (int(v) for v in (nsig, k_lo, L, M, n0, block, step, nblocks))
    sc = np.ascontiguousarray(np.asarray(scales, dtype=np.float64))
    if sc.ndim != 1 or sc.size < 2 or sc.size > WBIC_MAX_S:
        raise WbicRefused("%s: scales must be one-dimensional and hold 2 .. %d scales" % (who, WBIC_MAX_S))
    S = int(sc.size)
    if k_lo < 1 or k_lo > S - 1:
        raise WbicRefused("%s: k_lo = %d must lie in 1 .. S - 1 = %d (beyond it no pair is valid)" % (who, k_lo, S - 1))
    if not np.all(np.isfinite(sc)) or not np.all(sc > 0) or np.any(sc > 1e9):
        raise WbicRefused("%s: every scale must be positive and finite" % who)
    _range_check(WbicRefused, who, length=("L", L, CWT_MIN_L, CWT_MAX_L))
    if M > WBIC_MAX_M:
        raise WbicRefused("%s: M = %d is above %d: a scale does not fuse, and there is no composed path here" % (who, M, WBIC_MAX_M))
    if M < 0 or 2 * M >= L or L - 2 * M < L // 4:
        raise WbicRefused("%s: M = %d must lie in 0 .. L / 2 - 1 and leave hop = L - 2 M at L / 4 = %d or more" % (who, M, L // 4))
    if not isinstance(family, str) or family.lower() not in CWT_FAMILIES:
        raise WbicRefused("%s: family %r is not built: 'morlet' or 'paul' (analytic wavelets)" % (who, family))
    param = float(param)
    code = CWT_FAMILIES[family.lower()]
    if not np.isfinite(param) or not (0.0 < param <= 64.0) or (code == _ffi.CWT_PAUL and param < 1.0):
        raise WbicRefused("%s: the %s parameter %r is outside (0, 64] (Morlet's w0) or [1, 64] (Paul's m)" % (who, family, param))
    if nsig < 1:
        raise WbicRefused("%s: the record must hold at least one sample" % who)
    if nrec < 1 or nrec > 3:
        raise WbicRefused("%s: 1 .. 3 distinct records" % who)
    if block < 1 or step < 1:
        raise WbicRefused("%s: block = %d and step = %d must be at least 1" % (who, block, step))
    if step < block and block % step:
        raise WbicRefused("%s: either step >= block (disjoint blocks) or block %% step == 0 (overlapping blocks); block %d, step %d"
                          % (who, block, step))
    if nblocks < 1:
        raise WbicRefused("%s: nblocks = %d must be at least 1" % (who, nblocks))
    if nblocks * S * S * 24 > WBIC_OUT_BYTES:
        raise WbicRefused("%s: %d blocks of %d x %d pairs are above 1 GiB of B and b2" % (who, nblocks, S, S))
    if n0 < 0 or n0 + (nblocks - 1) * step + block > nsig:
        raise WbicRefused("%s: %d blocks of %d samples at step %d from %d on reach outside the %d samples of the record"
                          % (who, nblocks, block, step, n0, nsig))
    cpb = block // step if step < block else 1
    ntd = -(-S // WBIC_TILE)
    tiles = ntd * (ntd + 1) // 2 if sym else ntd * ntd
    if (nblocks - 1 + cpb) * tiles * 8 * 3 * WBIC_TILE * WBIC_TILE > WBIC_ACC_BYTES:
        raise WbicRefused("%s: the float64 sums of %d cells and %d tiles are above 2 GiB" % (who, nblocks - 1 + cpb, tiles))
    return sc, code, param


def _wbic_records(who, md, x, y, z):
    """-> [x, y, z] as contiguous samples, the same object where they are the same record (None and x itself mean x)"""
    xs = md.samples(x)
    if xs.ndim != 1:
        raise WbicRefused("%s: one record per call: leading axes are not built" % who)
    out = [xs]
    for v, earlier in ((y, ((x, 0),)), (z, ((x, 0), (y, 1)))):
        same = [k for w, k in earlier if v is w]
        if v is None or same:
            out.append(out[same[0]] if same else xs)
            continue
        if _mode(v) is not md:
            raise TypeError("%s: the records must all be numpy arrays or all device tensors" % who)
        vs = md.samples(v)
        if tuple(vs.shape) != tuple(xs.shape) or not md.alike(xs, vs):
            raise WbicRefused("%s: the records must share x's %s" % (who, md.ALIKE))
        out.append(vs)
    return out


def wbic(x, scales, k_lo, family, param, L, M, n0, block, step, nblocks, y=None, z=None):
    """Wavelet bispectrum of one record, or of a triple of records (sp_wbic): the rows i of `scales` (in samples) stand for the frequencies
    (k_lo + i) df, block b covers the `block` samples from n0 + b step on, and over it
        B[b, i, j] = mean_n Wx[i, n] Wy[j, n] conj(Wz[m, n]),  m = i + j + k_lo,   b2 = |B|^2 / (mean |Wx Wy|^2 mean |Wz[m]|^2),
        P[b, m] = mean_n |Wz[m, n]|^2
    with W the transforms `cwt` defines (family, param, frames of L samples with margin M).  y and z default to x; a record given
    twice (the same object) is transformed once.  Returns a dict: 'B' complex128 [nblocks, S, S] and 'b2' float64 (NaN where
    m > S - 1), 'P' float64 [nblocks, S], 'passes' the passes over the record the call made.  numpy in -> numpy out; device tensors
    in -> device tensors on x's stream."""
    md = _mode(x)
    xs, ys, zs = _wbic_records("wbic", md, x, y, z)
    nsig = int(xs.shape[-1])
    nrec = 1 + (ys is not xs) + (zs is not xs and zs is not ys)
    sc, code, param = wbic_check("wbic", nsig, scales, k_lo, family, param, L, M, n0, block, step, nblocks, nrec, ys is xs)
    S, nblocks = int(sc.size), int(nblocks)
    md.bind(xs)
    B = md.empty((nblocks, S, S), "complex128", xs)
    b2 = md.empty((nblocks, S, S), "float64", xs)
    P = md.empty((nblocks, S), "float64", xs)
    passes = _ffi.C.c_int(0)
    md.call(lib().sp_wbic, md.addr(xs), None if ys is xs else md.addr(ys), None if zs is xs else md.addr(zs), md.code(xs), md.code(ys),
            md.code(zs), nsig, ptr(sc), S, int(k_lo), code, param, int(L), int(M), int(n0), int(block), int(step), nblocks, md.addr(B),
            md.addr(b2), md.addr(P), _ffi.C.byref(passes))
    return dict(B=B, b2=b2, P=P, passes=int(passes.value))


def wbic_plan(nsig, nscales, k_lo, L, M, n0, block, step, nblocks, nrec=1, sym=True):
    """sp_wbic_plan as a dict (host only): cells, cell_len (samples of a cell), groups, passes, workgroups (of the tile kernel, over all
    passes), scratch (bytes: transforms, partials and cell sums), chunk (samples a pass may span), tiles."""
    wbic_check("wbic_plan", nsig, np.ones(max(int(nscales), 0)), k_lo, "morlet", 6.0, L, M, n0, block, step, nblocks, int(nrec), bool(sym))
    return _plan(lib().sp_wbic_plan, ("cells", "cell_len", "groups", "passes", "workgroups", "scratch", "chunk", "tiles"), WbicRefused,
                 "wbic_plan", int(nsig), int(nscales), int(k_lo), int(L), int(M), int(n0), int(block), int(step), int(nblocks), int(nrec),
                 1 if sym else 0)


FAM_MIN_N, FAM_MAX_N, FAM_MAX_PAIRS, FAM_PASSES, FAM_ACC_BYTES = 32, 8192, 1 << 22, 5, 2 << 30


class FamRefused(ValueError, NotImplementedError):
    """A shape the FFT accumulation method does not take: outside the limits, and what is not built (channel counts, block lengths and
    hops that are no power of two, hop above the channel count, leading axes)."""


def fam_check(who, np_, hop, P, nblocks, npairs, nsig=None, pairs=None, scale=1.0):
    """The refusals of sp_fam and sp_fam_plan, before the library is touched -> Q."""
    _range_check(FamRefused, who, ("np", np_, FAM_MIN_N, FAM_MAX_N))
    _range_check(FamRefused, who, ("P", P, FAM_MIN_N, FAM_MAX_N))
    if hop < 1 or hop > np_ or hop & (hop - 1):
        raise FamRefused("%s: hop = %d must be a power of two from 1 to np = %d" % (who, hop, np_))
    if P * hop < 2 * np_:
        raise FamRefused("%s: P hop = %d is below 2 np = %d: no bin lies within half a channel spacing" % (who, P * hop, 2 * np_))
    _range_check(FamRefused, who, count=("nblocks", nblocks))
    if nsig is not None and nblocks > 0 and (nsig < np_ or nblocks * P > (nsig - np_) // hop + 1):
        raise FamRefused("%s: nblocks = %d blocks of %d frames of %d at hop %d reach outside the nsig = %d samples of the row"
                         % (who, nblocks, P, np_, hop, nsig))
    if npairs < 1 or npairs > FAM_MAX_PAIRS:
        raise FamRefused("%s: npairs = %d is outside 1 .. 2^22" % (who, npairs))
    if pairs is not None and (pairs.min() < 0 or pairs.max() >= np_):
        raise FamRefused("%s: a channel of pairs lies outside 0 .. np - 1 = %d" % (who, np_ - 1))
    _range_check(FamRefused, who, scale=scale)
    return P * hop // (2 * np_)


def fam(x, a, hop, g, nblocks, pairs, y=None, conj=False, detrend=True, mean_value=None, scale=1.0, S=True, Pw=True):
    """The FFT accumulation method on one record, or one pair of records (sp_fam): the channelizer window a (np taps) at step hop, the
    taper g (P taps) over the frames of a block, nblocks disjoint blocks of P frames, and for every pair (k, l) of pairs[npairs, 2]
        S[i, j] = scale sum_b sum_p g[p] Y[bP + p, k] conj(X[bP + p, l]) e(-(j - Q) p / P),  j < 2Q,  Q = P hop / (2 np)
    with X, Y the channelizer outputs demodulated to absolute time (conj: X without the conjugate), Pwx[k] = scale sum g |X[., k]|^2
    and Pwy alike.  y None: y = x.  Returns (S complex64 [npairs, 2Q], Pwx, Pwy float32 [np]), None for what was not asked for (Pw
    asks for both powers).  detrend: True removes the record's mean (computed on the device), mean_value a given constant (a pair
    (mx, my) in the cross form), False nothing.  numpy in -> numpy out; device tensors in -> device tensors on x's stream."""
    hop, nblocks, scale = int(hop), int(nblocks), float(scale)
    aw, gw = _win32(a), _win32(g)
    pr = np.ascontiguousarray(np.asarray(pairs), dtype=np.int32)
    md = _mode(x)
    x = md.checked(x)
    if x.ndim != 1:
        raise FamRefused("fam: x must be one record: leading axes are not built")
    if aw.ndim != 1 or gw.ndim != 1 or pr.ndim != 2 or pr.shape[1] != 2:
        raise FamRefused("fam: a and g need exactly one axis, pairs the shape [npairs, 2]")
    if not (np.all(np.isfinite(aw)) and np.all(np.isfinite(gw))):
        raise FamRefused("fam: the windows a and g must be finite")
    n, P, nsig, npairs = int(aw.size), int(gw.size), int(x.shape[-1]), int(pr.shape[0])
    Q = fam_check("fam", n, hop, P, nblocks, npairs, nsig, pr if npairs else None, scale)
    if not (S or Pw):
        raise FamRefused("fam: no output is asked for")
    y = _second_record("fam", FamRefused, md, x, y)
    cross = y is not None
    md.bind(x)
    xs = md.samples(x)
    ys = md.samples(y) if cross else None
    means = []
    for i, v in enumerate((xs, ys) if cross else (xs,)):
        m = np.zeros(1, dtype=np.complex128)
        if detrend not in (None, False, 0, "none"):
            if mean_value is not None:
                m[0] = complex(mean_value[i] if isinstance(mean_value, (tuple, list)) else mean_value)
            else:
                m[0] = mean(v)
        if not np.isfinite(m[0]):
            raise FamRefused("fam: the mean of the record is not finite")
        means.append(m)
    outs = [md.empty((npairs, 2 * Q), "complex64", xs) if S else None, md.empty(n, "float32", xs) if Pw else None,
            md.empty(n, "float32", xs) if Pw else None]
    if nblocks == 0:                        # a sum over no blocks: the library launches nothing and leaves the outputs as they are
        for o in outs:
            if o is not None:
                o[...] = 0
        return tuple(outs)
    md.call(lib().sp_fam, md.addr(xs), md.addr(ys), md.code(xs), nsig, ptr(aw), n, hop, ptr(gw), P, nblocks, ptr(pr), npairs,
            1 if conj else 0, ptr(means[0]), ptr(means[1]) if cross else None, scale, md.addr(outs[0]), md.addr(outs[1]), md.addr(outs[2]))
    return tuple(outs)


def fam_plan(np_, hop, P, nblocks, npairs, cplx=False, cross=False):
    """sp_fam_plan as a dict (host only): Q, blocks_per_pass, passes, workgroups (of the pair kernel, over all passes), scratch (bytes of
    the bin-major frames of a pass)."""
    np_, hop, P, nblocks, npairs = int(np_), int(hop), int(P), int(nblocks), int(npairs)
    fam_check("fam_plan", np_, hop, P, nblocks, npairs)
    return _plan(lib().sp_fam_plan, ("Q", "blocks_per_pass", "passes", "workgroups", "scratch"), FamRefused, "fam_plan",
                 _ffi.DTYPE_C64 if cplx else _ffi.DTYPE_F32, 1 if cross else 0, np_, hop, P, nblocks, npairs)


AR_MAX_ORDER, BURG_MAX_N, BURG_WAVE_MAX, YULE_MAX_N, AR_PASSES, AR_BAD_RECORD = 256, 16384, 1024, (1 << 31) - 1, 7, -2
AR_METHODS = {"burg": 0, "yule": 1}


class ArRefused(ValueError, NotImplementedError):
    """A segment, an order or a model the autoregressive fits and spectra do not take: outside the limits, values a record must not
    hold, and what is not built (a Burg fit of a segment beyond 16384 samples, orders beyond 256, float64 samples)."""


def ar_check(who, method, n, hop, first, nframes, order, rows, nsig=None, x_ld=None, mean=0j):
    """The refusals of sp_burg, sp_yule and sp_ar_plan, before the library is touched."""
    if method not in (0, 1):
        raise ArRefused("%s: method must be 0 (Burg) or 1 (Yule-Walker)" % who)
    if order < 1 or order > AR_MAX_ORDER:
        raise ArRefused("%s: order = %d is outside 1 .. %d" % (who, order, AR_MAX_ORDER))
    most = BURG_MAX_N if method == 0 else YULE_MAX_N
    if n < 2 or n > most:
        raise ArRefused("%s: n = %d samples of a segment are outside 2 .. %d" % (who, n, most))
    if order > n // 2:
        raise ArRefused("%s: order = %d exceeds n / 2 = %d" % (who, order, n // 2))
    _frames_check(ArRefused, who, n, hop, first, nframes, rows, nsig, x_ld, mean)


def _ar_detrend(who, detrend, mean_value, Refused):
    """-> (the C ABI's detrend code, the constant): True every segment's own mean, or with an explicit mean_value that constant; False
    or None nothing, and then a mean_value is refused"""
    flag = isinstance(detrend, (bool, np.bool_))
    if detrend is None or (flag and not detrend):
        if mean_value is not None:
            raise Refused("%s: mean_value = %r is given, but detrend is off" % (who, mean_value))
        return _ffi.DETREND_CONST, 0j
    if not flag:
        raise Refused("%s: detrend must be True (every segment's own mean, or mean_value) or False, not %r" % (who, detrend))
    if mean_value is not None:
        return _ffi.DETREND_CONST, complex(mean_value)
    return _ffi.DETREND_SEGMEAN, 0j


def _ar_fit(who, method, x, n, hop, first, nframes, order, detrend, mean_value):
    n, hop, first, nframes, order = int(n), int(hop), int(first), int(nframes), int(order)
    md, xs, xld, nsig, rows, lead, cplx, code, mean = _framed_record(
        who, ArRefused, x, detrend, mean_value, lambda rows, nsig, mean: ar_check(who, method, n, hop, first, nframes, order, rows, nsig, None, mean))
    dt = "complex128" if cplx else "float64"
    a = md.empty(lead + (nframes, order + 1), dt, xs)
    e = md.empty(lead + (nframes, order + 1), "float64", xs)
    k = md.empty(lead + (nframes, order + 1), dt, xs)               # the three share one pitch: k is handed out as a view of order columns
    if rows * nframes:
        _bad_record_call(md, ArRefused, lib().sp_burg if method == 0 else lib().sp_yule, md.addr(xs), md.code(xs), xld, nsig, rows, n, hop,
                         first, nframes, order, code, mean.real, mean.imag, md.addr(a), md.addr(e), md.addr(k), order + 1)
    return a, e, k[..., :order]


def burg(x, n, hop, first, nframes, order, detrend=True, mean_value=None):
    """Burg's autoregressive fit (sp_burg; MATLAB's arburg) of the segments x[..., first + g hop + i], i < n, g < nframes, of every row:
    -> (a, evar, k): the polynomial a[..., g, 0 .. order] with a[..., 0] = 1, the prediction-error power by order evar[..., g, 0 .. order]
    and the reflection coefficients k[..., g, 0 .. order - 1]; float64 for float32 rows, complex128 (evar float64) for complex64 rows.
    detrend: True every segment's own mean, mean_value a given constant, False nothing.  n <= 16384, order <= 256 and <= n / 2.
    numpy in -> numpy out; device tensors in -> device tensors on x's stream; the two agree bitwise."""
    return _ar_fit("burg", 0, x, n, hop, first, nframes, order, detrend, mean_value)


def yule(x, n, hop, first, nframes, order, detrend=True, mean_value=None):
    """The Yule-Walker fit (sp_yule; MATLAB's aryule) of the same segments as `burg`, from the biased lags by Levinson-Durbin:
    the same triple.  n up to 2^31 - 1."""
    return _ar_fit("yule", 1, x, n, hop, first, nframes, order, detrend, mean_value)


def ar_psd(a, e, m, start, step, scale=1.0, out64=False):
    """The spectra of all-pole models (sp_ar_psd): P[..., q] = scale e[...] / |sum_j a[..., j] exp(-2 pi i j (start + q step))|^2,
    q = 0 .. m - 1, frequencies in cycles per sample (the start, step, m of `czt`).  a[..., order + 1] float64 or complex128, e[...]
    float64 of a's leading shape.  float32 [..., m], or float64 with out64.  e == 0 gives zeros; a row padded with zeros is a model of
    lower order.  numpy in -> numpy out; device tensors in -> a device tensor."""
    who = "ar_psd"
    m, start, step, scale = int(m), float(start), float(step), float(scale)
    md = _enter(a)
    if _mode(e) is not md:
        raise TypeError("%s: a and e must both be numpy arrays or both device tensors" % who)
    if md.dev:
        if a.dtype not in (torch.float64, torch.complex128) or e.dtype != torch.float64:
            raise ArRefused("%s: on the device a is a float64 or complex128 tensor and e float64" % who)
        a, e = a.contiguous(), e.contiguous()
        cplx = a.dtype == torch.complex128
    else:
        a = np.asarray(a)
        cplx = np.iscomplexobj(a)
        a = np.ascontiguousarray(a, dtype=np.complex128 if cplx else np.float64)
        e = np.ascontiguousarray(np.asarray(e), dtype=np.float64)
    if len(a.shape) < 1 or tuple(a.shape[:-1]) != tuple(e.shape):
        raise ArRefused("%s: a needs at least one axis and e the shape of a's leading axes" % who)
    order = int(a.shape[-1]) - 1
    if order < 0 or order > AR_MAX_ORDER:
        raise ArRefused("%s: %d coefficients are outside 1 .. %d" % (who, order + 1, AR_MAX_ORDER + 1))
    if m < 1 or m > (1 << 31) - 1:
        raise ArRefused("%s: m = %d bins are outside 1 .. 2^31 - 1" % (who, m))
    if not (math.isfinite(start) and math.isfinite(step) and math.isfinite(scale)):
        raise ArRefused("%s: start, step and scale must be finite" % who)
    lead, models = _lead_rows(a.shape)
    if models * -(-m // 256) > (1 << 31) - 1:
        raise ArRefused("%s: %d models of %d bins are more than one launch takes" % (who, models, m))
    if not md.dev and not (np.all(np.isfinite(a)) and np.all(np.isfinite(e))):
        raise ArRefused("%s: a and e must be finite" % who)
    P = md.empty(lead + (m,), "float64" if out64 else "float32", a)
    if models:
        md.call(lib().sp_ar_psd, md.addr(a), 1 if cplx else 0, order + 1, md.addr(e), 1, order, models, m, start, step, scale,
                1 if out64 else 0, md.addr(P), m)
    return P


def ar_plan(method, n, order, rows=1, nframes=1, cplx=False):
    """sp_ar_plan as a dict (host only): form (0 the wave form of k_burg, 1 its workgroup form, 2 lags and Levinson), segs_per_wg,
    samples (per lane of k_burg, or per tile of the lags), lds_bytes, workgroups (over all passes), passes, threads, tiles."""
    method = AR_METHODS.get(method, method)
    n, order, rows, nframes = int(n), int(order), int(rows), int(nframes)
    ar_check("ar_plan", method, n, 1, 0, nframes, order, rows)
    return _plan(lib().sp_ar_plan, ("form", "segs_per_wg", "samples", "lds_bytes", "workgroups", "passes", "threads", "tiles"), ArRefused,
                 "ar_plan", method, _ffi.DTYPE_C64 if cplx else _ffi.DTYPE_F32, n, order, rows, nframes)


SUB_MAX_M, SUB_PASSES = 64, 8
SUB_WHAT = {"covmat": 0, "ls": 1}
SUB_WEIGHTINGS = {"music": 0, "ev": 1}


class SubRefused(ValueError, NotImplementedError):
    """A segment, a matrix order, a signal dimension or an eigendecomposition the covariance matrices, the covariance least-squares
    fits and the pseudospectra do not take: outside the limits, values a record must not hold, and what is not built (m above 64)."""


def sub_check(who, what, n, hop, first, nframes, m, rows, nsig=None, mean=0j):
    """The refusals of sp_covmat, sp_ar_ls and sp_sub_plan about the record and the matrix order m (order + 1 for a fit), before the
    library is touched."""
    if what not in (0, 1):
        raise SubRefused("%s: what must be 0 (covmat) or 1 (the least-squares fit)" % who)
    if what == 1 and (m < 2 or m > SUB_MAX_M):
        raise SubRefused("%s: order = %d is outside 1 .. %d" % (who, m - 1, SUB_MAX_M - 1))
    if m < 2 or m > SUB_MAX_M:
        raise SubRefused("%s: m = %d is outside 2 .. %d" % (who, m, SUB_MAX_M))
    if n < 2 or n > YULE_MAX_N:
        raise SubRefused("%s: n = %d samples of a segment are outside 2 .. %d" % (who, n, YULE_MAX_N))
    if what == 1 and m - 1 > n // 2:
        raise SubRefused("%s: order = %d exceeds n / 2 = %d" % (who, m - 1, n // 2))
    if m > n:
        raise SubRefused("%s: m = %d exceeds n = %d" % (who, m, n))
    _frames_check(SubRefused, who, n, hop, first, nframes, rows, nsig, None, mean)


def _sub_record(who, what, x, n, hop, first, nframes, m, detrend, mean_value):
    """the record of `covmat` and `ar_ls`: `_framed_record`, judged by `sub_check`"""
    return _framed_record(who, SubRefused, x, detrend, mean_value,
                          lambda rows, nsig, mean: sub_check(who, what, n, hop, first, nframes, m, rows, nsig, mean))


def covmat(x, n, hop, first, nframes, m, fb=True, detrend=True, mean_value=None):
    """The m x m data covariance matrices (sp_covmat) of the segments x[..., first + g hop + t], t < n, g < nframes, of every row:
    C[i,j] = (1 / N) sum_{t=m-1}^{n-1} conj(s[t-i]) s[t-j], N = n - m + 1 (fb=False: MATLAB's corrmtx(.., 'covariance') as X'X), or
    its forward-backward average (C + J conj(C) J) / 2 (fb=True: 'modified').  -> C[..., g, m, m] complex128, exactly Hermitian,
    what `eigh` takes.  2 <= m <= 64, m <= n.  The detrended samples stay float64 and every sum is float64 in a fixed order.
    detrend as for `burg`.  numpy in -> numpy out; device tensors in -> a device tensor on x's stream; the two agree bitwise."""
    who = "covmat"
    n, hop, first, nframes, m = int(n), int(hop), int(first), int(nframes), int(m)
    md, xs, xld, nsig, rows, lead, cplx, code, mean = _sub_record(who, 0, x, n, hop, first, nframes, m, detrend, mean_value)
    C = md.empty(lead + (nframes, m, m), "complex128", xs)
    if rows * nframes:
        _bad_record_call(md, SubRefused, lib().sp_covmat, md.addr(xs), md.code(xs), xld, nsig, rows, n, hop, first, nframes, m, 1 if fb else 0, code,
                         mean.real, mean.imag, md.addr(C), m * m)
    return C


def ar_ls(x, n, hop, first, nframes, order, fb=False, detrend=True, mean_value=None, check=True):
    """The covariance (fb=False, MATLAB's arcov) or modified-covariance (fb=True, armcov) least-squares fit (sp_ar_ls) of the segments
    of `covmat`: with C at m = order + 1, sum_j C[i,j] a_j = -C[i,0], i, j = 1 .. order, by Cholesky -> (a, e, status):
    a[..., g, 0 .. order] with a[..., 0] = 1 (float64 for float32 rows, complex128 for complex64 rows), e[..., g] =
    Re(C[0,0] + sum_j C[0,j] a_j) and status[..., g] int32: 0, or the 1-based index of the first pivot at or below m 2^-52 C[j,j]
    (then a = (1, 0 ..) and e = 0).  order <= 63 and <= n / 2.  check=True reads status back and raises numpy.linalg.LinAlgError
    naming the first singular model, as `eigh` does.  numpy in -> numpy out; device tensors in -> device tensors, the same bits."""
    who = "ar_ls"
    n, hop, first, nframes, order = int(n), int(hop), int(first), int(nframes), int(order)
    md, xs, xld, nsig, rows, lead, cplx, code, mean = _sub_record(who, 1, x, n, hop, first, nframes, order + 1, detrend, mean_value)
    a = md.empty(lead + (nframes, order + 1), "complex128" if cplx else "float64", xs)
    e = md.empty(lead + (nframes,), "float64", xs)
    st = md.empty(lead + (nframes,), "int32", xs)
    if rows * nframes:
        _bad_record_call(md, SubRefused, lib().sp_ar_ls, md.addr(xs), md.code(xs), xld, nsig, rows, n, hop, first, nframes, order, 1 if fb else 0, code,
                         mean.real, mean.imag, md.addr(a), md.addr(e), md.addr(st), order + 1)
    if check and rows * nframes:                                    # (the read-back of a device tensor waits for the stream)
        bad = (st.reshape(-1).cpu().numpy() if md.dev else st.reshape(-1)) > 0
        if bad.any():
            i = int(np.argmax(bad))
            raise np.linalg.LinAlgError("ar_ls: model %s (flat index %d) is singular: no positive pivot at row %d of %d"
                                        % (np.unravel_index(i, lead + (nframes,)), i, int(st.reshape(-1)[i]), order))
    return a, e, st


def pseudospectrum(V, w, p, nbins, start, step, weighting="music", out64=False):
    """The MUSIC (weighting='music') or eigenvector (weighting='ev') pseudospectrum (sp_pseudospectrum) of the eigendecompositions
    V[..., m, m] complex128, w[..., m] float64 descending, as `eigh` returns them, with signal dimension 0 <= p < m:
    P[..., q] = 1 / sum_{k >= p} g_k |sum_i V[..., i, k] exp(-2 pi i nu_q i)|^2 at nu_q = start + q step cycles per sample, g_k = 1
    or 1 / w_k (g_k = 0 and status 1 where w_k <= 0) -> (P float32 [..., nbins], or float64 with out64; status int32 [...]).
    numpy in -> numpy out; device tensors in -> device tensors."""
    who = "pseudospectrum"
    p, nbins, start, step = int(p), int(nbins), float(start), float(step)
    if weighting not in SUB_WEIGHTINGS:
        raise SubRefused("%s: weighting must be 'music' or 'ev', not %r" % (who, weighting))
    md, V, w, shape, m = _eigen_models(who, SubRefused, V, w)
    if m < 2 or m > SUB_MAX_M:
        raise SubRefused("%s: m = %d is outside 2 .. %d" % (who, m, SUB_MAX_M))
    if p < 0 or p > m - 1:
        raise SubRefused("%s: p = %d is outside 0 .. m - 1 = %d" % (who, p, m - 1))
    if nbins < 1 or nbins > (1 << 31) - 1:
        raise SubRefused("%s: nbins = %d is outside 1 .. 2^31 - 1" % (who, nbins))
    if not (math.isfinite(start) and math.isfinite(step)):
        raise SubRefused("%s: start and step must be finite" % who)
    lead, models = _lead_rows(shape, 2)
    if models * -(-nbins // 256) > (1 << 31) - 1:
        raise SubRefused("%s: %d models of %d bins are more than one launch takes" % (who, models, nbins))
    if not md.dev and not (np.all(np.isfinite(V)) and np.all(np.isfinite(w))):
        raise SubRefused("%s: V and w must be finite" % who)
    P = md.empty(lead + (nbins,), "float64" if out64 else "float32", V)
    st = md.empty(lead, "int32", V)
    if models:
        md.call(lib().sp_pseudospectrum, md.addr(V), m, md.addr(w), m, p, models, SUB_WEIGHTINGS[weighting], nbins, start, step, 1 if out64 else 0,
                md.addr(P), nbins, md.addr(st))
    return P, st


def sub_plan(what, n, m, rows=1, nframes=1, cplx=False):
    """sp_sub_plan as a dict (host only): what 'covmat' or 'ls' (m = order + 1) -> chunk (samples of a tile), tiles, shares (of a stage
    of k_cov_row), lds_bytes, workgroups (of k_cov_row over all passes), passes, seg_bytes (scratch of a segment), segs_per_pass."""
    what = SUB_WHAT.get(what, what)
    n, m, rows, nframes = int(n), int(m), int(rows), int(nframes)
    sub_check("sub_plan", what, n, 1, 0, nframes, m, rows)
    return _plan(lib().sp_sub_plan, ("chunk", "tiles", "shares", "lds_bytes", "workgroups", "passes", "seg_bytes", "segs_per_pass"), SubRefused,
                 "sub_plan", what, _ffi.DTYPE_C64 if cplx else _ffi.DTYPE_F32, n, m, rows, nframes)


BEAM_MAX_M, BEAM_TQ = 64, 64
BEAM_METHODS = {"bartlett": 0, "capon": 1, "music": 2, "ev": 3}
BEAM_PLAN_NAMES = ("tq", "tiles", "stage_vectors", "lds_bytes", "workgroups", "items_per_workgroup", "stages", "spare")


class BeamRefused(ValueError, NotImplementedError):
    """An array, a scan grid, a method or an eigendecomposition the array scan does not take: outside the limits, tables that are not
    finite, and what is not built (more than 64 sensors)."""


def _beam_table(who, name, t, cols=None):
    """a host table as contiguous float64 [rows, ndim]; a device tensor is read back (the tables are host arrays, as windows are)"""
    if _is_torch(t):
        t = t.detach().cpu().numpy()
    t = np.ascontiguousarray(np.asarray(t), dtype=np.float64)
    if t.ndim == 1:
        t = t.reshape(-1, 1)
    if t.ndim != 2 or t.shape[1] < 1 or t.shape[1] > 3 or (cols is not None and t.shape[1] != cols):
        raise BeamRefused("%s: %s must be [n] or [n, ndim] with ndim 1 .. 3, the same for pos and kv" % (who, name))
    if not np.all(np.isfinite(t)):
        raise BeamRefused("%s: %s must be finite" % (who, name))
    return t


def beam_check(who, m, ndim, nk, models, method, p, loading=0.0):
    """The refusals of sp_beamscan and sp_beamscan_plan about the shape, before the library is touched -> the method's code."""
    if method not in BEAM_METHODS:
        raise BeamRefused("%s: method must be 'bartlett', 'capon', 'music' or 'ev', not %r" % (who, method))
    code = BEAM_METHODS[method]
    if m < 2 or m > BEAM_MAX_M:
        raise BeamRefused("%s: m = %d sensors are outside 2 .. %d" % (who, m, BEAM_MAX_M))
    if ndim < 1 or ndim > 3:
        raise BeamRefused("%s: ndim = %d is outside 1 .. 3" % (who, ndim))
    if nk < 1 or nk > (1 << 31) - 1:
        raise BeamRefused("%s: nk = %d is outside 1 .. 2^31 - 1" % (who, nk))
    if code >= 2 and (p < 0 or p > m - 1):
        raise BeamRefused("%s: p = %d is outside 0 .. m - 1 = %d" % (who, p, m - 1))
    if models < 0 or models * -(-nk // BEAM_TQ) > 1 << 40:
        raise BeamRefused("%s: %d models of %d scan points are more than 2^40 tiles" % (who, models, nk))
    if not (math.isfinite(loading) and loading >= 0.0):
        raise BeamRefused("%s: loading must be finite and not negative" % who)
    return code


def beamscan(V, w, pos, kv, method="bartlett", p=0, loading=0.0, scale=None, out64=False):
    """The scan of a sensor array over steering vectors (sp_beamscan) from the eigendecompositions V[..., m, m] complex128, w[..., m]
    float64 descending, as `eigh` returns them for the array's cross-spectral-density matrices.  pos[m] or [m, ndim] are the sensor
    positions, kv[nk] or [nk, ndim] the scan vectors in TURNS per unit of pos, scale[...] (one number per model, or None = 1) multiplies
    the phase: a_q[i] = exp(2 pi i scale pos[i] . kv[q]), which is `pseudospectrum`'s steering vector for pos = 0, 1, ..  With
    D = sum_k g_k |a_q^H v_k|^2:
      'bartlett'  g_k = w_k,                 P = D / m^2      (a^H G a / m^2)
      'capon'     g_k = 1 / (w_k + delta),   P = 1 / D        (1 / a^H (G + delta I)^-1 a), delta = loading max(trace, 0) / m
      'music'     g_k = 1, k >= p,           P = 1 / D
      'ev'        g_k = 1 / w_k, k >= p,     P = 1 / D
    -> (P float32 [..., nk], or float64 with out64; status int32 [...]: 1 where a weight that was needed had a denominator <= 0 and
    was left out).  pos, kv and scale are host tables (a device tensor is read back).  numpy in -> numpy out; device tensors in ->
    device tensors on torch's current stream; the two agree bitwise."""
    who = "beamscan"
    p, loading = int(p), float(loading)
    md, V, w, shape, m = _eigen_models(who, BeamRefused, V, w)
    pos = _beam_table(who, "pos", pos)
    kv = _beam_table(who, "kv", kv, pos.shape[1])
    ndim, nk = int(pos.shape[1]), int(kv.shape[0])
    lead, models = _lead_rows(shape, 2)
    code = beam_check(who, m, ndim, nk, models, method, p, loading)
    if pos.shape[0] != m:
        raise BeamRefused("%s: pos holds %d sensors, V has order %d" % (who, pos.shape[0], m))
    if scale is not None:
        if _is_torch(scale):
            scale = scale.detach().cpu().numpy()
        scale = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), lead)).reshape(-1)
        if not np.all(np.isfinite(scale)):
            raise BeamRefused("%s: scale must be finite" % who)
    if not md.dev and not (np.all(np.isfinite(V)) and np.all(np.isfinite(w))):
        raise BeamRefused("%s: V and w must be finite" % who)
    P = md.empty(lead + (nk,), "float64" if out64 else "float32", V)
    st = md.empty(lead, "int32", V)
    if models:
        md.call(lib().sp_beamscan, md.addr(V), m, md.addr(w), m, models, ptr(pos), ndim, ptr(kv), nk, ptr(scale), code, p, loading, 1 if out64 else 0,
                md.addr(P), nk, md.addr(st))
    return P, st


def beam_plan(m, nk, models=1, method="bartlett", p=0, ndim=1):
    """sp_beamscan_plan as a dict (host only): tq (steering vectors of a tile), tiles (of a model), stage_vectors (eigenvectors staged in
    LDS at a time), lds_bytes (of a workgroup), workgroups (launched), items_per_workgroup (the most (model, tile) items one walks),
    stages (of a tile), spare."""
    m, nk, models, p, ndim = int(m), int(nk), int(models), int(p), int(ndim)
    code = beam_check("beam_plan", m, ndim, nk, models, method, p)
    return _plan(lib().sp_beamscan_plan, BEAM_PLAN_NAMES, BeamRefused, "beam_plan", m, ndim, nk, models, code, p)


DWT_MAX_L, DWT_MAX_LEVELS, DWT_MODWT_MAX_LEVELS, DWT_PASSES, DWT_MAX_N = 64, 32, 30, 9, (1 << 31) - 1
DWT_MODES = {"zero": 0, "constant": 1, "symmetric": 2, "reflect": 3, "periodic": 4, "periodization": 5}
DWT_FORMS = {"auto": 0, "row": 1, "tile": 2}
DWT_WHAT = {"dwt": 0, "idwt": 1, "modwt": 2, "imodwt": 3}


class DwtRefused(ValueError, NotImplementedError):
    """A filter bank, an extension mode, a depth or a layout the discrete wavelet transforms do not take: outside the limits, and what is
    not built (the extrapolating modes 'smooth', 'antisymmetric' and 'antireflect', which are not index maps; filters beyond 64 taps)."""


def dwt_coeff_len(n, L, mode="symmetric"):
    """coefficients of one analysis level of n samples: floor((n + L - 1) / 2), ceil(n / 2) for 'periodization'"""
    return (n + 1) // 2 if DWT_MODES.get(mode, mode) == 5 else (n + L - 1) // 2


def dwt_max_levels(n, L, mode="symmetric"):
    """the deepest level the library takes: the one at which a row has one coefficient, 32 at the most"""
    j = 0
    while j < DWT_MAX_LEVELS:
        n, j = dwt_coeff_len(n, L, mode), j + 1
        if n <= 1:
            break
    return j


def _dwt_code(who, table, what, value):
    if isinstance(value, str):
        if value in ("smooth", "antisymmetric", "antireflect") and table is DWT_MODES:
            raise DwtRefused("%s: mode %r extrapolates the row, which is not a map of the index: not built" % (who, value))
        if value not in table:
            raise DwtRefused("%s: %s must be one of %s, not %r" % (who, what, ", ".join(table), value))
        return table[value]
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) not in table.values():
        raise DwtRefused("%s: %s must be one of %s, not %r" % (who, what, ", ".join(table), value))
    return int(value)


def _dwt_filters(who, lo, hi):
    """the two filters of a call as contiguous float64 arrays of one even length 2 .. 64, finite"""
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    if lo.ndim != 1 or hi.ndim != 1 or lo.size != hi.size:
        raise DwtRefused("%s: the two filters must be one-dimensional and of one length" % who)
    L = int(lo.size)
    if L < 2 or L > DWT_MAX_L or L % 2:
        raise DwtRefused("%s: the filter length L = %d must be even and lie in 2 .. %d" % (who, L, DWT_MAX_L))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise DwtRefused("%s: the filters must be finite" % who)
    return lo, hi, L


def dwt_check(who, what, n, L, mode, levels, rows):
    """The refusals of the C entries about the shape (dwt_plan.h's dwt_shape), before the library is touched."""
    if n < 1 or n > DWT_MAX_N:
        raise DwtRefused("%s: n = %d samples of a row are outside 1 .. 2^31 - 1" % (who, n))
    if rows < 0 or rows > DWT_MAX_N:
        raise DwtRefused("%s: %d rows are outside 0 .. 2^31 - 1" % (who, rows))
    if what >= 2:
        if levels < 1 or levels > DWT_MODWT_MAX_LEVELS or (1 << (levels - 1)) * (L - 1) >= 1 << 31:
            raise DwtRefused("%s: levels = %d is outside 1 .. 30, or its dilated filter 2^(levels-1) (L - 1) reaches 2^31" % (who, levels))
    elif levels < 1 or levels > dwt_max_levels(n, L, mode):
        raise DwtRefused("%s: levels = %d is outside 1 .. %d, the level at which a row of %d samples has one coefficient"
                         % (who, levels, dwt_max_levels(n, L, mode), n))


def dwt_layout(n, L, mode, levels):
    """-> (lens, entries, total): lens[j] the samples of the approximation of level j (lens[0] = n); entries the (length, offset) of
    cA_J, cD_J, .., cD_1 in a row of the pyramid; total its elements"""
    lens = [int(n)]
    for _ in range(levels):
        lens.append(dwt_coeff_len(lens[-1], L, mode))
    entries, o = [], 0
    for e in range(levels + 1):
        ln = lens[levels if e == 0 else levels - e + 1]
        entries.append((ln, o))
        o += ln
    return lens, entries, o


def _dwt_rows(who, x):
    """the rows of a call -> (md, rows as the mode takes them, their pitch, lead, rows, the last axis)"""
    md = _enter(x)
    x = md.checked(x)
    if x.ndim < 1:
        raise DwtRefused("%s: the array needs at least one axis" % who)
    lead, rows = _lead_rows(x.shape)
    n = int(x.shape[-1])
    if n < 1:
        raise DwtRefused("%s: the rows must hold at least one sample" % who)
    if md.dev and x.ndim != 2:
        x = x.reshape(rows, n)
    xs, xld = md.rows(x)
    return md, xs, xld, lead, rows, n


def dwt(x, dec_lo, dec_hi, mode="symmetric", levels=1, form="auto"):
    """The pyramid (sp_dwt) of every row x[..., n] under the analysis filters (dec_lo, dec_hi) -> out[..., total] =
    [cA_J | cD_J | .. | cD_1] at the offsets of `dwt_layout`.  One level of n samples: cA[k] = sum_m dec_lo[m] xe[2k + 1 - m], k <
    floor((n + L - 1) / 2), xe the row extended by `mode` ('zero', 'constant', 'symmetric', 'reflect', 'periodic'; 'periodization':
    cA[k] = sum_m dec_lo[m] x[(2k + L / 2 - m) mod n'], k < n' / 2, an odd row repeating its last sample).  float32 FMAs with the taps
    ascending; complex rows take the real taps on both parts.  form 'row' (every level in LDS, one launch), 'tile' (a launch per
    level, any length) or 'auto' (the row form wherever it fits).  numpy in -> numpy out; device tensors in -> a device tensor on x's
    stream; the two, and the two forms, agree bitwise."""
    who = "dwt"
    lo, hi, L = _dwt_filters(who, dec_lo, dec_hi)
    mode, form, levels = _dwt_code(who, DWT_MODES, "mode", mode), _dwt_code(who, DWT_FORMS, "form", form), int(levels)
    md, xs, xld, lead, rows, n = _dwt_rows(who, x)
    dwt_check(who, 0, n, L, mode, levels, rows)
    total = dwt_layout(n, L, mode, levels)[2]
    out = md.empty(lead + (total,), "complex64" if md.code(xs) == _ffi.DTYPE_C64 else "float32", xs)
    if rows:
        md.call(lib().sp_dwt, md.addr(xs), md.code(xs), xld, n, rows, ptr(lo), ptr(hi), L, mode, levels, md.addr(out), total, form)
    return out


def dwt_level(x, dec_lo, dec_hi, mode="symmetric", form="auto", interleave=False):
    """One analysis level (sp_dwt_level) of every row -> (cA, cD), each [..., K]; interleave=True -> one array [..., 2, K] holding cA
    and cD side by side (the children 2p and 2p + 1 of a packet node; on the device the kernel writes it in place)."""
    who = "dwt_level"
    lo, hi, L = _dwt_filters(who, dec_lo, dec_hi)
    mode, form = _dwt_code(who, DWT_MODES, "mode", mode), _dwt_code(who, DWT_FORMS, "form", form)
    md, xs, xld, lead, rows, n = _dwt_rows(who, x)
    dwt_check(who, 0, n, L, mode, 1, rows)
    K = dwt_coeff_len(n, L, mode)
    dt = "complex64" if md.code(xs) == _ffi.DTYPE_C64 else "float32"
    if interleave and md.dev:
        out = md.empty(lead + (2, K), dt, xs)
        if rows:
            md.call(lib().sp_dwt_level, md.addr(xs), md.code(xs), xld, n, rows, ptr(lo), ptr(hi), L, mode, ptr(out.data_ptr()), 2 * K,
                    ptr(out.data_ptr() + K * out.element_size()), 2 * K, form)
        return out
    cA, cD = md.empty(lead + (K,), dt, xs), md.empty(lead + (K,), dt, xs)
    if rows:
        md.call(lib().sp_dwt_level, md.addr(xs), md.code(xs), xld, n, rows, ptr(lo), ptr(hi), L, mode, md.addr(cA), K, md.addr(cD), K, form)
    return np.stack((cA, cD), axis=-2) if interleave else (cA, cD)


def idwt(coef, n, rec_lo, rec_hi, mode="symmetric", levels=1, form="auto"):
    """The inverse of `dwt` (sp_idwt): rows of n samples from pyramids coef[..., total] laid out as `dwt` writes them for the same
    (n, L, mode, levels).  One level: x[i] = sum_q rec_lo[p + 2q] cA[k0 - q] + sum_q rec_hi[p + 2q] cD[k0 - q], t = i + L - 2, p = t mod 2,
    k0 = floor(t / 2) ('periodization': t = i + L / 2 - 1, k0 - q mod K); an approximation one longer than the detail it meets drops
    its last sample."""
    who = "idwt"
    lo, hi, L = _dwt_filters(who, rec_lo, rec_hi)
    mode, form, levels, n = _dwt_code(who, DWT_MODES, "mode", mode), _dwt_code(who, DWT_FORMS, "form", form), int(levels), int(n)
    md, cs, cld, lead, rows, total = _dwt_rows(who, coef)
    dwt_check(who, 1, n, L, mode, levels, rows)
    if total != dwt_layout(n, L, mode, levels)[2]:
        raise DwtRefused("%s: a pyramid of %d levels of %d samples has %d coefficients, not %d" % (who, levels, n, dwt_layout(n, L, mode, levels)[2], total))
    x = md.empty(lead + (n,), "complex64" if md.code(cs) == _ffi.DTYPE_C64 else "float32", cs)
    if rows:
        md.call(lib().sp_idwt, md.addr(cs), md.code(cs), cld, n, rows, ptr(lo), ptr(hi), L, mode, levels, md.addr(x), n, form)
    return x


def idwt_level(cA, cD, n, rec_lo, rec_hi, mode="symmetric", form="auto"):
    """The inverse of `dwt_level` (sp_idwt_level): rows of n samples from cA[..., K] and cD[..., K], K the coefficients n samples have.
    cD=None: cA is the interleaved [..., 2, K] of `dwt_level`."""
    who = "idwt_level"
    lo, hi, L = _dwt_filters(who, rec_lo, rec_hi)
    mode, form, n = _dwt_code(who, DWT_MODES, "mode", mode), _dwt_code(who, DWT_FORMS, "form", form), int(n)
    if cD is None:
        if cA.ndim < 2 or cA.shape[-2] != 2:
            raise DwtRefused("%s: the interleaved coefficients must be [..., 2, K]" % who)
        if _is_torch(cA):
            K = int(cA.shape[-1])
            pair = cA.contiguous().reshape(-1, 2, K)
            cA, cD, lead = pair[:, 0, :], pair[:, 1, :], tuple(map(int, cA.shape[:-2]))
        else:
            cA, cD, lead = cA[..., 0, :], cA[..., 1, :], None
    else:
        lead = None
    md, As, ald, lead_a, rows, K = _dwt_rows(who, cA)
    if _mode(cD) is not md:
        raise TypeError("%s: cA and cD must both be numpy arrays or both device tensors" % who)
    cD = md.checked(cD)
    if tuple(cD.shape) != tuple(cA.shape) or not md.alike(As, cD):
        raise DwtRefused("%s: cD must share cA's shape, %s" % (who, md.ALIKE))
    if md.dev and cD.ndim != 2:
        cD = cD.reshape(max(rows, 1), K)
    Ds, dld = md.rows(cD)
    lead = lead_a if lead is None else lead
    dwt_check(who, 1, n, L, mode, 1, rows)
    if K != dwt_coeff_len(n, L, mode):
        raise DwtRefused("%s: %d samples have %d coefficients, not %d" % (who, n, dwt_coeff_len(n, L, mode), K))
    x = md.empty(lead + (n,), "complex64" if md.code(As) == _ffi.DTYPE_C64 else "float32", As)
    if rows:
        md.call(lib().sp_idwt_level, md.addr(As), ald, md.addr(Ds), dld, md.code(As), n, rows, ptr(lo), ptr(hi), L, mode, md.addr(x), n, form)
    return x


def modwt(x, rec_lo, rec_hi, levels, form="auto"):
    """The maximal-overlap transform (sp_modwt) of every row x[..., n], circular, any n: with g = rec_lo / sqrt 2, h = rec_hi / sqrt 2 and
    V_0 = x, W_j[t] = sum_l h[l] V_{j-1}[(t - 2^(j-1) l) mod n] and V_j the same with g -> W[levels + 1, ..., n] = W_1 .. W_J, V_J."""
    who = "modwt"
    lo, hi, L = _dwt_filters(who, rec_lo, rec_hi)
    form, levels = _dwt_code(who, DWT_FORMS, "form", form), int(levels)
    md, xs, xld, lead, rows, n = _dwt_rows(who, x)
    dwt_check(who, 2, n, L, 0, levels, rows)
    W = md.empty((levels + 1,) + lead + (n,), "complex64" if md.code(xs) == _ffi.DTYPE_C64 else "float32", xs)
    if rows:
        md.call(lib().sp_modwt, md.addr(xs), md.code(xs), xld, n, rows, ptr(lo), ptr(hi), L, levels, md.addr(W), n, form)
    return W


def imodwt(W, rec_lo, rec_hi, form="auto"):
    """The inverse of `modwt` (sp_imodwt): x[..., n] from W[levels + 1, ..., n]:
    V_{j-1}[t] = sum_l h[l] W_j[(t + 2^(j-1) l) mod n] + sum_l g[l] V_j[(t + 2^(j-1) l) mod n]."""
    who = "imodwt"
    lo, hi, L = _dwt_filters(who, rec_lo, rec_hi)
    form = _dwt_code(who, DWT_FORMS, "form", form)
    md = _enter(W)
    W = md.samples(md.checked(W))
    if W.ndim < 2 or W.shape[0] < 2:
        raise DwtRefused("%s: W must be [levels + 1, ..., n] with at least one level" % who)
    levels, n = int(W.shape[0]) - 1, int(W.shape[-1])
    lead, rows = _lead_rows(W.shape[1:])
    if n < 1:
        raise DwtRefused("%s: the rows must hold at least one sample" % who)
    dwt_check(who, 3, n, L, 0, levels, rows)
    x = md.empty(lead + (n,), "complex64" if md.code(W) == _ffi.DTYPE_C64 else "float32", W)
    if rows:
        md.call(lib().sp_imodwt, md.addr(W), md.code(W), n, n, rows, ptr(lo), ptr(hi), L, levels, md.addr(x), n, form)
    return x


DWT_PLAN_NAMES = ("form", "tile", "lds_bytes", "workgroups", "launches", "passes", "scratch_bytes", "rows_per_pass", "max_levels", "rows_per_workgroup")


def dwt_plan(what, n, L, mode="symmetric", levels=1, rows=1, cplx=False, form="auto"):
    """sp_dwt_plan as a dict (host only): what 'dwt', 'idwt', 'modwt' or 'imodwt' -> form (1 row, 2 tile), tile (outputs of a tile),
    lds_bytes, workgroups, launches, passes, scratch_bytes, rows_per_pass, max_levels, rows_per_workgroup, and `entries`: the
    (length, offset) of every entry of the output in its order."""
    who = "dwt_plan"
    what = _dwt_code(who, DWT_WHAT, "what", what)
    mode = 0 if what >= 2 else _dwt_code(who, DWT_MODES, "mode", mode)
    form, n, L, levels, rows = _dwt_code(who, DWT_FORMS, "form", form), int(n), int(L), int(levels), int(rows)
    if L < 2 or L > DWT_MAX_L or L % 2:
        raise DwtRefused("%s: the filter length L = %d must be even and lie in 2 .. %d" % (who, L, DWT_MAX_L))
    dwt_check(who, what, n, L, mode, levels, rows)
    out = np.zeros(80, dtype=np.int64)
    if lib().sp_dwt_plan(what, _ffi.DTYPE_C64 if cplx else _ffi.DTYPE_F32, n, L, mode, levels, rows, form, ptr(out)) != 0:
        raise DwtRefused("%s: the shape is refused (a forced row form that does not fit)" % who)
    d = dict(zip(DWT_PLAN_NAMES, (int(v) for v in out[:10])))
    d["entries"] = [(int(out[10 + 2 * e]), int(out[11 + 2 * e])) for e in range(levels + 1)]
    return d


EIGH_MAX_N = 64


class OrderTooLarge(ValueError, NotImplementedError):
    """A matrix order above 64: outside the limits, and a path that is not built (A and V of one matrix live in the LDS of one CU)."""


def eigh(A, nvec=None, max_sweeps=30, check=True):
    """Eigendecomposition of the Hermitian matrices A[..., n, n], 1 <= n <= 64, on the GPU (sp_eigh: parallel cyclic Jacobi in
    float64, one matrix per workgroup) -> (w, V, sweeps):
      w      [..., n] float64, DESCENDING (numpy.linalg.eigh ascends);
      V      [..., n, nvec] complex128, column j the unit eigenvector of w[..., j]; nvec (default n) leading ones, 0 for none.  Each is
             turned so that its component of largest modulus is real and positive;
      sweeps [...] int32 Jacobi sweeps used; max_sweeps + 1 marks a matrix that did not converge (or holds a NaN or an infinity),
             whose w and V mean nothing.
    Only the LOWER triangle and the real part of the diagonal are read, as numpy.linalg.eigh's UPLO='L' does.  complex128 is native;
    complex64, float32 and float64 are cast.  check=True reads sweeps back and raises numpy.linalg.LinAlgError naming the first
    matrix that did not converge; check=False leaves the judgement (and, for device tensors, the asynchrony) to the caller.
    numpy in -> numpy out; a device tensor in -> device tensors out on the same device and on torch's current stream."""
    shape = tuple(A.shape)
    if len(shape) < 2 or shape[-1] != shape[-2]:
        raise ValueError("eigh: A must be [..., n, n], got %s" % (shape,))
    n = int(shape[-1])
    if n < 1:
        raise ValueError("eigh: the order must be at least 1")
    if n > EIGH_MAX_N:
        raise OrderTooLarge("eigh: order n = %d above %d is not built (one matrix and its vectors live in the LDS of one CU)"
                            % (n, EIGH_MAX_N))
    nvec = n if nvec is None else int(nvec)
    if not 0 <= nvec <= n:
        raise ValueError("eigh: nvec = %d outside 0 .. n = %d" % (nvec, n))
    max_sweeps = int(max_sweeps)
    if max_sweeps < 1:
        raise ValueError("eigh: max_sweeps must be at least 1")
    lead, batch = _lead_rows(shape, 2)
    md = _enter(A)
    a = md.cast(A, "complex128")
    w = md.empty(lead + (n,), "float64", a)
    V = md.empty(lead + (n, nvec), "complex128", a)
    sw = md.empty(lead, "int32", a)
    md.call(lib().sp_eigh, md.addr(a), n, batch, nvec, max_sweeps, md.addr(w), md.addr(V) if nvec > 0 and batch > 0 else None,
            md.addr(sw))
    if check:                               # (the read-back of a device tensor waits for the stream)
        bad = (sw.reshape(-1).cpu().numpy() if md.dev else sw.reshape(-1)) > max_sweeps
    if check and bad.any():
        first = int(np.argmax(bad))
        raise np.linalg.LinAlgError("eigh: matrix %s (flat index %d) did not converge in %d sweeps (non-finite input?)"
                                    % (np.unravel_index(first, lead) if lead else (), first, max_sweeps))
    return w, V, sw


# ------------------------------------------------------------------------------------------ F1
def fir_filter(h, x, nfft=0):
    """Causal FIR y = lfilter(h, 1, x) (float32) by overlap-save on the GPU."""
    taps = np.ascontiguousarray(h, dtype=np.float32)
    md = _enter(x)
    xs = md.cast(x, "float32")
    out = md.empty(xs.shape, "float32", xs)
    md.call(lib().sp_fftfilt, ptr(taps), taps.size, md.addr(xs), md.count(xs), int(nfft), md.addr(out))
    return out


# ------------------------------------------------------------------------------------------ F2
def biquad_filter(b, a, x):
    """y = scipy.signal.lfilter(b, a, x) for one second-order section (b[3], a[3]), float32 samples, evaluated exactly
    on the GPU (float64 recurrence, blocked scan of the state maps; include/spectral.h: sp_biquad)."""
    bb = np.ascontiguousarray(b, dtype=np.float64).ravel()
    aa = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if bb.size > 3 or aa.size > 3 or aa.size < 1 or bb.size < 1:
        raise ValueError("biquad_filter: b and a hold at most 3 coefficients")
    bb = np.concatenate([bb, np.zeros(3 - bb.size)])
    aa = np.concatenate([aa, np.zeros(3 - aa.size)])
    if aa[0] == 0.0:
        raise ValueError("biquad_filter: a[0] must not be zero")
    rts = np.roots(aa)
    if rts.size and float(np.max(np.abs(rts))) > 1.0 + 1e-12:
        # (the device scan raises the state map to powers up to len(x): an unstable section would overflow them to inf / NaN)
        raise ValueError("biquad_filter: unstable section (pole radius %.9g > 1)" % float(np.max(np.abs(rts))))
    md = _enter(x)
    if (x.is_complex() if md.dev else np.iscomplexobj(x)) or np.ndim(x) != 1:
        raise TypeError("biquad_filter: one real 1-D signal")
    xs = md.cast(x, "float32")
    out = md.empty(xs.shape, "float32", xs)
    md.call(lib().sp_biquad, ptr(bb), ptr(aa), md.addr(xs), md.count(xs), md.addr(out))
    return out


# ------------------------------------------------------------------------------------------ F3
PADTYPES = {None: 0, "none": 0, "odd": 1, "even": 2, "constant": 3}
MAX_SECTIONS = 8


def sos_array(sos):
    """(n_sections, 6) float64 copy of a second-order-section design, checked the way sp_sosfilt checks it (1 to 8
    sections, finite, a0 != 0, every pole radius <= 1) -- refused here before any device work."""
    s = np.array(sos, dtype=np.float64)
    if s.ndim == 1 and s.size == 6:
        s = s[None, :]
    if s.ndim != 2 or s.shape[1] != 6:
        raise ValueError("sos must have shape (n_sections, 6)")
    if not 1 <= s.shape[0] <= MAX_SECTIONS:
        raise ValueError("sos: %d sections; 1 to %d are supported (filter order <= %d)" % (s.shape[0], MAX_SECTIONS,
                                                                                             2 * MAX_SECTIONS))
    if not np.all(np.isfinite(s)):
        raise ValueError("sos: non-finite coefficient")
    if np.any(s[:, 3] == 0.0):
        raise ValueError("sos: a0 must not be zero")
    for k in range(s.shape[0]):
        rts = np.roots(s[k, 3:])
        if rts.size and float(np.max(np.abs(rts))) > 1.0 + 1e-12:
            raise ValueError("sos: section %d is unstable (pole radius %.9g > 1)" % (k, float(np.max(np.abs(rts)))))
    return np.ascontiguousarray(s)


def _sos_rows(x):
    """x (numpy or device tensor, rows along the last axis) -> (float32 [R, n] contiguous rows, lead shape, complex?);
    complex input becomes its real rows followed by its imaginary rows."""
    if _is_torch(x):
        cplx = x.is_complex()
        lead, n = tuple(x.shape[:-1]), int(x.shape[-1])
        parts = torch.stack([x.real, x.imag]) if cplx else x
        return parts.reshape(-1, n).to(torch.float32).contiguous(), lead, cplx
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    lead, n = x.shape[:-1], x.shape[-1]
    parts = np.stack([x.real, x.imag]) if cplx else x
    return np.ascontiguousarray(parts.reshape(-1, n), dtype=np.float32), lead, cplx


def _sos_out(y, x, lead, cplx):
    """device rows -> the input's shape; float64 / complex128 (and integer) input comes back in double precision"""
    n = y.shape[-1]
    if _is_torch(x):
        if cplx:
            y = torch.complex(y[:y.shape[0] // 2], y[y.shape[0] // 2:])
            return y.reshape(lead + (n,)).to(torch.complex64 if x.dtype == torch.complex64 else torch.complex128)
        return y.reshape(lead + (n,)).to(torch.float32 if x.dtype == torch.float32 else torch.float64)
    xd = np.asarray(x).dtype
    if cplx:
        y = y[:y.shape[0] // 2] + 1j * y[y.shape[0] // 2:]
        return y.reshape(lead + (n,)).astype(np.complex64 if xd == np.complex64 else np.complex128)
    return y.reshape(lead + (n,)).astype(np.float32 if xd == np.float32 else np.float64, copy=False)


def sos_filter(sos, x, zi=None):
    """y = scipy.signal.sosfilt(sos, x, axis=-1) on the GPU, exact (float64 recurrence, blocked scan of the state maps;
    include/spectral.h: sp_sosfilt), float32 samples.  x: numpy, or a device tensor that stays on the device (torch's
    current stream).  zi (or None): scipy's shape (n_sections, ...lead, 2); with zi, returns (y, zf) of the same shapes."""
    s = sos_array(sos)
    nsec = s.shape[0]
    if np.ndim(x) < 1 or x.shape[-1] < 1:
        raise ValueError("sos_filter: empty signal")
    rows, lead, cplx = _sos_rows(x)
    R, n = rows.shape
    zr = None
    if zi is not None:
        want = (nsec,) + tuple(lead) + (2,)
        if tuple(zi.shape) != want:
            raise ValueError("sos_filter: zi must have shape %s, got %s" % (want, tuple(zi.shape)))
    md = _enter(x)
    if zi is not None:
        if md.dev:
            z = torch.as_tensor(zi, device=x.device).reshape(nsec, -1, 2)
            if cplx:                          # a real zi is the real parts' state; the imaginary parts start from rest
                z = torch.cat([z.real, z.imag if z.is_complex() else torch.zeros_like(z)], 1)
            elif z.is_complex():
                z = z.real
            zr = md.cast(z.permute(1, 0, 2), "float64")
        else:
            z = np.asarray(zi).reshape(nsec, -1, 2)
            z = np.concatenate([z.real, z.imag], 1) if cplx else np.real(z)
            zr = md.cast(z.transpose(1, 0, 2), "float64")
    y = md.empty(rows.shape, "float32", rows)
    zf = md.empty(zr.shape, "float64", zr) if zr is not None else None
    md.call(lib().sp_sosfilt, ptr(s), nsec, md.addr(rows), R, n, md.addr(zr), md.addr(y), md.addr(zf))
    out = _sos_out(y, x, lead, cplx)
    if zi is None:
        return out
    zf = zf.permute(1, 0, 2) if _is_torch(zf) else zf.transpose(1, 0, 2)       # [nsec][R][2]
    if cplx:
        h = zf.shape[1] // 2
        zf = zf[:, :h] + 1j * zf[:, h:]
    return out, zf.reshape((nsec,) + tuple(lead) + (2,))


def sos_filtfilt(sos, x, padtype="odd", padlen=0):
    """y = scipy.signal.sosfiltfilt(sos, x, axis=-1, padtype, padlen) on the GPU: forward over the extended record from
    sosfilt_zi times its first sample, then backwards (include/spectral.h: sp_sosfiltfilt).  padlen is explicit here
    (pyfft_amd.filters.sosfiltfilt applies scipy's default); numpy or device-tensor x as in sos_filter."""
    s = sos_array(sos)
    nsec = s.shape[0]
    if padtype not in PADTYPES:
        raise ValueError("padtype must be 'odd', 'even', 'constant' or None, got %r" % (padtype,))
    pt = PADTYPES[padtype]
    padlen = 0 if pt == 0 else int(padlen)
    if padlen < 0:
        raise ValueError("padlen must not be negative")
    if np.ndim(x) < 1 or x.shape[-1] < 1:
        raise ValueError("sos_filtfilt: empty signal")
    n = int(x.shape[-1])
    if padlen > 0 and n <= padlen:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    if np.any(s[:, 3] + s[:, 4] + s[:, 5] == 0.0):
        raise ValueError("sos_filtfilt: a section with a pole at z = 1 has no steady state")
    rows, lead, cplx = _sos_rows(x)
    R = rows.shape[0]
    md = _enter(x)
    y = md.empty(rows.shape, "float32", rows)
    md.call(lib().sp_sosfiltfilt, ptr(s), nsec, md.addr(rows), R, n, pt, padlen, md.addr(y))
    return _sos_out(y, x, lead, cplx)


# ------------------------------------------------------------------------------------------ A6 / N1
def csd_epilogue(pxx, pyy, pxy, nfft, onesided, enbw):
    """The fft_pwelch epilogue (fft_analysis.py:489-648) on the averaged spectra, on the device: pxx[nb], pyy[nch, nb],
    pxy[nch, nb] complex as welch_csd returns them (numpy, or torch tensors that stay on the GPU).  Returns a dict of
    channel-major arrays: Cxy[nch, nb] complex, Cxy2, phi, Lyy, Lxy [nch, nb], Lxx[nb], and the fftshifted correlations
    Rxx[nfft], Ryy / Rxy / iCxy / corrcoef [nch, nfft] (real for one-sided input, complex otherwise), Ex, Ey[nch]."""
    nfft, onesided = int(nfft), bool(onesided)
    md = _enter(pxx)
    if md.dev:                              # the real parts of the powers; (re, im) pairs of the result -> complex
        a, b = (v.real if v.is_complex() else v for v in (pxx, pyy))
        cplx = lambda v: torch.complex(v[..., 0], v[..., 1])          # noqa: E731  (slices of `out` may start at odd offsets)
    else:
        a, b = np.real(pxx), np.real(pyy)
        cplx = lambda v: v[..., 0] + 1j * v[..., 1]                     # noqa: E731
    a, b, c = md.cast(a, "float64"), md.cast(b, "float64"), md.cast(pxy, "complex128")
    if b.ndim == 1:
        b, c = b[None, :], c[None, :]
    nch, nb = b.shape
    out = md.empty(int(lib().sp_csd_epilogue_doubles(nch, nb, nfft)), "float64", a)
    md.call(lib().sp_csd_epilogue, md.addr(a), md.addr(b), md.addr(c), nch, nb, nfft, 1 if onesided else 0, float(enbw), md.addr(out))
    pos = [0]

    def take(*shape):
        n = 1
        for d in shape:
            n *= d
        v = out[pos[0]:pos[0] + n].reshape(shape)
        pos[0] += n
        return v
    r = {}
    r["Cxy"] = cplx(take(nch, nb, 2))
    r["Cxy2"] = take(nch, nb)
    r["phi"] = take(nch, nb)
    r["Lxx"] = take(nb)
    r["Lyy"] = take(nch, nb)
    r["Lxy"] = take(nch, nb)
    corr = {"Rxx": take(nfft, 2), "Ryy": take(nch, nfft, 2), "Rxy": take(nch, nfft, 2), "iCxy": take(nch, nfft, 2),
            "corrcoef": take(nch, nfft, 2)}
    e = take(1 + nch, 2)
    for k, v in corr.items():
        r[k] = v[..., 0] if onesided else cplx(v)
    r["Ex"] = e[0, 0] if onesided else cplx(e[0])
    r["Ey"] = e[1:, 0] if onesided else cplx(e[1:])
    return r
