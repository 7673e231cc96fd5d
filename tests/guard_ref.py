"""The instrument of the offset-pointer tests, and the table of cases both of its test modules walk.

Every other kernel test enters the library with pointers that are at least 256-byte aligned and never looks around a buffer.  Here

    poisoned_input   puts the samples `lead` elements past a front guard inside an allocation whose every other element (front guard,
                     lead, row gaps, tail guard) is NaN: a load outside [ptr, ptr + extent) that reaches a result makes it non-finite;
    sentinel_output  gives an output region in the interior of an allocation filled with one fixed NaN bit pattern per 4-byte word;
    guards_intact    compares the words around the interior as integers (a store outside the extent), and
    all_written      finds an interior word that still holds the pattern (a store that was skipped).

The front guard is GUARD elements (a multiple of 16 bytes for every element size), so the pointer's residue modulo 16 is that of
`lead` elements, which poisoned_input asserts; GUARD elements on either side keep the overrun of a whole workgroup's vector store inside
the allocation, where it is reported instead of faulting.  numpy arrays and torch tensors are handled alike: there is no GPU code here.

The second half is the case table of tests/test_gpu_offset_pointers.py with its inputs and float64 references (scipy, numpy or
oracle.cpu_ref on the float32-rounded samples); tests/test_host_guard_ref.py computes every reference on the CPU.
A helper module, not a test: nothing here is collected."""
import collections
import functools

import numpy as np

GUARD = 1024
SENTINEL = 0xFFF5A5A5            # every 4-byte word of an output allocation: a NaN with a payload (not the canonical 0x7FC00000), as
#                                   float32, as either half of a complex64 and, doubled, as a float64
_SENTINEL_I32 = SENTINEL - (1 << 32)


class GuardDamaged(AssertionError):
    """A word outside the interior changed; .index = the first damaged element relative to the interior (negative: before it)."""

    def __init__(self, index):
        AssertionError.__init__(self, "guard word damaged at element %d relative to the interior" % index)
        self.index = index


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _addr(a):
    return int(a.data_ptr()) if _is_torch(a) else int(a.ctypes.data)


def _np_empty(total, dtype):
    """numpy storage that starts on a 64-byte boundary, as a device allocation does"""
    dtype = np.dtype(dtype)
    raw = np.empty(total * dtype.itemsize + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + total * dtype.itemsize].view(dtype)


def _geometry(nelem, lead, guard, rows, pitch):
    ld = nelem if pitch is None else int(pitch)
    assert ld >= nelem and rows >= 1 and lead >= 0
    span = (rows - 1) * ld + nelem if pitch is not None else rows * nelem
    return ld, span, guard + lead, guard + lead + span + guard


def _rows_view(flat, rows, nelem, ld, two_d):
    if not two_d:
        return flat
    if ld == nelem:
        return flat.reshape(rows, nelem)
    if _is_torch(flat):
        return flat.as_strided((rows, nelem), (ld, 1))
    return np.lib.stride_tricks.as_strided(flat, (rows, nelem), (ld * flat.itemsize, flat.itemsize))


def poisoned_input(a, lead, guard=GUARD, pitch=None):
    """-> (base, view): `view` holds a's values (1-D, or 2-D rows) and starts guard + lead elements into `base`; everything else in base
    is NaN (both parts for complex).  Without pitch the view is contiguous (2-D: a flat view reshaped); with pitch > n its rows lie
    pitch elements apart.  Asserts that the view's address has the residue of `lead` elements modulo 16."""
    shape = tuple(int(d) for d in a.shape)
    assert len(shape) in (1, 2)
    rows, n = (1, shape[0]) if len(shape) == 1 else shape
    assert pitch is None or (len(shape) == 2 and pitch > n)
    ld, span, start, total = _geometry(n, lead, guard, rows, pitch)
    if _is_torch(a):
        import torch
        base = torch.full((total,), complex(np.nan, np.nan) if a.is_complex() else np.nan, dtype=a.dtype, device=a.device)
        itemsize = base.element_size()
        view = _rows_view(base[start:start + span], rows, n, ld, len(shape) == 2)
        view.copy_(a)
        contiguous = view.is_contiguous()
    else:
        a = np.asarray(a)
        base = _np_empty(total, a.dtype)
        base[:] = complex(np.nan, np.nan) if np.iscomplexobj(a) else np.nan
        itemsize = base.itemsize
        view = _rows_view(base[start:start + span], rows, n, ld, len(shape) == 2)
        view[...] = a
        contiguous = view.flags["C_CONTIGUOUS"]
    assert _addr(base) % 16 == 0 and (guard * itemsize) % 16 == 0
    assert _addr(view) % 16 == (lead * itemsize) % 16
    assert contiguous == (pitch is None)
    return base, view


def _words(base):
    """the allocation as 4-byte integer words (a view)"""
    if _is_torch(base):
        import torch
        flat = torch.view_as_real(base) if base.is_complex() else base
        return flat.reshape(-1).view(torch.int32)
    return base.view(np.uint32)


def _host_words(base):
    """[elements, words per element] uint32 on the host"""
    w = _words(base)
    w = w.cpu().numpy().view(np.uint32) if _is_torch(w) else np.asarray(w)
    return w.reshape(base.shape[0], -1)


def sentinel_output(nelem, dtype, lead, guard=GUARD, device=None, rows=1, pitch=None):
    """-> (base, interior): an allocation of `dtype` whose every 4-byte word is SENTINEL (written through an integer view), and its
    interior of rows x nelem elements (rows `pitch` apart, dense by default) that starts guard + lead elements in.  device=None: numpy,
    and `interior` is the typed view a stand-in kernel writes; otherwise a torch tensor on `device`, and `interior` is the device
    address to hand to the C ABI."""
    ld, span, start, total = _geometry(nelem, lead, guard, rows, pitch)
    if device is None:
        base = _np_empty(total, dtype)
        _words(base)[:] = SENTINEL
        assert _addr(base) % 16 == 0
        return base, interior_of(base, lead, nelem, guard, rows, pitch)
    import torch
    base = torch.empty(total, dtype=dtype, device=device)
    _words(base).fill_(_SENTINEL_I32)
    assert _addr(base) % 16 == 0 and (guard * base.element_size()) % 16 == 0
    return base, _addr(base) + start * base.element_size()


def interior_of(base, lead, nelem, guard=GUARD, rows=1, pitch=None):
    """the typed view of the interior: [nelem], or [rows, nelem] for rows > 1"""
    ld, span, start, total = _geometry(nelem, lead, guard, rows, pitch)
    assert base.shape[0] == total
    return _rows_view(base[start:start + span], rows, nelem, ld, rows > 1)


def _inside(base, lead, nelem, guard, rows, pitch):
    ld, span, start, total = _geometry(nelem, lead, guard, rows, pitch)
    assert base.shape[0] == total
    inside = np.zeros(total, dtype=bool)
    for r in range(rows):
        inside[start + r * ld:start + r * ld + nelem] = True
    return inside, start


def guards_intact(base, lead, nelem, guard=GUARD, rows=1, pitch=None):
    """True when every word outside the interior still holds SENTINEL, compared as integers; otherwise raises GuardDamaged with the
    first damaged element's index relative to the start of the interior (negative: before it; row gaps count from the same origin)."""
    inside, start = _inside(base, lead, nelem, guard, rows, pitch)
    bad = np.any(_host_words(base) != np.uint32(SENTINEL), axis=1) & ~inside
    if bad.any():
        raise GuardDamaged(int(np.argmax(bad)) - start)
    return True


def first_unwritten(base, lead, nelem, guard=GUARD, rows=1, pitch=None):
    """index (relative to the interior) of the first interior element with a word that still holds SENTINEL, or None"""
    inside, start = _inside(base, lead, nelem, guard, rows, pitch)
    left = np.any(_host_words(base) == np.uint32(SENTINEL), axis=1) & inside
    return int(np.argmax(left)) - start if left.any() else None


def all_written(base, lead, nelem, guard=GUARD, rows=1, pitch=None):
    """False when any interior word still holds SENTINEL: a store that was skipped"""
    return first_unwritten(base, lead, nelem, guard, rows, pitch) is None


def snapshot(base):
    """a copy of an allocation's words, for `unchanged` after the call"""
    return _words(base).clone() if _is_torch(base) else _words(base).copy()


def unchanged(base, snap):
    """True when no word of the allocation differs from the snapshot (an input, poison included, that a call must only read)"""
    w = _words(base)
    return bool((w == snap).all())


# ======================================================================================================================================
# The cases.  A case names a family of pyfft_amd.engine (group A) with its shape; `inputs` gives its sample arrays (float32 / complex64:
# what the device sees) and whatever tables go with them, `reference` the float64 result.  `places` lists, per run, one (lead, extra
# pitch) pair for every sample array: the first run of a bitwise family is the aligned one, which the others are compared against.
# ======================================================================================================================================
Case = collections.namedtuple("Case", "id family cplx p places")

F32_LEADS, C64_LEADS = (0, 1, 2, 3), (0, 1)
TILE = 8192                                   # samples of a tile of k_biquad_tile and k_sos_tile
BITWISE = ("biquad_filter", "sos_filter", "upfirdn", "ddc")      # the pointer only changes how samples are staged
ROW_PITCH = 3                                 # the strided cases: pitch = n + 3
NU, N0 = 0.1234, 12345                        # the oscillator of the ddc cases (tests/test_gpu_baseband.py)
PFB_N0 = 123457


def _leads(cplx, ninputs=1):
    return tuple((((lead, 0),) * ninputs) for lead in (C64_LEADS if cplx else F32_LEADS))


def _build():
    cases = []

    def add(family, tag, cplx=False, places=None, **p):
        name = "%s-%s-%s" % (family, "c64" if cplx else "f32", tag)
        cases.append(Case(name, family, cplx, p, _leads(cplx) if places is None else places))

    # rows n + 3 apart, aligned and at lead 1.  (The aligned run is pitched too: k_ddc splits a sample's phase into a float64 base and a
    # float32 table entry at shift = (row * x_ld + first staged sample) mod 4, so the bits of the rows after the first follow the row
    # pitch -- never the pointer -- and only placements of one pitch can be compared bit for bit.)
    pitched = (((0, ROW_PITCH),), ((1, ROW_PITCH),))
    for n in (1, 2, 3, 5, 4099):
        add("mean", "n%d" % n, n=n)
    for n in (1, 4099):
        add("mean", "n%d" % n, cplx=True, n=n)
    for filt in ("notch", "integrator"):
        for n in (5, TILE, 2 * TILE + 5):
            add("biquad_filter", "%s-n%d" % (filt, n), filt=filt, n=n)
    for family in ("sos_filter", "sosfiltfilt"):
        for K in (1, 3):
            for kind in ("lowpass", "highpass", "bandpass"):
                add(family, "K%d-%s" % (K, kind), K=K, kind=kind, rows=2, n=2 * TILE + 5)
    for cplx in (False, True):
        for up, down in ((3, 2), (1, 4)):
            add("upfirdn", "%d-%d" % (up, down), cplx, up=up, down=down, T=37)
            add("upfirdn", "%d-%d-pitch" % (up, down), cplx, pitched, up=up, down=down, T=37)
        add("ddc", "q8", cplx, q=8, T=65)
        add("ddc", "q8-pitch", cplx, pitched, q=8, T=65)
    add("fir_filter", "31-5000-1024", ntaps=31, n=5000, nfft=1024)
    for family in ("hilbert_rows", "spectral_filter_rows"):
        for rows, n in ((2, 1000), (2, 4096), (1, 1 << 21)):
            add(family, "%dx%d" % (rows, n), rows=rows, n=n)
    for n in (777, 1 << 20):
        add("xcorr_normalised", "n%d" % n, places=(((1, 0), (3, 0)), ((2, 0), (0, 0))), n=n)
    for cplx in (False, True):
        for nfft, hop, M in ((256, 64, 37), (1000, 250, 9)):
            shape = dict(nfft=nfft, hop=hop, M=M)
            for mode in ("mean", "linear"):
                add("welch_psd", "%s-%dx%d" % (mode, nfft, hop), cplx, mode=mode, **shape)
                add("frame_sum", "%s-%dx%d" % (mode, nfft, hop), cplx, mode=mode, **shape)
            add("stft_frames", "%dx%d" % (nfft, hop), cplx, **shape)
            add("stft_cog", "%dx%d" % (nfft, hop), cplx, **shape)
    for cplx in (False, True):
        for mode in ("mean", "linear"):
            add("welch_csd", "%s-3ch" % mode, cplx, _leads(cplx, 2), mode=mode, nch=3, nfft=256, hop=128, M=40)
    add("csd_matrix", "3ch", nch=3, nfft=256, hop=128, M=40)
    one = (((1, 0),),)
    for cplx in (False, True):
        add("pfb", "M16", cplx, one, M=16, P=1, D=16, nf=257)
        add("pfb", "M16-pitch", cplx, (((1, ROW_PITCH),),), M=16, P=1, D=16, nf=257)
        add("czt", "n8-m5", cplx, one, n=8, m=5, batch=37)
        add("czt", "n8-m5-pitch", cplx, (((1, ROW_PITCH),),), n=8, m=5, batch=37)
    add("xcorr_frames", "16-15-5", places=(((1, 0), (3, 0)),), k=0, nframes=37)
    add("welch_blocks", "32x16", places=(((1, 0), (3, 0)),), nfft=32, hop=16, navg=5, step=2)
    add("multitaper", "8x33", places=(((1, 0), (3, 0)),), nfft=8, M=33, K=2)
    add("bispectrum", "8x2", places=one, nfft=8, M=2)
    add("skf", "32-16-nk16", places=(((1, 0), (3, 0)),), k=0, nframes=37)
    return tuple(cases)


def noise(n, cplx, seed, offset=0.0):
    """unit white noise + an offset (its conjugate half on the imaginary part), rounded to what the device sees"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) + offset
    if cplx:
        return (x + 1j * (rng.standard_normal(n) - 0.5 * offset)).astype(np.complex64)
    return x.astype(np.float32)


def wide(x):
    x = np.asarray(x)
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def taps32(h):
    """the taps as the device sees them, in float64"""
    return np.asarray(h, dtype=np.float32).astype(np.float64)


def sos_design(K, kind):
    """designs(K)[kind] of tests/test_gpu_iir.py"""
    import scipy.signal as ss
    if kind == "lowpass":
        return ss.butter(2 * K, 0.001, output="sos")
    if kind == "highpass":
        return ss.butter(2 * K, 0.1, btype="high", output="sos")
    return ss.butter(K, [0.0005, 0.25], btype="band", output="sos")


def biquad_design(filt):
    """the narrow notch of test_fftfilt_and_notch (w0 = 0.01, Q = 30: pole radius 0.99948), and an integrator (pole radius 1)"""
    import scipy.signal as ss
    if filt == "notch":
        return ss.iirnotch(0.01, 30.0)
    return np.array([1.0, 0.0, 0.0]), np.array([1.0, -1.0, 0.0])


def hann(n):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


DETREND_MODE = {"mean": 1, "linear": 2}          # engine's detrend argument and detrend_ref's mode alike


def upfirdn_n(case):
    """samples giving two tiles plus 37 outputs (sp_upfirdn_tile: host only)"""
    from pyfft_amd import engine
    K = engine.upfirdn_tile(case.p["up"], case.p["down"], case.p["T"], case.cplx)
    return -(-(2 * K + 37) * case.p["down"] // case.p["up"]), K


def ddc_n(case):
    """samples giving two tiles plus a remainder (sp_ddc_tile: host only)"""
    from pyfft_amd import engine
    K = engine.ddc_tile(case.p["q"])
    return case.p["q"] * (2 * K + 37) + 3, K


def inputs(case):
    """dict: 'arrays' = the sample arrays to poison, in the order of the engine call; whatever else the call and the reference need.
    Computed once per case and shared: treat it as read-only."""
    return _inputs(case.id)


def reference(case):
    """the float64 result of the case: an array, or a tuple of arrays in the order the engine returns them.  Computed once."""
    return _reference(case.id)


@functools.lru_cache(maxsize=None)
def _inputs(case_id):
    case = BY_ID[case_id]
    import scipy.signal as ss
    import detrend_ref as R
    p, cplx, f = case.p, case.cplx, case.family
    seed = sum(case.id.encode()) + 1000 * len(case.id)
    d = {}
    if f == "mean":
        d["arrays"] = [noise(p["n"], cplx, seed, 3.0)]
    elif f == "biquad_filter":
        n = p["n"]
        d["b"], d["a"] = biquad_design(p["filt"])
        d["arrays"] = [(noise(n, False, seed) + 0.3 * np.sin(2 * np.pi * 0.06 * np.arange(n))).astype(np.float32)]
    elif f in ("sos_filter", "sosfiltfilt"):
        d["sos"] = sos_design(p["K"], p["kind"])
        d["arrays"] = [noise(p["rows"] * p["n"], False, seed).reshape(p["rows"], p["n"])]
    elif f == "upfirdn":
        n, _ = upfirdn_n(case)
        d["h"] = ss.firwin(p["T"], 1.0 / max(p["up"], p["down"])) * p["up"]
        d["arrays"] = [noise(2 * n, cplx, seed, 0.7).reshape(2, n)]
    elif f == "ddc":
        n, _ = ddc_n(case)
        d["h"] = ss.firwin(p["T"], 0.8 / p["q"])
        d["arrays"] = [noise(2 * n, cplx, seed, 0.7).reshape(2, n)]
    elif f == "fir_filter":
        d["h"] = np.random.default_rng(seed + 1).standard_normal(p["ntaps"]) / np.sqrt(p["ntaps"])
        d["arrays"] = [noise(p["n"], False, seed)]
    elif f in ("hilbert_rows", "spectral_filter_rows"):
        d["arrays"] = [noise(p["rows"] * p["n"], False, seed, 0.7).reshape(p["rows"], p["n"])]
        if f == "spectral_filter_rows":
            rng = np.random.default_rng(seed + 1)
            d["H"] = (rng.standard_normal(p["n"]) + 1j * rng.standard_normal(p["n"])).astype(np.complex64)
    elif f == "xcorr_normalised":
        n = p["n"]
        rng = np.random.default_rng(seed)
        x1 = (np.sin(0.01 * np.arange(n)) + rng.standard_normal(n) + 1.5).astype(np.float32)
        x2 = (np.roll(x1, 37) + 0.5 * rng.standard_normal(n) - 0.5).astype(np.float32)
        d["arrays"] = [x1, x2]
    elif f in ("welch_psd", "stft_frames", "stft_cog"):
        d["win"] = hann(p["nfft"])
        d["arrays"] = [R.case_signal(p["nfft"], p["hop"], p["M"], cplx)]
    elif f == "frame_sum":
        d["arrays"] = [np.stack([R.case_signal(p["nfft"], p["hop"], p["M"], cplx, ch) for ch in (0, 1)])]
    elif f == "welch_csd":
        d["win"] = hann(p["nfft"])
        nsig = p["nfft"] + p["hop"] * (p["M"] - 1) + 7
        sig = [R.signal(seed + ch, nsig, cplx, p["nfft"], R.CHANNEL_OFFSETS[ch]) for ch in range(p["nch"] + 1)]
        d["arrays"] = [sig[0], np.stack(sig[1:])]
    elif f == "csd_matrix":
        d["win"] = hann(p["nfft"])
        nsig = p["nfft"] + p["hop"] * (p["M"] - 1) + 7
        k = np.arange(nsig)
        rng = np.random.default_rng(seed)
        common = np.sin(0.13 * k) + 0.5 * rng.standard_normal(nsig)
        d["arrays"] = [np.stack([(0.3 + 0.05 * c) * np.roll(common, c) + rng.standard_normal(nsig) + 0.1 * c
                                 for c in range(p["nch"])]).astype(np.float32)]
    elif f == "pfb":
        from pyfft_amd import channelizer as CH
        M, P, D, nf = p["M"], p["P"], p["D"], p["nf"]
        d["h"] = CH.pfb_prototype(M, P) * M
        nsig = M * P + (nf - 1) * D + D - 1
        d["first"], d["r0"] = 0, PFB_N0 % M
        d["arrays"] = [noise(2 * nsig, cplx, seed, 0.7).reshape(2, nsig)]
    elif f == "czt":
        d["start"], d["step"] = 0.1037, 0.3 / p["m"]
        d["arrays"] = [noise(p["batch"] * p["n"], cplx, seed, 0.7).reshape(p["batch"], p["n"])]
    elif f == "xcorr_frames":
        from test_host_xcorr_frames import SHAPES, shape_case
        d["shape"] = SHAPES[p["k"]]
        x, y, raw, En = shape_case(p["k"], p["nframes"])
        d["arrays"], d["ref"] = [np.array(x), np.array(y)], raw / En[:, None]                  # (the shared arrays are read-only)
    elif f == "welch_blocks":
        from welch_blocks_ref import make_pair
        nsig = 40 * p["hop"] + p["nfft"] + 7
        d["win"] = hann(p["nfft"])
        d["arrays"] = list(make_pair(nsig, cplx, 100 + p["nfft"]))
    elif f == "multitaper":
        from pyfft_amd import multitaper as MT
        from test_host_multitaper import make_signal
        hop = p["nfft"] - p["nfft"] // 3
        nsig = (p["M"] - 1) * hop + p["nfft"] + hop // 3
        d["kw"] = dict(fs=250.0, nfft=p["nfft"], noverlap=p["nfft"] - hop, NW=1.5, Kmax=p["K"], weights="unity", detrend="linear")
        d["plan"] = MT.multitaper_plan(nsig, cplx, **d["kw"])
        d["arrays"] = [np.asarray(make_signal(nsig, cplx, seed + s)).astype(np.complex64 if cplx else np.float32) for s in (0, 1)]
    elif f == "bispectrum":
        from test_host_bispectrum import make_signal
        hop = p["nfft"] - p["nfft"] // 3
        d["win"], d["hop"] = hann(p["nfft"]), hop
        d["arrays"] = [np.asarray(make_signal((p["M"] - 1) * hop + p["nfft"] + hop // 3, cplx, seed)).astype(np.float32)]
    elif f == "skf":
        from test_host_skf import SHAPES, shape_case
        x, y, win, scale, ref, psd = shape_case(p["k"], p["nframes"])
        d.update(shape=SHAPES[p["k"]], win=win, scale=scale, ref=ref["mean"], psd=psd)
        d["arrays"] = [np.array(x), np.array(y)]
    else:
        raise KeyError(f)
    for a in d["arrays"]:
        assert a.dtype == (np.complex64 if cplx else np.float32), case.id
    return d


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    case = BY_ID[case_id]
    import scipy.signal as ss
    import detrend_ref as R
    from oracle import cpu_ref as O
    p, cplx, f = case.p, case.cplx, case.family
    d = inputs(case)
    x = wide(d["arrays"][0])
    if f == "mean":
        return x.mean()
    if f == "biquad_filter":
        return ss.lfilter(d["b"], d["a"], x)
    if f == "sos_filter":
        return ss.sosfilt(d["sos"], x, axis=-1)
    if f == "sosfiltfilt":
        return ss.sosfiltfilt(d["sos"], x, axis=-1)
    if f == "upfirdn":
        from test_host_resample import upfirdn_ref
        return upfirdn_ref(taps32(d["h"]), x, p["up"], p["down"])
    if f == "ddc":
        from test_host_baseband import ddc_ref
        return ddc_ref(x, NU, p["q"], taps32(d["h"]), N0)
    if f == "fir_filter":
        return O.fftfilt(taps32(d["h"]), x)
    if f == "hilbert_rows":
        return np.asarray(O.hilbert(x)).reshape(x.shape)
    if f == "spectral_filter_rows":
        return np.fft.ifft(d["H"].astype(np.complex128)[None, :] * np.fft.fft(x, axis=-1), axis=-1)
    if f == "xcorr_normalised":
        return O.ccf_fft(x, wide(d["arrays"][1]), 1.0)[1]
    if f in ("welch_psd", "stft_frames", "stft_cog", "frame_sum", "welch_csd"):
        mode = DETREND_MODE[p.get("mode", "mean")]
        nfft, hop, M = p["nfft"], p["hop"], p["M"]
        if f == "frame_sum":
            return np.stack([R.frames(row, nfft, hop, M, mode).sum(axis=0) for row in d["arrays"][0]])
        win = d["win"]
        if f == "welch_psd":
            return R.psd(d["arrays"][0], win, hop, M, mode, R.SIDED_TWO, scale=1.0 / float(np.sum(win ** 2)))
        if f == "stft_frames":
            return (R.stft(d["arrays"][0], win, hop, M, mode, R.SIDED_ONE, amp=1.0 / float(np.sum(win))),
                    R.pseg(d["arrays"][0], win, hop, M, mode))
        if f == "stft_cog":
            return R.cog(d["arrays"][0], win, hop, M, mode, R.FS)[0]
        return R.csd(d["arrays"][0], d["arrays"][1], win, hop, M, mode, R.SIDED_ONE, scale=1.0 / float(np.sum(win ** 2)))
    if f == "csd_matrix":
        win = d["win"]
        return O.csd_matrix(x, win, p["nfft"], p["hop"], p["M"], 1.0) * np.sum(win ** 2)
    if f == "pfb":
        from test_host_channelizer import pfb_ref
        X = pfb_ref(x, taps32(d["h"]), p["M"], p["D"], d["first"], p["nf"], 1, d["r0"])
        return X if cplx else X[..., :p["M"] // 2 + 1]
    if f == "czt":
        return ss.czt(x, p["m"], w=np.exp(-2j * np.pi * d["step"]), a=np.exp(2j * np.pi * d["start"]))
    if f == "xcorr_frames":
        return d["ref"]
    if f == "welch_blocks":
        from welch_blocks_ref import welch_blocks_ref, coherence_ref
        win = d["win"]
        nframes = (len(d["arrays"][0]) - p["nfft"]) // p["hop"] + 1
        pxx, pyy, pxy = welch_blocks_ref(d["arrays"][0], d["arrays"][1], p["nfft"], p["hop"], nframes, p["navg"], p["step"], win, True,
                                         1.0 / float(np.sum(win ** 2)), True)
        return pxx, pyy, pxy, coherence_ref(pxx, pyy, pxy)
    if f == "multitaper":
        from test_host_multitaper import scipy_oracle
        r = scipy_oracle(x, wide(d["arrays"][1]), d["plan"], "linear")
        return r["pxx"], r["pyy"], r["pxy"]
    if f == "bispectrum":
        from test_host_bispectrum import oracle_bispectrum
        return oracle_bispectrum(x, d["win"], d["hop"], p["M"], None, None, 1)          # (B, b2, A, P)
    if f == "skf":
        return d["ref"][0]
    raise KeyError(f)


def leaves(ref):
    """the arrays of a reference, NaN entries (outside a bispectrum's valid region) taken out"""
    out = []
    for a in (ref if isinstance(ref, tuple) else (ref,)):
        a = np.asarray(a).ravel()
        out.append(a[~np.isnan(a)])
    return out


INPUT_CASES = _build()
BY_ID = {c.id: c for c in INPUT_CASES}
assert len(BY_ID) == len(INPUT_CASES)
