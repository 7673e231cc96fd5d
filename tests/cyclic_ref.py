"""Spectral correlation by the averaged cyclic periodogram restated in numpy, the shapes of tests/test_gpu_cyclic.py and the allowance
they hold the kernel to.  A helper module, not a test: nothing here is collected.

The definition (include/spectral_cyclo.h): rows x, y of one dtype, nu in cycles per sample, nu_h = nu / 2 rounded once to a multiple of
2^-64 turn, e(t) = exp(2 pi i t), sample j of a row at the absolute index first + j, frame g = the n samples from s = g hop on, w a real
window of n taps, m the row's mean (or 0):

    Z+[g][k] = DFT_n( w[j] (y[s + j] - m_y) e(-nu_h (first + s + j)) )
    Z-[g][k] = DFT_n( w[j] (x'[s + j] - m_x') e(+nu_h (first + s + j)) ),   x' = conj(x) in the conjugate form, else x
    S = scale sum_g Z+ conj(Z-),   Pp = scale sum_g |Z+|^2,   Pm = scale sum_g |Z-|^2

cyclic_def is that in float64.  Its phases come from the same 64-bit integer arithmetic as the kernel's: numpy uint64 products wrap
exactly, and the turn fraction is phase / 2^64 in float64.  cyclic_def32 is the same with the float32 table w[j] e(-+nu_h j), the
frame's factor e(-nu (first + s)) on the product, complex64 transforms and float32 sums.

The allowance.  F32_DEV is the largest deviation of cyclic_def32 from cyclic_def over SHAPES -- S relative to its row's largest
sqrt(Pp Pm), Pp and Pm relative to the row's largest Pp, a row being one (record, nu) -- as measured by tests/test_host_cyclic.py (which
prints it and asserts it against the constant).  The kernel gets that figure times a margin of 4 -- a different but legal summation
order and its own transform rounding -- which must stay below the project's parity figure of 2e-4, plus an absolute term of 1e-6 of
the call's largest cell.  On the device (MI355X) the worst cell of tests/test_gpu_cyclic.py used DEVICE_SHARE of that allowance."""
import functools
import math

import numpy as np

F32_DEV = 3.0e-7          # measured 2.78e-7 (test_float32_restatement_deviation: n256-cplx, 41 frames; numpy's complex64 transform)
MARGIN = 4.0
PARITY = 2e-4
ABS_TERM = 1e-6
ALLOWANCE = MARGIN * F32_DEV
DEVICE_SHARE = 0.137      # measured on an MI355X: the worst cell over SHAPES (n4096-runs-of-three); 0.039 .. 0.137 per shape

NU_AM = 0.0371            # the modulation rate of signals(): cycles per sample
GAMMA_AM = 0.8 / (1 + 0.8 ** 2 / 2)      # |gamma| of (1 + 0.8 cos) e[n] at nu = NU_AM: 0.606


def nuh_units(nu):
    """nu / 2 to the nearest multiple of 2^-64 turn (ties to even) as a Python int modulo 2^64"""
    return int(round(math.ldexp(float(nu) * 0.5, 64))) % (1 << 64)


def turn(units, idx):
    """the fraction of a turn, in [0, 1), of units * idx modulo 2^64: uint64 products wrap exactly"""
    ph = np.asarray(units % (1 << 64), dtype=np.uint64) * np.asarray(idx, dtype=np.int64).astype(np.uint64)
    return ph.astype(np.float64) / 18446744073709551616.0


def e(t):
    return np.cos(2 * np.pi * t) + 1j * np.sin(2 * np.pi * t)


def hann(n):
    """scipy.signal.get_window('hann', n): periodic"""
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def row_mean(x):
    """the mean the kernel subtracts: float64 sum of the float32 samples, rounded to float32"""
    m = np.mean(np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64))
    return np.complex64(m) if np.iscomplexobj(x) else np.float32(m)


def _frames(a, n, hop, nframes):
    return a[np.arange(nframes)[:, None] * hop + np.arange(n)[None, :]]


def cyclic_def(x, w, hop, nframes, nu, y=None, conj=False, first=0, mx=0.0, my=None, scale=1.0):
    """float64: (S complex128, Pp, Pm float64) [A, n] of one row"""
    x = np.asarray(x)
    y = x if y is None else np.asarray(y)
    my = mx if my is None else my
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    xp, mxp = (np.conj(x), np.conj(mx)) if conj else (x, mx)
    fx = _frames(xp.astype(np.complex128), n, hop, nframes) - complex(mxp)
    fy = _frames(y.astype(np.complex128), n, hop, nframes) - complex(my)
    idx = first + np.arange(nframes)[:, None] * hop + np.arange(n)[None, :]
    S, Pp, Pm = [], [], []
    for v in np.atleast_1d(nu):
        rot = e(turn(nuh_units(v), idx))                     # e(+nu_h t)
        Zp = np.fft.fft(w * fy * np.conj(rot), axis=-1)
        Zm = np.fft.fft(w * fx * rot, axis=-1)
        S.append(scale * np.sum(Zp * np.conj(Zm), axis=0))
        Pp.append(scale * np.sum(np.abs(Zp) ** 2, axis=0))
        Pm.append(scale * np.sum(np.abs(Zm) ** 2, axis=0))
    return np.array(S), np.array(Pp), np.array(Pm)


def cyclic_def32(x, w, hop, nframes, nu, y=None, conj=False, first=0, mx=0.0, my=None, scale=1.0):
    """the same with the float32 table, complex64 transforms and float32 sums: (S complex64, Pp, Pm float32) [A, n]"""
    c64, f32 = np.complex64, np.float32
    x = np.asarray(x)
    y = x if y is None else np.asarray(y)
    my = mx if my is None else my
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    xp, mxp = (np.conj(x), np.conj(mx)) if conj else (x, mx)
    fx = (_frames(xp.astype(c64), n, hop, nframes) - c64(mxp)).astype(c64)
    fy = (_frames(y.astype(c64), n, hop, nframes) - c64(my)).astype(c64)
    s0 = first + np.arange(nframes) * hop
    S, Pp, Pm = [], [], []
    for v in np.atleast_1d(nu):
        u = nuh_units(v)
        tab = (w * np.conj(e(turn(u, np.arange(n))))).astype(c64)           # w[j] e(-nu_h j)
        p2 = np.conj(e(turn(2 * u, s0))).astype(c64)[:, None]              # e(-nu (first + s))
        Up = np.fft.fft((tab * fy).astype(c64), axis=-1).astype(c64)
        Um = np.fft.fft((np.conj(tab) * fx).astype(c64), axis=-1).astype(c64)
        S.append(f32(scale) * np.sum((p2 * (Up * np.conj(Um)).astype(c64)).astype(c64), axis=0, dtype=c64))
        Pp.append(f32(scale) * np.sum((Up.real ** 2 + Up.imag ** 2).astype(f32), axis=0, dtype=f32))
        Pm.append(f32(scale) * np.sum((Um.real ** 2 + Um.imag ** 2).astype(f32), axis=0, dtype=f32))
    return np.array(S), np.array(Pp), np.array(Pm)


# the smallest shapes at which each mechanism first engages (test_gpu_cyclic.py): rows x nsig samples, x_ld = nsig + pitch
SHAPES = {
    "n32-real-tail": dict(cplx=False, n=32, hop=8, nframes=37, nu=(0.0, 1 / 32, NU_AM, -NU_AM, 1.0), first=0, rows=1, pitch=0, b0=0, nb=32,
                          forms=("auto",)),
    "n256-cplx": dict(cplx=True, n=256, hop=64, nframes=41, nu=(0.0, NU_AM, -NU_AM, 1 / 256, 0.25, 0.7, -1.0), first=(1 << 40) + 3, rows=1,
                      pitch=0, b0=0, nb=256, forms=("conj", "plain")),
    "n1024-cross-batch-pitch": dict(cplx=False, n=1024, hop=256, nframes=9, nu=(0.0, NU_AM, -0.2), first=-17, rows=3, pitch=5, b0=1000, nb=48,
                                    forms=("cross",)),
    "n4096-gaps": dict(cplx=True, n=4096, hop=5000, nframes=3, nu=(NU_AM, -0.5), first=0, rows=1, pitch=0, b0=0, nb=4096,
                       forms=("conj", "plain")),
    "n8192-hop1": dict(cplx=False, n=8192, hop=1, nframes=5, nu=(0.0, NU_AM), first=0, rows=1, pitch=0, b0=0, nb=8192, forms=("auto",)),
    "n64-many-alpha": dict(cplx=False, n=64, hop=16, nframes=13, nu=tuple((np.arange(300) - 150) / 160.0), first=0, rows=1, pitch=0, b0=0,
                           nb=64, forms=("auto",)),
    # frames per group above one without a hook: 600 cycle frequencies leave 4 x 256 CUs / 600 = 2 groups, 3 frames each, for 5 frames
    "n4096-runs-of-three": dict(cplx=False, n=4096, hop=16, nframes=5, nu=tuple(NU_AM + (np.arange(600) - 300) / 4096.0), first=0, rows=1,
                                pitch=0, b0=0, nb=4096, forms=("auto",)),
}
# SP_CYCLIC_FPG per shape: frames per group that do not divide the frame count, so that a group walks the frame loop (accumulation
# across frames, the exchange image reused, the frame's factor and the window table read again) and the last group its clamped tail
FPG = {"n32-real-tail": 3, "n256-cplx": 3, "n1024-cross-batch-pitch": 4, "n4096-gaps": 2, "n8192-hop1": 2, "n64-many-alpha": 5,
       "n4096-runs-of-three": 2}
MANY_ALPHA_CHUNK = 128            # SP_CYCLIC_CHUNK for n64-many-alpha: 300 cycle frequencies in 3 passes, seams at 128 and 256
CASES = [(name, form) for name, s in SHAPES.items() for form in s["forms"]]


def nsig_of(s):
    return (s["nframes"] - 1) * s["hop"] + s["n"] + 3          # three samples beyond the last frame


def am_noise(rng, nsig, cplx, depth=0.8):
    """amplitude-modulated noise (1 + depth cos(2 pi NU_AM n + 0.3)) e[n]; complex rows add a modulated carrier at 0.11"""
    t = np.arange(nsig)
    env = 1 + depth * np.cos(2 * np.pi * NU_AM * t + 0.3)
    if not cplx:
        return (env * rng.standard_normal(nsig)).astype(np.float32)
    z = env * (rng.standard_normal(nsig) + 1j * rng.standard_normal(nsig)) / np.sqrt(2)
    z = z + 0.5 * (1 + 0.5 * np.cos(2 * np.pi * NU_AM * t)) * np.exp(2j * np.pi * 0.11 * t) + (0.05 - 0.02j)
    return z.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def signals(name):
    """(x, y) [rows, nsig], float32 or complex64, cyclostationary at NU_AM; y = a delayed, rescaled x plus noise of its own.
    Computed once and shared: read-only."""
    s = SHAPES[name]
    rng = np.random.default_rng(sum(name.encode()))
    nsig = nsig_of(s)
    x = np.stack([am_noise(rng, nsig, s["cplx"]) for _ in range(s["rows"])])
    y = np.stack([(0.7 * np.roll(x[r], 2) + 0.5 * am_noise(rng, nsig, s["cplx"], 0.3)).astype(x.dtype) for r in range(s["rows"])])
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def form_args(form):
    """(cross, conj) of a form"""
    return form == "cross", form == "conj"


def _reference(name, form, fn):
    s = SHAPES[name]
    x, y = signals(name)
    cross, conj = form_args(form)
    w = hann(s["n"]).astype(np.float32)
    out = [fn(x[r], w, s["hop"], s["nframes"], s["nu"], y[r] if cross else None, conj, s["first"], row_mean(x[r]),
              row_mean(y[r]) if cross else None) for r in range(s["rows"])]
    out = tuple(np.stack([o[i] for o in out]) for i in range(3))
    for o in out:
        o.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, form):
    """float64 (S, Pp, Pm) [rows, A, n] of a shape on the float32-rounded samples, window and means; computed once, read-only"""
    return _reference(name, form, cyclic_def)


@functools.lru_cache(maxsize=None)
def reference32(name, form):
    return _reference(name, form, cyclic_def32)


def band(a, s):
    """the nb bins from b0 on, modulo n"""
    return a[..., (s["b0"] + np.arange(s["nb"])) % s["n"]]


def row_scales(ref):
    """per (record, nu) row of a reference triple over all n bins: the largest sqrt(Pp Pm) and the largest Pp, [..., 1]"""
    S, Pp, Pm = ref
    return np.max(np.sqrt(Pp * Pm), axis=-1, keepdims=True), np.max(Pp, axis=-1, keepdims=True)


def deviation(got, ref):
    """the largest deviation of a triple from the reference triple (whole spectra): S relative to its row's largest sqrt(Pp Pm), Pp and Pm
    relative to the row's largest Pp"""
    ts, tp = row_scales(ref)
    return max(float(np.max(np.abs(got[0] - ref[0]) / ts)), float(np.max(np.abs(got[1] - ref[1]) / tp)), float(np.max(np.abs(got[2] - ref[2]) / tp)))


def bounds(ref, sel=lambda a: a):
    """the allowed |error| per cell of (S, Pp, Pm): ALLOWANCE of the row's scale plus ABS_TERM of the call's largest cell; sel picks the
    cells of the call (a band) out of whole spectra"""
    ts, tp = row_scales(ref)
    return tuple(ALLOWANCE * t + ABS_TERM * float(np.max(np.abs(sel(r)))) + 0 * sel(np.abs(r)) for t, r in zip((ts, tp, tp), ref))


def assert_within(got, ref, what="", sel=lambda a: a, which=(0, 1, 2)):
    """every cell of the outputs within its bound; returns the largest share of a bound that was used"""
    bd = bounds(ref, sel)
    worst = 0.0
    for i in which:
        g, r = np.asarray(got[i]), sel(ref[i])
        assert g.shape == r.shape, (what, i, g.shape, r.shape)
        worst = max(worst, float(np.max(np.abs(g - r) / bd[i])))
    print("%s: worst cell at %.3f of its allowance" % (what, worst))
    assert worst <= 1.0, (what, worst)
    return worst


def coherence(S, Pp, Pm):
    """gamma = S / sqrt(Pp Pm) in float64 (0 where the denominator is 0)"""
    den = np.sqrt(np.asarray(Pp, dtype=np.float64) * np.asarray(Pm, dtype=np.float64))
    return np.where(den > 0, np.asarray(S, dtype=np.complex128) / np.where(den > 0, den, 1.0), 0.0)


# the significance test: seeded white noise against cyclic_level
LEVEL_NU = (NU_AM, 0.028, 0.05, 0.11, 0.21, 0.27, 0.333, -0.4107)
LEVEL_N, LEVEL_HOP, LEVEL_NSIG = 256, 64, 1 << 15
LEVEL_FRAMES = (LEVEL_NSIG - LEVEL_N) // LEVEL_HOP + 1      # 509


@functools.lru_cache(maxsize=None)
def level_rows():
    """(white noise, amplitude-modulated noise) float32 [2^15], seeded; read-only"""
    rng = np.random.default_rng(20240607)
    white = rng.standard_normal(LEVEL_NSIG).astype(np.float32)
    am = am_noise(rng, LEVEL_NSIG, False)
    white.setflags(write=False)
    am.setflags(write=False)
    return white, am


@functools.lru_cache(maxsize=None)
def level_reference(which):
    """float64 (S, Pp, Pm) [8, 256] of level_rows()[which] at LEVEL_NU, Hann 256 / hop 64 / 509 frames, the mean removed"""
    x = level_rows()[which]
    out = cyclic_def(x, hann(LEVEL_N).astype(np.float32), LEVEL_HOP, LEVEL_FRAMES, LEVEL_NU, mx=row_mean(x))
    for o in out:
        o.setflags(write=False)
    return out
