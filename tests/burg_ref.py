"""float64 restatements of include/spectral_ar.h (burg_def, yule_def, psd_def), restatements of the kernels' arithmetic (burg_def32,
yule_def32: float32 state and products, float64 sums), the cases of tests/test_gpu_parametric.py, the metrics and the measured
figures its allowances rest on.  numpy only."""
import numpy as np

MARGIN, PARITY = 4.0, 2e-4
SEGS_HOOK = 7                   # SP_AR_SEGS of the two-pass test


# ---- the definitions -----------------------------------------------------------------------------------------------------------
def segment(x, n, first=0, g=0, hop=1, detrend=True, mean_value=None):
    """segment g of a row in float64 / complex128, less its own mean, a constant, or nothing"""
    s = np.asarray(x)[first + g * hop:first + g * hop + n]
    s = s.astype(np.complex128 if np.iscomplexobj(s) else np.float64)
    assert s.size == n
    if detrend:
        s = s - (s.mean() if mean_value is None else mean_value)
    return s


def stepup(a, k):
    """a_m from a_{m-1} (length m) and k_m"""
    out = np.concatenate([a, [0]]).astype(np.result_type(a, k))
    out[1:] += k * np.conj(a[::-1])
    return out


def burg_def(x, p, f32=False):
    """MATLAB's arburg of one detrended segment -> a[p + 1], E[p + 1], k[p].  f32: the kernel's split -- f, b and every product in
    float32 (complex64), the sums, k, a and E in float64"""
    cplx = np.iscomplexobj(x)
    wide = np.complex128 if cplx else np.float64
    st = (np.complex64 if cplx else np.float32) if f32 else wide
    n = x.size
    f = np.asarray(x, dtype=wide).astype(st)
    b = f.copy()
    E = np.zeros(p + 1)
    k = np.zeros(p, dtype=wide)
    E[0] = np.sum((np.abs(f) ** 2).astype(np.float64)) / n if not f32 else np.sum(_nrm32(f).astype(np.float64)) / n
    a = np.ones(1, dtype=wide)
    for m in range(1, p + 1):
        fm, bm = f[m:], b[m - 1:n - 1]
        if f32:
            num = np.sum((fm * np.conj(bm)).astype(wide))
            den = np.sum((_nrm32(fm) + _nrm32(bm)).astype(np.float64))
        else:
            num, den = np.sum(fm * np.conj(bm)), np.sum(np.abs(fm) ** 2 + np.abs(bm) ** 2)
        km = -2.0 * num / den if den > 0 else 0.0
        k[m - 1] = km
        ks = st(km)
        fn = fm + ks * bm
        bn = bm + np.conj(ks) * fm
        f, b = f.copy(), b.copy()
        f[m:], b[m:] = fn, bn
        a = stepup(a, wide(km))
        E[m] = max(E[m - 1] * (1.0 - abs(km) ** 2), 0.0)                # never below zero, as the kernel
    return a, E, k


def _nrm32(v):
    return v.real * v.real + v.imag * v.imag if np.iscomplexobj(v) else v * v


def lags_def(x, p, f32=False):
    """the biased lags r[l] = (1 / n) sum_{i >= l} x[i] conj(x[i - l]), l = 0 .. p; f32: float32 samples and products, float64 sums"""
    cplx = np.iscomplexobj(x)
    wide = np.complex128 if cplx else np.float64
    v = np.asarray(x, dtype=wide)
    if f32:
        v = v.astype(np.complex64 if cplx else np.float32)
    n = v.size
    return np.array([np.sum((v[l:] * np.conj(v[:n - l])).astype(wide)) for l in range(p + 1)], dtype=wide) / n


def levinson_def(r, p):
    """Levinson-Durbin in float64 on the lags r[0 .. p] -> a, E, k; r[0] == 0 gives the zero model"""
    wide = r.dtype
    a = np.ones(1, dtype=wide)
    E = np.zeros(p + 1)
    k = np.zeros(p, dtype=wide)
    E[0] = max(r[0].real, 0.0)
    for m in range(1, p + 1):
        acc = r[m] + np.sum(a[1:] * r[m - 1:0:-1])
        km = -acc / E[m - 1] if E[m - 1] > 0 else 0.0
        k[m - 1] = km
        a = stepup(a, wide.type(km))
        E[m] = max(E[m - 1] * (1.0 - abs(km) ** 2), 0.0)
    return a, E, k


def yule_def(x, p, f32=False):
    return levinson_def(lags_def(x, p, f32), p)


def psd_def(a, E, m, start, step, scale=1.0):
    """P[q] = scale E / |sum_j a[j] e^{-2 pi i j nu_q}|^2, nu_q = start + q step, with the phase j nu reduced exactly"""
    nu = start + np.arange(m) * step
    fr = nu - np.floor(nu)
    j = np.arange(len(a))
    ph = np.outer(fr, j)
    A = np.exp(-2j * np.pi * (ph - np.round(ph))) @ np.asarray(a, dtype=np.complex128)
    return np.zeros(m) if E == 0 else scale * E / np.abs(A) ** 2


def fit_def(x, n, hop, first, nframes, p, method, detrend=True, mean_value=None, f32=False):
    """the fits of every (row, frame) of x[rows, nsig] -> a[rows, nframes, p + 1], E, k"""
    x = np.atleast_2d(x)
    cplx = np.iscomplexobj(x)
    wide = np.complex128 if cplx else np.float64
    a = np.zeros((x.shape[0], nframes, p + 1), dtype=wide)
    E = np.zeros((x.shape[0], nframes, p + 1))
    k = np.zeros((x.shape[0], nframes, p), dtype=wide)
    fn = burg_def if method == "burg" else yule_def
    for r in range(x.shape[0]):
        for g in range(nframes):
            a[r, g], E[r, g], k[r, g] = fn(segment(x[r], n, first, g, hop, detrend, mean_value), p, f32)
    return a, E, k


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
PSD_BINS = 257


def psd_grid(cplx):
    """the bins the metric on P looks at: 0 .. 1/2 for a real record, the full circle for a complex one"""
    return (PSD_BINS, 0.0, (1.0 if cplx else 0.5) / (PSD_BINS - 1))


def deviations(got, ref):
    """(P, k, a, E): P per bin relative to that bin's own float64 value, k absolute, a relative to sum|a|, E_m relative; the worst over
    the models.  got, ref: (a, E, k) of [..., p + 1] / [..., p]"""
    ga, gE, gk = (np.asarray(v).reshape((-1,) + np.asarray(v).shape[-1:]) for v in got)
    ra, rE, rk = (np.asarray(v).reshape((-1,) + np.asarray(v).shape[-1:]) for v in ref)
    cplx = np.iscomplexobj(ra)
    dP = 0.0
    for s in range(ra.shape[0]):
        Pg, Pr = psd_def(ga[s], gE[s, -1], *psd_grid(cplx)), psd_def(ra[s], rE[s, -1], *psd_grid(cplx))
        dP = max(dP, float(np.max(np.abs(Pg - Pr) / Pr)))
    dk = float(np.max(np.abs(gk - rk)))
    da = float(np.max(np.max(np.abs(ga - ra), axis=-1) / np.sum(np.abs(ra), axis=-1)))
    dE = float(np.max(np.abs(gE - rE) / rE))
    return dP, dk, da, dE


def dynamic_range_db(a, E, cplx):
    P = psd_def(a, E, *psd_grid(cplx))
    return 10.0 * np.log10(P.max() / P.min())


# ---- the cases of the GPU test ---------------------------------------------------------------------------------------------------
# name -> n, p, complex; a case may also set rows, nframes, hop, first and form (SP_BURG_FORM: 0 by length, 2 the workgroup form), whose
# defaults (one row, one frame, hop 1, first 0, form 0) live in shape_of
CROSSOVER = 1024
CASES = {
    "w64":     dict(n=64, p=4, cplx=False),                          # one sample per lane
    "w65":     dict(n=65, p=1, cplx=False),                          # a partly filled lane chunk
    "w333c":   dict(n=333, p=8, cplx=True),                          # odd chunking
    "w1024":   dict(n=CROSSOVER, p=16, cplx=False),                  # the last of the wave form
    "g1024":   dict(n=CROSSOVER, p=16, cplx=False, form=2),          # the crossover length in the workgroup form
    "g1025":   dict(n=CROSSOVER + 1, p=16, cplx=False),
    "g1100":   dict(n=1100, p=12, cplx=True),                        # a whole wave of the workgroup holds no sample
    "g4096":   dict(n=4096, p=64, cplx=False),
    "g8192c":  dict(n=8192, p=128, cplx=True),
    "g16384":  dict(n=16384, p=256, cplx=False),                     # the largest
    "frames":  dict(n=200, p=6, cplx=False, rows=3, nframes=5, hop=77, first=13),
    "ragged":  dict(n=64, p=3, cplx=True, rows=1, nframes=11, hop=32, first=0),   # 11 segments at 4 a workgroup
}
YULE_ONLY = {
    "long":    dict(n=100003, p=20, cplx=False),                     # many tiles, a ragged last one, halo across every seam
    "step":    dict(n=3 * 2048 + 5, p=9, cplx=False),                # a step at a tile seam
}


def shape_of(name):
    c = dict(rows=1, nframes=1, hop=1, first=0, form=0)
    c.update(CASES.get(name) or YULE_ONLY[name])
    c["nsig"] = c["first"] + (c["nframes"] - 1) * c["hop"] + c["n"] + (3 if c["first"] else 0)
    return c


_signals = {}


def signals(name):
    """the record of a case, float32 or complex64 [rows, nsig]: two resonances (pole radii 0.97 and 0.9) driven by white noise, a
    constant offset, and white noise 30 dB below; `step` adds a step of height 2 at sample 2048"""
    if name in _signals:
        return _signals[name]
    c = shape_of(name)
    rng = np.random.default_rng(sorted(list(CASES) + list(YULE_ONLY)).index(name) + 100)
    rows, nsig = c["rows"], c["nsig"]
    lead = 512
    w = rng.standard_normal((rows, nsig + lead)) + (1j * rng.standard_normal((rows, nsig + lead)) if c["cplx"] else 0)
    poles = [0.97 * np.exp(2j * np.pi * 0.11), 0.9 * np.exp(2j * np.pi * 0.31)]
    if not c["cplx"]:
        poles = poles + [np.conj(z) for z in poles]
    den = np.poly(poles)
    den = den if c["cplx"] else den.real
    y = np.zeros_like(w)
    for i in range(w.shape[1]):
        acc = w[:, i].copy()
        for j in range(1, len(den)):
            if i - j >= 0:
                acc -= den[j] * y[:, i - j]
        y[:, i] = acc
    y = y[:, lead:]
    y = y / np.std(y) + 0.03 * (rng.standard_normal(y.shape) + (1j * rng.standard_normal(y.shape) if c["cplx"] else 0)) + (0.7 - (0.4j if c["cplx"] else 0))
    if name == "step":
        y[:, 2048:] += 2.0
    x = y.astype(np.complex64 if c["cplx"] else np.float32)
    x.setflags(write=False)
    _signals[name] = x
    return x


_refs = {}


def reference(name, method, f32=False):
    """(a, E, k) of the case in float64 (f32: the kernels' split), computed once"""
    key = (name, method, f32)
    if key not in _refs:
        c = shape_of(name)
        _refs[key] = fit_def(signals(name), c["n"], c["hop"], c["first"], c["nframes"], c["p"], method, True, None, f32)
    return _refs[key]


def ar4(n, seed=5):
    """a real AR(4) record of n samples and its polynomial, for the recovery test"""
    rng = np.random.default_rng(seed)
    poles = [0.9 * np.exp(2j * np.pi * 0.1), 0.8 * np.exp(2j * np.pi * 0.3)]
    den = np.poly(poles + [np.conj(z) for z in poles]).real
    w = rng.standard_normal(n + 1000)
    y = np.zeros(n + 1000)
    for i in range(n + 1000):
        y[i] = w[i] - sum(den[j] * y[i - j] for j in range(1, 5) if i - j >= 0)
    return y[1000:], den


# ---- measured on the CPU over the cases above (tests/test_host_parametric.py holds them to within a factor of two) ----------------
# the worst of the four metrics (P per bin, k, a, E_m) of burg_def32 against burg_def, and of yule_def32 against yule_def
BURG_F32_DEV = 9.0e-7
YULE_F32_DEV = 2.2e-6
BURG_ALLOWANCE = MARGIN * BURG_F32_DEV
YULE_ALLOWANCE = MARGIN * YULE_F32_DEV
# the spectrum kernel is float64 throughout: what remains is the rounding of a float32 output (tests/test_gpu_parametric.py derives the
# bound on the float64 sums per bin)
PSD_ALLOWANCE32 = 2.0 ** -23
# the share of the allowances tests/test_gpu_parametric.py used on an MI355X
BURG_DEVICE_SHARE = 0.24
YULE_DEVICE_SHARE = 0.26
