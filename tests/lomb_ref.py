"""The generalised Lomb-Scargle periodogram restated in numpy, the cases of tests/test_gpu_lomb.py and the allowance they hold the
kernels to.  A helper module, not a test: nothing here is collected.

The definition (include/spectral_uneven.h; scipy.signal.lombscargle of scipy 1.15): times t[N], rows y[r][N], weights w[N] >= 0
normalised to sum to one, frequencies f[M] in cycles per unit of t, e(p) = exp(2 pi i p), phi = f (t - t_ref), d_r = y_r - m_r.  Per
frequency three complex sums

    A1 = sum w e(phi) = C + iS      A2 = sum w e(2 phi) = C2 + iS2      B_r = sum w d_r e(phi) = YC' + iYS'

and once W = sum w, Y'_r = sum w d_r, YY'_r = sum w d_r^2.  `finish` is scipy's body on these after a division by W: its second pass at
the offset tau is a rotation of the same sums, CC_tau = (1 + C2 cos 2 tau + S2 sin 2 tau) / 2, and m_r is a conditioning offset only
(YC = YC' + m C; with a floating mean it never enters).  lomb_def is that in float64 (sums by numpy, the phase reduced by p - rint(p)),
with `exact=True` from phases formed in rational arithmetic (fractions.Fraction of f t), for records far from the time origin.

lomb_def32 restates the kernel's arithmetic: the float64 phase product and its reduction, the turn rounded to float32, correctly
rounded float32 sine and cosine of it, e(2 phi) from c^2 - s^2 and 2cs, float32 weights w32 and products wy32 (formed in float64),
float32 sums over sub-runs of LOMB_SUB samples taken in order, float64 across the sub-runs, W, Y', YY' from the rounded values.

The allowance.  F32_DEV is the largest deviation of lomb_def32 from lomb_def over CASES -- every cell relative to its row's largest
magnitude -- as measured by tests/test_host_lomb.py (which prints it and asserts it against the constant).  The kernel gets that
figure times the project's margin of 4, for another order of summation (sample runs) and the hardware's sine and cosine; it must stay
below the project's parity figure of 2e-4.  On the device (MI355X, v_sin_f32 / v_cos_f32 of the reduced turn) the worst cell of
tests/test_gpu_lomb.py used DEVICE_SHARE of that allowance."""
import fractions
import functools
import itertools

import numpy as np

F32_DEV = 1.5e-6          # measured 1.487e-6 (test_float32_restatement_deviation: split-hook, equal weights, floating mean, 'normalize')
MARGIN = 4.0
PARITY = 2e-4
ALLOWANCE = MARGIN * F32_DEV
DEVICE_SHARE = 0.428      # measured on an MI355X: 'amplitude' of a record 2^31 from the time origin; 0.02 .. 0.21 over CASES
LOMB_SUB = 256
NORMALIZE = ("power", "normalize", "amplitude")
EPSNEG = float(np.finfo(np.float64).epsneg)


def e(p):
    return np.exp(2j * np.pi * p)


def _turn_of_products(f, t):
    """frac(f t) per frequency in rational arithmetic -> float64 [M]; t one number"""
    ft = fractions.Fraction(float(t))
    out = np.empty(len(f))
    for i, fv in enumerate(f):
        p = fractions.Fraction(float(fv)) * ft
        out[i] = float(p - round(p))
    return out


def exact_turns(f, t):
    """frac(f_m t_n) in rational arithmetic, float64 [N, M]"""
    return np.stack([_turn_of_products(f, tv) for tv in t])


def finish(common, rows, totals, mean, f, N, t_ref, floating_mean, normalize):
    """scipy's body on the sums: common [M, 4], rows [R, M, 2], totals [1 + 2R] -> P [R, M] (float64, or complex128)"""
    W = totals[0]
    C, S, C2, S2 = (common[:, k] / W for k in range(4))
    R = rows.shape[0]
    m = np.asarray(mean, dtype=np.float64).reshape(R, 1)
    Yp, YYp = (totals[1::2] / W).reshape(R, 1), (totals[2::2] / W).reshape(R, 1)
    YC, YS = rows[:, :, 0] / W, rows[:, :, 1] / W
    CC, CS = 0.5 * (1.0 + C2), 0.5 * S2
    SS = 1.0 - CC
    if floating_mean:
        YC, YS = YC - Yp * C, YS - Yp * S
        CC, SS, CS = CC - C * C, SS - S * S, CS - C * S
    else:
        YC, YS = YC + m * C, YS + m * S
    tau = 0.5 * np.arctan2(2.0 * CS, CC - SS)
    ct, st = np.cos(tau), np.sin(tau)
    YCt, YSt = YC * ct + YS * st, YS * ct - YC * st
    CCt = 0.5 * (1.0 + C2 * np.cos(2 * tau) + S2 * np.sin(2 * tau))
    SSt = 1.0 - CCt
    if floating_mean:
        Ct, St = C * ct + S * st, S * ct - C * st
        CCt, SSt = CCt - Ct * Ct, SSt - St * St
    CCt, SSt = np.maximum(CCt, EPSNEG), np.maximum(SSt, EPSNEG)
    a, b = YCt / CCt, YSt / SSt
    pg = 2.0 * (a * YCt + b * YSt)
    if normalize == "power":
        return pg * (N / 4.0)
    if normalize == "normalize":
        YY = YYp - Yp * Yp if floating_mean else YYp + 2.0 * m * Yp + m * m
        with np.errstate(divide="ignore", invalid="ignore"):
            return pg * (0.5 / YY)
    assert normalize == "amplitude"
    return (a + 1j * b) * np.exp(1j * tau) * e(_turn_of_products(f, t_ref))


def _prepare(t, y, w, precenter):
    t = np.asarray(t, dtype=np.float64)
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    w = np.ones(t.size) if w is None else np.asarray(w, dtype=np.float64)
    if precenter:
        y = y - y.mean(axis=-1, keepdims=True)
    return t, y, w / w.sum()


def sums_def(t, y, f, w=None, t_ref=None, mean=None, exact=False):
    """the float64 sums of rows y [R, N]: (common [M, 4], rows [R, M, 2], totals [1 + 2R]), weights normalised to sum to one"""
    t, y, wn = _prepare(t, y, w, False)
    f = np.asarray(f, dtype=np.float64)
    t_ref = float(t[0]) if t_ref is None else float(t_ref)
    m = np.zeros(y.shape[0]) if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
    d = y - m[:, None]
    if exact:
        assert t_ref == 0.0
        p = exact_turns(f, t)
    else:
        p = (t - t_ref)[:, None] * f[None, :]
        p -= np.rint(p)
    E1 = e(p)                                    # [N, M]
    A1, A2, B = wn @ E1, wn @ (E1 * E1), (wn * d) @ E1
    common = np.stack([A1.real, A1.imag, A2.real, A2.imag], axis=-1)
    rows = np.stack([B.real, B.imag], axis=-1)
    totals = np.empty(1 + 2 * y.shape[0])
    totals[0], totals[1::2], totals[2::2] = wn.sum(), (wn * d).sum(axis=-1), (wn * d * d).sum(axis=-1)
    return common, rows, totals


def lomb_def(t, y, f, w=None, floating_mean=False, normalize="power", precenter=False, exact=False):
    """the float64 closed form: P [R, M] of rows y [R, N] (one row: [1, M]); f in cycles per unit of t.  The conditioning offset is
    each row's mean, as it is on the device."""
    t, y, wn = _prepare(t, y, w, precenter)
    mean = y.mean(axis=-1)
    t_ref = 0.0 if exact else float(t[0])
    common, rows, totals = sums_def(t, y, f, wn, t_ref, mean, exact)
    return finish(common, rows, totals, mean, f, t.size, t_ref, floating_mean, normalize)


def front32(y, w, precenter, floating_mean):
    """pyfft_amd.lombscargle's way from float64 values to float32: centred in float64 first"""
    y = np.array(y, dtype=np.float64)
    if precenter:
        y -= y.mean()
    elif floating_mean:
        y -= np.average(y, weights=w)
    return y.astype(np.float32)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def sums_def32(t, y32, f, w=None, t_ref=None, mean=None):
    """the kernel's arithmetic on float32 rows y32 [R, N]: the sums as float64, in the layout of sums_def"""
    t = np.asarray(t, dtype=np.float64)
    y32 = np.atleast_2d(np.asarray(y32, dtype=np.float32))
    f = np.asarray(f, dtype=np.float64)
    w = np.ones(t.size) if w is None else np.asarray(w, dtype=np.float64)
    R, N, M = y32.shape[0], t.size, f.size
    t_ref = float(t[0]) if t_ref is None else float(t_ref)
    m = y32.astype(np.float64).mean(axis=-1) if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
    inv = 1.0 / w.sum()
    d = y32.astype(np.float64) - m[:, None]
    w32 = _f32(w * inv)
    wy32 = _f32((w * inv)[None, :] * d)
    totals = np.empty(1 + 2 * R)
    totals[0] = w32.astype(np.float64).sum()
    totals[1::2], totals[2::2] = wy32.astype(np.float64).sum(axis=-1), (wy32.astype(np.float64) * d).sum(axis=-1)
    acc64 = np.zeros((4 + 2 * R, M))
    tp = t - t_ref
    for n0 in range(0, N, LOMB_SUB):
        sl = slice(n0, min(n0 + LOMB_SUB, N))
        p = tp[sl, None] * f[None, :]
        p -= np.rint(p)
        pf = p.astype(np.float32).astype(np.float64)
        c, s = _f32(np.cos(2 * np.pi * pf)).astype(np.float64), _f32(np.sin(2 * np.pi * pf)).astype(np.float64)
        c2 = _f32(c * c - _f32(s * s).astype(np.float64)).astype(np.float64)         # fmaf(c, c, -(s s))
        s2 = _f32(2.0 * c * s).astype(np.float64)
        V = np.stack([c, s, c2, s2], axis=1)                                          # [n, 4, M]
        acc = np.zeros((4 + 2 * R, M), dtype=np.float32)
        wv, wyv = w32[sl].astype(np.float64), wy32[:, sl].astype(np.float64)
        for i in range(V.shape[0]):                                                   # float32 FMAs in the order of the samples
            acc[:4] = (acc[:4].astype(np.float64) + wv[i] * V[i]).astype(np.float32)
            if R:
                prod = wyv[:, i, None, None] * V[i, None, :2]                         # [R, 2, M]
                acc[4:] = (acc[4:].astype(np.float64) + prod.reshape(2 * R, M)).astype(np.float32)
        acc64 += acc.astype(np.float64)
    common = np.ascontiguousarray(acc64[:4].T)
    rows = np.ascontiguousarray(acc64[4:].reshape(R, 2, M).transpose(0, 2, 1))
    return common, rows, totals, m, t_ref


def lomb_def32(t, y32, f, w=None, floating_mean=False, normalize="power", t_ref=None, mean=None):
    """the kernels restated: P [R, M] as float64 / complex128, before the last rounding to float32"""
    common, rows, totals, m, t_ref = sums_def32(t, y32, f, w, t_ref, mean)
    return finish(common, rows, totals, m, np.asarray(f, dtype=np.float64), np.asarray(t).size, t_ref, floating_mean, normalize)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# a form: (weights, floating_mean, precenter, normalize)
FORMS24 = [(wt, fm, pc, nz) for wt, fm, pc in itertools.product((False, True), repeat=3) for nz in NORMALIZE]
SHAPES = {
    # a unit line over a 1 % floor, through pyfft_amd.lombscargle (float64 in): all 24 forms; f = 0 heads the list without a floating mean
    "n1000-m300": dict(N=1000, M=300, rows=1, pitch=0, seed=11, forms=FORMS24),
    # no multiple of LOMB_SUB or of a staged piece; a full tile of frequencies and one lane
    "tails": dict(N=777, M=257, rows=3, pitch=0, seed=16, forms=[(True, True, False, "normalize"), (False, False, False, "amplitude")]),
    # three row groups of eight whatever R <= 16 becomes; rows 3 and 11 ride on 10^3, row 7 is all zeros
    "rows-17": dict(N=500, M=130, rows=17, pitch=3, seed=13, forms=[(False, True, False, "power"), (True, False, False, "power")]),
    # SP_LOMB_SPLIT = 5: five runs of 300 samples
    "split-hook": dict(N=1500, M=100, rows=3, pitch=0, seed=14, forms=[(False, True, False, "normalize")]),
    # the plan itself deals the record to runs: 64 frequencies do not fill a device
    "split-plan": dict(N=1 << 16, M=64, rows=1, pitch=0, seed=15, forms=[(False, True, False, "normalize")]),
    # SP_LOMB_FREQS = 128: three passes, seams at 128 and 256
    "passes": dict(N=600, M=300, rows=2, pitch=0, seed=12, forms=[(True, True, False, "normalize")]),
    # times in no order, with duplicates, on both sides of zero
    "unsorted": dict(N=400, M=100, rows=1, pitch=0, seed=17, forms=[(False, True, False, "normalize"), (True, False, False, "amplitude")]),
    # the largest batch: 65537 columns of the prepared record go into more than one launch of the prep kernel, and 8192 row groups do not
    # fit one launch of the sums kernel (a tile of one group is 40 KiB of partials, 6553 of them make 256 MiB); the last group holds 7 rows
    "rows-max": dict(N=8, M=3, rows=65535, pitch=0, seed=18, forms=[(False, False, False, "power")]),
}
CASES = [(name, form) for name, s in SHAPES.items() for form in s["forms"]]
SPLIT_HOOK, FREQS_HOOK = 5, 128
LINE_F = 1.7                  # the line of every record, cycles per unit of t; the records span 100 units at a mean rate N / 100


def form_id(form):
    wt, fm, pc, nz = form
    return "%s%s%s-%s" % ("w" if wt else "e", "f" if fm else "n", "p" if pc else "r", nz)


@functools.lru_cache(maxsize=None)
def signals(name):
    """(t [N], y [rows, N] float64, w [N], f [M]); the rows of every shape but the first are float32 values"""
    s = SHAPES[name]
    N, M, rows = s["N"], s["M"], s["rows"]
    rng = np.random.default_rng(s["seed"])
    t = np.sort(rng.uniform(0.0, 100.0, N))
    if name == "unsorted":
        t = np.round(rng.uniform(-50.0, 50.0, N), 1)            # a grid of 0.1: duplicates are certain among 400 of 1001 values
        assert np.unique(t).size < N and t.min() < 0 < t.max() and np.any(np.diff(t) < 0)
    w = rng.uniform(0.2, 1.8, N)
    w[::17] = 0.0                                                # weights may be zero
    # from 1 / span on: below it a sinusoid, a constant and the record's window are close to collinear, and with a floating mean
    # the fit amplifies rounding in float64 as well (0.002 = 1 / (5 span) alone sets a restatement figure 100 times the rest's)
    f = np.linspace(0.01, 4.0, M)
    y = np.empty((rows, N))
    for r in range(rows if name != "rows-max" else 0):
        y[r] = np.sin(2 * np.pi * (LINE_F + 0.13 * r) * t + 0.3 + r) + 0.01 * rng.standard_normal(N) + 0.3
    if name == "rows-17":
        y[3] = 1e3 + rng.standard_normal(N)
        y[11] = 1e3 + rng.standard_normal(N) + np.sin(2 * np.pi * LINE_F * t)
        y[7] = 0.0
    if name == "rows-max":
        y = rng.standard_normal((rows, N)) + 0.3
    if name != "n1000-m300":
        y = y.astype(np.float32).astype(np.float64)
    for a in (t, y, w, f):
        a.setflags(write=False)
    return t, y, w, f


def freqs_of(name, form):
    """the frequency list of a case: f = 0 heads it where no floating mean is fitted (with one, 0 / 0 is rounding noise in scipy too)"""
    f = signals(name)[3]
    if not form[1]:
        f = np.concatenate([[0.0], f[1:]])
    return f


@functools.lru_cache(maxsize=None)
def reference(name, form):
    t, y, w, _ = signals(name)
    wt, fm, pc, nz = form
    out = lomb_def(t, y, freqs_of(name, form), w if wt else None, fm, nz, pc)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _sums32(name, wt, fm, pc, zero):
    t, y, w, _ = signals(name)
    ww = w if wt else None
    if name == "n1000-m300":
        y32 = front32(y[0], ww, pc, fm)[None, :]
    else:
        y32 = y.astype(np.float32)
    return sums_def32(t, y32, freqs_of(name, (wt, not zero, pc, "power")), ww)


def reference32(name, form):
    wt, fm, pc, nz = form
    key_fm, key_pc = (fm, pc) if name == "n1000-m300" else (False, False)      # what the float32 rows depend on
    common, rows, totals, m, t_ref = _sums32(name, wt, key_fm, key_pc, not fm)
    return finish(common, rows, totals, m, freqs_of(name, form), SHAPES[name]["N"], t_ref, fm, nz)


def deviation(got, ref):
    """the largest |got - ref| over the cells, each relative to its row's largest |ref|; a row of zeros must be met exactly"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.max(np.abs(ref), axis=-1, keepdims=True)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    assert not np.any(np.isnan(rel)), "a cell that is not a number"
    return float(np.max(rel))


def assert_within(got, ref, what="", allowance=None):
    """every cell within the allowance of its row's largest magnitude; returns the share of the allowance that was used"""
    allowance = ALLOWANCE if allowance is None else allowance
    used = deviation(got, ref) / allowance
    print("%s: worst cell at %.3f of its allowance" % (what, used))
    assert used <= 1.0, (what, used)
    return used
