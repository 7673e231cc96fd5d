"""The FFT accumulation method restated in numpy, the shapes of tests/test_gpu_fam.py and the allowance they hold the kernel to.  A
helper module, not a test: nothing here is collected.

The definition (include/spectral_fam.h), in cycles per sample with e(t) = exp(2 pi i t): frame p = the np samples from p hop on, block b =
the frames bP .. bP + P - 1, Q = P hop / (2 np),

    X[p][k] = e(-k p hop / np) DFT_np( a[j] (x[p hop + j] - m_x) )[k]          (demodulated to absolute time; Y alike from y)
    T_b[q]  = sum_{p < P} g[p] Y[bP + p][k] conj(X[bP + p][l]) e(-q p / P)     (conj: ... X[bP + p][l], no conjugate)
    S[i][j] = scale sum_b T_b[j - Q],  j < 2Q,  for pair i = (k, l);   Pwx[k] = scale sum_b sum_p g[p] |X[bP + p][k]|^2

fam_def is that in float64, written with the explicit demodulation (shift=True: without it, the output bin moved instead, which is what
the kernel does).  fam_def32 is the same with complex64 transforms, a complex64 demodulation factor and float32 products; the blocks
add in complex64, the channel powers' float32 products in float64.

The allowance.  F32_DEV is the largest deviation of fam_def32 from fam_def over SHAPES -- S relative to the call's largest
sqrt(Pw_k Pw_l), Pw relative to the call's largest Pw -- as measured by tests/test_host_fam.py (which prints it and asserts it against
the constant).  The kernel gets that figure times a margin of 4 -- a different but legal summation order and its own transform
rounding -- which must stay below the project's parity figure of 2e-4, plus an absolute term of 1e-6 of the call's largest cell.  On
the device (MI355X) the worst cell of tests/test_gpu_fam.py used DEVICE_SHARE of that allowance."""
import functools

import numpy as np

import cyclic_ref as CR

F32_DEV = 1.0e-7          # measured 9.40e-8 (test_float32_restatement_deviation: np32-seven-blocks; numpy's complex64 transform)
MARGIN = 4.0
PARITY = 2e-4
ABS_TERM = 1e-6
ALLOWANCE = MARGIN * F32_DEV
DEVICE_SHARE = 0.086      # measured on an MI355X: the worst cell over tests/test_gpu_fam.py (np32-seven-blocks in 3 passes); 0.038 .. 0.086 per shape

NU_AM, GAMMA_AM = CR.NU_AM, CR.GAMMA_AM


def e(t):
    return np.cos(2 * np.pi * t) + 1j * np.sin(2 * np.pi * t)


def hamming(n):
    """scipy.signal.get_window('hamming', n): periodic"""
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / n)


def _frames(v, n, hop, nframes):
    return v[np.arange(nframes)[:, None] * hop + np.arange(n)[None, :]]


def _channels(v, a, hop, nframes, m, demod, ct):
    """[nframes][np] channelizer output of one record in the complex type ct"""
    n = a.size
    fr = ((_frames(v.astype(ct), n, hop, nframes) - ct(m)) * a.astype(ct).real).astype(ct)
    Z = np.fft.fft(fr, axis=-1).astype(ct)
    if demod:
        ph = (np.arange(n)[None, :] * ((np.arange(nframes)[:, None] * hop) % n)) % n          # k p hop mod np, exact
        Z = (Z * np.conj(e(ph / float(n))).astype(ct)).astype(ct)
    return Z


def _fam(x, a, hop, g, nblocks, pairs, y, conj, mx, my, scale, shift, ct, ft):
    x = np.asarray(x)
    a, g = np.asarray(a, dtype=np.float64), np.asarray(g, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    n, P = a.size, g.size
    nframes = nblocks * P
    twoQ = P * hop // n
    Q = twoQ // 2
    X = _channels(x, a, hop, nframes, mx, not shift, ct)
    Y = X if y is None else _channels(np.asarray(y), a, hop, nframes, mx if my is None else my, not shift, ct)
    gt = np.tile(g, nblocks).astype(ft)
    k, l = pairs[:, 0], pairs[:, 1]
    second = X[:, l] if conj else np.conj(X[:, l])
    prod = (gt[:, None] * (Y[:, k] * second).astype(ct)).astype(ct)
    T = np.fft.fft(prod.reshape(nblocks, P, -1), axis=1).astype(ct).sum(axis=0, dtype=ct)           # [P][npairs]
    j = np.arange(twoQ)
    if shift:
        d = (k + l) if conj else (k - l)
        rows = (j[None, :] - Q + d[:, None] * twoQ) % P
    else:
        rows = np.broadcast_to((j - Q) % P, (k.size, twoQ))
    S = ft(scale) * T[rows, np.arange(k.size)[:, None]]
    # (the products in ft, their sum over the frames in float64: a float32 sum that runs down 8192 frames loses 5e-6 by itself)
    pw = lambda Z: (ft(scale) * np.sum((gt[:, None] * (Z.real ** 2 + Z.imag ** 2).astype(ft)).astype(ft), axis=0, dtype=np.float64)).astype(ft)
    return S, pw(X), pw(Y)


def fam_def(x, a, hop, g, nblocks, pairs, y=None, conj=False, mx=0.0, my=None, scale=1.0, shift=False):
    """float64: (S complex128 [npairs, 2Q], Pwx, Pwy float64 [np])"""
    return _fam(x, a, hop, g, nblocks, pairs, y, conj, mx, my, scale, shift, np.complex128, np.float64)


def fam_def32(x, a, hop, g, nblocks, pairs, y=None, conj=False, mx=0.0, my=None, scale=1.0):
    """the same with complex64 transforms and float32 products (the module docstring says how they are summed): (S complex64, Pwx, Pwy float32)"""
    return _fam(x, a, hop, g, nblocks, pairs, y, conj, mx, my, scale, False, np.complex64, np.float32)


def all_pairs(n):
    k, l = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([k.ravel(), l.ravel()], axis=1).astype(np.int32)


def _pairs_p8192(n):
    """200 pairs: every k = l, the wrap pairs (0, np - 1) and (np / 2, np / 2 - 1), a run of l under k = 5, the rest seeded"""
    rng = np.random.default_rng(8192)
    fixed = [(k, k) for k in range(n)] + [(0, n - 1), (n // 2, n // 2 - 1)] + [(5, l) for l in range(n) if l != 5]
    rest = rng.integers(0, n, size=(200 - len(fixed), 2)).tolist()
    pr = np.array(fixed + rest, dtype=np.int32)
    return pr[np.lexsort((pr[:, 1], pr[:, 0]))]


def _pairs_seeded(n, count, seed):
    rng = np.random.default_rng(seed)
    pr = np.concatenate([np.array([(0, 0), (n - 1, n - 1), (0, n - 1), (n // 2, n // 2 - 1)]), rng.integers(0, n, size=(count - 4, 2))])
    return pr[np.lexsort((pr[:, 1], pr[:, 0]))].astype(np.int32)


# the shapes of test_gpu_fam.py: `tail` samples beyond the last block's last frame
SHAPES = {
    "np32-real-all": dict(cplx=False, np=32, hop=8, P=32, nblocks=3, conj=False, cross=False, tail=7 * 8 + 3, pairs=lambda: all_pairs(32)),
    "np64-cplx-q1": dict(cplx=True, np=64, hop=4, P=32, nblocks=2, conj=False, cross=False, tail=0, pairs=lambda: all_pairs(64)),
    "np64-p8192": dict(cplx=False, np=64, hop=16, P=8192, nblocks=1, conj=False, cross=False, tail=0, pairs=lambda: _pairs_p8192(64)),
    "np256-hop-np-conj": dict(cplx=True, np=256, hop=256, P=64, nblocks=2, conj=True, cross=False, tail=1,
                              pairs=lambda: _pairs_seeded(256, 300, 256)),
    "np128-cross": dict(cplx=False, np=128, hop=32, P=256, nblocks=2, conj=False, cross=True, tail=5, pairs=lambda: _pairs_seeded(128, 256, 128)),
    "np32-seven-blocks": dict(cplx=False, np=32, hop=8, P=32, nblocks=7, conj=False, cross=False, tail=3, pairs=lambda: all_pairs(32)),
}


def nsig_of(s, nblocks=None):
    nb = s["nblocks"] if nblocks is None else nblocks
    return (nb * s["P"] - 1) * s["hop"] + s["np"] + s["tail"]


@functools.lru_cache(maxsize=None)
def pairs_of(name):
    pr = np.ascontiguousarray(SHAPES[name]["pairs"]())
    pr.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def signals(name):
    """(x, y) of a shape, float32 or complex64, cyclostationary at NU_AM; y = a delayed, rescaled x plus noise of its own.  Computed once
    and shared: read-only."""
    s = SHAPES[name]
    rng = np.random.default_rng(sum(name.encode()))
    nsig = nsig_of(s)
    x = CR.am_noise(rng, nsig, s["cplx"])
    y = (0.7 * np.roll(x, 2) + 0.5 * CR.am_noise(rng, nsig, s["cplx"], 0.3)).astype(x.dtype)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def windows(name):
    """(a, g) float32: Hamming over the channelizer frame and over the block"""
    s = SHAPES[name]
    return hamming(s["np"]).astype(np.float32), hamming(s["P"]).astype(np.float32)


def _reference(name, fn):
    s = SHAPES[name]
    x, y = signals(name)
    a, g = windows(name)
    out = fn(x, a, s["hop"], g, s["nblocks"], pairs_of(name), y if s["cross"] else None, s["conj"], CR.row_mean(x),
             CR.row_mean(y) if s["cross"] else None)
    for o in out:
        o.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 (S, Pwx, Pwy) of a shape on the float32-rounded samples, windows and means; computed once, read-only"""
    return _reference(name, fam_def)


@functools.lru_cache(maxsize=None)
def reference32(name):
    return _reference(name, fam_def32)


def scales(ref, pairs):
    """the call's largest sqrt(Pwy[k] Pwx[l]) over its pairs, and its largest Pw"""
    S, Pwx, Pwy = ref
    pairs = np.asarray(pairs)
    return float(np.max(np.sqrt(Pwy[pairs[:, 0]] * Pwx[pairs[:, 1]]))), float(max(np.max(Pwx), np.max(Pwy)))


def deviation(got, ref, pairs):
    """the largest deviation of a triple from the reference triple: S relative to the call's largest sqrt(Pw_k Pw_l), Pw to its largest Pw"""
    ts, tp = scales(ref, pairs)
    return max(float(np.max(np.abs(got[0] - ref[0]))) / ts, float(np.max(np.abs(got[1] - ref[1]))) / tp,
               float(np.max(np.abs(got[2] - ref[2]))) / tp)


def bounds(ref, pairs):
    """the allowed |error| of a cell of S and of Pw: ALLOWANCE of the call's scale plus ABS_TERM of the call's largest cell"""
    ts, tp = scales(ref, pairs)
    return (ALLOWANCE * ts + ABS_TERM * float(np.max(np.abs(ref[0]))), ALLOWANCE * tp + ABS_TERM * tp, ALLOWANCE * tp + ABS_TERM * tp)


def assert_within(got, ref, pairs, what="", which=(0, 1, 2)):
    """every cell of the outputs within its bound; returns the largest share of a bound that was used"""
    assert ALLOWANCE > 0 and ALLOWANCE < PARITY
    bd = bounds(ref, pairs)
    worst = 0.0
    for i in which:
        g, r = np.asarray(got[i]), np.asarray(ref[i])
        assert g.shape == r.shape, (what, i, g.shape, r.shape)
        assert np.all(np.isfinite(g)), (what, i)
        worst = max(worst, float(np.max(np.abs(g - r))) / bd[i])
    print("%s: worst cell at %.3f of its allowance" % (what, worst))
    assert worst <= 1.0, (what, worst)
    return worst


# the amplitude-modulated noise records of the profile tests.  AM: the shape of the host test (tests/test_host_fam.py), under Hamming
# windows.  AM_GPU: the shape of the device test.  A cell that lies delta away from the centre of its tile is attenuated by the
# channelizer window's own response, |sum a^2 e(-delta j)| / sum a^2 in S and its square in |gamma|^2: NU_AM lies 0.00585 from the
# centre 1/32 = 2/64 of its tile, which costs |gamma|^2 3 % under a Hamming window of 32 taps and 12 % under one of 64 taps -- more than
# the 0.05 the check allows around GAMMA_AM^2 = 0.367 (the float64 reference gives 0.295 there).  The device test therefore runs its 64
# channels under a Gaussian window of standard deviation 7 samples, whose response costs 3 % as the host test's does.
AM = dict(np=32, hop=8, P=64, nblocks=3, window="hamming")
AM_GPU = dict(np=64, hop=16, P=256, nblocks=4, window=("gaussian", 7.0))


def tile_offset_loss(a, delta):
    """the factor on |gamma|^2 of a cell delta (cycles per sample) away from the centre of its tile, under the channelizer window a"""
    a = np.asarray(a, dtype=np.float64)
    return float(abs(np.sum(a * a * e(-delta * np.arange(a.size)))) / np.sum(a * a)) ** 2


@functools.lru_cache(maxsize=None)
def am_record(gpu=False):
    s = AM_GPU if gpu else AM
    rng = np.random.default_rng(20240611)
    x = CR.am_noise(rng, (s["nblocks"] * s["P"] - 1) * s["hop"] + s["np"], False)
    x.setflags(write=False)
    return x


def assert_am_profile(alphas, prof, s=AM):
    """the largest alpha > 0 bin below 0.5 is the grid point nearest NU_AM, and the mean |gamma|^2 there is within 0.05 of GAMMA_AM^2"""
    alphas, prof = np.asarray(alphas), np.asarray(prof)
    sel = np.nonzero((alphas > 0) & (alphas < 0.5))[0]
    peak = sel[np.argmax(prof[sel])]
    dalpha = 1.0 / (s["P"] * s["hop"])
    want = round(NU_AM / dalpha) * dalpha
    print("profile peak at alpha %.6f (grid point nearest NU_AM: %.6f), mean |gamma|^2 %.3f against GAMMA_AM^2 %.3f, median %.4f"
          % (alphas[peak], want, prof[peak], GAMMA_AM ** 2, float(np.median(prof[sel]))))
    assert abs(alphas[peak] - want) < 1e-9, (alphas[peak], want)
    assert abs(prof[peak] - GAMMA_AM ** 2) <= 0.05, prof[peak]
    return float(prof[peak])
