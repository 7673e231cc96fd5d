"""The dynamic-range helper (tests/dynrange_ref.py) itself, on the CPU: the record is what it claims to be, the float64 references
agree with the oracle and with scipy, float32 arithmetic keeps a factor of two under the per-bin bound on every record the GPU
tests run (so the bound 2e-4 with no absolute term asks nothing that float32 cannot give), and the per-bin checkers reject a
-70 dB spur that the tolerance with an absolute term accepts."""
import numpy as np
import pytest
import scipy.signal

import dynrange_ref as D
from oracle import cpu_ref as O

NCU = D.NCU_MI355X
NFFT = D.NFFT


def hann():
    return O.windows("Hanning", nwins=NFFT)


# ---------------------------------------------------------------------------------------------------------------- the record
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_record_spans_80_db(cplx):
    win, hop, M = hann(), 2048, 300
    x = D.coloured_record(1, D.nsig_of(NFFT, hop, M), 5, NFFT, win, cplx=cplx)[0]
    assert x.dtype == (np.complex64 if cplx else np.float32)
    p = D.welch_psd64(x, win, hop, M)
    assert p.max() / np.median(p) >= 1e7
    assert np.mean(p <= 1e-6 * p.max()) >= 0.9                               # 90 % of the bins 60 dB or more below the line
    k = int(np.argmax(p)) - NFFT // 2
    assert abs(k - D.LINE_F * NFFT) < 1.0 and abs(D.LINE_F * NFFT - round(D.LINE_F * NFFT)) > 0.2      # at LINE_F, off bin centre
    # the line stands line_db over the floor at its frequency: the peak bin of an off-centre Hann line holds 0.5 - 1 of it
    floor = (2.0 if cplx else 1.0) * D.floor_at(D.LINE_F) * np.sum(win ** 2)
    assert 0.4e8 < p.max() / floor < 1.1e8


def test_record_weak_pair_and_channel_spread():
    win, hop, M = hann(), 2048, 300
    x = D.coloured_record(16, D.nsig_of(NFFT, hop, M), 6, NFFT, win)
    G = D.csd_matrix64(x, win, hop, M)
    d = np.einsum("kii->ki", G).real
    i, j = D.weak_pair_of(16)
    g2 = np.abs(G[:, i, j]) ** 2 / (d[:, i] * d[:, j])
    assert 0.003 < np.median(g2) < 0.03                                      # weak, and not lost
    other = np.abs(G[:, 0, 1]) ** 2 / (d[:, 0] * d[:, 1])
    assert np.median(other) < np.median(g2)                                  # (an independent pair: the estimator's bias 1/M only)
    peaks = d.max(axis=0)
    assert peaks.max() / peaks.min() < 10 ** 0.4                             # the channels stay within 4 dB of each other
    # the offsets dc (1 + c) / nch are there
    np.testing.assert_allclose(x.astype(np.float64).mean(axis=1), 3.0 * (1 + np.arange(16)) / 16, atol=0.5)


def test_record_256_is_the_one_the_nfft_256_test_always_had():
    """coloured_record_256 restated from the text it replaced in test_gpu_kernels.py"""
    from scipy.signal import lfilter
    nch, nsig, seed = 9, 3000, 33
    rng = np.random.default_rng(seed)
    x = np.stack([lfilter([1.0], [1.0, -0.97], rng.standard_normal(nsig)) for _ in range(nch)])
    common = lfilter([1.0], [1.0, -0.97], rng.standard_normal(nsig)) * np.sqrt(0.1 / 0.9)
    x[3] += common
    x[7] += common
    plain = x.astype(np.float32)
    assert np.array_equal(D.coloured_record_256(nch, nsig, seed), plain)
    w = 2 * np.pi * 0.237
    floor = 1.0 / abs(1.0 - 0.97 * np.exp(-1j * w)) ** 2
    for c in range(nch):
        x[c] += np.sqrt(floor * 1e8 * 4.0 * 1.5 / 256.0) * (1.0 + 0.1 * c) * np.cos(w * np.arange(nsig) + 0.4 * c)
    x += 0.3
    assert np.array_equal(D.coloured_record_256(nch, nsig, seed, line_db=80.0), x.astype(np.float32))


# ------------------------------------------------------------------------------------------------- the float64 references
def close(a, b, tol=1e-10):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= tol * np.max(np.abs(b))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_float64_psd_and_csd_against_oracle_and_scipy(cplx):
    """float64 input, nfft 256: welch_psd64 / welch_csd64 == oracle.welch_psd_stream == scipy.signal.welch / csd at 1e-10 of
    the peak (scipy detrends per segment, so the record's mean is taken off beforehand and both run without detrend)"""
    nfft, hop, M = 256, 64, 37
    win = O.windows("Nuttall4c", nwins=nfft)
    S2 = np.sum(win ** 2)
    rec = D.coloured_record(3, (M - 1) * hop + nfft, 8, nfft, win, line_db=40.0, cplx=cplx)
    rec = rec.astype(np.complex128 if cplx else np.float64)
    x, y = rec[0], rec[1:]
    p = D.welch_psd64(x, win, hop, M)
    close(p, O.welch_psd_stream(x, win, nfft, hop, M, 1.0) * S2)
    close(D.welch_psd64(x, win, hop, M, detrend=False), O.welch_psd_stream(x, win, nfft, hop, M, 1.0, detrend_style=0) * S2)
    close(D.welch_psd64(x, win, hop, M, detrend=0.25), O.welch_psd_stream(x - 0.25, win, nfft, hop, M, 1.0, detrend_style=0) * S2)
    xd, yd = x - x.mean(), y - y.mean(axis=1, keepdims=True)
    kw = dict(fs=1.0, window=win, nperseg=nfft, noverlap=nfft - hop, detrend=False, return_onesided=False, scaling="density")
    sh = lambda a: np.fft.fftshift(a, axes=-1) * S2
    close(p, sh(scipy.signal.welch(xd, **kw)[1]))
    pxx, pyy, pxy = D.welch_csd64(x, y, win, hop, M)
    close(pxx, p)
    close(pyy, sh(scipy.signal.welch(yd, **kw)[1]))
    close(pxy, sh(scipy.signal.csd(np.broadcast_to(xd, yd.shape), yd, **kw)[1]))       # scipy: conj(X) Y, ours: Y conj(X)
    if not cplx:
        one = D.one_sided(p)
        assert one.shape == (nfft // 2,)
        close(one[1:-1], 2.0 * np.fft.ifftshift(p)[1:nfft // 2 - 1])
        assert one[0] == np.fft.ifftshift(p)[0] and one[-1] == np.fft.ifftshift(p)[nfft // 2 - 1]


def test_float64_matrix_against_oracle():
    """csd_matrix64 (chunks of frames, batched matmul) == oracle.csd_matrix (frame by frame) at 1e-10; more than one chunk"""
    nfft, hop, M, nch = 256, 128, 23, 5
    win = O.windows("Hanning", nwins=nfft)
    x = D.coloured_record(nch, (M - 1) * hop + nfft + 17, 9, nfft, win, line_db=40.0).astype(np.float64)
    ref = O.csd_matrix(x, win, nfft, hop, M, 1.0) * np.sum(win ** 2)
    close(D.csd_matrix64(x, win, hop, M), ref)
    chunks = D._chunks
    try:
        D._chunks = lambda M, rows, nfft: [(g, min(M, g + 4)) for g in range(0, M, 4)]
        close(D.csd_matrix64(x, win, hop, M), ref)
    finally:
        D._chunks = chunks
    ref0 = O.csd_matrix(x, win, nfft, hop, M, 1.0, detrend_style=0) * np.sum(win ** 2)
    close(D.csd_matrix64(x, win, hop, M, detrend=False), ref0)
    # diagonal and first row are the PSD / CSD helpers (rfft bins)
    pxx, pyy, pxy = D.welch_csd64(x[0], x[1:], win, hop, M)
    half = lambda a: np.fft.ifftshift(a, axes=-1)[..., : nfft // 2 + 1]
    G = D.csd_matrix64(x, win, hop, M)
    close(G[:, 0, 0].real, half(pxx))
    close(G[:, 1:, 0].T, half(pxy))                                          # G_c0 = X_c conj(X_0) = pxy of channel c against x


# ---------------------------------------------------------------------------- the bound: what float32 costs on these records
def test_float32_costs_half_the_bound_at_most_psd():
    """every PSD record of tests/test_gpu_dynamic_range.py (at the MI355X's 256 CUs): the float32 restatement against the
    float64 reference, per bin, no absolute term.  <= 0.5 of the bound, i.e. a loss <= 1e-4 of the bin's own level."""
    worst = {}
    for name, case in D.psd_cases(NCU).items():
        if case["env"]:
            continue                                                         # (same record kind as its neighbour: the kernel differs)
        win = O.windows(case["window"], nwins=NFFT)
        x, det = D.psd_record(case, win)
        ref, f32 = D.welch_psd64(x, win, case["hop"], case["M"], det), D.welch_psd32(x, win, case["hop"], case["M"], det)
        worst[name], k = D.psd_excess(f32, ref)
        print("float32 restatement, %-32s loses %.2e of the bin's level at bin %d: %.2f of the bound"
              % (name, worst[name] * D.RTOL, k, worst[name]))
        assert 0 < worst[name] <= 0.5, name
        if not case["cplx"]:
            assert D.psd_excess(D.one_sided(f32), D.one_sided(ref))[0] <= 0.5, name


def test_float32_costs_half_the_bound_at_most_csd_pair():
    win, hop, M = hann(), D.CSD_PAIR["hop"], D.CSD_PAIR["M"]
    rec = D.coloured_record(3, D.nsig_of(NFFT, hop, M), D.CSD_PAIR["seed"], NFFT, win)
    ref, f32 = D.welch_csd64(rec[0], rec[1:], win, hop, M), D.welch_csd32(rec[0], rec[1:], win, hop, M)
    e = (D.psd_excess(f32[0], ref[0])[0], D.psd_excess(f32[1], ref[1])[0], D.cross_excess(f32[2], ref[2], ref[0][None], ref[1])[0])
    print("float32 restatement, welch_csd pair: pxx %.2f, pyy %.2f, pxy %.2f of the bound" % e)
    assert 0 < max(e) <= 0.5


@pytest.mark.parametrize("name", ["ch64", "ch16"])
def test_float32_costs_half_the_bound_at_most_matrix(name):
    """the matrix records' seeds and frame counts, the first 4 channels' worth (a 4-channel record of the same seed)"""
    case = D.matrix_cases(NCU)[name]
    win = hann()
    x = D.coloured_record(4, D.nsig_of(NFFT, case["hop"], case["M"]), case["seed"], NFFT, win)
    e, at = D.csd_excess(D.csd_matrix32(x, win, case["hop"], case["M"]), D.csd_matrix64(x, win, case["hop"], case["M"]))
    print("float32 restatement, csd_matrix %s: loses %.2e of sqrt(G_ii G_jj) at %s: %.2f of the bound" % (name, e * D.RTOL, at, e))
    assert 0 < e <= 0.5


# ---------------------------------------------------------------------------------------------- the gap the old tolerance left
def test_spur_70_db_below_the_line_passes_the_old_tolerance_and_fails_the_new():
    win, hop, M = hann(), 2048, 300
    x = D.coloured_record(1, D.nsig_of(NFFT, hop, M), 5, NFFT, win, cplx=True)[0]
    ref = D.welch_psd64(x, win, hop, M)
    k = NFFT // 2 + int(0.4 * NFFT)                                          # a quiet bin, far from the line and from the red end
    assert ref[k] < 1e-7 * ref.max()
    got = ref.copy()
    got[k] += 1e-7 * ref.max()                                               # a spur 70 dB below the line: twice the floor and more
    assert np.all(np.abs(got - ref) <= 2e-4 * ref + 1e-6 * ref.max())        # rtol 2e-4, atol 1e-6 max(Pxx): accepted
    e, at = D.psd_excess(got, ref)
    assert at == k and e > 1000.0                                            # per bin: off by more than 1000 x the bound
    assert D.psd_excess(ref * (1 + 1.9e-4), ref)[0] <= 1.0 < D.psd_excess(ref * (1 + 2.1e-4), ref)[0]


def test_spur_in_one_cross_term_passes_the_old_matrix_tolerance_and_fails_the_new():
    from test_gpu_kernels import _csd_per_bin_excess
    win, hop, M = hann(), 2048, 300
    x = D.coloured_record(4, D.nsig_of(NFFT, hop, M), 7, NFFT, win)
    ref = D.csd_matrix64(x, win, hop, M)
    gm = np.sqrt(np.einsum("kii->ki", ref).real)
    k = int(0.4 * NFFT)
    peak = (gm[:, 1] * gm[:, 2]).max()
    assert gm[k, 1] * gm[k, 2] < 1e-7 * peak
    G = ref.copy()
    G[k, 1, 2] += 0.9e-6 * peak * np.exp(0.7j)                               # 60 dB below the pair's peak, the floor 20 dB lower still
    assert _csd_per_bin_excess(G, ref) <= 1.0                                # 2e-4 sqrt(G_ii G_jj) + 1e-6 max_k: accepted
    e, at = D.csd_excess(G, ref)
    assert at == (k, 1, 2) and e > 1000.0
    G = ref.copy()
    G[k, 1, 2] += 1e-7 * peak                                                # and the 70 dB spur
    assert _csd_per_bin_excess(G, ref) <= 1.0 < D.csd_excess(G, ref)[0]
