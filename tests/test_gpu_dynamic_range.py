"""The nfft-4096 Welch, CSD and CSD-matrix kernels against float64 PER BIN over 80 dB: a coloured floor with a line 80 dB above
it (tests/dynrange_ref.py), every bin held to 2e-4 of its OWN level and every cross term to 2e-4 sqrt(G_ii G_jj), with no
absolute term.  The parity tests elsewhere allow 1e-6 of the peak on top, which on such a record is 100 x the floor: a spur
70 dB below the line would pass them.  float32 arithmetic itself loses 2e-5 .. 8e-5 on these records
(tests/test_host_dynrange_ref.py measures it on the CPU), so the bound asks nothing that the number format cannot give.

Everything runs at nfft 4096, the length the pipeline kernels are compiled for, and the frame counts are derived from the
chip's CU count so that the DEFAULT dispatch takes the kernel each case names (asserted with E.profile_last_kernel() where the
entry point records one)."""
import contextlib
import os

import numpy as np
import pytest

import dynrange_ref as D
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

NFFT = D.NFFT


@pytest.fixture(scope="module")
def E():
    from pyfft_amd import engine
    from pyfft_amd import _ffi
    _ffi.init()
    return engine


@pytest.fixture(scope="module")
def ncu(E):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def environ(env):
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def ran(kernel, how, text):
    return {"startswith": kernel.startswith(text), "equals": kernel == text, "contains": text in kernel}[how]


# ------------------------------------------------------------------------------------------------------------------- PSD
@pytest.mark.parametrize("name", list(D.psd_cases(D.NCU_MI355X)))
def test_welch_psd_per_bin_over_80_db(E, ncu, name):
    """one-pass pipeline (Hann, Nuttall4c; hop 2048, 1024), symmetric one-pass kernel (hop 4096), plain pipeline (no detrend),
    register-carried and generic kernels below the pipeline's threshold, and for real input the real-pair pipeline (mean and
    a given constant) and the symmetric real-pair kernel on an odd frame count (a lone last frame).  Two-sided, and one-sided
    as well for real input."""
    case = D.psd_cases(ncu)[name]
    hop, M = case["hop"], case["M"]
    win = O.windows(case["window"], nwins=NFFT)
    x, det = D.psd_record(case, win)
    kw = dict(detrend=det) if isinstance(det, bool) else dict(detrend=True, mean_value=det)
    with environ(case["env"]):
        got = E.welch_psd(x, win, hop, M, sided=E.SIDED_TWO, scale=1.0, **kw)
        kernel = E.profile_last_kernel()
        got1 = None if case["cplx"] else E.welch_psd(x, win, hop, M, sided=E.SIDED_ONE, scale=1.0, **kw)
    assert ran(kernel, *case["kernel"]), (kernel, case["kernel"], M)
    ref = D.welch_psd64(x, win, hop, M, det)
    e, k = D.psd_excess(got, ref)
    print("welch_psd %-32s %-32s M = %4d: per-bin excess %.3f (bin %d, %.1f dB below the line)"
          % (name, kernel, M, e, k, 10 * np.log10(ref.max() / ref[k])))
    assert e <= 1.0, (name, kernel, e, k)
    if got1 is not None:
        e1, k1 = D.psd_excess(got1, D.one_sided(ref))
        print("welch_psd %-32s one-sided: per-bin excess %.3f (bin %d)" % (name, e1, k1))
        assert e1 <= 1.0, (name, kernel, e1, k1)


# -------------------------------------------------------------------------------------------------------------- CSD pair
def test_welch_csd_per_bin_over_80_db(E):
    """x against two channels, one of them its weakly coherent partner (gamma^2 ~ 0.01): pxx and pyy to 2e-4 of each bin, pxy to
    2e-4 sqrt(pxx pyy) of each bin"""
    hop, M = D.CSD_PAIR["hop"], D.CSD_PAIR["M"]
    win = O.windows("Hanning", nwins=NFFT)
    rec = D.coloured_record(3, D.nsig_of(NFFT, hop, M), D.CSD_PAIR["seed"], NFFT, win)
    assert D.weak_pair_of(3) == (0, 2)
    x, y = rec[0], rec[1:]
    pxx, pyy, pxy = E.welch_csd(x, y, win, hop, M, detrend=True, sided=E.SIDED_TWO, scale=1.0)
    rxx, ryy, rxy = D.welch_csd64(x, y, win, hop, M)
    g2 = np.abs(rxy[1]) ** 2 / (rxx * ryy[1])
    assert 0.003 < np.median(g2) < 0.03
    e = {"pxx": D.psd_excess(pxx, rxx), "pyy": D.psd_excess(pyy, ryy), "pxy": D.cross_excess(pxy, rxy, rxx[None], ryy)}
    print("welch_csd M = %d: per-bin excess %s" % (M, ", ".join("%s %.3f at %s" % (n, v[0], np.array(v[1])) for n, v in e.items())))
    assert max(v[0] for v in e.values()) <= 1.0, e


# ------------------------------------------------------------------------------------------------------------ CSD matrix
def run_matrix(E, case, variants):
    """every variant's G against csd_matrix64 over all bins and pairs: ({variant: (excess, where)}, {variant: max |G - G_default|})"""
    nch, hop, M = case["nch"], case["hop"], case["M"]
    win = O.windows("Hanning", nwins=NFFT)
    x = D.coloured_record(nch, D.nsig_of(NFFT, hop, M), case["seed"], NFFT, win)
    ref = D.csd_matrix64(x, win, hop, M)
    d = np.einsum("kii->ki", ref).real
    assert d[:, 0].max() / np.median(d[:, 0]) >= 1e7
    i, j = D.weak_pair_of(nch)
    assert 0.003 < np.median(np.abs(ref[:, i, j]) ** 2 / (d[:, i] * d[:, j])) < 0.03
    worst, moved, G0 = {}, {}, None
    for tag, env in variants:
        with environ(env):
            G = E.csd_matrix(x, win, hop, M, detrend=True, scale=1.0)
        worst[tag] = D.csd_excess(G, ref)
        if G0 is None:
            G0 = G
        else:
            moved[tag] = float(np.max(np.abs(G - G0)))
        print("csd_matrix %d channels, M = %d, %-12s per-bin excess %.3f at (bin, i, j) = %s" % ((nch, M, tag) + worst[tag]))
    return worst, moved


def test_csd_matrix_64_channels_per_bin_over_80_db(E, ncu):
    """The shipped cfg5 path at its smallest: 64 channels and 64 ceil(ncu / 64) + 1 frames send the spectra through
    k_welch_pipe mode 5 (packed pair spectra), k_csdm_bf16 in its three-piece form, k_csdm_fold and the one-pass mean
    correction; the odd frame count leaves a half-filled last pair.  Also with the means by their own pass, with the per-frame
    spectra (k_stft_rp, no fold) and with the float32-MFMA contraction."""
    case = D.matrix_cases(ncu)["ch64"]
    assert 0 <= (case["M"] + 1) // 2 - 32 * ((ncu + 63) // 64) <= 1                     # at the pipeline spectra's threshold
    assert (case["M"] + 1) // 2 < 1024                                                  # three pieces
    worst, moved = run_matrix(E, case, (("default", {}), ("two_pass", {"SP_CSDM_TWOPASS": "1"}),
                                        ("no_pipe_spec", {"SP_CSDM_NOPIPESPEC": "1"}), ("fp32_mfma", {"SP_CSDM_FP32": "1"})))
    assert moved["no_pipe_spec"] > 0 and moved["two_pass"] > 0               # the packed path and the one-pass means really ran
    assert max(v[0] for v in worst.values()) <= 1.0, worst


def test_csd_matrix_16_channels_two_piece_per_bin_over_80_db(E, ncu):
    """16 channels, 2051 frames = 1026 frame pairs: the pipeline spectra and the TWO-piece contraction (operands rounded to 16
    significant bits), against the forced three-piece form"""
    case = D.matrix_cases(ncu)["ch16"]
    worst, moved = run_matrix(E, case, (("two_piece", {}), ("three_piece", {"SP_CSDM_SPLIT3": "1"})))
    assert moved["three_piece"] > 0                                          # two different kernels ran
    assert max(v[0] for v in worst.values()) <= 1.0, worst
