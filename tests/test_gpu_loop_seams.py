"""Every chunk, slice and row-batch loop of the host code past its first pass, on the MI355X, against the float64 references of
tests/seam_ref.py (whose planted defects tests/test_host_seam_ref.py shows to be 100 tolerances away on these very inputs).

    frame chunks     long_chunk_frames (192 MiB of spectra, at most 32768 frames) behind sp_welch_psd, sp_welch_csd, sp_stft, sp_stft_cog
                     and sp_zoom_welch on segments beyond one workgroup transform; the chunks of sp_csd_matrix (at most 16384 frames)
    row slices       dev_fft_any and sp_czt: 256 MiB of work buffer per slice of a batch of long transforms
    row batches      65535 rows per launch where the row is grid.y (cascaded sections, the filter bank's finish), and the
                     one-dimensional rows x blocks grids that recover the row by a division

At the DEFAULT budgets the shapes are the smallest that cross (re-derived from the constants by seam_ref and asserted in the host
test); under the hooks SP_LONG_CHUNK_FRAMES, SP_LONG_SLICE_ROWS and SP_CSDM_CHUNK_FRAMES tiny shapes walk three and more passes with
every detrend mode, real and complex, one- and two-sided.  Every test asserts engine.last_passes, or its row count, so that a later
change of a budget cannot quietly turn it back into a one-pass test.

Chunk independence is BITWISE where the code's summation order does not depend on the chunking, and the tests below hold it so:
k_long_acc_psd / k_long_acc_csd and k_zoom_acc add the frames in order into float64 sums that carry over from chunk to chunk; STFT
rows, centre-of-gravity rows, FFT rows and chirp-z rows are each computed from their own row alone.  Two outputs are held to their
tolerance instead: pseg of sp_stft on long segments (k_long_pack adds one float64 atomic per workgroup and a frame has several
workgroups, in an order that changes from run to run), and sp_csd_matrix (every chunk is contracted in float32 and added to G).

Tolerances, the project's own: PSD / CSD rtol 2e-4 with atol 1e-6 (2e-6 for cross spectra) of the largest value; CSD matrix 2e-4
sqrt(G_ii G_jj) + 1e-6 max_k; STFT, Hilbert and chirp-z rows 1e-4 of the largest value; FFT 4e-6 sqrt(log2 n); cascaded sections 5e-7
of the row's peak; resampler and down-converter 4 x the loss of a float32 restatement; filter bank as tests/test_gpu_channelizer.py."""
import functools

import numpy as np
import pytest
import scipy.signal as ss

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

import detrend_ref as R                                                      # noqa: E402
import seam_ref as S                                                         # noqa: E402
from pyfft_amd import engine as E, channelizer as CH                   # noqa: E402

FS = 1000.0
RAW, TWO, ONE = E.SIDED_RAW, E.SIDED_TWO, E.SIDED_ONE
MODE_ARG = {R.CONST: 0, R.MEAN: 1, R.LINEAR: 2, R.SEGMEAN: 3, R.SEGLINEAR: 4}


def close(got, ref, tol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = float(np.max(np.abs(got - ref) / np.maximum(tol, 1e-300)))
    print("%s: worst error %.3g of its tolerance" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def passed(chunks=None, slices=None):
    """the passes the last call made; asserted equal to what the test claims"""
    if chunks is not None:
        assert E.last_passes(0) == chunks, ("frame chunks", E.last_passes(0), chunks)
    if slices is not None:
        assert E.last_passes(1) == slices, ("row slices", E.last_passes(1), slices)


def interest(case, L=None):
    return S.rows_of_interest(case.nframes, S.seams_of(case.nframes, case.mc, case.nfft if L is None else L))


# ================================================================================================ default budgets: frame chunks
@functools.lru_cache(maxsize=None)
def psd_ref(case, mode):
    return S.psd_sum(S.case_record(case), S.window(case.nfft), case.hop, np.arange(case.nframes), mode) / case.nframes


@functools.lru_cache(maxsize=None)
def rows_ref(case, mode):
    """(rows, X[rows, nfft], pseg[rows]) on the rows of interest"""
    rows = interest(case)
    return (rows,) + S.spectra_rows(S.case_record(case), S.window(case.nfft), case.hop, rows, mode)


@pytest.mark.parametrize("mode", [R.MEAN, R.LINEAR], ids=["mean", "linear"])
@pytest.mark.parametrize("case", [S.W4100, S.W16384], ids=lambda c: c.id)
def test_welch_psd_crosses_a_chunk(case, mode):
    """6138 + 7 frames of 4100 (float32; the first chunk's transform makes three Bluestein slices) and 1536 + 7 of 16384 (complex64)"""
    got = E.welch_psd(S.case_record(case), S.window(case.nfft), case.hop, case.nframes, detrend=MODE_ARG[mode], sided=RAW, scale=1.0)
    passed(chunks=2, slices=S.passes(case.mc, S.long_slice_rows(case.nfft)))
    ref = psd_ref(case, mode)
    close(got, ref, S.tol_psd(ref), "welch_psd %s mode %d" % (case.id, mode))


@pytest.mark.parametrize("mode", [R.MEAN, R.SEGMEAN, R.SEGLINEAR], ids=["mean", "segmean", "seglinear"])
def test_stft_crosses_a_chunk(mode):
    """sp_stft on 6145 frames of 4100: frames and pseg (segmean and seglinear go through k_long_segstats with f0); with mean detrend
    also the power output in the bin-major layout.  Compared on the rows around every chunk and slice seam, the first and last rows
    and every 61st."""
    case = S.W4100
    x, win = S.case_record(case), S.window(case.nfft)
    rows, X, pseg = rows_ref(case, mode)
    out, ps = E.stft_frames(x, win, case.hop, case.nframes, detrend=MODE_ARG[mode], sided=RAW, amp_scale=0.5, want_pseg=True)
    passed(chunks=2, slices=3)
    assert out.shape == (case.nframes, case.nfft)
    close(out[rows], 0.5 * X, S.tol_rows(0.5 * X), "frames")
    close(ps[rows], pseg, 1e-4 * pseg, "pseg")
    assert np.all(np.abs(out).max(axis=1) > 0) and np.all(ps > 0)             # every row was written
    if mode == R.MEAN:
        pw, _ = E.stft_frames(x, win, case.hop, case.nframes, detrend=1, sided=TWO, amp_scale=2.0, power=True, bin_major=True)
        passed(chunks=2, slices=3)
        assert pw.shape == (case.nfft, case.nframes) and pw.dtype == np.float32
        ref = np.fft.fftshift(2.0 * np.abs(X) ** 2, axes=1).T
        close(pw[:, rows], ref, S.tol_psd(ref), "power, bin-major")


def test_welch_csd_and_cog_cross_a_chunk():
    """sp_welch_csd (x against 2 channels) and sp_stft_cog on 1536 + 7 complex frames of 16384"""
    case = S.W16384
    x, win, M = S.case_record(case), S.window(case.nfft), case.nframes
    y = np.stack([S.case_record(case, 1), S.case_record(case, 2)])
    pxx, pyy, pxy = E.welch_csd(x, y, win, case.hop, M, detrend=True, sided=TWO, scale=1.0)
    passed(chunks=2, slices=1)
    sxx, syy, sxy = (np.fft.fftshift(a, axes=-1) / M for a in S.csd_sums(x, y, win, case.hop, np.arange(M), R.MEAN))
    close(pxx, sxx, S.tol_psd(sxx), "pxx")
    close(pyy, syy, S.tol_psd(syy), "pyy")
    close(pxy, sxy, S.tol_csd(sxy), "pxy")
    rows, X, _ = rows_ref(case, R.MEAN)
    cog = E.stft_cog(x, win, case.hop, M, FS, detrend=True)
    passed(chunks=2, slices=1)
    ref = S.cog_of(X, FS)
    close(cog[rows], ref, 2e-4 * np.abs(ref) + 1e-4, "cog")
    assert np.all(cog != 0)


def test_zoom_crosses_a_chunk():
    """zoom_psd / zoom_csd / zoom_stft: 1536 + 7 frames of 8100 on an arc of 100 bins (a chirp-z on 16384 points): launch_czt_pre,
    launch_czt_post and k_zoom_acc with f0 > 0"""
    case = S.Z8100
    x, y, win, M = S.case_record(case), S.case_record(case, 1), S.window(case.nfft), case.nframes
    Em = S.arc(case.nfft, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP)
    sxx, syy, sxy = (a / M for a in S.zoom_sums(x, y, win, case.hop, np.arange(M), R.MEAN, Em))
    pxx, _, _ = E.zoom_welch(x, win, case.hop, M, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP, detrend=True)
    passed(chunks=2)
    close(pxx, sxx, S.tol_psd(sxx), "zoom psd")
    pxx, pyy, pxy = E.zoom_welch(x, win, case.hop, M, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP, y=y, detrend=True)
    passed(chunks=2)
    close(pxx, sxx, S.tol_psd(sxx), "zoom csd pxx")
    close(pyy, syy, S.tol_psd(syy), "zoom csd pyy")
    close(pxy, sxy, S.tol_csd(sxy), "zoom csd pxy")
    fr = E.zoom_welch(x, win, case.hop, M, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP, detrend=True, frames=True)
    passed(chunks=2)
    rows = S.rows_of_interest(M, [case.mc])
    Z = S.zoom_rows(x, win, case.hop, rows, R.MEAN, Em)
    close(fr[rows], Z, S.tol_rows(Z), "zoom stft")
    assert np.all(np.abs(fr).max(axis=1) > 0)


@pytest.mark.parametrize("mode", [R.MEAN, R.LINEAR], ids=["mean", "linear"])
@pytest.mark.parametrize("case", S.CSDM_DEFAULT, ids=lambda c: c.id)
def test_csd_matrix_crosses_a_chunk(case, mode):
    """16500 frames = chunks of 8256 + 8244: k_trend_shift by f0 hop, the ragged padding of the second chunk; k_stft_rp + bf16 (nfft 32,
    2 channels), k_stft + k_csdm_fused (nfft 30, 3 channels) and the transposed fp32-MFMA form (65 channels)"""
    x, win, M = S.csdm_record(case), S.window(case.nfft), case.nframes
    assert S.passes(M, S.csdm_mc(case)) == 2
    got = E.csd_matrix(x, win, case.hop, M, detrend=MODE_ARG[mode], scale=1.0)
    passed(chunks=2)
    ref = S.csdm_sum(x, win, case.hop, np.arange(M), mode) / M
    close(got, ref, S.tol_csdm(ref), "csd_matrix %s mode %d" % (case.id, mode))


def test_csd_matrix_pipeline_crosses_a_chunk():
    """nfft 4096 / hop 2048, 2 channels, 2 x 8191 + 33 frames: chunks of 8224 + 8191, the fewest frames with which both chunks
    satisfy pipe_spec (32 pairs per run on each of ceil(256 / 2) runs).  The second chunk runs with h_init = 0 on the packed spectra
    and cm_onepass is off.  The record is generated on the device (seam_ref.pipe_channels); the reference is float64 over the same
    samples, in blocks."""
    import torch
    nch, nfft, hop = 2, 4096, 2048
    need = S.pipe_spec_min_frames(nch)
    M = 2 * need + 33
    mc = S.csdm_chunk_frames(nch, nfft, M)
    assert [m for _, m in S.chunks(M, mc)] == [mc, need] and mc >= need
    xt = S.pipe_channels(torch, nch, (M - 1) * hop + nfft, device="cuda")
    win = S.window(nfft)
    got = E.csd_matrix(xt, win, hop, M, detrend=True, scale=1.0)
    passed(chunks=2)
    assert E.profile_last_kernel() == "k_welch_pipe(spectra)"
    ref = S.csdm_sum(xt.cpu().numpy(), win, hop, np.arange(M), R.MEAN, block=1024) / M
    close(got.cpu().numpy(), ref, S.tol_csdm(ref), "csd_matrix, pipeline")


# ================================================================================================= default budgets: row slices
@pytest.mark.parametrize("nrows,n", [(2049, 16384), (2051, 4100)], ids=["pow2", "bluestein"])
def test_fft_crosses_a_slice(nrows, n):
    """fft / ifft of 2049 x 16384 (slices of 2048 five-pass transforms) and 2051 x 4100 (Bluestein on 16384 points): every row against
    numpy in float64.  ifft(x)[k] = fft(x)[-k mod n] / n gives the inverse's reference from the forward one."""
    x = S.sliding_rows(n, nrows, n)
    assert S.passes(nrows, S.long_slice_rows(n)) == 2
    ref = np.concatenate([np.fft.fft(x[a:a + 256].astype(np.complex128), axis=1) for a in range(0, nrows, 256)])
    got = E.fft(x)
    passed(slices=2)
    close(got, ref, S.tol_fft(n, ref), "fft %d x %d" % (nrows, n))
    iref = ref[:, (-np.arange(n)) % n] / n
    got = E.ifft(x)
    passed(slices=2)
    close(got, iref, S.tol_fft(n, iref), "ifft %d x %d" % (nrows, n))


def test_czt_crosses_a_slice():
    """2050 rows of 8100 on an arc of 100 bins: slices of 2048 rows through launch_czt_pre / launch_czt_post with b0 > 0"""
    x = S.sliding_rows(3, 2050, S.CZT_N, False)
    got = E.czt(x, S.CZT_M, S.ZOOM_START, S.ZOOM_STEP)
    passed(slices=2)
    ref = x.astype(np.float64) @ S.arc(S.CZT_N, S.CZT_M, S.ZOOM_START, S.ZOOM_STEP)
    close(got, ref, S.tol_rows(ref), "czt 2050 x 8100")


# ===================================================================================================================== under the hooks
def hooked(monkeypatch, chunk=0, rows=0, csdm=0):
    for name, v in (("SP_LONG_CHUNK_FRAMES", chunk), ("SP_LONG_SLICE_ROWS", rows), ("SP_CSDM_CHUNK_FRAMES", csdm)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)


def _tiny_calls(case, label, arg, value):
    """name -> call: every long-path entry at a tiny shape under one detrend mode"""
    x, win, hop, M = S.case_record(case), S.window(case.nfft), case.hop, case.nframes
    y = np.stack([S.case_record(case, 1), S.case_record(case, 2)])
    two = TWO if case.cplx else ONE
    calls = {
        "psd-raw": lambda: E.welch_psd(x, win, hop, M, detrend=arg, sided=RAW, scale=1.0, mean_value=value),
        "psd-sided": lambda: E.welch_psd(x, win, hop, M, detrend=arg, sided=two, scale=1.0, mean_value=value),
        "stft-raw": lambda: E.stft_frames(x, win, hop, M, detrend=arg, sided=RAW, amp_scale=1.0, want_pseg=True, mean_value=value),
        "stft-sided": lambda: E.stft_frames(x, win, hop, M, detrend=arg, sided=two, amp_scale=1.0, mean_value=value)[0],
        "power-bin-major": lambda: E.stft_frames(x, win, hop, M, detrend=arg, sided=two, power=True, bin_major=True, mean_value=value)[0],
        "cog": lambda: E.stft_cog(x, win, hop, M, FS, detrend=arg, mean_value=value),
    }
    if value is None:                                    # (welch_csd takes no constant)
        calls["csd-raw"] = lambda: E.welch_csd(x, y, win, hop, M, detrend=arg, sided=RAW, scale=1.0)
        calls["csd-sided"] = lambda: E.welch_csd(x, y, win, hop, M, detrend=arg, sided=two, scale=1.0)
    return calls


@pytest.mark.parametrize("case", S.TINY, ids=lambda c: c.id)
def test_hooked_frame_chunks_are_bitwise(case, monkeypatch):
    """7 frames in chunks of 3 + 3 + 1 (and the transforms of a chunk in slices of 2 + 1 rows) against the same call in one pass:
    bit for bit, for every detrend mode of include/spectral.h, one- and two-sided; pseg to its tolerance (float64 atomics of several
    workgroups per frame).  The un-hooked results are also held to the float64 reference."""
    x, win, hop, M = S.case_record(case), S.window(case.nfft), case.hop, case.nframes
    idx = np.arange(M)
    for label, arg, value, mode in R.mode_cases(case.cplx):
        hooked(monkeypatch)
        calls = _tiny_calls(case, label, arg, value)
        plain = {}
        for name, call in calls.items():
            plain[name] = call()
            passed(chunks=1, slices=1)
        hooked(monkeypatch, chunk=3, rows=2)
        for name, call in calls.items():
            again = call()
            passed(chunks=3, slices=2)
            what = "%s %s %s" % (case.id, label, name)
            if name == "stft-raw":
                same_bits(again[0], plain[name][0], what)
                close(again[1], plain[name][1], 1e-4 * np.abs(plain[name][1]), what + " pseg")
            elif name.startswith("csd"):
                for a, b in zip(again, plain[name]):
                    same_bits(a, b, what)
            else:
                same_bits(again, plain[name], what)
        xs = S._wide(x) - (0 if value is None else value)
        X, pseg = S.spectra_rows(xs, win, hop, idx, mode)
        P = (np.abs(X) ** 2).mean(axis=0)
        close(plain["psd-raw"], P, S.tol_psd(P), "%s %s psd against float64" % (case.id, label))
        close(plain["stft-raw"][0], X, S.tol_rows(X), "%s %s frames against float64" % (case.id, label))
        close(plain["stft-raw"][1], pseg, 1e-4 * pseg, "%s %s pseg against float64" % (case.id, label))
        if case.cplx:
            ref = S.cog_of(X, FS)
            close(plain["cog"], ref, 2e-4 * np.abs(ref) + 1e-4, "%s %s cog against float64" % (case.id, label))
        if value is None:
            y = np.stack([S.case_record(case, 1), S.case_record(case, 2)])
            sums = S.csd_sums(x, y, win, hop, idx, mode)
            for got, ref, tol in zip(plain["csd-raw"], sums, (S.tol_psd, S.tol_psd, S.tol_csd)):
                close(got, ref / M, tol(ref / M), "%s %s csd against float64" % (case.id, label))


@pytest.mark.parametrize("case", S.TINY_ZOOM, ids=lambda c: c.id)
def test_hooked_zoom_chunks_are_bitwise(case, monkeypatch):
    """zoom_psd / zoom_csd / zoom_stft, 7 frames of 8100 in chunks of 3 + 3 + 1: k_zoom_acc adds the frames in order into float64
    sums that carry over, so the result does not depend on the chunking"""
    x, y, win, hop, M = S.case_record(case), S.case_record(case, 1), S.window(case.nfft), case.hop, case.nframes
    Em = S.arc(case.nfft, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP)
    for mode in (R.CONST, R.MEAN, R.LINEAR):
        calls = {"psd": lambda: E.zoom_welch(x, win, hop, M, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP, detrend=MODE_ARG[mode])[0],
                 "csd": lambda: E.zoom_welch(x, win, hop, M, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP, y=y, detrend=MODE_ARG[mode]),
                 "stft": lambda: E.zoom_welch(x, win, hop, M, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP, detrend=MODE_ARG[mode], frames=True)}
        hooked(monkeypatch)
        plain = {}
        for name, call in calls.items():
            plain[name] = call()
            passed(chunks=1)
        hooked(monkeypatch, chunk=3)
        for name, call in calls.items():
            again = call()
            passed(chunks=3)
            for a, b in zip(again, plain[name]) if name == "csd" else ((again, plain[name]),):
                same_bits(a, b, "%s mode %d zoom %s" % (case.id, mode, name))
        sums = S.zoom_sums(x, y, win, hop, np.arange(M), mode, Em)
        for got, ref, tol in zip(plain["csd"], sums, (S.tol_psd, S.tol_psd, S.tol_csd)):
            close(got, ref / M, tol(ref / M), "%s mode %d zoom csd against float64" % (case.id, mode))
        Z = S.zoom_rows(x, win, hop, np.arange(M), mode, Em)
        close(plain["stft"], Z, S.tol_rows(Z), "%s mode %d zoom stft against float64" % (case.id, mode))


def test_hooked_row_slices_are_bitwise(monkeypatch):
    """fft / ifft of 7 x 16384 and 7 x 4100 and a chirp-z of 7 x 8100 in slices of 2 + 2 + 2 + 1 rows: every row is computed from
    its own samples alone"""
    calls = {}
    for n in (16384, 4100):
        x = S.sliding_rows(n, 7, n)
        calls["fft %d" % n] = (lambda x=x: E.fft(x), np.fft.fft(x.astype(np.complex128), axis=1), n)
        calls["ifft %d" % n] = (lambda x=x: E.ifft(x), np.fft.ifft(x.astype(np.complex128), axis=1), n)
    xr = S.sliding_rows(3, 7, S.CZT_N, False)
    calls["czt"] = (lambda: E.czt(xr, S.CZT_M, S.ZOOM_START, S.ZOOM_STEP),
                    xr.astype(np.float64) @ S.arc(S.CZT_N, S.CZT_M, S.ZOOM_START, S.ZOOM_STEP), 0)
    for name, (call, ref, n) in calls.items():
        hooked(monkeypatch)
        plain = call()
        passed(slices=1)
        hooked(monkeypatch, rows=2)
        again = call()
        passed(slices=4)
        same_bits(again, plain, name)
        close(plain, ref, S.tol_fft(n, ref) if n else S.tol_rows(ref), name + " against float64")


@pytest.mark.parametrize("mode", [R.MEAN, R.LINEAR], ids=["mean", "linear"])
@pytest.mark.parametrize("case", S.CSDM_HOOKED, ids=lambda c: c.id)
def test_hooked_csd_matrix_chunks(case, mode, monkeypatch):
    """sp_csd_matrix under SP_CSDM_CHUNK_FRAMES = 32, 64 and 96 (5 channels, nfft 256, 333 frames: 11, 6 and 4 chunks, the last one
    ragged), and on the long path (3 channels, nfft 9000, 70 frames: 32 + 32 + 6, then with SP_LONG_CHUNK_FRAMES = 20 the smaller of
    the two chunk lengths, 20 + 20 + 20 + 10).  Every chunk is contracted in float32 and added to G, so the result is held to the
    tolerance, not to the bits of the one-chunk run."""
    x, win, M = S.csdm_record(case), S.window(case.nfft), case.nframes
    ref = S.csdm_sum(x, win, case.hop, np.arange(M), mode) / M
    tol = S.tol_csdm(ref)
    hooked(monkeypatch)
    close(E.csd_matrix(x, win, case.hop, M, detrend=MODE_ARG[mode], scale=1.0), ref, tol, case.id + " one chunk")
    passed(chunks=1)
    hooked(monkeypatch, csdm=case.cap)
    close(E.csd_matrix(x, win, case.hop, M, detrend=MODE_ARG[mode], scale=1.0), ref, tol, case.id)
    passed(chunks=S.passes(M, S.csdm_mc(case)))
    if not S.wg_capable(case.nfft):
        hooked(monkeypatch, csdm=case.cap, chunk=20)
        close(E.csd_matrix(x, win, case.hop, M, detrend=MODE_ARG[mode], scale=1.0), ref, tol, case.id + ", long chunks of 20")
        passed(chunks=4)


# ===================================================================================================== more than 65535 rows
def by_batch(got, ref, rel, what):
    """max error over `rel` of the largest reference value, taken separately over the rows of either row batch (the second is louder)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for name, sl in (("rows below 65535", slice(0, S.ROW_BATCH)), ("rows from 65535", slice(S.ROW_BATCH, None))):
        if ref[sl].size:
            close(got[sl], ref[sl], rel * np.max(np.abs(ref[sl])), "%s, %s" % (what, name))


def by_row(got, ref, rel, what):
    """every row against `rel` of its own peak (tests/test_gpu_iir.py)"""
    ref = np.asarray(ref)
    close(got, ref, rel * np.max(np.abs(ref.reshape(ref.shape[0], -1)), axis=1).reshape((-1,) + (1,) * (ref.ndim - 1)), what)


def alone(call, whole, what):
    """row r of the whole batch equals the same row computed alone, bit for bit, on either side of the seam"""
    for r in S.ALONE:
        one = call(r)
        same_bits(np.asarray(one).reshape(np.asarray(whole[r]).shape), whole[r], "%s, row %d alone" % (what, r))


@pytest.mark.parametrize("K", [1, 8])
def test_row_batches_sos_filter(K):
    """sp_sosfilt, 65538 rows of 40 samples with zi given and zf returned: sos_pass_k offsets x, y, zi, zf, tile_end and tile_in by r0"""
    sos = S.sos_design(K)
    x = S.batch_rows(40 + K, S.SOS_N)
    x64 = x.astype(np.float64)
    zi = S.sos_zi(sos, x64)
    want, zf_want = ss.sosfilt(sos, x64, axis=-1, zi=zi)
    y, zf = E.sos_filter(sos, x, zi=zi)
    assert y.shape == (S.ROWS, S.SOS_N) and zf.shape == zi.shape
    by_row(y, want, 5e-7, "sos_filter K %d" % K)
    by_batch(zf.transpose(1, 0, 2), zf_want.transpose(1, 0, 2), 1e-6, "zf")
    alone(lambda r: E.sos_filter(sos, x[r:r + 1], zi=zi[:, r:r + 1])[0], y, "sos_filter")
    plain = E.sos_filter(sos, x)
    by_row(plain, ss.sosfilt(sos, x64, axis=-1), 5e-7, "sos_filter K %d, from rest" % K)


def test_row_batches_sos_filtfilt():
    sos = S.sos_design(3)
    x = S.batch_rows(50, S.SOS_N)
    y = E.sos_filtfilt(sos, x, padtype="odd", padlen=S.FILTFILT_PAD)
    assert y.shape == (S.ROWS, S.SOS_N)
    by_row(y, ss.sosfiltfilt(sos, x.astype(np.float64), axis=-1, padtype="odd", padlen=S.FILTFILT_PAD), 5e-7, "sos_filtfilt")
    alone(lambda r: E.sos_filtfilt(sos, x[r:r + 1], padtype="odd", padlen=S.FILTFILT_PAD), y, "sos_filtfilt")


def test_row_batches_filter_bank():
    """pfb_psd (launch_pfb_finish: partial + b0 G M, out + b0 nb), channelize and synthesize at M = 8, 2 taps per channel, 5 frames:
    the one-dimensional rows x blocks grids of k_pfb and k_pfb_synth recover the row by a division"""
    from test_host_channelizer import pfb_ref
    from test_host_pfb_synth import pfb_synth_ref
    from test_gpu_pfb_synth import tap64
    M, P, hop, nf = S.PFB_M, S.PFB_P, S.PFB_HOP, S.PFB_FRAMES
    h = CH.pfb_prototype(M, P) * M
    h64 = np.asarray(h, dtype=np.float32).astype(np.float64)
    nsig = M * P + (nf - 1) * hop
    x = S.batch_rows(nsig, nsig)
    ref = pfb_ref(x.astype(np.float64), h64, M, hop, 0, nf)[..., :M // 2 + 1]
    X = E.pfb(x, h, M, hop, 0, nf)
    assert X.shape == (S.ROWS, nf, M // 2 + 1)
    by_batch(X, ref, 1e-4, "pfb frames")
    alone(lambda r: E.pfb(x[r:r + 1], h, M, hop, 0, nf), X, "pfb frames")
    Xt = E.pfb(x, h, M, hop, 0, nf, out_major=1)
    same_bits(np.swapaxes(Xt, -1, -2), X, "channelize layout")
    psd = E.pfb(x, h, M, hop, 0, nf, power=True, scale=1.0)
    pref = (np.abs(ref) ** 2).mean(axis=1)
    close(psd, pref, 2e-4 * pref + 1e-6 * pref.max(axis=1, keepdims=True), "pfb_psd")
    for r in S.ALONE:
        one = E.pfb(x[r:r + 1], h, M, hop, 0, nf, power=True, scale=1.0)[0]
        close(one, pref[r], 2e-4 * pref[r] + 1e-6 * pref[r].max(), "pfb_psd, row %d alone" % r)
    yref = pfb_synth_ref(X, tap64(h, M, 1.0), M, hop, 0, nsig, onesided=True)
    y = E.pfb_synth(X, h, M, hop, 0, nsig, onesided=True)
    assert y.shape == (S.ROWS, nsig) and y.dtype == np.float32
    by_batch(y, yref, 1e-4, "pfb_synth")
    alone(lambda r: E.pfb_synth(X[r:r + 1], h, M, hop, 0, nsig, onesided=True), y, "pfb_synth")


def _restated(got, ref, f32, what):
    """the bound of tests/test_gpu_baseband.py and tests/test_gpu_resample.py, per row batch: max error over the rms of the
    reference at most 4 x what the float32 restatement loses"""
    for name, sl in (("rows below 65535", slice(0, S.ROW_BATCH)), ("rows from 65535", slice(S.ROW_BATCH, None))):
        rms = float(np.sqrt(np.mean(np.abs(ref[sl]) ** 2)))
        loss = float(np.max(np.abs(f32[sl].astype(ref.dtype) - ref[sl]))) / rms
        assert 0 < loss < 1e-4, (what, name, loss)
        close(got[sl], ref[sl], 4.0 * loss * rms, "%s, %s" % (what, name))


def test_row_batches_ddc_and_upfirdn():
    """the one-dimensional tiles x rows grids of k_ddc (q = 4) and k_upfirdn (3 / 2) on 65538 rows of a few hundred samples"""
    from test_host_baseband import ddc_ref
    from test_host_resample import upfirdn_ref
    from test_gpu_baseband import ddc_f32, taps32
    x = S.batch_rows(S.DDC_N, S.DDC_N)
    h = ss.firwin(S.DDC_T, 0.8 / S.DDC_Q)
    got = E.ddc(x, S.DDC_NU, S.DDC_Q, h, n0=S.DDC_N0)
    assert got.shape == (S.ROWS, S.DDC_N // S.DDC_Q)
    _restated(got, ddc_ref(x.astype(np.float64), S.DDC_NU, S.DDC_Q, taps32(h), S.DDC_N0), ddc_f32(x, S.DDC_NU, S.DDC_Q, h, S.DDC_N0), "ddc")
    alone(lambda r: E.ddc(x[r:r + 1], S.DDC_NU, S.DDC_Q, h, n0=S.DDC_N0), got, "ddc")
    x = S.batch_rows(S.UPF_N, S.UPF_N)
    h = ss.firwin(S.UPF_T, 1.0 / S.UPF_UP) * S.UPF_UP
    got = E.upfirdn(x, h, S.UPF_UP, S.UPF_DOWN)
    ref = upfirdn_ref(taps32(h), x.astype(np.float64), S.UPF_UP, S.UPF_DOWN)
    assert got.shape == ref.shape and got.shape[0] == S.ROWS
    _restated(got, ref, upfirdn_ref(h, x, S.UPF_UP, S.UPF_DOWN, dtype=np.float32), "upfirdn")
    alone(lambda r: E.upfirdn(x[r:r + 1], h, S.UPF_UP, S.UPF_DOWN), got, "upfirdn")


def test_row_batches_hilbert_fft_and_czt():
    """hilbert_rows 65538 x 64, fft 65538 x 8 and 65538 x 12 (Bluestein), and the fused chirp-z at 65535 rows"""
    x = S.batch_rows(64, 64)
    got = E.hilbert_rows(x, 64)
    by_batch(got, ss.hilbert(x.astype(np.float64), axis=-1), 1e-4, "hilbert_rows")
    alone(lambda r: E.hilbert_rows(x[r:r + 1], 64), got, "hilbert_rows")
    for n in (8, 12):
        z = S.batch_rows(n, n, True)
        got = E.fft(z)
        assert got.shape == (S.ROWS, n)
        by_batch(got, np.fft.fft(z.astype(np.complex128), axis=-1), 4e-6 * np.sqrt(np.log2(n)), "fft %d" % n)
        alone(lambda r: E.fft(z[r:r + 1]), got, "fft %d" % n)
    z = S.batch_rows(S.CZT_SMALL_N, S.CZT_SMALL_N)[:S.ROW_BATCH]
    got = E.czt(z, S.CZT_SMALL_M, S.ZOOM_START, 0.3 / S.CZT_SMALL_M)
    assert got.shape == (S.ROW_BATCH, S.CZT_SMALL_M)
    by_batch(got, z.astype(np.float64) @ S.arc(S.CZT_SMALL_N, S.CZT_SMALL_M, S.ZOOM_START, 0.3 / S.CZT_SMALL_M), 1e-4, "czt")
    for r in (0, S.ROW_BATCH - 2, S.ROW_BATCH - 1):
        same_bits(E.czt(z[r:r + 1], S.CZT_SMALL_M, S.ZOOM_START, 0.3 / S.CZT_SMALL_M)[0], got[r], "czt, row %d alone" % r)
