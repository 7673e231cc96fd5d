"""The loop-seam instrument (tests/seam_ref.py) itself, on the CPU.  The budgets it restates give the shapes the GPU tests claim; its
float64 references agree with tests/detrend_ref.py, scipy and the oracle; and every planted defect moves at least one output element
by 100 tolerances or more -- the tolerances of tests/test_gpu_loop_seams.py -- on every input that file uses.  So a wrong offset in a
chunk, slice or row-batch loop cannot pass there.

Which defect each part of an input is for: the chirp makes a chunk read at f0 = 0, or written at the first chunk's place, differ
(read_f0_zero, write_first); the tone burst in the samples that only the last chunk covers makes a few ragged frames count in an
average of thousands (drop_last, and read_f0_zero where the last chunk is short); the ramp per channel leaves an offset of the line's
value at the chunk's first sample when sp_csd_matrix fails to re-base its trend (trend_unshifted); the gains and tones of the rows
tell a row of the second row batch from the row 65535 before it (batch_from_first).

The refusals the seam audit added are tested here too, through the raw ABI with null or tiny buffers: they come
before the device is touched, so they pass without a GPU."""
import ctypes

import numpy as np
import pytest
import scipy.signal as ss

import detrend_ref as R
import seam_ref as S
from oracle import cpu_ref as O
from pyfft_amd import _ffi

FS = 1000.0


# ------------------------------------------------------------------------------------------------------------------- the budgets
def test_budgets_give_the_shapes_the_gpu_tests_claim():
    assert S.long_chunk_frames(4100, 1 << 30) == 6138 and S.W4100.nframes == 6145 and S.W4100.mc == 6138
    assert S.long_chunk_frames(16384, 1 << 30) == 1536 and S.W16384.nframes == 1543
    assert S.long_chunk_frames(5000, 4000) == 4000 and S.long_chunk_frames(16384, 700) == 700       # tests/test_gpu_long.py: one chunk
    assert S.long_chunk_frames(1 << 17, 1 << 30) == 192
    assert S.czt_len(8100, 100) == 16384 and S.Z8100.nframes == 1543
    assert S.long_len(4100) == 16384 and S.long_slice_rows(4100) == 2048 and S.long_slice_rows(16384) == 2048
    assert S.passes(S.W4100.mc, S.long_slice_rows(4100)) == 3                                       # three Bluestein slices per chunk
    assert S.passes(4000, S.long_slice_rows(5000)) == 2                                             # tests/test_gpu_long.py: two slices
    assert [m for _, m in S.chunks(7, 3)] == [3, 3, 1]
    assert S.csdm_chunk_frames(2, 32, 16500) == 8256 and S.csdm_chunk_frames(65, 32, 16500) == 8256
    assert S.csdm_chunk_frames(16, 4096, 8191) == 8191                                              # cfg5 at full size: one chunk
    assert [S.passes(c.nframes, S.csdm_mc(c)) for c in S.CSDM_HOOKED] == [11, 6, 4, 3]
    assert S.pipe_spec_min_frames(2) == 8191
    assert S.ROWS == 65538 and S.ALONE == (0, 65534, 65535, 65537)
    for c in S.TINY + S.TINY_ZOOM:
        assert c.nframes == 7 and c.mc == 3 and not S.wg_capable(c.nfft if c in S.TINY else S.czt_len(c.nfft, S.ZOOM_M))


def test_frame_maps():
    assert list(S.source_frames(7, 3)) == list(range(7))
    assert list(S.source_frames(7, 3, "read_f0_zero")) == [0, 1, 2, 0, 1, 2, 0]
    assert list(S.source_frames(7, 3, "drop_last")) == [0, 1, 2, 3, 4, 5]
    assert list(S.row_sources(7, 3, "read_f0_zero")) == [0, 1, 2, 0, 1, 2, 0]
    assert list(S.row_sources(7, 3, "write_first")) == [6, 4, 5, -1, -1, -1, -1]
    assert list(S.row_sources(7, 3, "drop_last")) == [0, 1, 2, 3, 4, 5, -1]
    assert list(S.plant_batches(np.arange(S.ROWS))[-3:]) == [0, 1, 2]
    assert S.tail_from(4100, 16, 6145, 6138) == 6137 * 16 + 4100 and S.tail_from(32, 4, 10, 16) == 0


# --------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("mode", R.MODES[1:], ids=[R.MODE_NAMES[m] for m in R.MODES[1:]])
def test_references_agree_with_detrend_ref(mode, cplx):
    nfft, hop, M = 300, 75, 9
    x = S.record(5, (M - 1) * hop + nfft + 5, cplx, 700)
    win = S.window(nfft)
    idx = np.arange(M)
    X, pseg = S.spectra_rows(x, win, hop, idx, mode)
    np.testing.assert_allclose(X, R.spectra(x, win, hop, M, mode), rtol=0, atol=1e-9 * np.abs(X).max())
    np.testing.assert_allclose(pseg, R.pseg(x, win, hop, M, mode), rtol=1e-12)
    np.testing.assert_allclose(S.psd_sum(x, win, hop, idx, mode, block=4) / M, R.psd(x, win, hop, M, mode, R.SIDED_RAW), rtol=1e-10)
    y = np.stack([S.record(6, x.size, cplx, 700, -1.0), S.record(7, x.size, cplx, 0, 2.0)])
    sxx, syy, sxy = S.csd_sums(x, y, win, hop, idx, mode, block=4)
    pxx, pyy, pxy = R.csd(x, y, win, hop, M, mode, R.SIDED_RAW)
    np.testing.assert_allclose(sxx / M, pxx, rtol=1e-10)
    np.testing.assert_allclose(syy / M, pyy, rtol=1e-10)
    np.testing.assert_allclose(sxy / M, pxy, rtol=0, atol=1e-10 * np.abs(pxy).max())
    np.testing.assert_allclose(S.cog_of(X, FS), R.cog(x, win, hop, M, mode, FS)[0], rtol=1e-10, atol=1e-9)


def test_zoom_and_matrix_references_agree_with_scipy_and_the_oracle():
    nfft, hop, M, m = 300, 75, 9, 40
    x = S.record(8, (M - 1) * hop + nfft + 5, False, 700)
    win = S.window(nfft)
    E = S.arc(nfft, m, S.ZOOM_START, 0.3 / m)
    xd = x.astype(np.float64) - x.astype(np.float64).mean()
    fr = np.stack([win * xd[g * hop:g * hop + nfft] for g in range(M)])
    ref = ss.czt(fr, m, w=np.exp(-2j * np.pi * 0.3 / m), a=np.exp(2j * np.pi * S.ZOOM_START))
    np.testing.assert_allclose(S.zoom_rows(x, win, hop, np.arange(M), R.MEAN, E), ref, rtol=0, atol=1e-9 * np.abs(ref).max())
    sxx, _, _ = S.zoom_sums(x, None, win, hop, np.arange(M), R.MEAN, E, block=4)
    np.testing.assert_allclose(sxx, (np.abs(ref) ** 2).sum(axis=0), rtol=1e-9)
    ch = S.channels(9, 3, x.size, 700)
    G = S.csdm_sum(ch, win, hop, np.arange(M), R.MEAN, block=4) / M
    want = O.csd_matrix(ch.astype(np.float64), win, nfft, hop, M, 1.0) * np.sum(win ** 2)
    np.testing.assert_allclose(G, want, rtol=0, atol=1e-10 * np.abs(want).max())
    # a line that is not re-based leaves its value at the chunk's first sample in every frame of the chunk
    xl, slope = S.detrended(ch, R.LINEAR)
    bad = S.csdm_sum(ch, win, hop, np.arange(M), R.LINEAR, block=4, unshifted_from=4)
    by_hand = np.zeros_like(bad)
    for g in range(M):
        f = np.fft.rfft(win[None, :] * (xl[:, g * hop:g * hop + nfft] + (slope * ((g // 4) * 4 * hop))[:, None]), axis=1)
        by_hand += np.einsum("ik,jk->kij", f, np.conj(f))
    np.testing.assert_allclose(bad, by_hand, rtol=0, atol=1e-10 * np.abs(by_hand).max())


# ------------------------------------------------------------------------------------------------- planted defects: frame chunks
def _replanted(total, gone, of, nframes, mc, plant):
    """an accumulated quantity under a defect, from the reference `total` (a tuple of sums over every frame once) and `gone` (the
    same over every chunk after the first): only the frames the defect puts in their place are summed again.  of(idx) -> the tuple of
    sums over the frames idx."""
    src = S.source_frames(nframes, mc, plant)
    return tuple(t - g + c for t, g, c in zip(total, gone, of(src[mc:])))


FRAME_PLANTS = ("read_f0_zero", "drop_last")
ROW_PLANTS = ("read_f0_zero", "drop_last", "write_first")


def _modes_of(case):
    return R.MODES[1:] if case.cap else (R.MEAN, R.LINEAR)


@pytest.mark.parametrize("case", (S.W4100, S.W16384) + S.TINY, ids=lambda c: c.id)
def test_planted_defects_move_the_welch_psd(case):
    """welch_psd: the burst is for both defects (the frames of the ragged last chunk hold it, the frames read instead do not)"""
    x, win, M = S.case_record(case), S.window(case.nfft), case.nframes
    for mode in _modes_of(case):
        of = lambda idx: (S.psd_sum(x, win, case.hop, idx, mode),)           # noqa: E731
        total, gone = of(np.arange(M)), of(np.arange(case.mc, M))
        ref = total[0] / M
        for plant in FRAME_PLANTS:
            bad = _replanted(total, gone, of, M, case.mc, plant)[0] / M
            assert S.exceeds(ref, bad, S.tol_psd(ref)), (case.id, mode, plant)


@pytest.mark.parametrize("case", (S.W16384,) + S.TINY, ids=lambda c: c.id)
def test_planted_defects_move_the_welch_csd(case):
    x, win, M = S.case_record(case), S.window(case.nfft), case.nframes
    y = np.stack([S.case_record(case, 1), S.case_record(case, 2)])
    for mode in (R.MEAN,) if not case.cap else _modes_of(case):
        of = lambda idx: S.csd_sums(x, y, win, case.hop, idx, mode)          # noqa: E731
        total, gone = of(np.arange(M)), of(np.arange(case.mc, M))
        for plant in FRAME_PLANTS:
            bad = _replanted(total, gone, of, M, case.mc, plant)
            for k, tol in ((0, S.tol_psd), (1, S.tol_psd), (2, S.tol_csd)):
                assert S.exceeds(total[k] / M, bad[k] / M, tol(total[k] / M)), (case.id, mode, plant, k)


@pytest.mark.parametrize("case", (S.W4100, S.W16384) + S.TINY, ids=lambda c: c.id)
def test_planted_defects_move_the_stft_rows_pseg_and_cog(case):
    """row outputs: the chirp tells a frame from the frame a chunk earlier, the burst marks the rows of the last chunk"""
    x, win, M = S.case_record(case), S.window(case.nfft), case.nframes
    rows = S.rows_of_interest(M, S.seams_of(M, case.mc, case.nfft))
    modes = R.MODES[1:] if case.cap else (R.MEAN, R.SEGMEAN, R.SEGLINEAR)
    for mode in modes:
        X, pseg = S.spectra_rows(x, win, case.hop, rows, mode)
        cog = S.cog_of(X, FS)
        for plant in ROW_PLANTS:
            src = S.row_sources(M, case.mc, plant)[rows]
            Xb, pb = S.spectra_rows(x, win, case.hop, np.maximum(src, 0), mode)
            Xb[src < 0] = 0
            pb[src < 0] = 0
            assert S.exceeds(X, Xb, S.tol_rows(X)), (case.id, mode, plant)
            assert S.exceeds(np.abs(X) ** 2, np.abs(Xb) ** 2, S.tol_psd(np.abs(X) ** 2)), (case.id, mode, plant)
            assert S.exceeds(pseg, pb, 1e-4 * pseg), (case.id, mode, plant)
            if case.cplx:              # (a real record's two-sided centre of gravity is zero up to noise: nothing to move)
                cb = np.where(src < 0, 0.0, S.cog_of(np.where(Xb == 0, 1.0, Xb), FS))
                assert S.exceeds(cog, cb, 2e-4 * np.abs(cog) + 1e-4), (case.id, mode, plant)


@pytest.mark.parametrize("case", (S.Z8100,) + S.TINY_ZOOM, ids=lambda c: c.id)
def test_planted_defects_move_the_zoom_spectra(case):
    x, y, win, M = S.case_record(case), S.case_record(case, 1), S.window(case.nfft), case.nframes
    E = S.arc(case.nfft, S.ZOOM_M, S.ZOOM_START, S.ZOOM_STEP)
    for mode in (R.MEAN,) if not case.cap else (R.CONST, R.MEAN, R.LINEAR):
        of = lambda idx: S.zoom_sums(x, y, win, case.hop, idx, mode, E)      # noqa: E731
        total, gone = of(np.arange(M)), of(np.arange(case.mc, M))
        for plant in FRAME_PLANTS:
            bad = _replanted(total, gone, of, M, case.mc, plant)
            for k, tol in ((0, S.tol_psd), (1, S.tol_psd), (2, S.tol_csd)):
                assert S.exceeds(total[k] / M, bad[k] / M, tol(total[k] / M)), (case.id, mode, plant, k)
        rows = S.rows_of_interest(M, [f0 for f0, _ in S.chunks(M, case.mc)[1:]])
        Z = S.zoom_rows(x, win, case.hop, rows, mode, E)
        for plant in ROW_PLANTS:
            src = S.row_sources(M, case.mc, plant)[rows]
            Zb = S.zoom_rows(x, win, case.hop, np.maximum(src, 0), mode, E)
            Zb[src < 0] = 0
            assert S.exceeds(Z, Zb, S.tol_rows(Z)), (case.id, mode, plant)


def _csdm_plants(x, win, hop, M, mc, modes):
    for mode in modes:
        of = lambda idx: (S.csdm_sum(x, win, hop, idx, mode),)               # noqa: E731
        total, gone = of(np.arange(M)), of(np.arange(mc, M))
        ref = total[0] / M
        tol = S.tol_csdm(ref)
        for plant in FRAME_PLANTS:
            bad = _replanted(total, gone, of, M, mc, plant)[0] / M
            assert S.exceeds(ref, bad, tol), (mode, plant)
        if mode == R.LINEAR:
            bad = S.csdm_sum(x, win, hop, np.arange(M), mode, unshifted_from=mc) / M
            assert S.exceeds(ref, bad, tol), (mode, "trend_unshifted")


@pytest.mark.parametrize("case", S.CSDM_DEFAULT + S.CSDM_HOOKED, ids=lambda c: c.id)
def test_planted_defects_move_the_csd_matrix(case):
    """sp_csd_matrix: equal chunks, so drop_last loses up to half of the frames; the ramps are for trend_unshifted"""
    _csdm_plants(S.csdm_record(case), S.window(case.nfft), case.hop, case.nframes, S.csdm_mc(case), (R.MEAN, R.LINEAR))


def test_planted_defects_move_the_pipeline_csd_matrix():
    """the nfft-4096 pipeline case of the GPU test, at a sixteenth of its frames (the record is the same formula; both chunks still
    hold different parts of the chirp)"""
    nch, nfft, hop = 2, 4096, 2048
    M = (2 * S.pipe_spec_min_frames(nch) + 33) // 16
    x = S.pipe_channels(np, nch, (M - 1) * hop + nfft)
    assert x.dtype == np.float32 and abs(float(np.std(x[0])) - 1.16) < 0.1
    _csdm_plants(x, S.window(nfft), hop, M, (M // 2 + 31) & ~31, (R.MEAN,))


# ------------------------------------------------------------------------------------------ planted defects: slices and row batches
def _rows_plants(x, ref_of, tol_of, per, plants=("read_f0_zero", "write_first", "drop_last")):
    n = x.shape[0]
    rows = S.rows_of_interest(n, list(range(per, n, per)))
    ref = ref_of(x[rows])
    for plant in plants:
        bad = S.take_rows(ref_of, x, S.row_sources(n, per, plant)[rows])
        assert S.exceeds(ref, bad, tol_of(ref)), plant


def test_planted_defects_move_the_sliced_transforms():
    """fft / ifft rows and czt rows: a slice after the first read at b0 = 0, written at the first slice's place, or dropped"""
    for nrows, n in ((2049, 16384), (2051, 4100), (7, 16384), (7, 4100)):
        x = S.sliding_rows(n, nrows, n)
        per = S.long_slice_rows(n, 2 if nrows == 7 else 0)
        assert S.passes(nrows, per) >= 2
        _rows_plants(x, lambda r: np.fft.fft(r.astype(np.complex128), axis=1), lambda ref: S.tol_fft(n, ref), per)
        _rows_plants(x, lambda r: np.fft.ifft(r.astype(np.complex128), axis=1), lambda ref: S.tol_fft(n, ref), per)
    E = S.arc(S.CZT_N, S.CZT_M, S.ZOOM_START, S.ZOOM_STEP)
    for nrows, cap in ((2050, 0), (7, 2)):
        x = S.sliding_rows(3, nrows, S.CZT_N, False)
        _rows_plants(x, lambda r: r.astype(np.float64) @ E, S.tol_rows, S.long_slice_rows(S.czt_len(S.CZT_N, S.CZT_M), cap))


def test_planted_defect_moves_every_row_batch_entry():
    """batch_from_first on the six rows around the seam of every entry of the 65538-row tests: rows 65535 .. 65537 are LOUD times
    louder than rows 0 .. 2 and carry other tones, far beyond each entry's tolerance"""
    from test_host_channelizer import pfb_ref
    from test_host_pfb_synth import pfb_synth_ref
    from test_host_resample import upfirdn_ref
    from test_host_baseband import ddc_ref
    from pyfft_amd import channelizer as CH
    pick = np.array([0, 1, 2, S.ROW_BATCH, S.ROW_BATCH + 1, S.ROW_BATCH + 2])
    h = CH.pfb_prototype(S.PFB_M, S.PFB_P) * S.PFB_M
    nsig = S.PFB_M * S.PFB_P + (S.PFB_FRAMES - 1) * S.PFB_HOP
    entries = {
        "sos1": (S.SOS_N, lambda r: ss.sosfilt(S.sos_design(1), r, axis=-1), 5e-7),
        "sos8": (S.SOS_N, lambda r: ss.sosfilt(S.sos_design(8), r, axis=-1), 5e-7),
        "filtfilt": (S.SOS_N, lambda r: ss.sosfiltfilt(S.sos_design(3), r, axis=-1, padlen=S.FILTFILT_PAD), 5e-7),
        "pfb": (nsig, lambda r: pfb_ref(r, h, S.PFB_M, S.PFB_HOP, 0, S.PFB_FRAMES).reshape(len(r), -1), 1e-4),
        "ddc": (S.DDC_N, lambda r: ddc_ref(r, S.DDC_NU, S.DDC_Q, ss.firwin(S.DDC_T, 0.8 / S.DDC_Q), S.DDC_N0), 1e-4),
        "upfirdn": (S.UPF_N, lambda r: upfirdn_ref(ss.firwin(S.UPF_T, 1.0 / 3) * 3, r, S.UPF_UP, S.UPF_DOWN), 1e-4),
        "hilbert": (64, lambda r: ss.hilbert(r, axis=-1), 1e-4),
        "fft8": (8, lambda r: np.fft.fft(r, axis=-1), 4e-6 * np.sqrt(3.0)),
        "fft12": (12, lambda r: np.fft.fft(r, axis=-1), 4e-6 * np.sqrt(np.log2(12.0))),
    }
    for name, (n, ref_of, rel) in entries.items():
        x = S.batch_rows(n, n)[pick].astype(np.float64)
        ref = ref_of(x)
        bad = ref_of(x[[0, 1, 2, 0, 1, 2]])
        peak = np.max(np.abs(ref), axis=-1, keepdims=True)
        assert S.exceeds(ref, bad, rel * peak), name
    X = pfb_ref(S.batch_rows(nsig, nsig)[pick].astype(np.float64), h, S.PFB_M, S.PFB_HOP, 0, S.PFB_FRAMES)[..., :S.PFB_M // 2 + 1]
    y = pfb_synth_ref(X, h / S.PFB_M, S.PFB_M, S.PFB_HOP, 0, nsig, onesided=True)
    assert S.exceeds(y, y[[0, 1, 2, 0, 1, 2]], 1e-4 * np.max(np.abs(y), axis=-1, keepdims=True)), "synth"


# ----------------------------------------------------------------------------------------- the pass counter and the new refusals
def _raw():
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for table in (_ffi.SIGNATURES, _ffi.EXT_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def test_last_passes_is_declared_bound_and_zero_before_any_call():
    lib = _raw()
    assert "sp_last_passes" in _ffi.EXT_SIGNATURES and _ffi.EXT_SIGNATURES["sp_last_passes"] == (ctypes.c_int, [ctypes.c_int])
    assert [lib.sp_last_passes(w) for w in (0, 1, 2, -1)] == [0, 0, 0, 0]
    from pyfft_amd import engine
    assert callable(engine.last_passes)


def test_grid_bound_counts_are_refused_by_name_before_the_device():
    """nch of sp_welch_csd and sp_istft, nframes of a bin-major sp_stft, nch of sp_csd_matrix: rc < 0 and a message that names the
    entry, the argument and its limit; nothing is read (the buffers are tiny) and no device is needed."""
    lib, p = _raw(), _ffi.ptr
    x = np.zeros(64, dtype=np.float32)
    win = np.ones(16, dtype=np.float32)
    out = np.zeros(64, dtype=np.complex128)
    calls = (
        ("sp_welch_csd", "nch = 65536", "65535", lambda: lib.sp_welch_csd(p(x), p(x), 0, 64, 65536, 64, p(win), 16, 8, 4, 1, None, None, 1, 1.0,
                                                                          p(out), p(out), p(out), 0)),
        ("sp_istft", "nch = 65536", "65535", lambda: lib.sp_istft(p(out), 4, 0, 65536, 4, p(win), 16, 8, 1.0, 0, 16, p(x), 0)),
        ("sp_stft", "nframes = %d" % (65535 * 32 + 1), str(65535 * 32),
         lambda: lib.sp_stft(p(x), 0, 64, p(win), 16, 8, 65535 * 32 + 1, 1, 0.0, 0.0, 1, 1.0, 0, 1, p(out), None, 0)),
        ("sp_csd_matrix", "nch = 23169", "23168", lambda: lib.sp_csd_matrix(p(x), 23169, 64, 64, p(win), 16, 8, 4, 1, 1.0, p(out), 0)),
        ("sp_csd_matrix_means", "nch = 23169", "23168",
         lambda: lib.sp_csd_matrix_means(p(x), 23169, 64, 64, p(win), 16, 8, 4, p(np.zeros(4)), 1.0, p(out), 0)),
    )
    for name, arg, limit, call in calls:
        assert call() < 0, name
        msg = (lib.sp_last_error() or b"").decode()
        assert msg.startswith(name + ": ") and arg in msg and limit in msg, msg
    assert not out.any() and not x.any()
