"""The time-resolved Welch spectra on the MI355X (sp_welch_blocks, engine.welch_blocks, running_*) against scipy.signal.welch / csd /
coherence of every block's slice.  The bounds are the project's Welch parity bounds (tests/test_gpu_kernels.py,
tests/test_gpu_multitaper.py) applied per block and per channel: PSD rtol 2e-4, atol 1e-6 max(ref of that block and channel); cross
spectra rtol 2e-4, atol 2e-6 max |ref of that block|; coherence 2e-4 absolute.  Every bin of every block is compared, nothing is masked.
Inputs are seeded noise plus a common component (welch_blocks_ref.make_pair), so no reference bin is zero."""
import functools

import numpy as np
import pytest
import scipy.signal as ss

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import engine as E, _running_mod as RN                                       # noqa: E402
from welch_blocks_ref import hann, nframes_of, nblocks_of, block_slice, make_pair            # noqa: E402
from test_host_welch_blocks import AVG_STEP, AVG_IDS                                         # noqa: E402


def scipy_blocks(x, y, win, nfft, hop, navg, step, detrend, nblocks, blocks=None, fs=1.0, scaling="density", onesided=None):
    """(Pxx, Pyy, Pxy, Cxy) [len(blocks), nf] float64 / complex128 from scipy on the slices; y None: (Pxx, None, None, None)."""
    cplx = np.iscomplexobj(x)
    onesided = (not cplx) if onesided is None else onesided
    dt = np.complex128 if cplx else np.float64
    win = np.ones(nfft) if win is None else np.asarray(win, dtype=np.float64)
    kw = dict(fs=fs, window=win, nperseg=nfft, noverlap=nfft - hop, detrend="constant" if detrend else False,
              return_onesided=onesided, scaling=scaling)
    out = [[], [], [], []]
    for b in (range(nblocks) if blocks is None else blocks):
        s, e = block_slice(b, nfft, hop, navg, step)
        xs = np.asarray(x[s:e]).astype(dt)
        out[0].append(ss.welch(xs, **kw)[1])
        if y is not None:
            ys = np.asarray(y[s:e]).astype(dt)
            out[1].append(ss.welch(ys, **kw)[1])
            out[2].append(ss.csd(xs, ys, **kw)[1])
            out[3].append(np.abs(out[2][-1]) ** 2 / (out[0][-1] * out[1][-1]))
    return tuple(np.stack(v) if v else None for v in out)


def coherence_of(pxx, pyy, pxy):
    return (pxy.real.astype(np.float64) ** 2 + pxy.imag.astype(np.float64) ** 2) / (pxx.astype(np.float64) * pyy.astype(np.float64))


def within(got, ref, what, coherence=True):
    """got = (Pxx, Pyy, Pxy) of one pair against ref = scipy_blocks(..): the bounds block by block, every bin."""
    gxx, gyy, gxy = got
    rxx, ryy, rxy, rcoh = ref
    assert gxx.shape == rxx.shape and gxx.dtype == np.float32, what
    worst = [0.0, 0.0, 0.0]
    for b in range(rxx.shape[0]):
        for g, r in ((gxx, rxx), (gyy, ryy)):
            if r is None:
                continue
            worst[0] = max(worst[0], float(np.max(np.abs(g[b] - r[b]) / (2e-4 * np.abs(r[b]) + 1e-6 * float(r[b].max())))))
            np.testing.assert_allclose(g[b], r[b], rtol=2e-4, atol=1e-6 * float(r[b].max()), err_msg="%s: PSD of block %d" % (what, b))
        if rxy is not None:
            assert gxy.shape == rxy.shape and gxy.dtype == np.complex64, what
            top = float(np.abs(rxy[b]).max())
            worst[1] = max(worst[1], float(np.max(np.abs(gxy[b] - rxy[b]) / (2e-4 * np.abs(rxy[b]) + 2e-6 * top))))
            np.testing.assert_allclose(gxy[b], rxy[b], rtol=2e-4, atol=2e-6 * top, err_msg="%s: CSD of block %d" % (what, b))
            if coherence:
                d = float(np.max(np.abs(coherence_of(gxx[b], gyy[b], gxy[b]) - rcoh[b])))
                worst[2] = max(worst[2], d)
                assert d <= 2e-4, "%s: coherence of block %d off by %.3g" % (what, b, d)
    print("%s: PSD uses %.3g and CSD %.3g of the allowance, coherence off by %.3g" % (what, worst[0], worst[1], worst[2]))


HOPS = {"half": lambda n: n // 2, "full": lambda n: n, "odd": lambda n: 3 * n // 8 + 1}
NFRAMES = 41


@functools.lru_cache(maxsize=None)
def record(nfft, hop, cplx):
    """About 40 frames, nsig no multiple of anything, samples left over behind the last frame."""
    nsig = (NFRAMES - 1) * hop + nfft + min(hop - 1, 7)
    x, y = make_pair(nsig, cplx, 100 + nfft + (1 if cplx else 0))
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize("hopkind", list(HOPS))
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("nfft", [32, 256, 1024, 8192])
def test_parity_with_scipy_on_slices(nfft, cplx, hopkind):
    hop = HOPS[hopkind](nfft)
    x, y = record(nfft, hop, cplx)
    nframes = nframes_of(len(x), nfft, hop)
    assert nframes == NFRAMES
    win = hann(nfft)
    scale = 1.0 / float(np.sum(win ** 2))
    for (navg, step), tag in zip(AVG_STEP, AVG_IDS):
        nblocks = nblocks_of(nframes, navg, step)
        assert nblocks >= 2 and (nblocks - 1) * step + navg <= nframes
        for detrend in (True, False):
            got = E.welch_blocks(x, win, hop, nframes, navg, step, y=y, detrend=detrend, scale=scale, doubled=not cplx)
            ref = scipy_blocks(x, y, win, nfft, hop, navg, step, detrend, nblocks)
            within(got, ref, "nfft %d %s hop %d %s %s" % (nfft, "cplx" if cplx else "real", hop, tag, "segmean" if detrend else "none"))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_boxcar_without_a_window(cplx):
    nfft, hop, navg, step = 256, 128, 6, 4
    x, y = record(nfft, hop, cplx)
    # (no detrend: under a boxcar a frame without its mean has no DC bin at all, and no reference bin may be zero)
    got = E.welch_blocks(x, None, hop, NFRAMES, navg, step, y=y, detrend=False, scale=1.0 / nfft, doubled=not cplx, nfft=nfft)
    ref = scipy_blocks(x, y, None, nfft, hop, navg, step, False, nblocks_of(NFRAMES, navg, step))
    within(got, ref, "boxcar %s" % ("cplx" if cplx else "real"))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("navg,step", [(8, 8), (6, 4)], ids=["navg8-step8", "navg6-step4"])
def test_amplitude_step_mid_record(navg, step, cplx):
    """The amplitude of both records steps by 10^3 at mid-record: the per-block bounds hold on both sides, and in the blocks that
    straddle the step."""
    nfft, hop = 256, 128
    x, y = record(nfft, hop, cplx)
    gain = np.where(np.arange(len(x)) < len(x) // 2 + 13, 1.0, 1e3).astype(np.float32)
    xs, ys = x * gain, y * gain
    win = hann(nfft)
    got = E.welch_blocks(xs, win, hop, NFRAMES, navg, step, y=ys, scale=1.0 / float(np.sum(win ** 2)), doubled=not cplx)
    nblocks = nblocks_of(NFRAMES, navg, step)
    ref = scipy_blocks(xs, ys, win, nfft, hop, navg, step, True, nblocks)
    assert ref[0][-1].max() > 1e5 * ref[0][0].max()
    within(got, ref, "amplitude step %s navg %d step %d" % ("cplx" if cplx else "real", navg, step))


@pytest.mark.parametrize("nfft", [256, 8192])
@pytest.mark.parametrize("ax,ay", [(1.0, 1e-4), (1e-4, 1.0)], ids=["y-weak", "x-weak"])
def test_channel_imbalance(nfft, ax, ay):
    """Real records 10^4 apart in amplitude: each PSD keeps the bounds relative to ITS OWN maximum.  (Packed into one transform as
    x + i y without a balance of the two halves, the weak channel's PSD is lost; here every record has its own transform.)"""
    hop, navg, step = nfft // 2, 8, 2
    nsig = (NFRAMES - 1) * hop + nfft + 5
    x, y = make_pair(nsig, False, 7 + nfft, ax=ax, ay=ay)
    win = hann(nfft)
    scale = 1.0 / float(np.sum(win ** 2))
    for detrend in (True, False):
        got = E.welch_blocks(x, win, hop, NFRAMES, navg, step, y=y, detrend=detrend, scale=scale, doubled=True)
        ref = scipy_blocks(x, y, win, nfft, hop, navg, step, detrend, nblocks_of(NFRAMES, navg, step))
        ratio = float(ref[0].max() / ref[1].max())
        assert ratio > 1e7 or ratio < 1e-7
        within(got, ref, "imbalance nfft %d x %g y %g %s" % (nfft, ax, ay, "segmean" if detrend else "none"))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("navg,step", [(8, 8), (6, 4)], ids=["navg8-step8", "navg6-step4"])
def test_several_channels(navg, step, cplx):
    """nch = 3 rows y_ld > nsig apart: every pair is bitwise the single-pair call, and so is Pxx, whichever channel the single-pair
    call takes: Pxx does not depend on y (real records: it comes from a transform of x alone and is bitwise the call without y too;
    complex records: x has its own transform in every pair, and the call without y agrees within the PSD bound)."""
    nfft, hop = 256, 100
    nsig = (NFRAMES - 1) * hop + nfft + 3
    x, y3 = make_pair(nsig, cplx, 31, nch=3)
    ybig = np.zeros((3, nsig + 37), dtype=y3.dtype)
    ybig[:, :nsig] = y3
    ybig[:, nsig:] = 1e6                                       # never read
    win = hann(nfft)
    scale = 1.0 / float(np.sum(win ** 2))
    pxx, pyy, pxy = E.welch_blocks(x, win, hop, NFRAMES, navg, step, y=ybig, scale=scale, doubled=not cplx)
    nblocks = nblocks_of(NFRAMES, navg, step)
    assert pyy.shape == pxy.shape == (3,) + pxx.shape == (3, nblocks, nfft if cplx else nfft // 2 + 1)
    ref = scipy_blocks(x, None, win, nfft, hop, navg, step, True, nblocks)
    for c in range(3):
        one = E.welch_blocks(x, win, hop, NFRAMES, navg, step, y=y3[c], scale=scale, doubled=not cplx)
        np.testing.assert_array_equal(one[1], pyy[c])
        np.testing.assert_array_equal(one[2], pxy[c])
        np.testing.assert_array_equal(one[0], pxx)
        within((one[0], None, None), ref, "Pxx of the pair with channel %d" % c)
    only = E.welch_blocks(x, win, hop, NFRAMES, navg, step, scale=scale, doubled=not cplx)
    assert only[1] is None and only[2] is None
    within((only[0], None, None), ref, "Pxx without y")
    if not cplx:
        np.testing.assert_array_equal(only[0], pxx)
    for b in range(nblocks):
        np.testing.assert_allclose(only[0][b], pxx[b], rtol=2e-4, atol=1e-6 * float(pxx[b].max()))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_one_block_over_everything(cplx):
    """navg == nframes: the one block is engine.welch_csd with the segments' own means removed."""
    nfft, hop = 1024, 512
    x, y = record(nfft, hop, cplx)
    win = hann(nfft)
    scale = 1.0 / float(np.sum(win ** 2))
    got = E.welch_blocks(x, win, hop, NFRAMES, NFRAMES, y=y, scale=scale)
    assert got[0].shape[0] == 1
    nb = got[0].shape[1]                                       # welch_csd: all nfft bins in FFT order; a real record's first nfft/2 + 1
    rxx, ryy, rxy = (v[..., :nb] for v in E.welch_csd(x, y, win, hop, NFRAMES, detrend="segmean", sided=E.SIDED_RAW, scale=scale))
    ref = (rxx[None, :], ryy, rxy, np.abs(rxy) ** 2 / (rxx[None, :] * ryy))
    within(got, ref, "one block, %s" % ("cplx" if cplx else "real"))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("nfft", [64, 1024])
@pytest.mark.parametrize("navg,step", [(8, 8), (6, 4)], ids=["navg8-step8", "navg6-step4"])
def test_reproducible_and_local(navg, step, nfft, cplx):
    """Two calls agree bitwise; and block b agrees bitwise with block 0 of the same call on the record cut to start at block b's first
    sample: the order of the additions does not depend on where in the record, the grid or the workgroup a block lies."""
    hop = 3 * nfft // 8 + 1
    x, y = record(nfft, hop, cplx)
    win = hann(nfft)
    full = E.welch_blocks(x, win, hop, NFRAMES, navg, step, y=y, scale=1.0, doubled=not cplx)
    again = E.welch_blocks(x, win, hop, NFRAMES, navg, step, y=y, scale=1.0, doubled=not cplx)
    for a, b in zip(full, again):
        np.testing.assert_array_equal(a, b)
    nblocks = nblocks_of(NFRAMES, navg, step)
    for b in (1, 2, nblocks // 2, nblocks - 1):
        s = block_slice(b, nfft, hop, navg, step)[0]
        xc, yc = np.ascontiguousarray(x[s:]), np.ascontiguousarray(y[s:])
        cut = E.welch_blocks(xc, win, hop, nframes_of(len(xc), nfft, hop), navg, step, y=yc, scale=1.0, doubled=not cplx)
        for f, c in zip(full, cut):
            np.testing.assert_array_equal(f[b], c[0], err_msg="block %d" % b)


def test_coherence():
    nfft, hop = 256, 128
    x, y = record(nfft, hop, False)
    fs = 2.0e6
    r = RN.running_spectra(x, y, fs=fs, nperseg=nfft, navg=8, step=2)
    assert r.coherence.shape == r.Pxy.shape == (17, 129) and r.coherence.dtype == np.float64
    assert r.coherence.min() >= 0.0 and r.coherence.max() <= 1.0 + 1e-6
    assert 0.05 < np.median(r.coherence) < 0.95                # neither independent nor identical records
    np.testing.assert_array_equal(r.phase, np.angle(r.Pxy))
    f, t, c = RN.running_coherence(x, y, fs=fs, nperseg=nfft, navg=8, step=2)
    np.testing.assert_array_equal(c, r.coherence)
    # a single frame: coherence 1, whatever the two spectra
    for cplx in (False, True):
        xs, ys = record(nfft, hop, cplx)
        c1 = RN.running_coherence(xs, ys, fs=fs, nperseg=nfft, navg=1)[2]
        print("navg = 1 (%s): coherence within %.3g of 1" % ("cplx" if cplx else "real", np.max(np.abs(c1 - 1))))
        assert c1.shape[0] == NFRAMES and np.max(np.abs(c1 - 1)) <= 1e-5 and c1.max() <= 1.0 + 1e-6
        cs = RN.running_coherence(xs, xs, fs=fs, nperseg=nfft, navg=8, step=2)[2]
        print("x against x (%s): coherence within %.3g of 1" % ("cplx" if cplx else "real", np.max(np.abs(cs - 1))))
        assert np.max(np.abs(cs - 1)) <= 1e-5


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_device_tensors(cplx):
    import torch
    nfft, hop, navg, step = 256, 128, 6, 4
    x, y = record(nfft, hop, cplx)
    win = hann(nfft)
    host = E.welch_blocks(x, win, hop, NFRAMES, navg, step, y=y, scale=0.5, doubled=not cplx)
    xd, yd = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    dev = E.welch_blocks(xd, win, hop, NFRAMES, navg, step, y=yd, scale=0.5, doubled=not cplx)
    for h, d in zip(host, dev):
        assert isinstance(d, torch.Tensor) and d.is_cuda and tuple(d.shape) == h.shape
        np.testing.assert_allclose(d.cpu().numpy(), h, rtol=1e-12, atol=0)
    r = RN.running_spectra(xd, yd, fs=10.0, nperseg=nfft, navg=navg, step=step)
    rh = RN.running_spectra(x, y, fs=10.0, nperseg=nfft, navg=navg, step=step)
    for name in ("Pxx", "Pyy", "Pxy", "coherence", "phase"):
        d = getattr(r, name)
        assert isinstance(d, torch.Tensor) and d.is_cuda
        if name != "phase":
            np.testing.assert_allclose(d.cpu().numpy(), getattr(rh, name), rtol=1e-12, atol=0)
    # the phase is angle(Pxy) where Pxy lives: the device's atan2 and the host's may differ in the last bit
    assert torch.equal(r.phase, torch.angle(r.Pxy))
    np.testing.assert_allclose(r.phase.cpu().numpy(), rh.phase, rtol=0, atol=1e-6)
    assert isinstance(r.f, np.ndarray) and isinstance(r.t, np.ndarray)
    with pytest.raises(TypeError):
        E.welch_blocks(xd, win, hop, NFRAMES, navg, step, y=y)


def test_more_blocks_than_cus():
    """2^22 real samples, 2046 overlapping blocks: every bin against the composed route (the spectrograms of both records from
    engine.stft_frames, block sums in float64 on the host), sixteen blocks spread over the record against scipy."""
    nsig, nfft, hop, navg, step = 1 << 22, 1024, 512, 8, 4
    x, y = make_pair(nsig, False, 77)
    nframes = nframes_of(nsig, nfft, hop)
    nblocks = nblocks_of(nframes, navg, step)
    assert (nframes, nblocks) == (8191, 2046)
    win = hann(nfft)
    scale = 1.0 / float(np.sum(win ** 2))
    got = E.welch_blocks(x, win, hop, nframes, navg, step, y=y, scale=scale, doubled=True)
    X = E.stft_frames(x, win, hop, nframes, detrend="segmean", sided=E.SIDED_HALF)[0].astype(np.complex128)
    Y = E.stft_frames(y, win, hop, nframes, detrend="segmean", sided=E.SIDED_HALF)[0].astype(np.complex128)
    s = np.full(nfft // 2 + 1, scale / navg)
    s[1:nfft // 2] *= 2

    def block_sums(v):
        c = np.concatenate((np.zeros((1,) + v.shape[1:], v.dtype), np.cumsum(v, axis=0)))
        first = np.arange(nblocks) * step
        return (c[first + navg] - c[first]) * s
    cxx, cyy, cxy = block_sums(np.abs(X) ** 2), block_sums(np.abs(Y) ** 2), block_sums(np.conj(X) * Y)
    within(got, (cxx, cyy, cxy, np.abs(cxy) ** 2 / (cxx * cyy)), "2046 blocks against the composed route")
    pick = [int(v) for v in np.linspace(0, nblocks - 1, 16)]
    ref = scipy_blocks(x, y, win, nfft, hop, navg, step, True, nblocks, blocks=pick)
    within(tuple(g[pick] for g in got), ref, "16 of 2046 blocks against scipy")


def test_python_surface():
    """f, t, the one-sided doubling, scaling='spectrum', the two-sided forms and the complex order against scipy on the slices."""
    nfft, noverlap, navg, step, fs = 256, 160, 6, 4, 250.0
    hop = nfft - noverlap
    x, y = record(nfft, hop, False)
    nblocks = nblocks_of(NFRAMES, navg, step)
    tref = (np.arange(nblocks) * step * hop + ((navg - 1) * hop + nfft) / 2.0) / fs
    for scaling in ("density", "spectrum"):
        for onesided in (True, False):
            kw = dict(fs=fs, window="hann", nperseg=nfft, noverlap=noverlap, navg=navg, step=step, scaling=scaling,
                      return_onesided=onesided)
            ref = scipy_blocks(x, y, hann(nfft), nfft, hop, navg, step, True, nblocks, fs=fs, scaling=scaling, onesided=onesided)
            fref = np.fft.rfftfreq(nfft, 1 / fs) if onesided else np.fft.fftfreq(nfft, 1 / fs)
            r = RN.running_spectra(x, y, **kw)
            np.testing.assert_allclose(r.f, fref, rtol=1e-15)
            np.testing.assert_allclose(r.t, tref, rtol=1e-15)
            within((r.Pxx, r.Pyy, r.Pxy), ref, "running_spectra %s onesided=%s" % (scaling, onesided))
            np.testing.assert_allclose(r.coherence, ref[3], rtol=0, atol=2e-4)
            f, t, pxx = RN.running_psd(x, **kw)
            np.testing.assert_array_equal(f, r.f)
            np.testing.assert_array_equal(t, r.t)
            within((pxx, None, None), (ref[0], None, None, None), "running_psd %s onesided=%s" % (scaling, onesided))
            f, t, pxy = RN.running_csd(x, y, **kw)
            np.testing.assert_array_equal(pxy, r.Pxy)
    f, t, c = RN.running_coherence(x, y, fs=fs, nperseg=nfft, noverlap=noverlap, navg=navg, step=step, detrend=False)
    ref = scipy_blocks(x, y, hann(nfft), nfft, hop, navg, step, False, nblocks, fs=fs)
    np.testing.assert_allclose(c, ref[3], rtol=0, atol=2e-4)
    # complex records: two-sided in fftfreq order whatever return_onesided says
    xc, yc = record(nfft, hop, True)
    ref = scipy_blocks(xc, yc, hann(nfft), nfft, hop, navg, step, True, nblocks, fs=fs, scaling="spectrum")
    r = RN.running_spectra(xc, yc, fs=fs, nperseg=nfft, noverlap=noverlap, navg=navg, step=step, scaling="spectrum")
    np.testing.assert_allclose(r.f, np.fft.fftfreq(nfft, 1 / fs), rtol=1e-15)
    np.testing.assert_allclose(r.t, tref, rtol=1e-15)
    within((r.Pxx, r.Pyy, r.Pxy), ref, "running_spectra, complex records")
