"""The polyphase filter-bank channelizer on the MI355X against pfb_ref of tests/test_host_channelizer.py (float64, the defining sum) run
on the float32-rounded taps and on the samples as the device sees them.  Bounds: those of tests/test_gpu_zoom.py -- check_spectrum for
frames (max err / max |ref| <= 1e-4), check_psd for power; the oscillator bound of tests/test_gpu_baseband.py (2e-7 per component of a
unit phasor) times sum |h| for a tone that the "time" phase reference makes constant.  Partition and chunk independence are bitwise."""
import numpy as np
import pytest
import scipy.signal as ss

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E, channelizer as CH                  # noqa: E402
from test_host_multitaper import make_signal                                # noqa: E402
from test_host_channelizer import pfb_ref                                   # noqa: E402
from test_gpu_zoom import samples, check_spectrum, check_psd                # noqa: E402


def taps32(h):
    """The taps as the device sees them, in float64."""
    return np.asarray(h, dtype=np.float32).astype(np.float64)


def ref_frames(x, h, M, hop, first, nframes, phase_ref, r0):
    """pfb_ref on what the device sees, cut to the bins the kernel writes: [..., nframes, nb]."""
    X = pfb_ref(samples(x), taps32(h), M, hop, first, nframes, phase_ref, r0)
    return X if np.iscomplexobj(x) else X[..., :M // 2 + 1]


# (M, P, D): one thread per transform; several groups per workgroup, one wave per transform; D neither divides nor is divided by M;
# 64 threads per transform and the taps held in registers; one group per workgroup; 512 threads; 32 branches and D > M
SHAPES = [(16, 1, 16), (64, 3, 48), (64, 8, 33), (1024, 4, 1024), (4096, 8, 3072), (8192, 2, 8192), (256, 32, 300)]
N0 = 123457


def prime_frames(M):
    """A prime frame count: whatever the run length, the last run of a row is ragged."""
    return 257 if M <= 1024 else 37


@pytest.mark.parametrize("M,P,D", SHAPES, ids=["M%d-P%d-D%d" % s for s in SHAPES])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_parity(M, P, D, cplx):
    """Three rows, numpy and device-resident with a row stride of nsig + 11; both phase references, both output layouts, centred (the
    first and last frames reach half a filter length outside the row) and not; 1, 2 and a prime number of frames."""
    import torch
    L = M * P
    h = CH.pfb_prototype(M, P) * M
    nfp = prime_frames(M)
    for center in (False, True):
        for nf in (1, 2, nfp):
            nsig = (nf - 1) * D + 1 if center else L + (nf - 1) * D + (D - 1 if nf > 1 else 0)
            x = make_signal(3 * nsig, cplx, 71).reshape(3, nsig)
            plan = CH.pfb_plan(nsig, cplx, M, hop=D, h=h, center=center, n0=N0)
            first, r0 = plan["first"], plan["r0"]
            assert plan["nframes"] == nf and first == (-(L // 2) if center else 0)
            base = torch.zeros((3, nsig + 11), dtype=torch.complex64 if cplx else torch.float32, device="cuda")
            base[:, :nsig] = torch.as_tensor(_ffi.as_samples(x), device="cuda")
            for phase_ref in (0, 1):
                if nf != nfp and phase_ref == 0:
                    continue
                rr = r0 if phase_ref else 0
                ref = ref_frames(x, h, M, D, first, nf, phase_ref, rr)
                what = "center %d, %d frames, phase_ref %d" % (center, nf, phase_ref)
                got = E.pfb(x, h, M, D, first, nf, phase_ref, rr)
                assert got.dtype == np.complex64
                check_spectrum(got, ref, what + ", numpy, frame-major")
                out = E.pfb(base[:, :nsig], h, M, D, first, nf, phase_ref, rr, out_major=1)
                assert out.is_cuda and out.dtype == torch.complex64
                dev = out.cpu().numpy()
                check_spectrum(dev, np.swapaxes(ref, -1, -2), what + ", device, x_ld = nsig + 11, bin-major")
                assert np.array_equal(np.swapaxes(dev, -1, -2), got), what      # the same frames, bit for bit, in either layout
                if nf == nfp:
                    check_spectrum(E.pfb(x[1], h, M, D, first, nf, phase_ref, rr, out_major=1), np.swapaxes(ref[1], -1, -2),
                                   what + ", numpy, one row, bin-major")
                    check_spectrum(E.pfb(base[:, :nsig], h, M, D, first, nf, phase_ref, rr).cpu().numpy(), ref, what + ", device")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_frames_that_barely_touch_the_row(cplx):
    """The first frame holds one sample of the row (its last), the last frame one (its first); a row shorter than the filter."""
    M, P, D = 64, 4, 40
    L = M * P
    h = CH.pfb_prototype(M, P) * M
    for nsig in (1000, 100):
        first = -(L - 1)
        nf = (nsig - 1 - first) // D + 1
        assert first + (nf - 1) * D <= nsig - 1 < first + nf * D
        x = make_signal(2 * nsig, cplx, 72).reshape(2, nsig)
        r0 = (N0 + first) % M
        check_spectrum(E.pfb(x, h, M, D, first, nf, 1, r0), ref_frames(x, h, M, D, first, nf, 1, r0), "nsig %d" % nsig)


@pytest.mark.parametrize("M,P,D", [(64, 3, 48), (1024, 4, 1024), (4096, 8, 3072)], ids=["M64", "M1024", "M4096"])
def test_channelize_axes_and_layout(M, P, D):
    """channelize: (f, t, X) with X in scipy's layout along any axis, numpy and device-resident, against the plan's geometry."""
    import torch
    nsig = M * P + 9 * D + 5
    x = make_signal(2 * nsig, True, 73).reshape(2, nsig)
    h = CH.pfb_prototype(M, P)
    for center in (False, True):
        plan = CH.pfb_plan(nsig, True, M, P, D, fs=48.0, center=center, n0=N0)
        ref = np.swapaxes(ref_frames(x, plan["h"], M, D, plan["first"], plan["nframes"], 1, plan["r0"]), -1, -2)
        f, t, X = CH.channelize(x, M, P, D, fs=48.0, center=center, n0=N0)
        assert np.array_equal(f, plan["f"]) and np.array_equal(t, plan["t"]) and X.shape == (2, M, plan["nframes"])
        check_spectrum(X, ref, "axis -1")
        _, _, Xt = CH.channelize(np.ascontiguousarray(x.T), M, P, D, fs=48.0, h=h, center=center, n0=N0, axis=0)
        assert Xt.shape == (M, 2, plan["nframes"]) and np.array_equal(np.moveaxis(Xt, 0, 1), X)
        _, _, Xd = CH.channelize(torch.as_tensor(_ffi.as_samples(x), device="cuda"), M, P, D, fs=48.0, center=center, n0=N0)
        assert Xd.is_cuda and np.array_equal(Xd.cpu().numpy(), X)
    xr = make_signal(nsig, False, 74)
    f, t, X = CH.channelize(xr, M, P, D, phase="frame")
    assert X.shape == (M // 2 + 1, (nsig - M * P) // D + 1) and f.shape == (M // 2 + 1,)
    check_spectrum(X, ref_frames(xr, h, M, D, 0, X.shape[1], 0, 0).T, "real, phase frame")


@pytest.mark.parametrize("M,P,D", [(64, 8, 33), (1024, 4, 1024), (4096, 8, 3072)], ids=["M64", "M1024", "M4096"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_partition_and_chunk_independence(M, P, D, cplx, monkeypatch):
    """Bitwise: (1) the frames [a, b) from a call of their own (first and r0 advanced); (2) the same call under other run lengths;
    (3) a record cut at sample a D and run as two chunks with n0 = a D gives the frames that lie wholly inside each chunk."""
    L = M * P
    nf = prime_frames(M)
    nsig = L + (nf - 1) * D + 3
    x = make_signal(2 * nsig, cplx, 75).reshape(2, nsig)
    h = CH.pfb_prototype(M, P) * M
    for center in (False, True):
        first = -(L // 2) if center else 0
        nfc = -(-nsig // D) if center else nf
        for phase_ref in (0, 1):
            r0 = (N0 + first) % M if phase_ref else 0
            full = E.pfb(x, h, M, D, first, nfc, phase_ref, r0)
            a, b = nfc // 3, nfc - 2
            part = E.pfb(x, h, M, D, first + a * D, b - a, phase_ref, (r0 + a * D) % M if phase_ref else 0)
            assert part.tobytes() == full[:, a:b].tobytes(), (center, phase_ref)
            for fpg in (1, 3, nfc):
                monkeypatch.setenv("SP_PFB_FPG", str(fpg))
                again = E.pfb(x, h, M, D, first, nfc, phase_ref, r0)
                monkeypatch.delenv("SP_PFB_FPG")
                assert again.tobytes() == full.tobytes(), (center, phase_ref, fpg)
    # chunks of one stream: frame m of the record starts at m D; the second chunk starts at sample a D
    a = nf // 2
    _, _, whole = CH.channelize(x, M, hop=D, h=h, n0=N0)
    _, _, head = CH.channelize(x[:, :a * D], M, hop=D, h=h, n0=N0) if a * D >= L else (None, None, None)
    _, _, tail = CH.channelize(x[:, a * D:], M, hop=D, h=h, n0=N0 + a * D)
    assert whole.shape[-1] == nf and tail.shape[-1] == nf - a
    assert tail.tobytes() == np.ascontiguousarray(whole[..., a:]).tobytes()
    if head is not None:
        nh = head.shape[-1]
        assert nh == (a * D - L) // D + 1 and head.tobytes() == np.ascontiguousarray(whole[..., :nh]).tobytes()


@pytest.mark.parametrize("M,P", [(64, 8), (1024, 4)], ids=["M64", "M1024"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_tone_is_constant_in_its_channel(M, P, cplx):
    """A float32 tone at k / M cycles per sample of absolute time, phase "time", D = 3 M / 4: the interior frames of channel k hold
    sum(h) (half of it for a real tone) to the oscillator bound 2e-7 per component times sum |h|; every other channel sits below the
    prototype's stopband, as in pfb_ref."""
    D, k, n0 = 3 * M // 4, 5, N0
    L = M * P
    nsig = L + 40 * D
    ph = 2 * np.pi * ((k * (n0 + np.arange(nsig))) % M) / M
    x = (np.cos(ph) if not cplx else np.exp(1j * ph)).astype(np.float32 if not cplx else np.complex64)
    h = CH.pfb_prototype(M, P)
    _, _, X = CH.channelize(x, M, hop=D, h=h, n0=n0)
    assert X.shape == (M if cplx else M // 2 + 1, 41)
    plan = CH.pfb_plan(nsig, cplx, M, hop=D, h=h, n0=n0)
    ref = ref_frames(x, h, M, D, 0, 41, 1, plan["r0"]).T
    sabs = float(np.sum(np.abs(taps32(h))))
    A = 8.0 / 0.1102 + 8.7                        # the design attenuation of the Kaiser (beta = 8) prototype, dB
    const = np.sum(taps32(h)) * (1.0 if cplx else 0.5)
    floor = abs(const) * 10 ** (-(A - 3.0) / 20)
    want = ref[k]
    d = X[k].astype(np.complex128) - (const if cplx else want)
    print("tone: worst deviation in channel %d: re %.3g im %.3g (bound %.3g)" %
          (k, float(np.max(np.abs(d.real))), float(np.max(np.abs(d.imag))), 2e-7 * sabs))
    if cplx:                                      # the channel is the constant sum(h) itself
        assert np.max(np.abs(want - const)) <= 2e-7 * sabs
    else:                                         # half of it, plus the image at -k seen through the stopband (it rotates)
        assert np.max(np.abs(want - const)) <= floor
    assert np.max(np.abs(d.real)) <= 2e-7 * sabs and np.max(np.abs(d.imag)) <= 2e-7 * sabs
    # the other channels: the Kaiser (beta = 8) design attenuation is 81.3 dB; the reference sits below it, and so does the device
    # within the bound of the frames
    others = np.ones(X.shape[0], dtype=bool)
    others[[k - 1, k, k + 1]] = False
    assert np.max(np.abs(ref[others])) <= floor
    assert np.max(np.abs(X[others])) <= floor + 2e-7 * sabs
    check_spectrum(X, ref, "tone")


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_pfb_psd(cplx, scaling):
    """pfb_psd against the mean power of pfb_ref's frames in float64, centred and not, numpy and device-resident rows; two calls agree
    bit for bit; the P = 1 Hann bank is scipy.signal.welch."""
    import torch
    fs = 250.0
    for (M, P, D) in ((64, 8, 33), (1024, 4, 1024), (4096, 8, 3072)):
        L = M * P
        nsig = L + (prime_frames(M) - 1) * D + 7
        x = make_signal(2 * nsig, cplx, 76).reshape(2, nsig)
        h = CH.pfb_prototype(M, P)
        h64 = taps32(h)
        for center in (False, True):
            plan = CH.pfb_plan(nsig, cplx, M, hop=D, h=h, fs=fs, center=center)
            X = ref_frames(x, h, M, D, plan["first"], plan["nframes"], 0, 0)
            ref = np.mean(np.abs(X) ** 2, axis=-2) * (1.0 / (fs * np.sum(h64 * h64)) if scaling == "density" else 1.0 / np.sum(h64) ** 2)
            if not cplx:
                ref[..., 1:M // 2] *= 2.0
            f, pxx = CH.pfb_psd(x, M, hop=D, h=h, fs=fs, center=center, scaling=scaling)
            assert pxx.dtype == np.float64 and pxx.shape == ref.shape and np.array_equal(f, plan["f"])
            check_psd(pxx, ref, "M %d center %d" % (M, center))
            _, again = CH.pfb_psd(x, M, hop=D, h=h, fs=fs, center=center, scaling=scaling)
            assert again.tobytes() == pxx.tobytes()
            _, dev = CH.pfb_psd(torch.as_tensor(_ffi.as_samples(x), device="cuda"), M, hop=D, h=h, fs=fs, center=center, scaling=scaling)
            assert dev.is_cuda and dev.dtype == torch.float64 and dev.cpu().numpy().tobytes() == pxx.tobytes()
    M = 256
    x = make_signal(40000, cplx, 77)
    win = ss.get_window("hann", M)
    f, pxx = CH.pfb_psd(x, M, hop=M // 2, h=win, fs=fs, scaling=scaling)
    fw, want = ss.welch(samples(x), fs=fs, window=taps32(win), nperseg=M, noverlap=M // 2, detrend=False, scaling=scaling,
                        return_onesided=not cplx)
    assert np.array_equal(f, fw)
    check_psd(pxx, want, "P = 1 Hann against scipy.signal.welch")


def test_refusals_through_the_raw_library():
    """Every limit of one launch returns < 0, sp_last_error() names sp_pfb, and a poisoned output buffer is unchanged."""
    lib = _ffi.load_library()
    _ffi.init()
    M, L, nsig = 64, 256, 1000
    x = np.zeros(2 * nsig, dtype=np.complex64)
    h = np.ones(16 * 33, dtype=np.float32)
    out = np.full(4 * 2 * 64 * 64, 7.25, dtype=np.float32)
    ok = dict(dt=1, nsig=nsig, ld=nsig, batch=2, ntaps=L, M=M, hop=48, first=0, nframes=4, ref=1, r0=5, kind=0, major=0, scale=1.0)

    def call(hh=h, **kw):
        a = dict(ok, **kw)
        return lib.sp_pfb(_ffi.ptr(x), a["dt"], a["nsig"], a["ld"], a["batch"], _ffi.ptr(hh), a["ntaps"], a["M"], a["hop"], a["first"],
                          a["nframes"], a["ref"], a["r0"], a["kind"], a["major"], a["scale"], _ffi.ptr(out), 0)
    bad_h = h.copy()
    bad_h[100] = np.inf
    cases = [dict(M=48, ntaps=192), dict(M=1, ntaps=4), dict(M=16384, ntaps=16384), dict(ntaps=L + 1), dict(ntaps=0),
             dict(M=16, ntaps=16 * 33), dict(hop=0), dict(nframes=0), dict(r0=-1), dict(r0=M), dict(ref=2), dict(kind=2), dict(major=2),
             dict(scale=float("nan")), dict(dt=3), dict(ld=nsig - 1), dict(nsig=0, ld=0), dict(batch=-1),
             dict(first=-L), dict(first=nsig), dict(first=nsig - 48 * 3), dict(first=-(L - 1), nframes=28),
             dict(M=2, ntaps=2, hop=1, nsig=1 << 40, ld=1 << 40, batch=1 << 20, nframes=1 << 39), dict(hh=bad_h),
             dict(major=1, nframes=65535 * 32 + 1, hop=1, nsig=1 << 30, ld=1 << 30, batch=1)]
    for kw in cases:
        assert call(**kw) < 0, kw
        msg = lib.sp_last_error().decode()
        assert "sp_pfb" in msg, (kw, msg)
    assert np.all(out == 7.25)
    assert call() == 0 and not np.all(out == 7.25)
