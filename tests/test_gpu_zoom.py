"""The chirp-z transform and the zoom spectra on the MI355X against float64 references: scipy.signal.czt for sp_czt, the frame-loop
oracle of tests/test_host_zoom.py for the estimators, and the library's own FFT / Welch where an arc lies on the FFT grid.  Every bin
is compared.  Bounds (the project's own): complex spectra within 1e-4 of the largest |ref|; PSD rtol 2e-4, atol 1e-6 max; cross
spectra rtol 2e-4, atol 2e-6 max |ref|; coherence 2e-4 absolute and inside [0, 1 + 1e-5].  References are computed from the float32 /
complex64 samples the device sees."""
import numpy as np
import pytest
import scipy.signal as ss

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E, zoom as ZM                          # noqa: E402
from test_host_multitaper import make_signal                                # noqa: E402
from test_host_zoom import zoom_oracle                                       # noqa: E402

START, FS = 0.1037, 250.0


def samples(x):
    """The record as the device sees it, in float64."""
    return _ffi.as_samples(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def scipy_czt(x, m, start, step):
    return ss.czt(samples(x), m, w=np.exp(-2j * np.pi * step), a=np.exp(2j * np.pi * start))


def check_spectrum(got, ref, what=""):
    err = float(np.max(np.abs(np.asarray(got, dtype=np.complex128) - ref)) / np.max(np.abs(ref)))
    print("%s max err / max |ref| = %.3g" % (what, err))
    assert got.shape == ref.shape and err <= 1e-4, what


def check_psd(got, ref, what=""):
    print("%s psd max rel err %.3g" % (what, float(np.max(np.abs(got - ref) / ref.max()))))
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-6 * ref.max(), err_msg=what)


def check_csd(got, ref, what=""):
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-6 * np.abs(ref).max(), err_msg=what)


FUSED = [(8, 5), (1000, 300), (4096, 1024), (4096, 4096), (7000, 1000), (100, 8000)]


@pytest.mark.parametrize("n,m", FUSED)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_czt_fused(n, m, cplx):
    """One workgroup per transform: batch 37 and batch 1, numpy and device-resident, a row stride beyond n."""
    import torch
    step = 0.3 / m
    x = make_signal(37 * n, cplx, 21).reshape(37, n)
    ref = scipy_czt(x, m, START, step)
    check_spectrum(E.czt(x, m, START, step), ref, "numpy batch 37")
    check_spectrum(E.czt(x[5], m, START, step), ref[5], "numpy batch 1")
    base = torch.zeros((37, n + 5), dtype=torch.complex64 if cplx else torch.float32, device="cuda")
    base[:, :n] = torch.as_tensor(_ffi.as_samples(x), device="cuda")
    view = base[:, :n]                                                       # x_ld = n + 5
    out = E.czt(view, m, START, step)
    assert out.is_cuda and out.dtype == torch.complex64
    check_spectrum(out.cpu().numpy(), ref, "device batch 37, x_ld > n")
    check_spectrum(E.czt(view[7], m, START, step).cpu().numpy(), ref[7], "device batch 1")
    # the scipy signatures
    check_spectrum(ZM.czt(x, m, np.exp(-2j * np.pi * step), np.exp(2j * np.pi * START)), ref, "czt(w, a)")
    check_spectrum(ZM.czt(x.T, m, np.exp(-2j * np.pi * step), np.exp(2j * np.pi * START), axis=0), ref.T, "czt(axis=0)")
    check_spectrum(ZM.zoom_fft(x, [START * FS, (START + m * step) * FS], m, fs=FS), ref, "zoom_fft")


@pytest.mark.parametrize("n,m,batch,cplx", [(116508, 2048, 37, False), (116508, 2048, 1, True), (1 << 20, 4096, 1, False),
                                            (1 << 20, 4096, 2, True), (300, 1 << 17, 1, False), (300, 1 << 17, 3, True)])
def test_czt_long(n, m, batch, cplx):
    """Beyond one workgroup: the multi-pass form, numpy and device-resident, a row stride beyond n."""
    import torch
    step = 0.3 / m if m < n else 0.4 / m
    x = make_signal(batch * n, cplx, 22).reshape(batch, n)
    ref = scipy_czt(x, m, START, step)
    check_spectrum(E.czt(x, m, START, step), ref, "numpy")
    base = torch.zeros((batch, n + 3), dtype=torch.complex64 if cplx else torch.float32, device="cuda")
    base[:, :n] = torch.as_tensor(_ffi.as_samples(x), device="cuda")
    check_spectrum(E.czt(base[:, :n], m, START, step).cpu().numpy(), ref, "device, x_ld > n")


@pytest.mark.parametrize("n", [4096, 1000])
def test_full_circle_is_the_fft(n):
    x = make_signal(3 * n, True, 23).reshape(3, n)
    ref = E.fft(x).astype(np.complex128)
    check_spectrum(ZM.zoom_fft(x, [0, FS], n, fs=FS), ref, "zoom_fft over the circle")
    check_spectrum(ZM.czt(x), ref, "czt defaults")


def estimator_case(cplx, detrend, nperseg, noverlap, nsig, m, band, on_device):
    import torch
    x, y = make_signal(nsig, cplx, 24), make_signal(nsig, cplx, 25)
    kw = dict(fs=FS, window="hann", nperseg=nperseg, noverlap=noverlap, detrend=detrend)
    plan = ZM.zoom_plan(nsig, cplx, band, m, **kw)
    o = zoom_oracle(samples(x), samples(y), plan)
    Zref = zoom_oracle(samples(x), None, dict(plan, fold=np.ones(m)), stft=True)
    if on_device:
        x, y = (torch.as_tensor(_ffi.as_samples(v), device="cuda") for v in (x, y))
    host = (lambda a: a.cpu().numpy()) if on_device else (lambda a: a)
    f, pxx = ZM.zoom_psd(x, band, m, **kw)
    np.testing.assert_array_equal(f, plan["freq"])
    check_psd(host(pxx), o["pxx"], "pxx")
    f, pxy = ZM.zoom_csd(x, y, band, m, **kw)
    check_csd(host(pxy), o["pxy"], "pxy")
    _, pyy = ZM.zoom_psd(y, band, m, **kw)
    check_psd(host(pyy), o["pyy"], "pyy")
    f, cxy = ZM.zoom_coherence(x, y, band, m, **kw)
    cref = np.abs(o["pxy"]) ** 2 / (o["pxx"] * o["pyy"])
    cxy = host(cxy)
    assert np.all(cxy >= 0) and np.all(cxy <= 1 + 1e-5)
    assert np.max(np.abs(cxy - cref)) <= 2e-4
    f, t, Z = ZM.zoom_stft(x, band, m, **kw)
    np.testing.assert_allclose(t, (np.arange(plan["nframes"]) * plan["hop"] + nperseg / 2) / FS)
    check_spectrum(host(Z), Zref, "stft")
    return plan


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("detrend", [False, "constant", "linear"])
@pytest.mark.parametrize("nperseg,noverlap", [(256, 0), (256, 128), (1000, 667), (300, 223)], ids=["hop=n", "hop=n/2", "n1000-odd-hop", "n300-hop77"])
def test_estimators(cplx, detrend, nperseg, noverlap):
    """Hops nperseg, nperseg / 2 and odd ones; power-of-two and other segment lengths; all three detrends; a band around the strong
    line at 0.11 fs and one that holds the weak line at 0.31 fs, 50 dB down."""
    plan = estimator_case(cplx, detrend, nperseg, noverlap, 40 * nperseg + 11, 200, [0.09 * FS, 0.13 * FS], False)
    assert plan["nframes"] >= 40
    estimator_case(cplx, detrend, nperseg, noverlap, 12 * nperseg + 3, 96, [0.28 * FS, 0.34 * FS], True)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_estimators_ragged_runs_and_single_frame(cplx):
    """More frames than transform groups in a launch, and not a multiple of them (the clamped, zero-weighted tail of the last runs);
    and a single frame."""
    import ctypes
    info = (ctypes.c_int64 * 4)()
    _ffi.init()
    assert _ffi.lib().sp_device_info(info) == 0
    ncu = int(info[0])
    nperseg, m = 256, 200                                                    # L = 512: 8 transform groups per workgroup
    groups = ncu * 4 * 8
    nframes = groups + groups // 2 + 3                                       # runs of 2 frames; the last groups get 1 or 0
    plan = estimator_case(cplx, "constant", nperseg, 192, (nframes - 1) * 64 + nperseg, m, [0.10 * FS, 0.12 * FS], True)
    assert plan["nframes"] == nframes and nframes % groups != 0
    plan = estimator_case(cplx, "linear", 777, None, 777, 333, [0.10 * FS, 0.12 * FS], False)
    assert plan["nframes"] == 1


@pytest.mark.parametrize("nperseg,noverlap", [(4096, 2048), (1000, 500)])
def test_arc_on_the_fft_grid_is_welch(nperseg, noverlap):
    """An arc laid on FFT bins returns the library's own Welch PSD on those bins."""
    nsig, k0, m = 64 * nperseg, 37, nperseg // 4
    hop = nperseg - noverlap
    for cplx in (False, True):
        x = make_signal(nsig, cplx, 26)
        win = ss.get_window("hann", nperseg)
        M = 1 + (nsig - nperseg) // hop
        ref = E.welch_psd(x, win, hop, M, detrend=True, sided=E.SIDED_RAW, scale=1.0 / (FS * np.sum(win ** 2)))
        f, pxx = ZM.zoom_psd(x, [k0 * FS / nperseg, (k0 + m) * FS / nperseg], m, fs=FS, window=win, noverlap=noverlap, detrend="constant",
                             return_onesided=False)
        check_psd(pxx, np.asarray(ref)[k0:k0 + m], "grid-aligned")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_long_segments(cplx):
    """nperseg = 116 508 (the reference's default Navr = 8 regime), m = 1000 bins around the strong line: the multi-pass form."""
    nperseg, m = 116508, 1000
    nsig = 3 * nperseg + 1234
    x, y = make_signal(nsig, cplx, 27), make_signal(nsig, cplx, 28)
    band = [(0.11 - 2e-4) * FS, (0.11 + 2e-4) * FS]
    kw = dict(fs=FS, window="hann", nperseg=nperseg, noverlap=None, detrend="linear")
    plan = ZM.zoom_plan(nsig, cplx, band, m, **kw)
    assert plan["nframes"] == 5
    o = zoom_oracle(samples(x), samples(y), plan)
    Zref = zoom_oracle(samples(x), None, dict(plan, fold=np.ones(m)), stft=True)
    _, pxx = ZM.zoom_psd(x, band, m, **kw)
    check_psd(pxx, o["pxx"], "long pxx")
    _, pxy = ZM.zoom_csd(x, y, band, m, **kw)
    check_csd(pxy, o["pxy"], "long pxy")
    _, cxy = ZM.zoom_coherence(x, y, band, m, **kw)
    assert np.all(cxy >= 0) and np.all(cxy <= 1 + 1e-5)
    assert np.max(np.abs(cxy - np.abs(o["pxy"]) ** 2 / (o["pxx"] * o["pyy"]))) <= 2e-4
    _, _, Z = ZM.zoom_stft(x, band, m, **kw)
    check_spectrum(Z, Zref, "long stft")


def test_off_grid_sine_is_located():
    """A sine between two FFT bins, zoomed at 1 / 64 of the bin spacing: the peak lands within one zoom bin of its frequency."""
    n, m = 4096, 256
    f0 = 100.37 / n                                                          # cycles per sample
    x = np.sin(2 * np.pi * f0 * np.arange(8 * n) + 0.4)
    step = 1.0 / (64 * n)
    f1 = 100.0 / n
    f, pxx = ZM.zoom_psd(x, [f1, f1 + m * step], m, fs=1.0, window="hann", nperseg=n, noverlap=n // 2)
    assert abs(f[1] - f[0] - step) < 1e-15
    print("peak at %.9f, true %.9f, zoom bin %.3g" % (f[np.argmax(pxx)], f0, step))
    assert abs(f[np.argmax(pxx)] - f0) <= step


def test_two_calls_agree_bitwise():
    for nperseg, m in ((1000, 300), (116508, 1000)):
        nsig = 6 * nperseg + 17
        x, y = make_signal(nsig, False, 29), make_signal(nsig, False, 30)
        band = [0.10 * FS, 0.12 * FS]
        kw = dict(fs=FS, nperseg=nperseg, detrend="constant")
        a, b = ZM.zoom_psd(x, band, m, **kw)[1], ZM.zoom_psd(x, band, m, **kw)[1]
        assert a.tobytes() == b.tobytes()
        a, b = ZM.zoom_csd(x, y, band, m, **kw)[1], ZM.zoom_csd(x, y, band, m, **kw)[1]
        assert a.tobytes() == b.tobytes()
        a, b = ZM.zoom_stft(x, band, m, **kw)[2], ZM.zoom_stft(x, band, m, **kw)[2]
        assert a.tobytes() == b.tobytes()
        xr = x[:nperseg]
        a, b = E.czt(xr, m, START, 0.3 / m), E.czt(xr, m, START, 0.3 / m)
        assert a.tobytes() == b.tobytes()


def test_refusals_through_the_raw_abi():
    """rc < 0 with the entry point's name in the message; the checks come before the device is touched."""
    _ffi.init()
    lib, p = _ffi.lib(), _ffi.ptr
    x = np.zeros(4096, dtype=np.float32)
    out = np.zeros(4096, dtype=np.complex64)
    pxx = np.zeros(64)
    win = np.ones(256, dtype=np.float32)
    nan, inf, big = float("nan"), float("inf"), 1 << 26

    def czt(n=256, ld=256, batch=1, m=64, start=0.1, step=1e-3):
        return lib.sp_czt(p(x), 0, n, ld, batch, m, start, step, p(out), 0)

    def zw(nsig=4096, nfft=256, hop=128, nframes=4, m=64, start=0.1, step=1e-3, detrend=1, win_=win):
        return lib.sp_zoom_welch(p(x), None, 0, nsig, p(win_), nfft, hop, nframes, detrend, None, None, m, start, step, 1.0, p(pxx), None,
                                 None, None, 0)

    for name, call in (("sp_czt", lambda: czt(n=0)), ("sp_czt", lambda: czt(m=0)), ("sp_czt", lambda: czt(n=-3)),
                       ("sp_czt", lambda: czt(start=nan)), ("sp_czt", lambda: czt(step=inf)), ("sp_czt", lambda: czt(step=nan)),
                       ("sp_czt", lambda: czt(m=big)), ("sp_czt", lambda: czt(n=big + 1, ld=big + 1)), ("sp_czt", lambda: czt(ld=100)),
                       ("sp_zoom_welch", lambda: zw(nfft=0)), ("sp_zoom_welch", lambda: zw(m=0)), ("sp_zoom_welch", lambda: zw(m=-1)),
                       ("sp_zoom_welch", lambda: zw(start=inf)), ("sp_zoom_welch", lambda: zw(step=nan)),
                       ("sp_zoom_welch", lambda: zw(m=big)), ("sp_zoom_welch", lambda: zw(hop=0)), ("sp_zoom_welch", lambda: zw(hop=-5)),
                       ("sp_zoom_welch", lambda: zw(nframes=0)), ("sp_zoom_welch", lambda: zw(nframes=40)),
                       ("sp_zoom_welch", lambda: zw(detrend=3)),
                       ("sp_czt_chirp", lambda: lib.sp_czt_chirp(0, 4, nan, 0.0, p(out))),
                       ("sp_czt_chirp", lambda: lib.sp_czt_chirp(0, -1, 0.1, 0.0, p(out)))):
        assert call() < 0
        assert name in lib.sp_last_error().decode()
    assert czt() == 0 and zw() == 0                                          # the same calls with good arguments go through
