"""The digital down-converter and the band spectra on the MI355X against float64 references: ddc_ref of tests/test_host_baseband.py
(oscillator phases exact) for sp_ddc, and scipy.signal.welch / csd / stft run on the float64 baseband signal for the estimators.
Bounds.  Oscillator: 2e-7 absolute per component (float32 rounding of a unit phasor plus a 1e-9-turn phase budget, as
test_host_zoom.test_chirp_table_phases_are_exact).  Filtered outputs: max error relative to the rms of the reference at most 4 x what a
float32 numpy restatement of the same arithmetic (ddc_f32 below: phasor rounded to float32, complex64 product, taps accumulated in order
in float32) loses on the same input; the factor covers another summation order.  Spectra: the bounds of tests/test_gpu_zoom.py."""
import numpy as np
import pytest
import scipy.signal as ss

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E, baseband as BB                      # noqa: E402
from test_host_multitaper import make_signal                                # noqa: E402
from test_host_baseband import ddc_ref, cascade_ref, exact_turns            # noqa: E402
from test_gpu_zoom import samples, check_spectrum, check_psd, check_csd     # noqa: E402

NU = 0.1234


def taps32(h):
    """The taps as the device sees them, in float64."""
    return np.asarray(h, dtype=np.float32).astype(np.float64)


def ddc_f32(x, nu, q, h, n0=0):
    """The arithmetic of the kernel restated in float32 numpy, in the plainest order."""
    x = _ffi.as_samples(x).astype(np.complex64)
    n, T = x.shape[-1], len(h)
    if nu != 0.0:
        x = x * np.exp(-2j * np.pi * exact_turns(nu, n0, n)).astype(np.complex64)
    rows = x.reshape(-1, n)
    nout = -(-n // q)
    pad = np.zeros((rows.shape[0], n + 2 * T), dtype=np.complex64)
    pad[:, T:T + n] = rows
    idx = np.arange(nout) * q + (T - 1) // 2 + T
    h32 = np.asarray(h, dtype=np.float32)
    acc = np.zeros((rows.shape[0], nout), dtype=np.complex64)
    for j in range(T):
        acc = acc + h32[j] * pad[:, idx - j]
    assert acc.dtype == np.complex64
    return acc.reshape(x.shape[:-1] + (nout,))


def tolerance(ref, f32, what=""):
    rms = float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    loss = float(np.max(np.abs(f32.astype(np.complex128) - ref))) / rms
    print("%s float32 restatement loses %.3g of the rms" % (what, loss))
    assert 0 < loss < 1e-4                                                   # a guard on the restatement itself, not the bound
    return rms, 4.0 * loss


def check_against(got, ref, f32, what="", keep=None):
    rms, tol = tolerance(ref, f32, what)
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.complex64, what
    d = np.abs(got.astype(np.complex128) - ref)
    if keep is not None:
        d = d[..., keep]
    err = float(np.max(d)) / rms
    print("%s max err / rms = %.3g (bound %.3g)" % (what, err, tol))
    assert err <= tol, what


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_identity_is_bit_exact(cplx):
    """q = 1, h = [1], nu = 0: the input comes back bit for bit, over more than two tiles, numpy and device-resident."""
    import torch
    n = 2 * E.ddc_tile(1) + 905
    x = _ffi.as_samples(make_signal(3 * n, cplx, 51).reshape(3, n))
    want = x.astype(np.complex64)
    for got in (E.ddc(x, 0.0, 1, [1.0]), E.ddc(torch.as_tensor(x, device="cuda"), 0.0, 1, [1.0], n0=12345).cpu().numpy(),
                E.ddc(x, 0.0, 1, [1.0], n0=-7)):
        assert got.dtype == np.complex64 and got.shape == want.shape
        assert got.tobytes() == want.tobytes()


NUS = [0.25, 0.3 / 116508, -0.013, np.sqrt(2.0) - 1.0, 1e-9]


@pytest.mark.parametrize("nu", NUS, ids=["%g" % v for v in NUS])
@pytest.mark.parametrize("q", [1, 7])
def test_oscillator_phases(q, nu):
    """h = [1], x = 1: every output is the oscillator itself, at sample indices where a float64 product nu n has lost its fraction."""
    nsig = 3 * E.ddc_tile(q) * q + 5
    worst = 0.0
    for n0 in (0, (1 << 24) - 3, (1 << 31) + 5, (1 << 40) - 4096):
        t = exact_turns(nu, n0, nsig)[::q]
        ref = np.stack([np.cos(2 * np.pi * t), -np.sin(2 * np.pi * t)], axis=-1)
        for x in (np.ones(nsig, dtype=np.float32), np.ones(nsig, dtype=np.complex64)):
            got = E.ddc(x, nu, q, [1.0], n0=n0)
            assert got.shape == (t.size,)
            worst = max(worst, float(np.max(np.abs(got.view(np.float32).reshape(-1, 2).astype(np.float64) - ref))))
    print("q %d nu %r: worst phasor error %.3g" % (q, nu, worst))
    assert worst <= 2e-7


SHAPES = [(1, 33, 300), (4, 33, 1000), (7, 57, 1001), (16, 129, 257), (64, 4095, 64 * 40 + 13), (8, 65, 5)]


@pytest.mark.parametrize("q,T,nsig", SHAPES, ids=["q%d-T%d-n%d" % s for s in SHAPES])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_parity(q, T, nsig, cplx):
    """Three rows, numpy and device-resident with a row stride of nsig + 11; a record shorter than two filter spans; nsig < q."""
    import torch
    n0 = 12345
    x = make_signal(3 * nsig, cplx, 52).reshape(3, nsig)
    h = ss.firwin(T, 0.8 / q)
    ref = ddc_ref(samples(x), NU, q, taps32(h), n0)
    f32 = ddc_f32(x, NU, q, h, n0)
    assert ref.shape == (3, -(-nsig // q))
    check_against(E.ddc(x, NU, q, h, n0=n0), ref, f32, "numpy")
    check_against(E.ddc(x[1], NU, q, h, n0=n0), ref[1], f32[1], "numpy, one row")
    base = torch.zeros((3, nsig + 11), dtype=torch.complex64 if cplx else torch.float32, device="cuda")
    base[:, :nsig] = torch.as_tensor(_ffi.as_samples(x), device="cuda")
    out = E.ddc(base[:, :nsig], NU, q, h, n0=n0)
    assert out.is_cuda and out.dtype == torch.complex64
    check_against(out.cpu().numpy(), ref, f32, "device, x_ld = nsig + 11")
    check_against(E.ddc(base[2, :nsig], NU, q, h, n0=n0).cpu().numpy(), ref[2], f32[2], "device, one row")
    # the public function: the same stage from the caller's taps, and along another axis
    check_against(BB.ddc(x, NU * 50.0, q, fs=50.0, taps=h, n0=n0), ref, f32, "baseband.ddc(taps=)")
    check_against(BB.ddc(x.T, NU * 50.0, q, fs=50.0, taps=h, n0=n0, axis=0), ref.T, f32.T, "baseband.ddc(axis=0)")


@pytest.mark.parametrize("q,T", [(1, 129), (8, 459), (64, 1025)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_tile_seams_and_chunks(q, T, cplx):
    """A record over three of the kernel's largest tiles plus one sample equals the reference everywhere; cut in two chunks at a
    multiple of q, with n0 carried, it agrees away from the filter's reach either side of the cut."""
    largest = max(E.ddc_tile(k) * k for k in range(1, 65))
    assert largest == 4096 and E.ddc_tile(q) * q <= largest
    nsig, n0 = 3 * largest + 1, (1 << 31) - 1000
    x = make_signal(nsig, cplx, 53)
    h = ss.firwin(T, 0.8 / q)
    ref = ddc_ref(samples(x), NU, q, taps32(h), n0)
    f32 = ddc_f32(x, NU, q, h, n0)
    check_against(E.ddc(x, NU, q, h, n0=n0), ref, f32, "one piece")
    cut = (nsig // 2 // q) * q + q
    two = np.concatenate([E.ddc(x[:cut], NU, q, h, n0=n0), E.ddc(x[cut:], NU, q, h, n0=n0 + cut)])
    reach = (T - 1) // 2 // q + 1
    keep = np.abs(np.arange(ref.size) - cut // q) > reach
    assert two.shape == ref.shape and np.count_nonzero(~keep) <= 2 * reach + 1
    check_against(two, ref, f32, "two chunks", keep=keep)


def test_cascade():
    """ddc(x, fc, 256): two stages, 64 then 4, the intermediate on the device, against the float64 cascade."""
    import torch
    fs, fc, q = 48000.0, 5000.0, 256
    nsig = 300 * q + 17
    x = make_signal(nsig, False, 54)
    stages = BB.ddc_plan(q)
    assert [qi for qi, _ in stages] == [64, 4]
    st32 = [(qi, taps32(h)) for qi, h in stages]
    ref = cascade_ref(samples(x), fc / fs, st32)
    mid = ddc_f32(x, fc / fs, 64, stages[0][1])
    f32 = ddc_f32(mid, 0.0, 4, stages[1][1])
    assert ref.shape == (-(-(-(-nsig // 64)) // 4),) == (301,)
    check_against(BB.ddc(x, fc, q, fs), ref, f32, "numpy")
    out = BB.ddc(torch.as_tensor(_ffi.as_samples(x), device="cuda"), fc, q, fs)
    assert out.is_cuda
    check_against(out.cpu().numpy(), ref, f32, "device")


@pytest.fixture(scope="module")
def band_case():
    """Inputs, the float64 baseband signals and what the comparisons share, computed once."""
    out = {}
    fs, fc, q, nperseg = 8000.0, 1000.0, 8, 256
    st32 = [(qi, taps32(h)) for qi, h in BB.ddc_plan(q)]
    for cplx in (False, True):
        x, y = make_signal(1 << 16, cplx, 55), make_signal(1 << 16, cplx, 56)
        zx, zy = (cascade_ref(samples(v), fc / fs, st32) for v in (x, y))
        out[cplx] = (x, y, zx, zy)
    grid = np.fft.fftshift(np.fft.fftfreq(nperseg, q / fs))
    keep = np.abs(grid) <= 0.8 * fs / (2 * q) * (1 + 1e-12)
    out["const"] = (fs, fc, q, nperseg, fc + grid[keep], keep)
    return out


def shifted(a, keep):
    return np.fft.fftshift(a, axes=0)[keep]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
def test_band_spectra(band_case, cplx, scaling):
    """nperseg 256, q 8, 2^16 samples: welch / csd / coherence / stft of scipy on the float64 baseband signal, two-sided, shifted and cut
    the same way; numpy in and device-resident in."""
    import torch
    fs, fc, q, nperseg, fref, keep = band_case["const"]
    x, y, zx, zy = band_case[cplx]
    kw = dict(fs=fs / q, window="hann", nperseg=nperseg, noverlap=nperseg // 2, detrend=False, return_onesided=False, scaling=scaling)
    pxx = shifted(ss.welch(zx, **kw)[1], keep)
    pyy = shifted(ss.welch(zy, **kw)[1], keep)
    pxy = shifted(ss.csd(zx, zy, **kw)[1], keep)
    _, tref, Zref = ss.stft(zx, boundary=None, padded=False, **dict(kw, scaling="psd" if scaling == "density" else "spectrum"))
    Zref = shifted(Zref, keep)
    assert 180 <= fref.size < nperseg and abs(fref[0] - (fc - 400.0)) < 4.0
    bk = dict(fs=fs, nperseg=nperseg, scaling=scaling, return_onesided=False)
    for dev in (False, True):
        xx, yy = ((torch.as_tensor(_ffi.as_samples(v), device="cuda") for v in (x, y)) if dev else (x, y))
        host = (lambda a: a.cpu().numpy()) if dev else (lambda a: a)
        f, got = BB.band_psd(xx, fc, q, **bk)
        np.testing.assert_allclose(f, fref, rtol=1e-13)
        check_psd(host(got), pxx, "pxx")
        check_psd(host(BB.band_psd(yy, fc, q, **bk)[1]), pyy, "pyy")
        f, got = BB.band_csd(xx, yy, fc, q, **bk)
        check_csd(host(got), pxy, "pxy")
        f, cxy = BB.band_coherence(xx, yy, fc, q, **bk)
        cxy = host(cxy)
        assert np.all(cxy >= 0) and np.all(cxy <= 1 + 1e-5)
        assert np.max(np.abs(cxy - np.abs(pxy) ** 2 / (pxx * pyy))) <= 2e-4
        f, t, Z = BB.band_stft(xx, fc, q, **bk)
        np.testing.assert_allclose(t, tref, rtol=1e-13)
        check_spectrum(host(Z), Zref, "stft")
    if not cplx:                                                            # one-sided: a real record's band, doubled
        f, got = BB.band_psd(x, fc, q, fs=fs, nperseg=nperseg, scaling=scaling)
        check_psd(got, 2.0 * pxx, "one-sided pxx")
        check_csd(BB.band_csd(x, y, fc, q, fs=fs, nperseg=nperseg, scaling=scaling)[1], 2.0 * pxy, "one-sided pxy")


def test_line_power():
    """A real sinusoid of amplitude A on a kept bin: the one-sided 'spectrum' peak is A^2 / 2 within 1e-3 (passband ripple 7e-5,
    image below -87 dB, float32)."""
    A, q, nperseg = 1.7, 8, 256
    fc = 0.125
    f0 = fc + 5.0 / (q * nperseg)
    x = A * np.cos(2 * np.pi * f0 * np.arange(1 << 16) + 0.4)
    f, pxx = BB.band_psd(x, fc, q, nperseg=nperseg, scaling="spectrum")
    k = int(np.argmax(pxx))
    print("peak %.6g at %.9f; A^2 / 2 = %.6g, line at %.9f" % (pxx[k], f[k], A * A / 2, f0))
    assert abs(f[k] - f0) < 1e-12
    assert abs(pxx[k] - A * A / 2) <= 1e-3 * A * A / 2


def test_refusals_through_the_raw_abi():
    """rc < 0 with the entry point's name in the message; the checks come before the device is touched."""
    _ffi.init()
    lib, p = _ffi.lib(), _ffi.ptr
    x = np.zeros(4096, dtype=np.float32)
    out = np.zeros(4096, dtype=np.complex64)
    h = np.ones(4097, dtype=np.float32)
    nan = float("nan")

    def ddc(dtype=0, nsig=1024, ld=1024, batch=1, nu=0.1, n0=0, q=8, ntaps=33, xp=p(x), hp=p(h), op=p(out)):
        return lib.sp_ddc(xp, dtype, nsig, ld, batch, nu, n0, q, hp, ntaps, op, 0)

    for call in (lambda: ddc(q=0), lambda: ddc(q=65), lambda: ddc(q=-1), lambda: ddc(ntaps=32), lambda: ddc(ntaps=4097),
                 lambda: ddc(ntaps=0), lambda: ddc(ld=1000), lambda: ddc(nu=nan), lambda: ddc(nu=float("inf")),
                 lambda: ddc(n0=1 << 41), lambda: ddc(n0=-(1 << 41)), lambda: ddc(nsig=0), lambda: ddc(dtype=2),
                 lambda: ddc(batch=-1), lambda: ddc(xp=None), lambda: ddc(hp=None), lambda: ddc(op=None)):
        assert call() < 0
        assert "sp_ddc" in lib.sp_last_error().decode()
    assert ddc() == 0                                                        # the same call with good arguments goes through
