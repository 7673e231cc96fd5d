"""The polyphase synthesis bank on the MI355X against pfb_synth_ref of tests/test_host_pfb_synth.py (float64, the defining sum) run on
the frames as the device sees them (complex64) and on the taps as the library rounds them, float64(float32(g scale / M)).  Bound:
check_spectrum of tests/test_gpu_zoom.py (max err / max |ref| <= 1e-4, the project's bound for one transform stage); the round trip
through channelize has two stages, 2e-4 of max |x| on top of the float64 chain's own error.  Path (fused / composed) and partition
independence are bitwise."""
import numpy as np
import pytest

from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="no GPU")]

from pyfft_amd import _ffi, engine as E, channelizer as CH                  # noqa: E402
from test_host_multitaper import make_signal                                # noqa: E402
from test_host_channelizer import pfb_ref                                   # noqa: E402
from test_host_pfb_synth import pfb_synth_ref                               # noqa: E402
from test_gpu_zoom import samples, check_spectrum                           # noqa: E402

# (M, P, hop): one thread per transform; several groups per workgroup; a hop that neither divides nor is divided by M; 64 threads per
# transform; 32 branches and hop > M; one group per workgroup, a ring that fits for one-sided input only ... and one that never fits
SHAPES = [(16, 1, 8), (64, 3, 48), (64, 8, 33), (1024, 4, 512), (256, 32, 300), (4096, 8, 3072), (8192, 2, 8192)]
N0 = 123457
SCALE = 0.75


def prime_frames(M):
    return 257 if M <= 1024 else 37


def tap64(g, M, scale=SCALE):
    """The taps as the library rounds them, in float64."""
    g32 = np.asarray(g, dtype=np.float32).astype(np.float64)
    return (g32 * scale / M).astype(np.float32).astype(np.float64)


def random_frames(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("M,P,hop", SHAPES, ids=["M%d-P%d-D%d" % s for s in SHAPES])
@pytest.mark.parametrize("onesided", [True, False], ids=["half", "raw"])
def test_parity(M, P, hop, onesided):
    """Three rows of random frames under a random g; numpy and device-resident, both phase references, both input layouts, the
    centred geometry (first < 0) and not, 1, 2 and a prime number of frames, an nout that cuts the last frame short and one that goes
    past it (trailing zeros)."""
    import torch
    L, nb = M * P, (M // 2 + 1 if onesided else M)
    g = np.random.default_rng(91).standard_normal(L)
    tap = tap64(g, M)
    nfp = prime_frames(M)
    for center in (False, True):
        first = -(L // 2) if center else 0
        for nf in (1, 2, nfp):
            X = random_frames((3, nf, nb), 92 + nf)
            Xd = torch.as_tensor(X, device="cuda")
            end = first + (nf - 1) * hop + L
            r0 = (N0 + first) % M
            for phase_ref in (0, 1):
                if nf != nfp and phase_ref == 0:
                    continue
                rr = r0 if phase_ref else 0
                for nout in (end - 3, end + hop + 5):
                    ref = pfb_synth_ref(X, tap, M, hop, first, nout, phase_ref, rr, onesided=onesided)
                    what = "center %d, %d frames, phase_ref %d, nout %d" % (center, nf, phase_ref, nout)
                    got = E.pfb_synth(X, g, M, hop, first, nout, phase_ref, rr, onesided=onesided, scale=SCALE)
                    assert got.dtype == (np.float32 if onesided else np.complex64)
                    check_spectrum(got, ref, what + ", numpy, frame-major")
                    if nout > end:
                        assert np.all(got[..., end:] == 0), what
                    out = E.pfb_synth(Xd.transpose(-1, -2).contiguous(), g, M, hop, first, nout, phase_ref, rr, onesided=onesided,
                                      in_major=1, scale=SCALE)
                    assert out.is_cuda and out.dtype == (torch.float32 if onesided else torch.complex64)
                    assert np.array_equal(out.cpu().numpy(), got), what      # the same samples, bit for bit, from either layout
                    if nf == nfp:
                        one = E.pfb_synth(np.ascontiguousarray(np.swapaxes(X[1], -1, -2)), g, M, hop, first, nout, phase_ref, rr,
                                          onesided=onesided, in_major=1, scale=SCALE)
                        assert np.array_equal(one, got[1]), what
                        dev = E.pfb_synth(Xd, g, M, hop, first, nout, phase_ref, rr, onesided=onesided, scale=SCALE)
                        assert np.array_equal(dev.cpu().numpy(), got), what


def test_frames_outside_the_output_and_a_gap_before_the_first():
    """first > 0 (zeros before frame 0), a hop beyond the filter length (zeros between the frames), frames wholly past nout."""
    M, P = 64, 2
    L = M * P
    g = np.random.default_rng(93).standard_normal(L)
    for hop, first, nf, nout in ((L + 37, 50, 9, 5 * (L + 37)), (40, 300, 30, 700), (40, -(L - 1), 12, 200)):
        X = random_frames((2, nf, M), 94)
        ref = pfb_synth_ref(X, tap64(g, M), M, hop, first, nout, 1, 5)
        got = E.pfb_synth(X, g, M, hop, first, nout, 1, 5, onesided=False, scale=SCALE)
        check_spectrum(got, ref, "hop %d first %d" % (hop, first))
        assert np.array_equal(got == 0, ref == 0)


@pytest.mark.parametrize("M,P,hop", [(64, 8, 33), (1024, 4, 512)], ids=["M64", "M1024"])
@pytest.mark.parametrize("onesided", [True, False], ids=["half", "raw"])
def test_path_and_partition_independence(M, P, hop, onesided, monkeypatch):
    """Bitwise: the fused and the composed path; the fused path under run lengths of 1, halo + 1 and one that makes the last run
    ragged; two calls."""
    L, nb = M * P, (M // 2 + 1 if onesided else M)
    nf = prime_frames(M)
    g = np.random.default_rng(95).standard_normal(L)
    X = random_frames((3, nf, nb), 96)
    halo = -(-L // hop) - 1
    for first in (0, -(L // 2)):
        nout = first + (nf - 1) * hop + L + 11
        r0 = (N0 + first) % M
        args = (X, g, M, hop, first, nout, 1, r0)
        base = E.pfb_synth(*args, onesided=onesided, scale=SCALE)
        assert E.pfb_synth(*args, onesided=onesided, scale=SCALE).tobytes() == base.tobytes()
        check_spectrum(base, pfb_synth_ref(X, tap64(g, M), M, hop, first, nout, 1, r0, onesided=onesided), "default path")
        kernels = {}
        for path in ("fused", "composed"):
            monkeypatch.setenv("SP_PFBS_PATH", path)
            assert E.pfb_synth(*args, onesided=onesided, scale=SCALE).tobytes() == base.tobytes(), (first, path)
            E.profile_enable(True)
            E.pfb_synth(*args, onesided=onesided, scale=SCALE)
            kernels[path] = E.profile_last_kernel()
            E.profile_enable(False)
            if path == "fused":
                for fpg in (1, halo + 1, nf // 3 + 1):
                    assert nf % fpg != 0 or fpg == 1
                    monkeypatch.setenv("SP_PFBS_FPG", str(fpg))
                    assert E.pfb_synth(*args, onesided=onesided, scale=SCALE).tobytes() == base.tobytes(), (first, fpg)
                    monkeypatch.delenv("SP_PFBS_FPG")
            monkeypatch.delenv("SP_PFBS_PATH")
        assert "fused" in kernels["fused"] and "composed" in kernels["composed"], kernels


def chain_ref(x, h, g, M, hop, n0, mask=None):
    """The float64 chain on the float32-rounded taps: pfb_ref -> (mask) -> pfb_synth_ref under the centred plans; (y, valid)."""
    cplx = np.iscomplexobj(x)
    nsig = x.shape[-1]
    pa = CH.pfb_plan(nsig, cplx, M, hop=hop, h=h, center=True, n0=n0)
    h64 = np.asarray(h, dtype=np.float32).astype(np.float64)
    Xr = pfb_ref(samples(x), h64, M, hop, pa["first"], pa["nframes"], 1, pa["r0"])
    if not cplx:
        Xr = Xr[..., :M // 2 + 1]
    if mask is not None:
        Xr = Xr * mask[:, None].T
    ps = CH.pfb_synthesis_plan(pa["nframes"], not cplx, M, hop=hop, g=g, center=True, n0=n0, nsig=nsig)
    y = pfb_synth_ref(Xr, tap64(g, M, 1.0), M, hop, ps["first"], nsig, 1, ps["r0"], onesided=not cplx)
    return y, ps["valid"]


@pytest.mark.parametrize("M,taps,hop", [(64, 8, 32), (1024, 4, 512)], ids=["M64", "M1024"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_round_trip_on_the_device(M, taps, hop, cplx):
    """channelize then synthesize with the default dual, phase "time", n0 = 123457, centred: on `valid` the record comes back to
    e_ref + 2e-4 max |x|, e_ref the float64 chain's own round-trip error on the same float32-rounded taps."""
    import torch
    nsig = 30 * M + 7
    x = make_signal(nsig, cplx, 97)
    h = CH.pfb_prototype(M, taps)
    g, residual = CH.pfb_dual(h, M, hop)
    assert residual <= 1e-12
    xs = samples(x)
    yr, (lo, hi) = chain_ref(x, h, g, M, hop, N0)
    e_ref = float(np.max(np.abs(yr[lo:hi] - xs[lo:hi])))
    bound = e_ref + 2e-4 * float(np.max(np.abs(xs)))
    for dev in (False, True):
        xin = torch.as_tensor(_ffi.as_samples(x), device="cuda") if dev else x
        _, _, X = CH.channelize(xin, M, taps, hop, center=True, n0=N0)
        t, y = CH.synthesize(X, M, taps, hop, center=True, n0=N0, nsig=nsig, input_onesided=not cplx)
        if dev:
            assert y.is_cuda
            y = y.cpu().numpy()
        assert y.shape == (nsig,) and y.dtype == (np.complex64 if cplx else np.float32) and t.shape == (nsig,)
        err = float(np.max(np.abs(y[lo:hi] - xs[lo:hi])))
        print("M %d cplx %d device %d: round trip %.3g, e_ref %.3g, bound %.3g" % (M, cplx, dev, err, e_ref, bound))
        assert hi - lo > nsig // 2 and err <= bound


def test_masked_band():
    """An interferer's channels zeroed between channelize and synthesize: the device chain against the float64 chain doing the same."""
    M, taps, hop = 64, 8, 32
    nsig = 40 * M + 5
    n = np.arange(nsig)
    x = make_signal(nsig, True, 98) + 20.0 * np.exp(2j * np.pi * (9.3 / M) * n)
    h = CH.pfb_prototype(M, taps)
    g, _ = CH.pfb_dual(h, M, hop)
    mask = np.ones(M)
    mask[8:12] = 0.0
    _, _, X = CH.channelize(x, M, taps, hop, center=True, n0=N0)
    _, y = CH.synthesize(X * mask[:, None].astype(np.float32), M, taps, hop, center=True, n0=N0, nsig=nsig, input_onesided=False)
    yr, (lo, hi) = chain_ref(x, h, g, M, hop, N0, mask=mask)
    xs = samples(x)
    err = float(np.max(np.abs(y[lo:hi] - yr[lo:hi])))
    print("masked band: err %.3g of max |x| %.3g; residue of the interferer %.3g" %
          (err, float(np.max(np.abs(xs))), float(np.max(np.abs(yr[lo:hi])))))
    assert err <= 2e-4 * np.max(np.abs(xs))
    assert np.max(np.abs(yr[lo:hi])) < 0.5 * np.max(np.abs(xs))       # the interferer (amplitude 20) is gone from the reference


def test_refusals_through_the_raw_library(monkeypatch):
    """Every limit of one launch returns < 0, sp_last_error() names sp_pfb_synth, and a poisoned output buffer is unchanged; a forced
    fused path that does not fit is refused likewise."""
    lib = _ffi.load_library()
    _ffi.init()
    M, L, nf = 64, 256, 4
    X = np.zeros(2 * nf * M, dtype=np.complex64)
    g = np.ones(16 * 33, dtype=np.float32)
    nout = 3 * 48 + L
    y = np.full(2 * 2 * nout, 7.25, dtype=np.float32)
    ok = dict(sided=_ffi.SIDED_RAW, major=0, batch=2, nframes=nf, ntaps=L, M=M, hop=48, first=0, ref=1, r0=5, scale=1.0, nout=nout)

    def call(gg=g, Xp=X, yp=y, **kw):
        a = dict(ok, **kw)
        return lib.sp_pfb_synth(_ffi.ptr(Xp), a["sided"], a["major"], a["batch"], a["nframes"], _ffi.ptr(gg), a["ntaps"], a["M"],
                                a["hop"], a["first"], a["ref"], a["r0"], a["scale"], a["nout"], _ffi.ptr(yp), 0)
    bad_g = g.copy()
    bad_g[100] = np.inf
    cases = [dict(M=48, ntaps=192), dict(M=1, ntaps=4), dict(M=16384, ntaps=16384), dict(ntaps=L + 1), dict(ntaps=0),
             dict(M=16, ntaps=16 * 33), dict(hop=0), dict(nframes=0), dict(nout=0), dict(batch=-1), dict(r0=-1), dict(r0=M),
             dict(ref=2), dict(sided=_ffi.SIDED_ONE), dict(major=2), dict(scale=float("nan")), dict(scale=float("inf")),
             dict(gg=bad_g), dict(first=(1 << 40) + 1), dict(first=-(1 << 40) - 1),
             dict(nframes=(1 << 40) // 48 + 1), dict(M=2, ntaps=2, hop=1, batch=1 << 20, nframes=1 << 39),
             dict(Xp=None), dict(gg=None), dict(yp=None)]
    for kw in cases:
        assert call(**kw) < 0, kw
        msg = lib.sp_last_error().decode()
        assert "sp_pfb_synth" in msg, (kw, msg)
    # a forced fused path whose ring does not fit (two-sided, M = 8192, P = 2: 128 KiB behind a 64 KiB exchange image)
    Mb = 8192
    Xb, gb = np.zeros(nf * Mb, dtype=np.complex64), np.ones(2 * Mb, dtype=np.float32)
    yb = np.full(2 * (3 * 48 + 2 * Mb), 7.25, dtype=np.float32)
    big = dict(Xp=Xb, gg=gb, yp=yb, M=Mb, ntaps=2 * Mb, batch=1, nout=3 * 48 + 2 * Mb)
    monkeypatch.setenv("SP_PFBS_PATH", "fused")
    assert call(**big) < 0
    msg = lib.sp_last_error().decode()
    assert "sp_pfb_synth" in msg and "SP_PFBS_PATH=fused" in msg, msg
    assert np.all(yb == 7.25)
    monkeypatch.delenv("SP_PFBS_PATH")
    assert call(**big) == 0 and not np.all(yb == 7.25)              # the same call is served by the composed path
    monkeypatch.setenv("SP_PFBS_PATH", "sideways")
    assert call() < 0 and "sp_pfb_synth" in lib.sp_last_error().decode()
    monkeypatch.delenv("SP_PFBS_PATH")
    assert np.all(y == 7.25)
    assert call() == 0 and not np.all(y == 7.25)
