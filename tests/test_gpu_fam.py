"""The FFT accumulation method on the GPU (k_fam, sp_fam, pyfft_amd.fam) against the float64 definition of tests/fam_ref.py on the float32
inputs: every shape within the allowance, the seam between passes, parts cut at block starts, bitwise repeatability, host arrays
against device tensors, offset pointers inside poisoned buffers, the diagonal against the Welch kernel, the cycle frequency of
amplitude-modulated noise, and the outputs that are not asked for."""
import numpy as np
import pytest
import torch            # a missing torch fails these tests, it does not skip them

import fam_ref as R
import guard_ref as G
from pyfft_amd import _ffi, engine as E, fam as F

pytestmark = pytest.mark.gpu

USED = {}          # test -> the largest share of the allowance the device used


def run(name, device=True, nblocks=None, x=None, y=None, **over):
    """engine.fam of a shape: (S, Pwx, Pwy) as numpy arrays"""
    s = R.SHAPES[name]
    xs, ys = R.signals(name)
    x = xs if x is None else x
    y = (ys if y is None else y) if s["cross"] else None
    a, g = R.windows(name)
    put = (lambda v: torch.as_tensor(np.array(v), device="cuda")) if device else np.array
    kw = dict(y=None if y is None else put(y), conj=s["conj"])
    kw.update(over)
    out = E.fam(put(x), a, s["hop"], g, s["nblocks"] if nblocks is None else nblocks, R.pairs_of(name), **kw)
    return tuple(o.cpu().numpy() if device and o is not None else o for o in out)


def note(key, share):
    USED[key] = share
    print("the device has used at most %.3f of the allowance %.2e so far (%d tests)" % (max(USED.values()), R.ALLOWANCE, len(USED)))


# cases 1 - 4: the smallest sizes with a tail of unused frames; the smallest tile; the largest transform; hop = np in the conjugate form
@pytest.mark.parametrize("name", ["np32-real-all", "np64-cplx-q1", "np64-p8192", "np256-hop-np-conj"])
def test_shapes_against_definition(name):
    s = R.SHAPES[name]
    got = run(name)
    Q = s["P"] * s["hop"] // (2 * s["np"])
    assert got[0].dtype == np.complex64 and got[1].dtype == np.float32 and got[0].shape == (R.pairs_of(name).shape[0], 2 * Q)
    assert got[1].shape == got[2].shape == (s["np"],) and np.array_equal(got[1], got[2])
    assert E.last_passes(E.FAM_PASSES) == 1
    note(name, R.assert_within(got, R.reference(name), R.pairs_of(name), name))


def test_pair_table_of_the_largest_transform_holds_what_it_should():
    pr, n = R.pairs_of("np64-p8192"), 64
    have = set(map(tuple, pr))
    assert pr.shape == (200, 2) and all((k, k) in have for k in range(n)) and (0, n - 1) in have and (n // 2, n // 2 - 1) in have
    assert all((5, l) in have for l in range(n)) and R.nsig_of(R.SHAPES["np64-p8192"]) == 131120
    s = R.SHAPES["np256-hop-np-conj"]
    assert s["P"] * s["hop"] // (2 * s["np"]) == s["P"] // 2 and R.pairs_of("np256-hop-np-conj").shape == (300, 2)
    s = R.SHAPES["np64-cplx-q1"]
    assert s["P"] * s["hop"] // (2 * s["np"]) == 1


# case 5
def test_cross_form_at_offset_pointers_inside_poisoned_buffers():
    name = "np128-cross"
    s = R.SHAPES[name]
    x, y = R.signals(name)
    a, g = R.windows(name)
    bx, vx = G.poisoned_input(torch.as_tensor(np.array(x), device="cuda"), 1)
    by, vy = G.poisoned_input(torch.as_tensor(np.array(y), device="cuda"), 3)
    assert vx.data_ptr() % 8 == 4 and vy.data_ptr() % 16 == 12
    snaps = G.snapshot(bx), G.snapshot(by)
    out = E.fam(vx, a, s["hop"], g, s["nblocks"], R.pairs_of(name), y=vy)
    got = tuple(o.cpu().numpy() for o in out)
    assert G.unchanged(bx, snaps[0]) and G.unchanged(by, snaps[1])
    assert not np.array_equal(got[1], got[2])
    note(name, R.assert_within(got, R.reference(name), R.pairs_of(name), name))


# case 6
def test_pass_seam(monkeypatch):
    name = "np32-seven-blocks"
    monkeypatch.delenv("SP_FAM_BLOCKS", raising=False)
    one = run(name)
    assert E.last_passes(E.FAM_PASSES) == 1
    monkeypatch.setenv("SP_FAM_BLOCKS", "3")
    assert E.fam_plan(32, 8, 32, 7, 1024)["passes"] == 3
    got = run(name)
    assert E.last_passes(E.FAM_PASSES) == 3
    note(name, R.assert_within(got, R.reference(name), R.pairs_of(name), name + " in 3 passes"))
    # the one-pass call as the reference of the three-pass call
    R.assert_within(got, tuple(o.astype(np.float64) if i else o.astype(np.complex128) for i, o in enumerate(one)), R.pairs_of(name),
                    name + ": 3 passes against 1")
    again = run(name)
    for p, q in zip(got, again):
        assert np.array_equal(p, q)


# case 7
def test_parts_cut_at_block_starts_add_up():
    name = "np32-real-all"
    s = R.SHAPES[name]
    x, _ = R.signals(name)
    m = R.CR.row_mean(x)
    step = s["P"] * s["hop"]
    whole = run(name, detrend=True, mean_value=float(m))
    parts = [run(name, nblocks=nb, x=x[b0 * step:], detrend=True, mean_value=float(m)) for b0, nb in ((0, 1), (1, 2))]
    total = tuple(parts[0][i].astype(np.complex128 if i == 0 else np.float64) + parts[1][i] for i in range(3))
    R.assert_within(total, tuple(o.astype(np.complex128 if i == 0 else np.float64) for i, o in enumerate(whole)), R.pairs_of(name),
                    name + ": parts against the whole")
    note(name + "-parts", R.assert_within(total, R.reference(name), R.pairs_of(name), name + ": parts against the definition"))


# case 8
@pytest.mark.parametrize("name", ["np32-real-all", "np128-cross"])
def test_calls_agree_bitwise(name):
    first, again, host = run(name), run(name), run(name, device=False)
    for p, q, h in zip(first, again, host):
        assert np.array_equal(p, q) and np.array_equal(p, h)


# case 9
def test_diagonal_at_q0_is_the_welch_estimate():
    name = "np32-real-all"
    s = R.SHAPES[name]
    x, _ = R.signals(name)
    n, P, hop, nb = s["np"], s["P"], s["hop"], s["nblocks"]
    a, _ = R.windows(name)
    diag = np.stack([np.arange(n), np.arange(n)], axis=1)
    nframes = nb * P
    scale = 1.0 / (float(np.sum(a.astype(np.float64) ** 2)) * nframes)
    xd = torch.as_tensor(np.array(x), device="cuda")
    S, Pwx, _ = E.fam(xd, a, hop, np.ones(P, dtype=np.float32), nb, diag, detrend=False, scale=scale)
    psd = E.welch_psd(xd[:(nframes - 1) * hop + n], a, hop, nframes, detrend=False, sided=E.SIDED_TWO, scale=scale * nframes)
    psd, S, Pwx = np.fft.ifftshift(psd.cpu().numpy().astype(np.float64)), S.cpu().numpy(), Pwx.cpu().numpy()      # centred -> fft order
    Q = P * hop // (2 * n)
    dev = max(float(np.max(np.abs(S[:, Q].real - psd))), float(np.max(np.abs(S[:, Q].imag))), float(np.max(np.abs(Pwx - psd)))) / psd.max()
    print("pair (k, k) at q = 0 against welch_psd: %.2e of the largest bin" % dev)
    assert dev <= 2e-4
    # scd_fam's scaling is scipy.signal.csd's: under a rectangular taper the diagonal's centre column is scipy's Welch PSD of the frames
    import scipy.signal as ss
    fs = 250.0
    used = np.array(x[:(nframes - 1) * hop + n])
    plane = F.scd_fam(used, fs, nchan=n, hop=hop, nblock=P, taper="boxcar", detrend=False)
    _, pxx = ss.welch(used.astype(np.float64), fs, window=a.astype(np.float64), nperseg=n, noverlap=n - hop, detrend=False, return_onesided=False)
    on = np.nonzero(plane.pairs[:, 0] == plane.pairs[:, 1])[0]
    assert list(plane.pairs[on, 0]) == list(range(n // 2)) and np.all(plane.alpha[on, Q] == 0) and np.allclose(plane.f[on], np.arange(n // 2) * fs / n)
    dev = float(np.max(np.abs(plane.S[on, Q] - pxx[:n // 2]))) / pxx.max()
    print("scd_fam's diagonal against scipy.signal.welch: %.2e of the largest bin" % dev)
    assert dev <= 2e-4 and plane.S.shape == (n * n // 4, 2 * Q)


# case 10
def test_profile_of_am_noise_peaks_at_the_modulation_rate():
    """np 64, hop 16, P 256, 4 blocks.  The channelizer window is R.AM_GPU's: under the default Hamming window of 64 taps the cell of
    NU_AM, 0.37 of a channel spacing from the centre of its tile, loses 12 % of |gamma|^2 to the window's own response, and the mean
    |gamma|^2 is 0.295 in the float64 reference: outside 0.367 +- 0.05 by the estimator's bias, not by the kernel (tests/fam_ref.py)."""
    s = R.AM_GPU
    x = R.am_record(True)
    plane = F.scd_fam(torch.as_tensor(np.array(x), device="cuda"), nchan=s["np"], hop=s["hop"], nblock=s["P"], window=s["window"])
    assert torch.is_tensor(plane.S) and plane.S.shape == (s["np"] ** 2 // 4, s["P"] * s["hop"] // s["np"]) and plane.Pw.shape == (2, s["np"])
    assert plane.dalpha == 1.0 / (s["P"] * s["hop"])
    alphas, prof = F.fam_profile(plane)
    assert torch.is_tensor(prof) and prof.dtype == torch.float64
    peak = R.assert_am_profile(alphas, prof.cpu().numpy(), s)
    # the same plane from host arrays, reduced on the host
    host = F.scd_fam(np.array(x), nchan=s["np"], hop=s["hop"], nblock=s["P"], window=s["window"])
    assert np.array_equal(host.S, plane.S.cpu().numpy()) and np.array_equal(host.alpha, plane.alpha)
    ah, ph = F.fam_profile(host)
    assert np.array_equal(ah, alphas) and np.allclose(ph, prof.cpu().numpy(), rtol=1e-12, atol=0)
    assert abs(R.assert_am_profile(ah, ph, s) - peak) < 1e-12
    # the default Hamming window finds the same bin (the first condition), with the biased level
    ham = F.scd_fam(np.array(x), nchan=s["np"], hop=s["hop"], nblock=s["P"])
    ahm, phm = F.fam_profile(ham)
    sel = (ahm > 0) & (ahm < 0.5)
    at = ahm[sel][np.argmax(phm[sel])]
    print("under the default Hamming window: peak at %.6f, mean |gamma|^2 %.3f" % (at, phm[sel].max()))
    assert abs(at - round(R.NU_AM / ham.dalpha) * ham.dalpha) < 1e-9


# case 11
def test_outputs_not_asked_for_and_no_blocks():
    name = "np32-real-all"
    full = run(name)
    only_s, only_pw = run(name, Pw=False), run(name, S=False)
    assert only_s[1] is None and only_s[2] is None and np.array_equal(only_s[0], full[0])
    assert only_pw[0] is None and np.array_equal(only_pw[1], full[1]) and np.array_equal(only_pw[2], full[2])
    host_s, host_pw = run(name, device=False, Pw=False), run(name, device=False, S=False)           # the same through the staged host path
    assert host_s[1] is None and np.array_equal(host_s[0], full[0]) and host_pw[0] is None and np.array_equal(host_pw[1], full[1])
    # nblocks = 0 through the C entry: sentinel-filled device outputs stay as they are
    s = R.SHAPES[name]
    x, _ = R.signals(name)
    a, g = R.windows(name)
    pairs = np.ascontiguousarray(R.pairs_of(name))
    xd = torch.as_tensor(np.array(x), device="cuda")
    bases = [G.sentinel_output(n, dt, 1, device="cuda") for n, dt in ((pairs.shape[0] * 8, torch.complex64), (32, torch.float32), (32, torch.float32))]
    snaps = [G.snapshot(b) for b, _ in bases]
    E._bind_stream(xd)
    rc = _ffi.lib().sp_fam(_ffi.ptr(xd.data_ptr()), None, 0, xd.numel(), _ffi.ptr(a), 32, s["hop"], _ffi.ptr(g), 32, 0, _ffi.ptr(pairs),
                           pairs.shape[0], 0, None, None, 1.0, *(_ffi.ptr(addr) for _, addr in bases), 1)
    torch.cuda.synchronize()
    assert rc == 0 and all(G.unchanged(b, sn) for (b, _), sn in zip(bases, snaps))
