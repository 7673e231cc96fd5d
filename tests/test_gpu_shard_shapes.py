"""Sharded / split Welch PSD (sp_welch_export / _apply / _accum / _finish / _dist_*) at segment lengths and hops other than the
power-of-two nfft with hop = nfft/4, nfft/2 or nfft: the generic one-pass kernel (k_welch_opx) against the reference fixtures,
the float64 oracle and the single-GPU sp_welch_psd."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E():
    from pyfft_amd import engine
    from pyfft_amd import _ffi
    _ffi.init()
    return engine


def _shards(x, nfft, hop, M, cuts):
    """frames [a, b) of x for consecutive cuts: (samples read, own samples); the reads reach the next shard's first sample
    when hop > nfft, so that a shard holds every sample it owns"""
    nsig = x.shape[0]
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b < M:
            xs = x[a * hop: max((b - 1) * hop + nfft, b * hop)]
            own = (b - a) * hop
        else:
            xs = x[a * hop:]
            own = nsig - a * hop
        out.append((xs, own))
    return out


def test_reference_parity_through_shards(E):
    """SFT3F flat-top at its recommended overlap (nwins 2981, hop 992, real): 1, 2 and 3 shards of the reference record,
    exported (one of them from a device tensor), summed and applied == the reference Pxx"""
    import torch
    from pyfft_amd.dist import shard_plan
    g = load_golden("welch_class_real_SFT3F")
    x = np.asarray(g["x"], dtype=np.float32)
    nfft, nov, M = int(g["nwins"]), int(g["noverlap"]), int(g["Navr"])
    hop = nfft - nov
    win = O.windows("SFT3F", nwins=nfft)
    S2 = np.sum(win ** 2)
    ref = g["Pxx"].real
    for world in (1, 2, 3):
        states = []
        for r in range(world):
            p = shard_plan(x.size, nfft, hop, world, r)
            assert p.frames_total == M
            xl = x[p.first_sample: p.first_sample + p.nsamples]
            if r == world - 1 and world > 1:
                st = E.welch_export(torch.from_numpy(xl).cuda(), win, hop, p.frames, nmean=p.own_samples).cpu().numpy()
            else:
                st = E.welch_export(xl, win, hop, p.frames, nmean=p.own_samples)
            assert st.shape == (5 * nfft + 8,)
            states.append(st)
        tot = np.sum(states, axis=0)
        assert tot[5 * nfft + 5] == M and tot[5 * nfft + 6] == x.size
        P = E.welch_apply(tot, win, M, sided=E.SIDED_ONE, scale=1.0 / (float(g["Fs"]) * S2))
        np.testing.assert_allclose(P, ref, rtol=2e-4, atol=1e-6 * ref.max())


GRID = [(4096, 1351), (2048, 675), (8192, 2731), (3640, 1820), (1023, 511), (1001, 250), (30, 7), (512, 100), (256, 300),
        (1024, 1)]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("nfft,hop", GRID)
def test_shape_grid_three_shards(E, nfft, hop, cplx):
    """three unequal shards with different means and a DC offset 30x the noise: the summed states applied == the float64
    oracle and == sp_welch_psd of the whole stream, two-sided, one-sided and raw"""
    import torch
    rng = np.random.default_rng(nfft * 7 + hop)
    M = 61 if hop > 16 else 301
    nsig = (M - 1) * hop + nfft + hop // 3
    M = (nsig - nfft) // hop + 1
    noise = rng.standard_normal(nsig) + (1j * rng.standard_normal(nsig) if cplx else 0)
    x = (noise + ((30.0 - 11.0j) if cplx else 30.0)).astype(np.complex64 if cplx else np.float32)
    x[: nsig // 3] += 2.0
    x[-nsig // 5:] -= (1.0j if cplx else 1.0)
    win = O.windows("Hanning", nwins=nfft)
    cuts = [0, M // 4, M // 4 + M // 3, M]
    states = []
    for k, (xs, own) in enumerate(_shards(x, nfft, hop, M, cuts)):
        frames = cuts[k + 1] - cuts[k]
        if k == 1:
            st = E.welch_export(torch.from_numpy(xs).cuda(), win, hop, frames, nmean=own).cpu().numpy()
        else:
            st = E.welch_export(xs, win, hop, frames, nmean=own)
        states.append(st)
    tot = np.sum(states, axis=0)
    assert tot[5 * nfft + 5] == M and tot[5 * nfft + 6] == nsig
    oref = O.welch_psd_stream(x.astype(np.complex128 if cplx else np.float64), win, nfft, hop, M, 1.0) * np.sum(win ** 2) * 3.0
    for sided in (E.SIDED_TWO, E.SIDED_ONE, E.SIDED_RAW):
        p = E.welch_apply(tot, win, M, sided=sided, scale=3.0)
        one = E.welch_psd(x, win, hop, M, detrend=True, sided=sided, scale=3.0)
        np.testing.assert_allclose(p, one, rtol=2e-4, atol=2e-6 * one.max())
        if sided == E.SIDED_TWO:
            np.testing.assert_allclose(p, oref, rtol=2e-4, atol=2e-6 * oref.max())


def test_split_abi_global_mean(E):
    """welch_accum / welch_finish on a generic shape: two shards finished with the GLOBAL mean add up to the PSD of the
    whole stream; the returned own-sample sums are numpy's"""
    rng = np.random.default_rng(17)
    nfft, hop = 2048, 675
    nsig = nfft + hop * 150 + 77
    x = (rng.standard_normal(nsig) + 1j * rng.standard_normal(nsig) + (1.5 - 0.7j)).astype(np.complex64)
    x[: nsig // 2] += 2.0
    M = (nsig - nfft) // hop + 1
    win = O.windows("Hanning", nwins=nfft)
    ref = O.welch_psd_stream(x.astype(np.complex128), win, nfft, hop, M, 1.0) * np.sum(win ** 2)
    Ma = M // 2
    xa, xb = x[: (Ma - 1) * hop + nfft], x[Ma * hop:]
    own_a, own_b = Ma * hop, nsig - Ma * hop
    sa = E.welch_accum(xa, win, hop, Ma, nmean=own_a)
    np.testing.assert_allclose(sa[0] + 1j * sa[1], x[:own_a].astype(np.complex128).sum(), rtol=1e-6)
    sb_direct = x[Ma * hop:].astype(np.complex128).sum()
    gm = (sa[0] + 1j * sa[1] + sb_direct) / nsig
    pa = E.welch_finish(nfft, np.array([gm.real, gm.imag]), M, sided=E.SIDED_TWO, scale=1.0)
    sb = E.welch_accum(xb, win, hop, M - Ma, nmean=own_b)
    np.testing.assert_allclose(sb[0] + 1j * sb[1], sb_direct, rtol=1e-6)
    pb = E.welch_finish(nfft, np.array([gm.real, gm.imag]), M, sided=E.SIDED_TWO, scale=1.0)
    np.testing.assert_allclose(pa + pb, ref, rtol=2e-4, atol=1e-6 * ref.max())
    # finished with the shard's own mean: the PSD of that shard alone
    E.welch_accum(xb, win, hop, M - Ma, nmean=xb.size)
    pself = E.welch_finish(nfft, None, M - Ma, sided=E.SIDED_TWO, scale=1.0)
    rb = O.welch_psd_stream(xb.astype(np.complex128), win, nfft, hop, M - Ma, 1.0) * np.sum(win ** 2)
    np.testing.assert_allclose(pself, rb, rtol=2e-4, atol=1e-6 * rb.max())


@pytest.mark.parametrize("nfft,hop,cplx", [(4096, 1351, True), (2981, 992, False)])
def test_native_pipeline_generic_shape(E, nfft, hop, cplx):
    """the streaming engine without a communicator, two steps in flight on the two scratch sets: 5 submits with different data
    per step, every reported PSD == that step's welch_psd_sharded"""
    import torch
    from pyfft_amd.dist import shard_plan, welch_psd_sharded, NativeWelchPipeline
    total = nfft + hop * 3000 + 123
    plan = shard_plan(total, nfft, hop, 1, 0)
    win = O.windows("Blackman-Harris", nwins=nfft)
    gen = torch.Generator(device="cuda").manual_seed(5)
    xs = []
    for k in range(5):
        if cplx:
            z = torch.randn(total, 2, device="cuda", generator=gen) + torch.tensor([0.5 * k, -0.3 * k], device="cuda")
            xs.append(torch.view_as_complex(z.contiguous()))
        else:
            xs.append(torch.randn(total, device="cuda", generator=gen) * (1.0 + k) + 2.0 * k)
    pipe = NativeWelchPipeline(win, plan, scale=1.0, sided=E.SIDED_ONE)
    got = [r for r in (pipe.submit(x) for x in xs) if r is not None] + pipe.flush_all()
    assert len(got) == 5
    for x, g in zip(xs, got):
        one = welch_psd_sharded(x, win, plan, scale=1.0, sided=E.SIDED_ONE)
        torch.testing.assert_close(g, one, rtol=1e-6, atol=1e-9 * float(one.max()))


def test_rccl_world1_generic_shapes():
    """the same streaming engine with a communicator of one rank (the all-reduce between export and apply), in a child
    process whose first GPU call is the RCCL process group"""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_world1_shapes.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["backend"] == "nccl" and d["native_comm"] == [1, 0]
    assert d["steps"] == [5, 5]
    assert d["vs_sharded"] <= 1.0            # units of rtol 1e-6 |ref| + 1e-9 max
    assert d["vs_oracle"] <= 1.0             # units of rtol 2e-4 |ref| + 1e-6 max


def _gloo_worker(rank, world, port, total, nfft, hop, out_dir):
    import torch
    import torch.distributed as dist
    from pyfft_amd.dist import shard_plan, welch_psd_sharded
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    stream = _gloo_stream(total)
    plan = shard_plan(total, nfft, hop, world, rank)
    x_local = torch.from_numpy(stream[plan.first_sample: plan.first_sample + plan.nsamples]).cuda()
    win = O.windows("Blackman-Harris", nwins=nfft)
    p = welch_psd_sharded(x_local, win, plan, scale=1.0, sided=1)
    assert p.is_cuda
    np.save(os.path.join(out_dir, "p%d.npy" % rank), p.cpu().numpy())
    dist.destroy_process_group()


def _gloo_stream(total):
    rng = np.random.default_rng(78)
    x = (rng.standard_normal(total) + 0.8).astype(np.float32)
    x[: total // 2] += 1.5
    return x


def test_two_ranks_one_gpu_generic_shape(tmp_path):
    """two processes on the one GPU (gloo) at nwins 2981, hop 992 with a Blackman-Harris window: every rank holds the
    single-process PSD of the whole stream"""
    import torch.multiprocessing as mp
    world, nfft, hop = 2, 2981, 992
    total = nfft + hop * 600 + 311
    port = 31100 + os.getpid() % 300
    mp.spawn(_gloo_worker, args=(world, port, total, nfft, hop, str(tmp_path)), nprocs=world, join=True)
    x = _gloo_stream(total).astype(np.float64)
    win = O.windows("Blackman-Harris", nwins=nfft)
    M = (total - nfft) // hop + 1
    ref2 = O.welch_psd_stream(x, win, nfft, hop, M, 1.0) * np.sum(win ** 2)
    ref = np.fft.ifftshift(ref2)[: (nfft + 1) // 2].copy()
    ref[1:] *= 2.0
    for r in range(world):
        p = np.load(os.path.join(str(tmp_path), "p%d.npy" % r))
        np.testing.assert_allclose(p, ref, rtol=2e-4, atol=1e-6 * ref.max())


def test_full_size_four_shards(E):
    """2^26 complex64 samples at (4096, 1351) in 4 shards of device tensors against the float64 oracle"""
    import torch
    from pyfft_amd.dist import shard_plan
    nfft, hop, total = 4096, 1351, 1 << 26
    rng = np.random.default_rng(2026)
    x = (rng.standard_normal(total, dtype=np.float32) + 1j * rng.standard_normal(total, dtype=np.float32)).astype(np.complex64)
    x += np.complex64(0.7 - 0.2j)
    x[: total // 3] += np.complex64(0.5)
    win = O.windows("Hanning", nwins=nfft)
    states = []
    for r in range(4):
        p = shard_plan(total, nfft, hop, 4, r)
        xl = torch.from_numpy(x[p.first_sample: p.first_sample + p.nsamples]).cuda()
        states.append(E.welch_export(xl, win, hop, p.frames, nmean=p.own_samples).cpu().numpy())
    tot = np.sum(states, axis=0)
    M = p.frames_total
    got = E.welch_apply(tot, win, M, sided=E.SIDED_TWO, scale=1.0)
    ref = O.welch_psd_stream(x.astype(np.complex128), win, nfft, hop, M, 1.0) * np.sum(win ** 2)
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-6 * ref.max())


def test_dispatch_names_the_kernel(E):
    """generic shapes run k_welch_opx; the shapes of the carry / pipeline kernels keep them"""
    rng = np.random.default_rng(3)
    for nfft, hop, generic in ((2048, 675, True), (3640, 1820, True), (4096, 2048, False), (1024, 256, False)):
        nsig = nfft + hop * 40
        x = (rng.standard_normal(nsig) + 1j * rng.standard_normal(nsig)).astype(np.complex64)
        win = O.windows("Hanning", nwins=nfft)
        E.welch_export(x, win, hop, (nsig - nfft) // hop + 1)
        name = E.profile_last_kernel()
        if generic:
            assert name.startswith("k_welch_opx"), (nfft, hop, name)
        else:
            assert name.startswith("k_welch_carry") or name.startswith("k_welch_pipe"), (nfft, hop, name)
