"""A call's result is a function of its arguments alone: every public entry of pyfft_amd.engine after histories that leave the shared
scratch of libspectral (tests/history_ref.py) full of other shapes, NaN and 2^60.

test_result_ignores_history runs every case of the table, from host arrays (staged) and from device tensors, after the histories
quiet (twice), nan, loud, medley and, where the family has a refusal, refused.  After each the result must be finite where the
family's own check demands it, accepted by the family's own acceptance function against its float64 reference, and bit-identical to
the quiet baseline.  The predecessors' own outputs are discarded: an older family given NaN samples must simply return, a family that
refuses non-finite records must refuse in its documented words.  Each acceptance prints the worst error as a fraction of the family's
tolerance ("<case> after <history> [<memory>]: ... of the tolerance").

test_history_on_another_stream enqueues the medley on one torch stream without synchronisation and makes the case's call at once on
a second one: the only test of sp_set_stream's event for the families outside the streaming engine.

TOLERANCE_ONLY lists the families whose two quiet runs already differ, each with the line that makes its order vary; bits are not
demanded of them, acceptance and finiteness are.  It is empty: at the shapes of this table every family repeats its bits, the two
outputs tests/test_gpu_loop_seams.py names included: pseg of sp_stft varies on long segments only (k_long_pack in
pyfft_amd/csrc/k_long.hip adds one float64 atomic per workgroup, several workgroups a frame), which the 256-point stft_frames case
does not reach, and sp_csd_matrix differs between chunkings, not between two runs of one chunking.  A family is added here only with
such a pointer, and only when `quiet` and `quiet2` differ.

test_pending_accumulate_survives_other_families and test_streamed_step_ignores_its_neighbours hold the two pieces of state that
outlive a call: the pending sp_welch_accum and the streaming engine's slots."""
import time

import numpy as np
import pytest

import history_ref as H
from pyfft_amd import _ffi, engine as E
from pyfft_amd._ffi import SpectralError

pytestmark = pytest.mark.gpu

IDS = [c.id for c in H.CASES]
TOLERANCE_ONLY = ()


@pytest.fixture(scope="module")
def torch():
    import torch
    _ffi.init()
    return torch


def host(v):
    if isinstance(v, dict):
        return {k: host(u) for k, u in v.items()}
    if isinstance(v, (tuple, list)):
        return tuple(host(u) for u in v)
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def on_device(torch, arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]            # (the shared arrays are read-only: copied first)


def caller(torch):
    def call(run, arrays, memory):
        if memory == "host":
            return host(run(list(arrays)))
        out = host(run(on_device(torch, arrays)))
        torch.cuda.synchronize()
        return out
    return call


def judge(case, results, memory):
    labelled = H.HCase(case.id, case.family, case.arrays, case.run, lambda got, what: case.accept(got, "%s [%s]" % (what, memory)),
                       case.grown, case.finite, case.refusal, case.also)
    bad = {h: why for h, why in H.verdicts(labelled, results, bitwise=case.family not in TOLERANCE_ONLY).items() if why}
    assert not bad, "%s [%s]: %s" % (case.id, memory, bad)


@pytest.mark.parametrize("memory", H.MEMORIES)
@pytest.mark.parametrize("case", H.CASES, ids=IDS)
def test_result_ignores_history(torch, case, memory):
    t0 = time.time()
    results = H.run_histories(caller(torch), case, memory)
    assert list(results) == H.histories_of(case)
    if case.family in TOLERANCE_ONLY:
        print("%s [%s]: the two quiet runs %s" % (case.id, memory, "agree" if H.same_bits(results["quiet"], results["quiet2"]) else "differ"))
    judge(case, results, memory)
    print("%s [%s]: %.2f s" % (case.id, memory, time.time() - t0))


@pytest.mark.parametrize("case", H.CASES, ids=IDS)
def test_history_on_another_stream(torch, case):
    t0 = time.time()
    call = caller(torch)
    for c in H.history_calls(case, "quiet"):
        H.run_call(call, c, "device")
    base = call(case.run, case.arrays, "device")
    calls = [c for c in H.medley(host_entry=False) if c.family != case.family]      # (a host-array call synchronises by its nature)
    placed = [on_device(torch, c.arrays) for c in calls]
    mine = on_device(torch, case.arrays)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    keep = []
    with torch.cuda.stream(s1):
        for c, v in zip(calls, placed):
            keep.append(c.run(v))                           # enqueued, never waited for
    with torch.cuda.stream(s2):
        got = case.run(mine)
    s2.synchronize()
    got = host(got)
    torch.cuda.synchronize()
    del keep
    judge(case, {"quiet": base, "stream": got}, "device")
    print("%s [stream]: %.2f s" % (case.id, time.time() - t0))


# ======================================================================================================================================
# the pending accumulate
# ======================================================================================================================================
PENDING_SHAPES = {"pipeline": (4096, 2048, None), "one-workgroup": (1024, 512, 64), "generic": (1000, 339, 40)}


def pipe_frames(torch):
    """a frame count the nfft-4096 pipeline kernel takes by itself: welch_pipe_wanted (pyfft_amd/csrc/spectral.hip) asks for
    2 frames per CU less 2; 88 more (600 on the 256 CUs of an MI355X), and the callers assert the kernel's name"""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count + 88
SAME, GONE = "the uninterrupted bits", "no pending sp_welch_accum"


def _one_pass_psd(v):
    return E.welch_psd(v[0], H.G.hann(1024), 512, 9, detrend=True, sided=E.SIDED_TWO, scale=1.0)


def _mean(v):
    return E.mean(v[0])


def intervening():
    """(name, Call): every medley call, then welch_psd at a one-pass shape, stft_cog, mean, xcorr_normalised, fft, csd_matrix on
    unit noise"""
    out = [("medley %s %s" % (spec[0], fill), c) for fill, block in (("nan", H.medley(("nan",))), ("loud", H.medley(("loud",))))
           for spec, c in zip(H.MEDLEY_SPEC, block)]
    q = lambda shape, dt, k: (H.filled(shape, dt, "quiet", H.PRED_SEED + 900 + k),)          # noqa: E731
    out += [("welch_psd one-pass", H.Call(_one_pass_psd, q((1024 + 8 * 512,), np.complex64, 0), "welch_psd", None)),
            ("stft_cog", H.Call(H._m_cog, q((256 + 60 * 64 + 5,), np.float32, 1), "stft_cog", None)),
            ("mean", H.Call(_mean, q((4099,), np.float32, 2), "mean", None)),
            ("xcorr_normalised", H.Call(H._m_xcorr, q((777,), np.float32, 3) + q((777,), np.float32, 4), "xcorr_normalised", None)),
            ("fft", H.Call(H._m_fft, q((3, 1000), np.complex64, 5), "fft", None)),
            ("csd_matrix", H.Call(H._m_csdm, q((3, 256 + 39 * 128 + 7), np.float32, 6), "csd_matrix", None))]
    return out


# What sp_welch_finish does after each intervening call of THIS test, for every shape and both memories, written out: a call added to
# intervening() must be pinned here by hand.  Of these calls only the complex welch_psd with a whole-record mean at a power-of-two
# segment runs the one-pass path itself, which replaces the pending state (sp_welch_finish then refuses).  Other entries clear the
# pending state too and are not among these calls: a real welch_psd at hop = nfft / 2 that takes the one-pass branch, welch_export
# and welch_dist_submit.
OUTCOME = {
    "medley staged-xcorr nan": SAME, "medley welch-mean nan": SAME, "medley cog nan": SAME, "medley fft-10000 nan": SAME,
    "medley fft-2^20 nan": SAME, "medley welch-long nan": SAME, "medley csd-matrix nan": SAME,
    "medley staged-xcorr loud": SAME, "medley welch-mean loud": SAME, "medley cog loud": SAME, "medley fft-10000 loud": SAME,
    "medley fft-2^20 loud": SAME, "medley welch-long loud": SAME, "medley csd-matrix loud": SAME,
    "welch_psd one-pass": GONE, "stft_cog": SAME, "mean": SAME, "xcorr_normalised": SAME, "fft": SAME, "csd_matrix": SAME,
}
assert sorted(OUTCOME) == sorted(name for name, _ in intervening())


@pytest.mark.parametrize("memory", H.MEMORIES)
@pytest.mark.parametrize("shape", sorted(PENDING_SHAPES))
def test_pending_accumulate_survives_other_families(torch, shape, memory):
    nfft, hop, M = PENDING_SHAPES[shape]
    M = pipe_frames(torch) if M is None else M
    n = (M - 1) * hop + nfft + 5
    x = H.G.noise(n, True, 6000 + nfft, 0.4)
    win = H.G.hann(nfft)
    call = caller(torch)
    xs = x if memory == "host" else on_device(torch, [x])[0]
    mean = np.array([x.real.astype(np.float64).mean(), x.imag.astype(np.float64).mean()])
    mean = mean if memory == "host" else torch.from_numpy(mean).cuda()

    def finish():
        return host(E.welch_finish(nfft, mean, M, sided=E.SIDED_TWO, scale=1.0, like=xs))

    E.welch_accum(xs, win, hop, M)
    if shape == "pipeline":
        assert E.profile_last_kernel().startswith("k_welch_pipe"), E.profile_last_kernel()
    base = finish()
    from oracle import cpu_ref as O
    ref = O.welch_psd_stream(x, win, nfft, hop, M, 1.0, detrend_style=1) * np.sum(win ** 2)
    assert float(np.max(np.abs(base - ref) / (2e-4 * np.abs(ref) + 1e-6 * ref.max()))) <= 1.0          # tests/test_gpu_pipe.py's bound
    with pytest.raises(SpectralError, match=GONE):
        finish()                                                                                         # a finish consumes the state
    seen = {}
    for name, c in intervening():
        E.welch_accum(xs, win, hop, M)
        H.run_call(call, c, memory)
        try:
            got = finish()
        except SpectralError as e:
            assert GONE in str(e), (name, str(e))
            seen[name] = GONE
        else:
            assert H.same_bits(got, base), "%s: sp_welch_finish returned another spectrum after %s" % (shape, name)
            seen[name] = SAME
    assert seen == OUTCOME, {k: (v, OUTCOME[k]) for k, v in seen.items() if v != OUTCOME[k]}


# ======================================================================================================================================
# the streaming engine
# ======================================================================================================================================
@pytest.mark.parametrize("nfft,hop,M", [(4096, 2048, None), (1024, 512, 64)], ids=["pipeline", "1024x512x64"])
def test_streamed_step_ignores_its_neighbours(torch, nfft, hop, M):
    """steps A, nan, B, loud, C: A, B and C carry the bits of the same run with the two bad steps replaced by quiet records, and are
    within tests/test_gpu_stream.py's tolerance of the oracle"""
    from oracle import cpu_ref as O
    from pyfft_amd.dist import NativeWelchPipeline, shard_plan
    pipeline = M is None
    M = pipe_frames(torch) if pipeline else M
    total = (M - 1) * hop + nfft + 11
    win = O.windows("Hanning", nwins=nfft)
    plan = shard_plan(total, nfft, hop, 1, 0)
    assert plan.frames == M
    good = [H.G.noise(total, True, 7000 + nfft + k, 0.5 + 0.25 * k) for k in range(3)]
    fills = {f: H.filled((total,), np.complex64, f, H.PRED_SEED + 700 + i) for i, f in enumerate(("quiet", "nan", "loud"))}

    def run(bad1, bad2):
        pipe = NativeWelchPipeline(win, plan, scale=1.0, sided=E.SIDED_TWO)
        xs = on_device(torch, [good[0], fills[bad1], good[1], fills[bad2], good[2]])
        got = []
        for x in xs:
            r = pipe.submit(x)
            if pipeline:
                assert E.profile_last_kernel().startswith("k_welch_pipe"), E.profile_last_kernel()
            if r is not None:
                got.append(r)
        got += pipe.flush_all()
        assert len(got) == 5 and pipe.flush() is None
        torch.cuda.synchronize()
        return [g.cpu().numpy() for g in got]

    want = run("quiet", "quiet")
    got = run("nan", "loud")
    for k, name in ((0, "A"), (2, "B"), (4, "C")):
        ref = O.welch_psd_stream(good[k // 2], win, nfft, hop, M, 1.0, detrend_style=1) * np.sum(win ** 2)
        r = float(np.max(np.abs(got[k] - ref) / (2e-4 * np.abs(ref) + 1e-6 * ref.max())))               # test_gpu_stream.py: _excess
        print("step %s nfft %d: %.3g of the tolerance" % (name, nfft, r))
        assert np.all(np.isfinite(got[k])) and r <= 1.0, (name, r)
        assert H.same_bits(got[k], want[k]), "step %s differs from the run whose neighbours were quiet" % name
