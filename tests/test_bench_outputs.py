"""bench.py as a measuring instrument: --steps sets the number of timed steps, the JSON line carries ms_per_step, and
--dump-outputs DIR writes what the timed path returned for its last step (DIR/pxx.npy), so that two builds can be compared
output for output on the same seeded stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def test_bench_rejects_zero_steps():
    """no timed step, no ms_per_step: refused at argument parsing, before anything touches a GPU"""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], env=_env(), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_timed_psd(tmp_path):
    """the dumped array is the PSD of the seeded stream (float64, nfft bins, two-sided) and agrees with the CPU oracle"""
    import synth
    from oracle import cpu_ref as O
    log2n, nfft, hop, steps = 20, 4096, 2048, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--settle-steps", "0",
                        "--log2n", str(log2n), "--cpu-log2n", "0", "--dump-outputs", str(out)],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and "error" not in d
    assert d["dump_outputs"] == {"pxx": [nfft]}
    assert sorted(os.listdir(out)) == ["pxx.npy"]
    got = np.load(out / "pxx.npy")
    assert got.dtype == np.float64 and got.shape == (nfft,)
    n = 1 << log2n
    win = O.windows("Hanning", nwins=nfft)
    ref = O.welch_psd_stream(synth.stream_numpy(0, n), win, nfft, hop, (n - nfft) // hop + 1, 1.0)
    assert float(np.max(np.abs(got - ref) / (2e-4 * np.abs(ref) + 1e-6 * ref.max()))) <= 1.0
