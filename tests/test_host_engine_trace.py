"""pyfft_amd.engine assembles the same calls of the C ABI as the engine the golden trace was recorded from: every argument of every
sp_* call, the place of _ffi.init() and of the stream binding among them, what comes back (kind, dtype, shape, contiguity) and every
refusal (type and message), in both calling modes.  tests/engine_trace.py holds the stand-in library and the case table.  No GPU."""
import json
import os

import pytest

import engine_trace as T
from pyfft_amd import _ffi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_trace.json")

# declared entries no case of the table reaches, each for a stated reason
NOT_TRACED = {
    # life cycle, errors, stream, profiling, information: not array entry points (init and the stream binding are recorded as events)
    "sp_init", "sp_shutdown", "sp_last_error", "sp_set_stream", "sp_synchronize", "sp_device_info", "sp_profile_enable",
    "sp_profile_last_ms", "sp_profile_last_kernel",
    # the library's own communicator and the streamed / distributed Welch step: device only, their Python text is not shared
    "sp_comm_unique_id", "sp_comm_init", "sp_comm_info", "sp_comm_destroy", "sp_welch_dist_submit", "sp_welch_dist_flush",
    "sp_welch_psd_dist",
    # host arithmetic, answered by the built library under the stand-in
    *T.HOST_ARITHMETIC,
    # a host table of chirp phases for the tests; no engine function calls it
    "sp_czt_chirp",
}


@pytest.fixture(scope="module")
def golden_trace():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed():
    assert os.path.exists(_ffi.LIB_PATH), "the library is not built"
    mp = pytest.MonkeyPatch()
    try:
        return json.loads(json.dumps(T.run_table(mp)))          # tuples -> lists, as the golden file holds them
    finally:
        mp.undo()


def test_replay_equals_golden(golden_trace, replayed):
    want = golden_trace["cases"]
    assert len(golden_trace["engine_sha256"]) == 64
    assert sorted(replayed) == sorted(want)
    bad = [k for k in want if replayed[k] != want[k]]
    for k in bad[:5]:
        print("%s\n  golden   %s\n  replayed %s" % (k, json.dumps(want[k], sort_keys=True), json.dumps(replayed[k], sort_keys=True)))
    assert not bad, "%d of %d cases differ from the golden trace: %s" % (len(bad), len(want), bad[:20])


def test_every_abi_entry_has_a_case(replayed):
    seen = {ev[0] for kept in replayed.values() for ev in kept["events"] if ev[0].startswith("sp_")}
    assert len(T.TRACED_TABLES) == 9 and T.TRACED_TABLES[:6] == _ffi.TABLES
    assert NOT_TRACED <= set(T.DECLARED) and len(T.DECLARED) == sum(len(table) for table in T.TRACED_TABLES) == 91
    assert seen == set(T.DECLARED) - NOT_TRACED


def test_every_function_in_both_modes(replayed):
    assert len(T.FUNCTIONS) == 53 and {c[1] for c in T.CASES} == set(T.FUNCTIONS)
    for fn in T.FUNCTIONS:
        for mode in T.MODES:
            calls = [kept for k, kept in replayed.items() if k.startswith(fn + "/") and k.endswith("/" + mode)]
            assert any("returned" in kept and any(ev[0].startswith("sp_") for ev in kept["events"]) for kept in calls), (fn, mode)
