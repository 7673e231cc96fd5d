"""The call-history instrument on the CPU (tests/history_ref.py): the case table is complete against the engine's public names, its
predecessors change sample values and nothing else, the triples the GPU module runs are counted, and the driver catches the defects
it is for: a numpy stand-in "library" with one shared scratch goes through run_histories correct and with three planted defects."""
import inspect

import numpy as np
import pytest

import history_ref as H
from pyfft_amd import engine as E

IDS = [c.id for c in H.CASES]


def public_callables():
    return sorted(n for n, v in vars(E).items()
                  if not n.startswith("_") and callable(v) and not inspect.isclass(v) and not inspect.ismodule(v))


# ---------------------------------------------------------------------------------------------------------------- the table
def test_every_public_entry_is_a_case_or_excluded():
    """a family added to the engine later cannot skip the history tests silently"""
    pub = set(public_callables())
    covered = set(e for c in H.CASES for e in H.entries_of(c))
    assert covered <= pub, sorted(covered - pub)
    assert set(H.EXCLUDED) <= pub, sorted(set(H.EXCLUDED) - pub)
    assert not covered & set(H.EXCLUDED), sorted(covered & set(H.EXCLUDED))
    assert not H.PENDING, "cases still to be written: %s" % sorted(H.PENDING)
    missing = pub - covered - set(H.EXCLUDED)
    assert not missing, "public entries of pyfft_amd.engine without a history case or a reason in EXCLUDED: %s" % sorted(missing)
    assert all(isinstance(r, str) and r and "\n" not in r for r in H.EXCLUDED.values())


HELD_ELSEWHERE = ("welch_accum", "welch_finish", "welch_dist_submit", "welch_dist_flush")       # the module's two tests of lasting state


def test_no_excluded_entry_takes_samples_to_the_device():
    """a sentence in EXCLUDED is not enough: the source of an excluded entry must not enter the library with data (no calling mode, no
    stream binding, no md.call), unless another test of tests/test_gpu_call_history.py holds it"""
    for name, reason in H.EXCLUDED.items():
        fn = getattr(E, name)
        if not hasattr(fn, "__code__"):
            continue
        src = inspect.getsource(fn)
        enters = [k for k in ("md.call", "_enter(", "_mode(", "_bind_stream", "md.init") if k in src]
        if name in HELD_ELSEWHERE:
            assert "held by test_" in reason, name
        else:
            assert not enters, "%s is excluded (%r) but its source has %s" % (name, reason, enters)


def test_the_table_holds_what_the_contract_names():
    import guard_ref as G
    assert len(set(IDS)) == len(IDS)
    fam = [c.family for c in H.CASES]
    assert set(c.family for c in G.INPUT_CASES) <= set(fam) and len(set(c.family for c in G.INPUT_CASES)) == 23
    for name in H.GUARD_LONG:
        assert name in H.BY_ID
    assert sorted(c.arrays[0].shape[-1] for c in H.CASES if c.family == "fft") == [8, 1000, 10000, 16384, 1 << 20]
    assert [c.id for c in H.CASES if c.family == "welch_psd"][1:] == ["welch_psd-c64-long-16384x8192", "welch_psd-c64-pipe-4096x2048"]
    for f in ("istft_frames", "pfb_synth", "zoom_welch", "cwt", "icwt_sum", "wct_time", "ssq", "ssq_bands", "wvd", "cyclic", "lomb",
              "lomb_sums", "lomb_sums_grid", "nufft1", "nufft2", "wbic", "fam", "burg", "yule", "ar_psd", "covmat", "ar_ls",
              "pseudospectrum", "beamscan", "dwt", "idwt", "modwt", "imodwt", "eigh", "welch_export"):
        assert f in fam, f
    # the medley's host-array call stages at least twice the largest case
    largest = max(sum(a.nbytes for a in c.arrays) for c in H.CASES)
    assert H.MEDLEY_STAGED_BYTES >= 2 * largest, (H.MEDLEY_STAGED_BYTES, largest)
    assert H.MEDLEY_SPEC[0][4] and sum(int(np.prod(s)) * np.dtype(dt).itemsize for s, dt in H.MEDLEY_SPEC[0][3]) == H.MEDLEY_STAGED_BYTES


@pytest.mark.parametrize("case", H.CASES, ids=IDS)
def test_predecessors_change_the_samples_alone(case):
    for a in case.arrays:
        assert np.all(np.isfinite(a)), "a case's own samples are finite"
    for fill in H.FILLS:
        big, same = H.predecessors(case, fill)
        assert same.run is case.run                      # every argument that is no sample array: the case's own closure, bit for bit
        assert len(same.arrays) == len(case.arrays) == len(big.arrays)
        for a, p, b in zip(case.arrays, same.arrays, big.arrays):
            assert p.dtype == a.dtype == b.dtype and p.shape == a.shape, (case.id, fill)
            assert b.size >= 2 * a.size or case.family in ("beamscan",), (case.id, b.shape, a.shape)     # (beamscan doubles the wavenumbers)
            for v in (p, b):
                parts = (v.real, v.imag) if v.dtype.kind == "c" else (v,)
                for q in parts:
                    if fill == "nan":
                        assert np.all(np.isnan(q))
                    elif fill == "loud":
                        assert np.all(np.abs(q) >= 2.0 ** 50) and np.all(np.isfinite(q.astype(np.float32) ** 2 if q.dtype.itemsize <= 4 else q))
                    else:
                        assert np.all(np.isfinite(q)) and 0.5 < float(np.std(q)) < 2.0 or q.size < 16
            assert not np.array_equal(p, a) or fill == "quiet" and a.size == 0
        assert (same.expect is not None) == (fill == "nan" and case.refusal is not None)
        assert same.expect is None or H.FINITE in same.expect[1] or case.family == "eigh"


def test_the_triples_are_the_full_product():
    """every (case, history, memory): 4 histories x 2 memories, the medley on another stream for device memory, and `refused` in
    both memories for the families that have a refusal"""
    t = H.triples()
    n = len(H.CASES)
    refusing = [c for c in H.CASES if "refused" in H.histories_of(c)]
    assert sorted(c.family for c in refusing) == sorted(["eigh", "welch_psd", "nufft1", "nufft2", "lomb", "lomb_sums", "lomb_sums_grid",
                                                         "burg", "yule", "covmat", "ar_ls", "cyclic", "fam"])
    # refused for host arrays alone, before the library is entered: no refusal after a launch, so no `refused` history
    assert sorted(c.family for c in H.CASES if c.refusal is not None and len(c.refusal) == 3) == ["ar_psd", "beamscan", "pseudospectrum"]
    assert len(t) == len(set(t)) == n * (4 * 2 + 1) + 2 * len(refusing)
    assert n == 66 and len(t) == 620
    # what the GPU module runs, read from the parametrisation of its two tests
    import test_gpu_call_history as T

    def params(fn, name):
        return [m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == name][0]

    ran = set()
    for c in params(T.test_result_ignores_history, "case"):
        for memory in params(T.test_result_ignores_history, "memory"):
            ran |= {(c.id, h, memory) for h in H.histories_of(c) if h != "quiet2"}
    ran |= {(c.id, "stream", "device") for c in params(T.test_history_on_another_stream, "case")}
    assert ran == set(t) and len(ran) == len(t)


@pytest.mark.parametrize("case", H.CASES, ids=IDS)
def test_references_are_finite_where_the_check_demands_it(case):
    """every case names its float64 reference (the guard table's are shared with tests/test_host_guard_ref.py); it is finite wherever
    the family's check demands finite results (a bispectrum is NaN outside its valid region by definition)"""
    assert case.ref is not None, case.id
    leaves = H.leaves(case.ref())
    assert leaves and all(a.size for a in leaves), case.id
    if case.finite:
        assert H.all_finite(leaves), case.id
    else:
        assert case.family in ("bispectrum", "wbic") and any(np.all(np.isfinite(a)) for a in leaves)


# ---------------------------------------------------------------------------------------------------------------- the stand-in
class Refused(ValueError):
    pass


class StandIn(object):
    """A numpy 'library' with the engine's habits: one scratch array that only grows and is never cleared, rows staged into it and
    padded to a multiple of 8, an accumulator that lives across calls.  `defect` plants one of the three mistakes."""

    def __init__(self, defect=None):
        self.defect = defect
        self.scratch = np.zeros(0, dtype=np.float32)
        self.acc = np.zeros(1, dtype=np.float64)

    def _stage(self, x):
        x = np.asarray(x, dtype=np.float32).ravel()
        n = x.size
        npad = (n + 8) // 8 * 8                              # at least one element of padding
        if self.scratch.size < npad:
            grown = np.zeros(2 * npad, dtype=np.float32)    # a fresh allocation is zero
            grown[:self.scratch.size] = self.scratch
            self.scratch = grown
        self.scratch[:n] = x                                 # the padding keeps what the last call left there
        return n, npad

    def wsum(self, x, w):
        """sum_i w[i] x[i]"""
        n, npad = self._stage(x)
        wp = np.zeros(npad, dtype=np.float32)
        wp[:n] = w
        m = n + 1 if self.defect == "zero-weight" else n     # one element past what it wrote, times a zero weight
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float32(np.sum(self.scratch[:m].astype(np.float64) * wp[:m]))

    def peak(self, x):
        """max_i x[i]"""
        n, npad = self._stage(x)
        m = npad if self.defect == "padded-max" else n       # a max over the padded row
        return np.float32(np.fmax.reduce(self.scratch[:m]))  # (fmax swallows a NaN, as fmaxf does)

    def total(self, x):
        """sum_i x[i] in an accumulator the call zeroes when it is done; a record that is not finite is refused after the 'kernel' ran"""
        n, _ = self._stage(x)
        with np.errstate(invalid="ignore", over="ignore"):
            self.acc[0] += np.sum(self.scratch[:n].astype(np.float64))
        if not np.isfinite(self.scratch[:n]).all():          # the status flag, read back after the launch
            if self.defect != "stale-accumulator":
                self.acc[0] = 0.0
            raise Refused("total: x holds a value that is not finite")
        out = np.float64(self.acc[0])
        self.acc[0] = 0.0
        return out


def standin_cases(lib):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(37).astype(np.float32)
    w = rng.standard_normal(37).astype(np.float32)
    x.setflags(write=False)
    ref_w, ref_p, ref_t = float(np.sum(x.astype(np.float64) * w)), float(x.max()), float(np.sum(x.astype(np.float64)))

    def near(want):
        def accept(got, what):
            assert abs(float(got) - want) <= 1e-5 * max(1.0, abs(want)), (what, float(got), want)
        return accept

    def tile(v, k):
        return np.tile(np.asarray(v), k)

    a = H.HCase("standin-wsum", "wsum", [x], lambda v: lib.wsum(v[0], w), near(ref_w), lambda: ([(74,)], lambda v: lib.wsum(v[0], tile(w, 2))))
    b = H.HCase("standin-peak", "peak", [x], lambda v: lib.peak(v[0]), near(ref_p), lambda: ([(74,)], lambda v: lib.peak(v[0])))
    c = H.HCase("standin-total", "total", [x], lambda v: lib.total(v[0]), near(ref_t), lambda: ([(74,)], lambda v: lib.total(v[0])),
                refusal=((Refused,), "finite"))
    return a, b, c


def standin_medley(lib):
    """the stand-in's other routine over the shared scratch, with both fills, longer than any case"""
    calls = []
    for fill in ("nan", "loud"):
        calls.append(H.Call(lambda v: lib.peak(v[0]), (H.filled((80,), np.float32, fill, 5),), "other", None))
    return calls


def failing(defect):
    lib = StandIn(defect)
    out = {}
    for case in standin_cases(lib):
        res = H.run_histories(lambda run, arrays, memory: run(arrays), case, "host", medley_calls=standin_medley(lib))
        assert list(res) == H.histories_of(case)
        out[case.family] = sorted(h for h, bad in H.verdicts(case, res).items() if bad)
    return out


def test_the_driver_passes_a_correct_library():
    assert failing(None) == {"wsum": [], "peak": [], "total": []}


def test_the_driver_catches_a_zero_weight_on_a_stale_element_with_the_nan_fill():
    f = failing("zero-weight")
    assert "nan" in f["wsum"] and "loud" not in f["wsum"] and "quiet" not in f["wsum"], f       # NaN x 0 is NaN; 2^60 x 0 is 0
    assert f["peak"] == [] and f["total"] == []


def test_the_driver_catches_a_max_over_a_padded_row_with_the_loud_fill():
    f = failing("padded-max")
    assert "loud" in f["peak"] and "nan" not in f["peak"] and "quiet" not in f["peak"], f       # fmax swallows the NaN, not 2^60
    assert f["wsum"] == [] and f["total"] == []


def test_the_driver_catches_an_accumulator_left_after_a_refused_call():
    f = failing("stale-accumulator")
    assert "refused" in f["total"] and "quiet" not in f["total"] and "loud" not in f["total"], f
    assert f["wsum"] == [] and f["peak"] == []


def test_a_call_that_must_refuse_and_returns_is_reported():
    lib = StandIn()
    case = standin_cases(lib)[1]
    case.refusal = ((Refused,), "finite")                   # peak refuses nothing
    with pytest.raises(H.NotRefused):
        H.run_histories(lambda run, arrays, memory: run(arrays), case, "host", medley_calls=[])
