"""tests/guard_ref.py on the CPU: the instrument fails when it should, shown with numpy stand-ins for a kernel (y = 2 x, rows of n
samples), and every case of the table of tests/test_gpu_offset_pointers.py has a float64 reference that is finite and not trivial."""
import numpy as np
import pytest

import guard_ref as G

DTYPES = [np.float32, np.complex64, np.float64]
IDS = ["f32", "c64", "f64"]


def sample(n, dtype, rows=None):
    shape = (n,) if rows is None else (rows, n)
    x = np.arange(1, 1 + int(np.prod(shape)), dtype=np.float64).reshape(shape)
    return (x - 0.5j * x).astype(dtype) if np.dtype(dtype).kind == "c" else x.astype(dtype)


def checks(base, lead, n, **kw):
    return G.guards_intact(base, lead, n, **kw), G.all_written(base, lead, n, **kw), bool(np.all(np.isfinite(G.interior_of(base, lead, n, **kw))))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_correct_stand_in_passes(dtype, lead):
    n = 37
    xb, x = G.poisoned_input(sample(n, dtype), lead)
    assert x.ctypes.data % 16 == (lead * x.itemsize) % 16 and x.flags["C_CONTIGUOUS"]
    assert np.array_equal(x, sample(n, dtype))
    assert np.isnan(xb[:G.GUARD + lead].real).all() and np.isnan(xb[G.GUARD + lead + n:].real).all()
    assert xb.size == 2 * G.GUARD + lead + n
    if np.iscomplexobj(xb):
        assert np.isnan(xb[:G.GUARD + lead].imag).all() and np.isnan(xb[G.GUARD + lead + n:].imag).all()
    yb, y = G.sentinel_output(n, dtype, lead)
    assert y.ctypes.data % 16 == (lead * y.itemsize) % 16 and y.shape == (n,) and yb.size == 2 * G.GUARD + lead + n
    assert np.all(yb.view(np.uint32) == G.SENTINEL) and np.isnan(yb.real).all()
    if np.iscomplexobj(yb):
        assert np.isnan(yb.imag).all()
    assert not G.all_written(yb, lead, n) and G.first_unwritten(yb, lead, n) == 0 and G.guards_intact(yb, lead, n)
    y[:] = 2 * x
    assert checks(yb, lead, n) == (True, True, True)
    assert np.array_equal(y, 2 * sample(n, dtype))


def test_the_sentinel_is_a_non_canonical_nan():
    word = np.array([G.SENTINEL], dtype=np.uint32)
    assert np.isnan(word.view(np.float32)[0]) and G.SENTINEL not in (0x7FC00000, 0xFFC00000)
    assert np.isnan(np.array([G.SENTINEL, G.SENTINEL], dtype=np.uint32).view(np.float64)[0])
    assert np.array([np.nan], dtype=np.float32).view(np.uint32)[0] != G.SENTINEL          # a NaN a kernel computes is another word


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lead", [0, 1, 3])
def test_a_store_outside_the_interior_is_found(dtype, lead):
    n = 37
    x = sample(n, dtype)
    for where, index in ((-1, -1), (n, n), (-G.GUARD - lead, -G.GUARD - lead), (n + G.GUARD - 1, n + G.GUARD - 1)):
        yb, y = G.sentinel_output(n, dtype, lead)
        y[:] = 2 * x
        yb[G.GUARD + lead + where] = 1.0                            # the stand-in's stray store
        with pytest.raises(G.GuardDamaged) as e:
            G.guards_intact(yb, lead, n)
        assert e.value.index == index and str(index) in str(e.value)
        assert G.all_written(yb, lead, n)
    # a stray store of the value the guard already shows as a float (NaN) but in other bits: integers tell them apart
    yb, y = G.sentinel_output(n, dtype, lead)
    y[:] = 2 * x
    yb[G.GUARD + lead + n] = np.nan
    with pytest.raises(G.GuardDamaged) as e:
        G.guards_intact(yb, lead, n)
    assert e.value.index == n
    # two stray stores: the first one is reported
    yb[G.GUARD + lead - 2] = 0.0
    with pytest.raises(G.GuardDamaged) as e:
        G.guards_intact(yb, lead, n)
    assert e.value.index == -2


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
def test_a_store_into_a_row_gap_is_found(dtype):
    rows, n, pitch, lead = 3, 37, 40, 1
    x = sample(n, dtype, rows)
    yb, y = G.sentinel_output(n, dtype, lead, rows=rows, pitch=pitch)
    assert y.shape == (rows, n) and y.strides == (pitch * y.itemsize, y.itemsize)
    y[...] = 2 * x
    assert checks(yb, lead, n, rows=rows, pitch=pitch) == (True, True, True)
    yb[G.GUARD + lead + pitch + n] = 1.0                              # row 1 runs one element past its end
    with pytest.raises(G.GuardDamaged) as e:
        G.guards_intact(yb, lead, n, rows=rows, pitch=pitch)
    assert e.value.index == pitch + n
    assert G.all_written(yb, lead, n, rows=rows, pitch=pitch)
    # dense rows have no gap: the same store lands in the next row, and only the tail guard can tell
    yb, y = G.sentinel_output(n, dtype, lead, rows=rows)
    y[...] = 2 * x
    yb[G.GUARD + lead + rows * n] = 1.0
    with pytest.raises(G.GuardDamaged) as e:
        G.guards_intact(yb, lead, n, rows=rows)
    assert e.value.index == rows * n


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_skipped_store_is_found(dtype):
    n, lead = 37, 2
    x = sample(n, dtype)
    yb, y = G.sentinel_output(n, dtype, lead)
    y[:n - 1] = 2 * x[:n - 1]                                         # the stand-in forgets the last element
    assert G.guards_intact(yb, lead, n)
    assert not G.all_written(yb, lead, n) and G.first_unwritten(yb, lead, n) == n - 1
    if np.dtype(dtype).kind == "c":
        yb, y = G.sentinel_output(n, dtype, lead)
        y[:] = 2 * x
        y.view(np.float32)[2 * 5 + 1] = np.array([G.SENTINEL], dtype=np.uint32).view(np.float32)[0]      # one imaginary part left out
        assert not G.all_written(yb, lead, n) and G.first_unwritten(yb, lead, n) == 5


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
@pytest.mark.parametrize("lead", [0, 1])
def test_a_load_outside_the_samples_is_found(dtype, lead):
    """A stand-in that averages each sample with its right (or left) neighbour and forgets that the last (first) has none."""
    rows, n, pitch = 2, 37, 40
    for kw in (dict(), dict(pitch=pitch)):
        xb, x = G.poisoned_input(sample(n, dtype, rows), lead, **kw)
        ld = pitch if kw else n
        start = G.GUARD + lead
        for shift in (1, -1):
            yb, y = G.sentinel_output(n, dtype, lead, rows=rows)
            for r in range(rows):
                row = xb[start + r * ld + shift:start + r * ld + shift + n]      # x[r][shift : shift + n]: one element outside
                y[r] = 0.5 * (x[r] + row)
            assert G.guards_intact(yb, lead, n, rows=rows) and G.all_written(yb, lead, n, rows=rows)
            bad = ~np.isfinite(y)
            edge = n - 1 if shift == 1 else 0
            # the last row always reads a guard; with a pitch every row reads its gap; dense rows read their neighbour and stay finite
            assert bad[rows - 1 if shift == 1 else 0, edge] and bad.sum() == (rows if kw else 1)
        # the correct stand-in on the same views
        yb, y = G.sentinel_output(n, dtype, lead, rows=rows)
        y[...] = 2 * x
        assert checks(yb, lead, n, rows=rows) == (True, True, True)


def test_poisoned_input_geometry():
    a = sample(10, np.float32, 3)
    base, view = G.poisoned_input(a, 3)
    assert view.shape == (3, 10) and view.flags["C_CONTIGUOUS"] and view.ctypes.data - base.ctypes.data == 4 * (G.GUARD + 3)
    assert base.size == 2 * G.GUARD + 3 + 30 and np.isnan(base).sum() == base.size - 30
    base, view = G.poisoned_input(a, 1, pitch=13)
    assert view.strides == (52, 4) and np.array_equal(view, a)
    assert base.size == 2 * G.GUARD + 1 + 2 * 13 + 10 and np.isnan(base).sum() == base.size - 30
    assert np.isnan(base[G.GUARD + 1 + 10:G.GUARD + 1 + 13]).all()
    z = sample(5, np.complex64)
    base, view = G.poisoned_input(z, 1)
    assert view.ctypes.data % 16 == 8 and np.isnan(base.real).sum() == np.isnan(base.imag).sum() == base.size - 5
    with pytest.raises(AssertionError):
        G.poisoned_input(a, 0, pitch=10)                              # a pitch must leave a gap


def test_torch_tensors_are_handled_alike():
    import torch
    for dt, a in ((torch.float32, sample(9, np.float32, 2)), (torch.complex64, sample(9, np.complex64, 2))):
        for kw in (dict(), dict(pitch=12)):
            base, view = G.poisoned_input(torch.as_tensor(a), 1, **kw)
            assert view.dtype == dt and np.array_equal(view.numpy(), a) and view.data_ptr() % 16 == base.element_size() % 16
            assert view.is_contiguous() == (not kw)
            if not kw:
                assert view.contiguous().data_ptr() == view.data_ptr()      # what engine.py's .contiguous() hands through
            assert int(torch.isnan(torch.view_as_real(base) if base.is_complex() else base).sum()) == (base.numel() - 18) * (2 if base.is_complex() else 1)
        yb, ptr = G.sentinel_output(18, dt, 1, device="cpu")
        assert ptr == yb.data_ptr() + (G.GUARD + 1) * yb.element_size()
        assert not G.all_written(yb, 1, 18) and G.guards_intact(yb, 1, 18)
        G.interior_of(yb, 1, 18).copy_(torch.as_tensor(a).reshape(-1))
        assert G.all_written(yb, 1, 18) and G.guards_intact(yb, 1, 18)
        yb[G.GUARD] = 0.0
        with pytest.raises(G.GuardDamaged) as e:
            G.guards_intact(yb, 1, 18)
        assert e.value.index == -1


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_every_entry():
    fam = {c.family for c in G.INPUT_CASES}
    assert fam == {"mean", "biquad_filter", "sos_filter", "sosfiltfilt", "upfirdn", "ddc", "fir_filter", "hilbert_rows", "spectral_filter_rows",
                   "xcorr_normalised", "welch_psd", "stft_frames", "stft_cog", "frame_sum", "welch_csd", "csd_matrix", "pfb", "czt",
                   "xcorr_frames", "welch_blocks", "multitaper", "bispectrum", "skf"}
    by = {}
    for c in G.INPUT_CASES:
        by.setdefault((c.family, c.cplx), []).append(c)
        for run in c.places:
            assert len(run) == len(G.inputs(c)["arrays"]), c.id
            for lead, extra in run:
                assert lead in (G.C64_LEADS if c.cplx else G.F32_LEADS) and extra in (0, G.ROW_PITCH), c.id
    every = lambda c: {run[0][0] for run in c.places}                 # noqa: E731
    assert sorted(c.p["n"] for c in by["mean", False]) == [1, 2, 3, 5, 4099] and sorted(c.p["n"] for c in by["mean", True]) == [1, 4099]
    assert sorted({c.p["n"] for c in by["biquad_filter", False]}) == [5, 8192, 2 * 8192 + 5]
    for f in ("mean", "biquad_filter", "sos_filter", "sosfiltfilt", "fir_filter", "hilbert_rows", "spectral_filter_rows", "welch_psd",
              "stft_frames", "stft_cog", "frame_sum", "welch_csd", "csd_matrix"):
        for c in by[f, False]:
            assert every(c) == {0, 1, 2, 3}, c.id
        for c in by.get((f, True), []):
            assert every(c) == {0, 1}, c.id
    for f in ("welch_psd", "stft_frames", "stft_cog", "frame_sum", "welch_csd", "upfirdn", "ddc", "pfb", "czt"):
        assert (f, True) in by and (f, False) in by
    for f in ("upfirdn", "ddc", "pfb", "czt"):                        # the engine passes strided rows through: pitch n + 3 at lead 1
        for cplx in (False, True):
            assert any(run[0] == (1, G.ROW_PITCH) for c in by[f, cplx] for run in c.places), f
    for c in by["xcorr_normalised", False]:
        assert c.places[0] == ((1, 0), (3, 0))
    # two tiles and a ragged end
    for c in by["upfirdn", False] + by["upfirdn", True]:
        n, K = G.upfirdn_n(c)
        nout = -(-((n - 1) * c.p["up"] + c.p["T"]) // c.p["down"])
        assert nout > 2 * K and nout % K, c.id
    for c in by["ddc", False] + by["ddc", True]:
        n, K = G.ddc_n(c)
        assert -(-n // c.p["q"]) > 2 * K and -(-n // c.p["q"]) % K, c.id


@pytest.mark.parametrize("case", G.INPUT_CASES, ids=[c.id for c in G.INPUT_CASES])
def test_reference_is_finite_and_not_trivial(case):
    d = G.inputs(case)
    for a in d["arrays"]:
        assert np.all(np.isfinite(a)) and a.dtype == (np.complex64 if case.cplx else np.float32)
    for leaf in G.leaves(G.reference(case)):
        assert leaf.size > 0 and np.all(np.isfinite(leaf)) and float(np.max(np.abs(leaf))) > 0, case.id
