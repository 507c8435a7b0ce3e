"""CPU checks of the IIR filter's host side: the reference's known answers
through the literal restatement, the call accounting, the plan tables, the
error bound's reach, and the exported symbols. No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import dsp_ref
import iir_ref

F32 = np.float32


def feed(a, b, samples):
    """The reference's test Feeder (iir.rs:186-203): one new sample per
    call, the unconsumed tail presented again, one output slot."""
    mem, pending, got = None, [], []
    for s in samples:
        pending.append(s)
        y, cons, prod, _, mem = iir_ref.serial(a, b, pending, 1, F32, mem)
        assert cons == prod
        del pending[:cons]
        got.append(float(y[0]) if prod else None)
    return got


def test_reference_known_answers():
    y, cons, prod, st, _ = iir_ref.serial([1, 2, 3], [4, 5, 6],
                                          [1, 2, 3, 4, 5], 1, F32)
    assert (y.tolist(), cons, prod) == ([42.0], 1, 1)     # iir.rs:26-31
    assert st == iir_ref.INSUFFICIENT_OUTPUT
    assert feed([], [1, 2, 3], [10, 20, 30, 40]) == \
        [None, None, 100.0, 160.0]                          # iir.rs:218-226
    assert feed([0.5], [1], [10, 10, 10, 10]) == \
        [None, 15.0, 17.5, 18.75]                           # iir.rs:228-236


def test_count_matches_reference_on_grid(fsdr):
    n = 0
    for n_a in range(9):
        for n_b in (1, 2, 5, 64):
            for filled in range(n_a + 1):
                for n_in in range(n_a + n_b + 4):
                    for n_out in (0, 1, 5, 1000):
                        got = fsdr.iir_count(n_a, n_b, filled, n_in, n_out)
                        assert got == iir_ref.count(n_a, n_b, filled, n_in,
                                                    n_out), \
                            (n_a, n_b, filled, n_in, n_out)
                        n += 1
    assert n > 10000


@pytest.mark.parametrize("n_a,n_b", [(3, 2), (8, 1), (1, 64)])
def test_count_fill_split_over_calls(fsdr, n_a, n_b):
    # input grows by one sample per call; the fill continues where the
    # last call left it. A call that completes a fill begun earlier made
    # fewer pushes than it has inputs, so it goes on to produce (:119).
    filled_c = filled_r = 0
    for n_in in range(n_a + n_b + 3):
        got = fsdr.iir_count(n_a, n_b, filled_c, n_in, 5)
        want = iir_ref.count(n_a, n_b, filled_r, n_in, 5)
        assert got == want
        filled_c, filled_r = got[0], want[0]
        assert filled_c == min(n_in, n_a)
        if n_in < n_a:
            assert got[1:3] == (0, 0)
    assert got[1] == min(n_in - (n_b - 1), 5)


@functools.lru_cache(maxsize=None)
def _plan(fsdr, name):
    a = (iir_ref.FILTERS.get(name) or iir_ref.EXACT[name])[0]
    p = fsdr.IirPlan(a)
    return p.info(), p.tables()


@functools.lru_cache(maxsize=None)
def _case(fsdr, name):
    """Input, float64 serial reference and bound sum at 2*tile + L + 1."""
    a, b = iir_ref.FILTERS[name]
    (L, _, tile, _), _ = _plan(fsdr, name)
    n = 2 * tile + L + 1
    x = dsp_ref.loud_f32(dsp_ref._rng(0x11B, ord(name)), n + b.size - 1)
    y = iir_ref.serial(a, b, x, n, np.float64)[0]
    assert y.size == n
    return x, y, iir_ref.bound_sum(a, b, x, y)


@pytest.mark.parametrize("name", ["B", "Q", "O"])
def test_tables_reproduce_the_serial_filter(fsdr, name):
    a, b = iir_ref.FILTERS[name]
    info, tables = _plan(fsdr, name)
    x, y, _ = _case(fsdr, name)
    got = iir_ref.blocked(a, b, x, y.size, x[:a.size], tables, info)
    rel = np.abs(got - y).max() / np.abs(y).max()
    # the same with the entries as the kernels read them, for the record
    t32 = tuple(t.astype(F32) for t in tables)
    rel32 = np.abs(iir_ref.blocked(a, b, x, y.size, x[:a.size], t32, info)
                   - y).max() / np.abs(y).max()
    print(f"iir tables {name}: rel err {rel:.2e} (f32 entries {rel32:.2e})")
    assert rel <= 1e-9
    assert rel32 <= 64 * iir_ref.U


def test_plan_info_is_consistent(fsdr):
    (L, chunks, tile, per_pass), (H, pc, pt) = _plan(fsdr, "O")
    assert tile == L * chunks and L >= 8
    assert chunks & (chunks - 1) == 0 and per_pass & (per_pass - 1) == 0
    assert H.shape == (L, 8)
    assert pc.shape == (chunks.bit_length() - 1, 8, 8)
    assert pt.shape == (per_pass.bit_length() - 1, 8, 8)
    a = iir_ref.FILTERS["O"][0].astype(np.float64)
    A = np.zeros((8, 8))
    A[0] = a
    A[np.arange(1, 8), np.arange(7)] = 1.0
    np.testing.assert_allclose(H[0], a, rtol=0, atol=0)
    np.testing.assert_allclose(pc[0], np.linalg.matrix_power(A, L),
                               rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(pt[0], pc[-1] @ pc[-1], rtol=1e-10,
                               atol=1e-300)


@pytest.mark.parametrize("name", sorted(iir_ref.EXACT))
def test_exact_filters_have_unit_tables(fsdr, name):
    _, tables = _plan(fsdr, name)
    for t in tables:
        assert t.size and np.isin(t, (-1.0, 0.0, 1.0)).all()


def test_empty_feedback_has_empty_tables(fsdr):
    p = fsdr.IirPlan([])
    assert [t.size for t in p.tables()] == [0, 0, 0]


@pytest.mark.parametrize("a", [[1.01], [2.0, -1.01]])
def test_unstable_feedback_is_refused(fsdr, a):
    with pytest.raises(fsdr.FsdrError) as e:
        fsdr.IirPlan(a)
    assert e.value.code == fsdr.ERR_UNSUPPORTED


def test_unit_circle_poles_are_accepted(fsdr):
    for a in ([1.0], [-1.0], [0.0, 1.0], [2.0, -1.0]):
        fsdr.IirPlan(a)


def test_out_of_range_taps_are_invalid(fsdr):
    with pytest.raises(fsdr.FsdrError) as e:
        fsdr.IirPlan([0.1] * 9)
    assert e.value.code == fsdr.ERR_INVALID
    # the handle's own range checks come before it looks for a device
    lib = fsdr.lib()
    one = (ctypes.c_float * 65)(*([0.5] * 65))
    for n_a, n_b in ((9, 1), (1, 0), (1, 65)):
        assert not lib.fsdr_iir_f32_create(one, n_a, one, n_b)
        assert b"iir" in lib.fsdr_last_error()


@pytest.mark.parametrize("fault", ["drop", "hrow", "swap"])
@pytest.mark.parametrize("name", ["B", "Q", "O"])
def test_bound_catches_planted_faults(fsdr, name, fault):
    a, b = iir_ref.FILTERS[name]
    info, tables = _plan(fsdr, name)
    x, y, bsum = _case(fsdr, name)
    lim = iir_ref.gamma(128) * bsum
    clean = iir_ref.blocked(a, b, x, y.size, x[:a.size], tables, info)
    assert (np.abs(clean - y) <= lim).all()
    bad = iir_ref.blocked(a, b, x, y.size, x[:a.size], tables, info,
                          fault=fault)
    assert (np.abs(bad - y) > lim).any()


@pytest.mark.parametrize("name", sorted(iir_ref.FILTERS))
def test_serial_f32_within_its_bound(name):
    a, b = iir_ref.FILTERS[name]
    x = dsp_ref.loud_f32(dsp_ref._rng(0x11C, ord(name)), 600 + b.size - 1)
    y = iir_ref.serial(a, b, x, 600, np.float64)[0]
    y32 = iir_ref.serial(a, b, x, 600, F32)[0]
    lim = iir_ref.bound(a, b, x, y, a.size + b.size)
    assert (np.abs(y32 - y) <= lim).all()


@pytest.mark.parametrize("name", sorted(iir_ref.FILTERS))
def test_bound_condition_for_the_gpu_cases(fsdr, name):
    """Every (filter, length) the GPU test runs: c <= 128, and the bound at
    c = 128 is at most 2^-9 of the largest output, so a wrong sample or
    state cannot hide under it."""
    a, b = iir_ref.FILTERS[name]
    info = fsdr.IirPlan(a).info()
    x, y, bsum = iir_ref.value_stream(name, info)
    for n in iir_ref.value_counts(a.size, info) + [iir_ref.stream_len(info)]:
        n = min(n, y.size)
        assert iir_ref.kernel_c(a.size, b.size, n, info) <= 128
        worst = iir_ref.gamma(128) * bsum[:n].max()
        assert worst <= 2.0 ** -9 * np.abs(y[:n]).max(), (name, n)


def test_exact_closed_forms_match_the_serial_loop():
    for name, (a, b) in iir_ref.EXACT.items():
        x = iir_ref.exact_input(300, 3)
        y = iir_ref.serial(a, b, x, 1000, F32)[0]
        want = iir_ref.exact_closed_form(name, x)
        assert y.size == want.size == 300 - (b.size - 1)
        assert (y.astype(np.float64) == want).all(), name


def test_new_header_symbols_exported(fsdr):
    lib = fsdr.lib()
    for s in ("fsdr_iir_plan_create", "fsdr_iir_plan_destroy",
              "fsdr_iir_plan_info", "fsdr_iir_plan_tables", "fsdr_iir_count",
              "fsdr_iir_f32_create", "fsdr_iir_plan_of",
              "fsdr_fg_add_vector_source_f32"):
        assert s in fsdr.exported_symbols() and hasattr(lib, s)
