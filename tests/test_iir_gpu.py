"""The IIR filter on the GPU against tests/iir_ref.py: counts and status
equal to the reference's accounting, values inside the derived bound of a
float64 serial reference (exact filters: bit-equal to a closed form), under
every split of a stream into calls. Sizes come from the handle's plan.
FSDR_FIR_GRID_CAP=1 makes one block walk every tile, 3 gives blocks an
uneven share."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

import iir_ref

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(params=[None, "1", "3"], ids=["cap-", "cap1", "cap3"])
def grid_cap(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("FSDR_FIR_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("FSDR_FIR_GRID_CAP", request.param)
    return request.param


@pytest.fixture(params=[None, "1"], ids=["cap-", "cap1"])
def grid_cap2(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("FSDR_FIR_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("FSDR_FIR_GRID_CAP", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _info(gpu):
    return gpu.Iir([0.5], [1.0]).plan.info()


@functools.lru_cache(maxsize=None)
def _value_stream(gpu, name):
    x, y, bsum = iir_ref.value_stream(name, _info(gpu))
    for v in (x, y, bsum):
        v.setflags(write=False)
    return x, y, bsum


def _check_call(got, want_counts, y_ref, lim):
    """One call's result against the reference; returns worst err/bound."""
    y, cons, prod, st = got
    assert (cons, prod, st) == want_counts
    assert y.dtype == F32 and y.size == prod
    err = np.abs(y.astype(np.float64) - y_ref[:prod])
    assert (err <= lim[:prod]).all(), \
        f"worst err/bound {np.max(err / lim[:prod]):.3g}"
    return float(np.max(err / lim[:prod]))


# ---- 1. values and counts ---------------------------------------------------

@pytest.mark.parametrize("name", sorted(iir_ref.FILTERS))
def test_values_and_counts(gpu, name, grid_cap):
    a, b = iir_ref.FILTERS[name]
    info = _info(gpu)
    assert gpu.Iir(a, b).plan.info() == info
    x, y_ref, bsum = _value_stream(gpu, name)
    na, nb = a.size, b.size
    worst = 0.0
    for n in iir_ref.value_counts(na, info):
        lim = iir_ref.gamma(iir_ref.kernel_c(na, nb, n, info)) * bsum
        # output-limited: all the input, n slots
        want = iir_ref.count(na, nb, 0, x.size, n)[1:]
        assert want[:2] == (n, n)
        worst = max(worst, _check_call(gpu.Iir(a, b).filter(x, n), want,
                                       y_ref, lim))
        # input-limited: the inputs of n outputs, room to spare
        n_in = n + nb - 1
        if n_in > na:
            want = iir_ref.count(na, nb, 0, n_in, n + 5)[1:]
            assert want[:2] == (n, n)
            worst = max(worst, _check_call(
                gpu.Iir(a, b).filter(x[:n_in], n + 5), want, y_ref, lim))
    print(f"iir {name} cap={grid_cap}: worst err/bound {worst:.3f}")
    assert worst > 0


# ---- 2. exact at scale ------------------------------------------------------

@pytest.mark.parametrize("name", sorted(iir_ref.EXACT))
def test_exact_at_scale(gpu, name, grid_cap2):
    a, b = iir_ref.EXACT[name]
    L, _, tile, per_pass = _info(gpu)
    n = (per_pass + 1) * tile + L + 1   # the tile scan's second pass runs
    rest = tile + 3
    x = iir_ref.exact_input(n + rest + b.size - 1, ord(name))
    want = iir_ref.exact_closed_form(name, x)
    assert want.size == n + rest
    f = gpu.Iir(a, b)
    y, cons, prod, st = f.filter(x, n)
    assert (cons, prod, st) == (n, n, iir_ref.INSUFFICIENT_OUTPUT)
    assert np.array_equal(y.astype(np.float64), want[:n])
    # the memory the next call sees
    y2, cons, prod, _ = f.filter(x[n:], rest + 9)
    assert (cons, prod) == (rest, rest)
    assert np.array_equal(y2.astype(np.float64), want[n:])


# ---- 3. streaming -----------------------------------------------------------

def _stream(f, x, chunk):
    """Feed x in `chunk`-sample pieces, the unconsumed tail presented again.
    Returns (outputs, consumed, produced, largest produced of one call)."""
    pending = np.zeros(0, F32)
    outs, cons_all, biggest = [], 0, 0
    for pos in range(0, x.size, chunk):
        pending = np.concatenate([pending, x[pos: pos + chunk]])
        y, cons, prod, _ = f.filter(pending, pending.size + 4)
        assert cons == prod
        outs.append(y)
        pending = pending[cons:]
        cons_all += cons
        biggest = max(biggest, prod)
    y = np.concatenate(outs)
    return y, cons_all, y.size, biggest


def _chunks(nb, info):
    return [1, nb, 509, info[2] + 1]


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("name", ["B", "O"])
def test_streaming_within_bound(gpu, name, which):
    a, b = iir_ref.FILTERS[name]
    info = _info(gpu)
    chunk = _chunks(b.size, info)[which]
    n_in = iir_ref.stream_len(info)
    x, y_ref, bsum = _value_stream(gpu, name)
    x = x[:n_in]
    one = gpu.Iir(a, b).filter(x, n_in)
    y, cons, prod, biggest = _stream(gpu.Iir(a, b), x, chunk)
    assert (cons, prod) == (one[1], one[2]) == (n_in - (b.size - 1),) * 2
    if chunk == 1:
        # every call shifts the memory (the call that completes the fill
        # produces the n_a - (n_b-1) outputs its backlog allows, then one)
        assert biggest == max(1, a.size - (b.size - 1)) < a.size
    c = iir_ref.kernel_c(a.size, b.size, biggest, info)
    err = np.abs(y.astype(np.float64) - y_ref[:prod])
    ratio = float(np.max(err / (iir_ref.gamma(c) * bsum[:prod])))
    print(f"iir stream {name} chunk {chunk}: worst err/bound {ratio:.3f}")
    assert 0 < ratio <= 1


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("name", ["I", "E"])
def test_streaming_exact(gpu, name, which):
    a, b = iir_ref.EXACT[name]
    info = _info(gpu)
    chunk = _chunks(b.size, info)[which]
    x = iir_ref.exact_input(iir_ref.stream_len(info), ord(name) + 1)
    want = iir_ref.exact_closed_form(name, x)
    y, cons, prod, _ = _stream(gpu.Iir(a, b), x, chunk)
    assert cons == prod == want.size
    assert np.array_equal(y.astype(np.float64), want)


# ---- 4. the fill ------------------------------------------------------------

@pytest.mark.parametrize("name", ["D", "W"])
def test_fill_split_over_calls(gpu, name):
    # n_in < n_a, n_in == n_a, then everything: nothing twice, then the
    # one-call run (a call whose pushes equal its input returns, :119)
    a, b = iir_ref.FILTERS[name]
    x = _value_stream(gpu, name)[0][:700 + b.size - 1]
    one = gpu.Iir(a, b).filter(x, 705)
    assert one[2] == 700
    f = gpu.Iir(a, b)
    for n_in in (a.size - 1, a.size):
        y, cons, prod, st = f.filter(x[:n_in], 5)
        assert (cons, prod, st) == (0, 0, iir_ref.INSUFFICIENT_INPUT)
    y, cons, prod, st = f.filter(x, 705)
    assert (cons, prod, st) == one[1:]
    assert np.array_equal(y.view(np.uint32), one[0].view(np.uint32))


def test_fill_completed_by_a_later_call(gpu):
    # with n_a > 1 the call that completes a fill begun earlier pushed
    # fewer samples than it has, so the reference goes on to produce
    a, b = iir_ref.FILTERS["O"]
    x, y_ref, bsum = _value_stream(gpu, "O")
    x = x[:700 + b.size - 1]
    f = gpu.Iir(a, b)
    filled, pos, outs = 0, 0, []
    for n_in, n_out in ((a.size - 3, 5), (a.size, 5), (x.size, 705)):
        want = iir_ref.count(a.size, b.size, filled, min(n_in, x.size - pos),
                             n_out)
        y, cons, prod, st = f.filter(x[pos: pos + n_in], n_out)
        assert (cons, prod, st) == want[1:]
        filled, pos = want[0], pos + cons
        outs.append(y)
    assert [o.size for o in outs] == [0, 5, 695]
    y = np.concatenate(outs).astype(np.float64)
    lim = iir_ref.gamma(iir_ref.kernel_c(a.size, b.size, 700,
                                         _info(gpu))) * bsum[:700]
    assert (np.abs(y - y_ref[:700]) <= lim).all()


def test_fill_from_different_samples(gpu):
    # the fill takes in[memory.len()] of whatever the call presents
    a, b = iir_ref.FILTERS["Q"]
    r = np.random.default_rng(0x11D)
    x1 = r.uniform(0.5, 1.0, 2).astype(F32)
    x2 = -r.uniform(0.5, 1.0, 300 + b.size - 1).astype(F32)
    f = gpu.Iir(a, b)
    assert f.filter(x1, 9)[1:] == (0, 0, iir_ref.INSUFFICIENT_INPUT)
    _, _, _, _, mem = iir_ref.serial(a, b, x1, 9, np.float64)
    assert mem == [x1[0], x1[1]]
    y_ref, cons, prod, st, _ = iir_ref.serial(a, b, x2, 400, np.float64, mem)
    filled = [x1[0], x1[1], x2[2], x2[3]]
    lim = iir_ref.bound(a, b, x2, y_ref,
                        iir_ref.kernel_c(a.size, b.size, 300, _info(gpu)),
                        memory=filled)
    ratio = _check_call(f.filter(x2, 400), (cons, prod, st), y_ref, lim)
    assert prod == 300 and ratio > 0
    # a handle filled from x2 alone is a different filter
    other = gpu.Iir(a, b).filter(x2, 400)[0]
    assert (np.abs(other - y_ref) > lim).any()


# ---- 5. handle surface ------------------------------------------------------

def test_item_sizes_length_variant(gpu):
    a, b = iir_ref.FILTERS["O"]
    f = gpu.Iir(a, b)
    out_b = ctypes.c_size_t()
    assert gpu.lib().fsdr_filter_item_sizes(f._h, ctypes.byref(out_b)) == 4
    assert out_b.value == 4
    assert f.length == b.size
    assert f.variant() == (0, 0, 0)


def test_in_place_is_refused(gpu):
    lib = gpu.lib()
    f = gpu.Iir([0.5], [1.0])
    d = ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(d), 4096) == gpu.OK
    try:
        with pytest.raises(gpu.FsdrError, match="in-place"):
            f.filter_dev(d.value, 64, d.value, 64)
    finally:
        lib.fsdr_dev_free(d)


def test_empty_and_short_calls(gpu):
    f = gpu.Iir([0.5], [1.0, 2.0, 3.0])
    assert f.filter(np.zeros(0, F32), 0)[1:] == (0, 0, iir_ref.BOTH_SUFFICIENT)
    assert f.filter(np.zeros(0, F32), 4)[1:] == \
        (0, 0, iir_ref.INSUFFICIENT_INPUT)
    assert f.filter(np.ones(2, F32), 4)[1:] == iir_ref.count(1, 3, 0, 2, 4)[1:]


# ---- 6. through the flowgraph, and the example -------------------------------

def test_flowgraph_ends_and_delivers(gpu):
    a, b = iir_ref.FILTERS["B"]
    info = _info(gpu)
    x, y_ref, bsum = _value_stream(gpu, "B")
    n_in = 2 * info[2] + 100
    fg = gpu.Flowgraph()
    src = fg.vector_source_f32(x[:n_in])
    flt = fg.filter(gpu.Iir(a, b))
    snk = fg.vector_sink()
    fg.connect(src, flt, snk)
    fg.run()
    got = fg.sink_data(snk, F32)
    n = n_in - (b.size - 1)
    assert got.size == n == fg.n_received(snk)
    lim = iir_ref.gamma(iir_ref.kernel_c(a.size, b.size, n, info)) * bsum[:n]
    err = np.abs(got.astype(np.float64) - y_ref[:n])
    assert 0 < np.max(err / lim) <= 1


def test_fm_receiver_example_with_deemphasis(gpu):
    path = os.path.join(os.path.dirname(__file__), "..", "examples",
                        "fm_receiver.py")
    spec = importlib.util.spec_from_file_location("fm_receiver_iir", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    x = ex.synthesize(1 << 17)
    plain = ex.receive(x)
    audio = ex.receive(x, deemph_tau=75e-6)
    assert audio.dtype == F32 and audio.size == plain.size
    peak, want, _ = ex.tone_bin(audio)
    assert peak == want == ex.tone_bin(plain)[0]
    a, b = ex.deemph_taps(75e-6)
    y_ref = iir_ref.serial(a, b, plain, plain.size, np.float64)[0]
    assert y_ref.size == plain.size
    lim = iir_ref.bound(a, b, plain, y_ref,
                        iir_ref.kernel_c(1, 1, plain.size, _info(gpu)))
    err = np.abs(audio.astype(np.float64) - y_ref)
    print(f"fm receiver de-emphasis: worst err/bound {np.max(err / lim):.3f}")
    assert 0 < np.max(err / lim) <= 1
