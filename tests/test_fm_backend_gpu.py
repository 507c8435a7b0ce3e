"""FM receiver back end on the GPU: ResamplerF32, QuadDemod and the fused
FmDemodResampler against the float64 references of tests/fm_ref.py and
tests/dsp_ref.py, with the bounds derived there (fm_ref docstring), and
consumed/produced/status against the oracle's resamp_status arithmetic.

Sizes: one tile of the f32 resampler kernels is 512 outputs, so produced
counts of 511, 512, 513 and 1025 (rounded down to a multiple of interp,
as the block emits) sit on both sides of a tile edge and of a second
tile; FSDR_FIR_GRID_CAP=1 makes one block walk every tile.
"""
import importlib.util
import os

import numpy as np
import pytest

import dsp_ref as R
import fm_ref as F

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = ((1, 5, 22), (1, 4, 128), (3, 2, 6), (6, 25, 144), (2, 7, 10))
EDGES = (511, 512, 513, 1025)
SPAN_FALLBACK = (1, 40, 40)  # 511*40 + 42 floats of span: over 64 KiB


def _taps(interp, decim, n_taps):
    if (interp, decim, n_taps) == (3, 2, 6):
        return np.arange(1, 7, dtype=F32)  # the oracle KAT's taps
    return R.loud_f32(np.random.default_rng([11, interp, decim, n_taps]),
                      n_taps)


def _n_big(interp, decim, n_taps):
    """Inputs for more than 1025 outputs."""
    return (1030 + interp) * decim // interp + n_taps // interp + 8


def _sizes(interp, decim, n_taps):
    """(n_in, n_out): starved, one window, input-limited, output-limited,
    and the tile edges."""
    tpp = n_taps // interp
    big = _n_big(interp, decim, n_taps)
    s = [(1, 64), (tpp, 64), (3000, 10 ** 5), (3000, 7), (3000, 0)]
    if tpp > 1:
        s.append((tpp - 1, 64))
    return s + [(big, p) for p in EDGES]


def _env(monkeypatch, grid_cap, **switches):
    if grid_cap is None:
        monkeypatch.delenv("FSDR_FIR_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("FSDR_FIR_GRID_CAP", str(grid_cap))
    for k, v in switches.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# ---- 1. ResamplerF32 ----------------------------------------------------

@pytest.mark.parametrize("tiled", ["1", "0"])
@pytest.mark.parametrize("grid_cap", [None, 1])
@pytest.mark.parametrize("interp,decim,n_taps", SHAPES)
def test_resampler_f32(gpu, oracle_lib, monkeypatch, interp, decim, n_taps,
                       grid_cap, tiled):
    _env(monkeypatch, grid_cap, FSDR_RESAMP_TILED=tiled)
    taps = _taps(interp, decim, n_taps)
    x = R.loud_f32(np.random.default_rng([12, interp, decim, n_taps]),
                   max(3000, _n_big(interp, decim, n_taps)))
    rs = gpu.ResamplerF32(interp, decim, taps)
    assert rs.length == n_taps
    worst = 0.0
    for n_in, n_out in _sizes(interp, decim, n_taps):
        got, *counts = rs.filter(x[:n_in], n_out)
        _, *want = oracle_lib.resamp_f32(interp, decim, taps, x[:n_in],
                                         n_out)
        assert counts == want, (n_in, n_out, counts, want)
        prod = counts[1]
        if prod == 0:
            continue
        ref, a, _ = R.resamp(interp, decim, taps, x[:n_in], prod)
        err = np.abs(got.astype(np.float64) - ref)
        bound = R.gamma(n_taps // interp + 1) * a
        worst = max(worst, float((err / bound).max()))
        print(f"resamp_f32 {interp}/{decim}/{n_taps} n_in={n_in} "
              f"n_out={n_out} prod={prod}: err/bound={(err / bound).max()}")
        assert np.all(err <= bound), (n_in, n_out, (err / bound).max())
    assert worst > 0.0  # something was computed and compared


def test_resampler_f32_item_sizes(gpu):
    import ctypes
    rs = gpu.ResamplerF32(1, 5, np.ones(22, F32))
    ob = ctypes.c_size_t()
    assert gpu.lib().fsdr_filter_item_sizes(rs._h, ctypes.byref(ob)) == 4
    assert ob.value == 4
    fm = gpu.FmDemodResampler(1, 5, np.ones(22, F32))
    assert gpu.lib().fsdr_filter_item_sizes(fm._h, ctypes.byref(ob)) == 8
    assert ob.value == 4 and fm.length == 22
    assert gpu.QuadDemod().length == 1


# ---- 2. QuadDemod -------------------------------------------------------

@pytest.mark.parametrize("x0,want,neg", [
    (0.6 + 0.7j, 0.0, False), (0.6 - 0.7j, 0.0, True),
    (-0.6 + 0.7j, 0.0, False), (-0.6 - 0.7j, np.pi, False)])
def test_quad_demod_first_sample(gpu, x0, want, neg):
    """Fresh handle, last = 0+0i: the reference's signed-zero results."""
    x = np.array([x0], np.complex64)
    ref = F.demod(x)
    assert ref[0] == want and bool(np.signbit(ref[0])) == neg
    got, cons, prod, status = gpu.QuadDemod().filter(x, 1)
    assert (cons, prod, status) == (1, 1, gpu.BOTH_SUFFICIENT)
    assert got.dtype == F32 and got[0] == F32(want)
    assert bool(np.signbit(got[0])) == neg


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_quad_demod_values(gpu, n):
    x, ref = F.demod_case(1, 4097)
    got, cons, prod, status = gpu.QuadDemod().filter(x[:n], n + 5)
    assert (cons, prod, status) == (n, n, gpu.BOTH_SUFFICIENT)
    err = np.abs(got.astype(np.float64) - ref[:n])
    print(f"quad demod n={n}: max err {err.max():.3e} (E_D {F.E_D:.3e})")
    assert np.all(err <= F.E_D), err.max()


def test_quad_demod_output_limited_and_empty(gpu):
    """apply.rs:108: m = min(n_in, n_out); m == 0 leaves `last` alone."""
    x, ref = F.demod_case(1, 4097)
    qd = gpu.QuadDemod()
    got, cons, prod, status = qd.filter(x[:100], 37)
    assert (cons, prod, status) == (37, 37, gpu.BOTH_SUFFICIENT)
    assert qd.filter(x[37:100], 0)[1:] == (0, 0, gpu.BOTH_SUFFICIENT)
    assert qd.filter(x[:0], 10)[1:] == (0, 0, gpu.BOTH_SUFFICIENT)
    more = qd.filter(x[37:100], 100)[0]
    err = np.abs(np.concatenate((got, more)).astype(np.float64) - ref[:100])
    assert np.all(err <= F.E_D), err.max()


@pytest.fixture(scope="module")
def demod_one_call(gpu):
    x, _ = F.demod_case(1, 4097)
    got = gpu.QuadDemod().filter(x, x.size)[0].copy()
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("chunk", [1, 7, 64, 1000])
def test_quad_demod_chunked_is_bit_equal(gpu, demod_one_call, chunk):
    x, _ = F.demod_case(1, 4097)
    qd = gpu.QuadDemod()
    parts = [qd.filter(x[i:i + chunk], chunk)[0]
             for i in range(0, x.size, chunk)]
    got = np.concatenate(parts)
    assert got.size == x.size
    assert np.array_equal(got.view(np.uint32),
                          demod_one_call.view(np.uint32))


# ---- 3. FmDemodResampler ------------------------------------------------

def _check_fm(gpu, oracle_lib, interp, decim, n_taps, sizes, want_fused):
    taps = _taps(interp, decim, n_taps)
    x = F.fm_input(2, max(n for n, _ in sizes))
    worst = 0.0
    for n_in, n_out in sizes:
        fm = gpu.FmDemodResampler(interp, decim, taps)  # fresh: last = 0
        assert fm.fused is want_fused
        got, *counts = fm.filter(x[:n_in], n_out)
        _, *want = oracle_lib.resamp_f32(interp, decim, taps,
                                         np.zeros(n_in, F32), n_out)
        assert counts == want, (n_in, n_out, counts, want)
        prod = counts[1]
        if prod == 0:
            continue
        ref, a, h1 = F.chain(interp, decim, taps, x[:n_in], prod)
        err = np.abs(got.astype(np.float64) - ref)
        bound = F.chain_bound(n_taps, interp, a, h1)
        worst = max(worst, float((err / bound).max()))
        print(f"fm {interp}/{decim}/{n_taps} fused={want_fused} n_in={n_in} "
              f"n_out={n_out} prod={prod}: err/bound={(err / bound).max()}")
        assert np.all(err <= bound), (n_in, n_out, (err / bound).max())
    assert worst > 0.0


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("grid_cap", [None, 1])
@pytest.mark.parametrize("interp,decim,n_taps", SHAPES)
def test_fm_demod_resampler(gpu, oracle_lib, monkeypatch, interp, decim,
                            n_taps, grid_cap, fused):
    _env(monkeypatch, grid_cap, FSDR_FM_FUSED=None if fused else "0",
         FSDR_RESAMP_TILED=None)
    _check_fm(gpu, oracle_lib, interp, decim, n_taps,
              _sizes(interp, decim, n_taps), fused)


@pytest.mark.parametrize("grid_cap", [None, 1])
def test_fm_span_over_lds_budget_falls_back(gpu, oracle_lib, monkeypatch,
                                            grid_cap):
    _env(monkeypatch, grid_cap, FSDR_FM_FUSED=None, FSDR_RESAMP_TILED=None)
    interp, decim, n_taps = SPAN_FALLBACK
    big = _n_big(interp, decim, n_taps)
    _check_fm(gpu, oracle_lib, interp, decim, n_taps,
              [(n_taps, 64), (3000, 10 ** 5), (big, 513), (big, 1025)],
              False)


def test_fm_carried_last_matches_two_blocks(gpu, monkeypatch):
    """A second call starts from last = x[consumed-1], on either path,
    and both paths give the same bits."""
    taps = _taps(1, 5, 22)
    x = F.fm_input(3, 6000)
    outs = []
    for env in (None, "0"):
        _env(monkeypatch, None, FSDR_FM_FUSED=env, FSDR_RESAMP_TILED=None)
        fm = gpu.FmDemodResampler(1, 5, taps)
        y0, c0, p0, _ = fm.filter(x[:3000], 3000)
        assert c0 == 5 * p0 and 0 < c0 < 3000
        assert fm.filter(x[c0:c0 + 10], 100)[1:3] == (0, 0)  # last stays
        y1, c1, p1, _ = fm.filter(x[c0:], 3000)
        ref, a, h1 = F.chain(1, 5, taps, x[c0:], p1, last=x[c0 - 1])
        err = np.abs(y1.astype(np.float64) - ref)
        assert np.all(err <= F.chain_bound(22, 1, a, h1))
        outs.append(np.concatenate((y0, y1)))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ---- 4. streaming -------------------------------------------------------

STREAM_N = 20000


@pytest.fixture(scope="module")
def stream_one_call(gpu):
    taps = _taps(1, 5, 22)
    x = F.fm_input(4, STREAM_N)
    fm = gpu.FmDemodResampler(1, 5, taps)
    assert fm.fused
    y, cons, prod, _ = fm.filter(x, STREAM_N)
    ref, a, h1 = F.chain(1, 5, taps, x, prod)
    assert prod == (STREAM_N - 22) // 5 and cons == 5 * prod
    assert np.all(np.abs(y.astype(np.float64) - ref)
                  <= F.chain_bound(22, 1, a, h1))
    y = y.copy()
    y.setflags(write=False)
    return taps, x, y, cons


@pytest.mark.parametrize("chunk", [1, 22, 23, 509, 4096])
def test_fm_streaming_is_bit_equal(gpu, stream_one_call, chunk):
    taps, x, y_one, cons_one = stream_one_call
    fm = gpu.FmDemodResampler(1, 5, taps)
    assert fm.fused
    parts, consumed, lo = [], 0, 0
    for hi in range(chunk, STREAM_N + chunk, chunk):
        hi = min(hi, STREAM_N)
        # the unconsumed tail [lo, previous hi) is presented again
        y, c, p, _ = fm.filter(x[lo:hi], hi - lo)
        parts.append(y)
        lo += c
        consumed += c
    got = np.concatenate(parts)
    assert consumed == cons_one and got.size == y_one.size
    assert np.array_equal(got.view(np.uint32), y_one.view(np.uint32))


def test_fm_streaming_through_flowgraph(gpu, stream_one_call):
    taps, x, y_one, _ = stream_one_call
    fg = gpu.Flowgraph()
    src = fg.vector_source(x)
    fm = fg.filter(gpu.FmDemodResampler(1, 5, taps))
    snk = fg.vector_sink()
    fg.connect(src, fm, snk)
    fg.run()
    got = fg.sink_data(snk, F32)
    assert got.size == y_one.size
    assert np.array_equal(got.view(np.uint32), y_one.view(np.uint32))


# ---- 5. end to end ------------------------------------------------------

def test_fm_receiver_example_recovers_the_tone(gpu):
    path = os.path.join(os.path.dirname(__file__), "..", "examples",
                        "fm_receiver.py")
    spec = importlib.util.spec_from_file_location("fm_receiver_example", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    audio = ex.receive(ex.synthesize(1 << 17))
    # 2^17 * 6/25 / 5 samples less the two filters' windows
    assert audio.dtype == F32 and 6200 < audio.size < 6300
    peak, want, bins = ex.tone_bin(audio)
    print(f"fm receiver: peak bin {peak}, expected {want} of {bins}")
    assert peak == want
