"""The LoRa FFT demodulator on the GPU against tests/lora_ref.py (float64
numpy). Hard and raw decisions are bit-equal wherever the reference's own
top two bins are further apart than the FFT budget allows them to move;
soft LLRs lie inside the bound lora_ref derives from that budget. Shapes:
sf 5 (16 symbols per block), 7 and 11 (odd log2, radix-2 tail), 8, 12 (one
symbol per block, the LDS maximum); 1, 7, 37 symbols, at sf 5 also 15 and
17, at sf 12 at most 5. FSDR_FIR_GRID_CAP=1 makes one block walk every
batch, 3 gives blocks an uneven share."""
import ctypes
import functools

import numpy as np
import pytest

import lora_ref
from lora_ref import HARD, RAW, SOFT

pytestmark = pytest.mark.gpu

SFS = (5, 7, 8, 11, 12)
COUNTS = {5: (1, 7, 15, 17, 37), 7: (1, 7, 37), 8: (1, 7, 37),
          11: (1, 7, 37), 12: (1, 3, 5)}
CFO = (3, 0.25)


def snr_of(sf, which):
    """Per-sample SNR (linear) that puts the largest Bessel argument, about
    N * snr, near 300 ("lo": the ln I0 branch; 3 at sf 5, where a higher
    SNR makes the noise-sum term of the bound pass 1 % of the LLRs) or near
    3000 ("hi": past 709, the clipped branch)."""
    n = 1 << sf
    return min(3.0, 300.0 / n) if which == "lo" else 3000.0 / n


@pytest.fixture(params=[None, "1", "3"], ids=["cap-", "cap1", "cap3"])
def grid_cap(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("FSDR_FIR_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("FSDR_FIR_GRID_CAP", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _stream(sf, which, cfo):
    """(x, ids) of the longest case of this sf, plus N - 1 samples of a
    further symbol that no call may touch."""
    n = 1 << sf
    x, ids = lora_ref.stream(sf, max(COUNTS[sf]) + 1, snr_of(sf, which),
                             seed=1000 * sf + (which == "hi") + 2 * bool(cfo),
                             cfo=cfo)
    x = x[:max(COUNTS[sf]) * n + n - 1].copy()
    x.setflags(write=False)
    return x, ids[:max(COUNTS[sf])]


@functools.lru_cache(maxsize=None)
def _spectrum(sf, which, cfo_on, preamble):
    cfo = CFO if cfo_on else (0, 0.0)
    x, ids = _stream(sf, which, sum(cfo) if cfo_on else 0.0)
    X = lora_ref.spectrum(x, lora_ref.downchirp(sf, *cfo, preamble=preamble))
    X.setflags(write=False)
    return x, ids, X


@functools.lru_cache(maxsize=None)
def _soft_ref(sf, which, reduced):
    x, ids, X = _spectrum(sf, which, False, False)
    return (x, ids, X) + lora_ref.soft(X, sf, reduced)


def _call(f, sf, x, count, room):
    """`count` whole symbols plus N - 1 samples, `room` output slots."""
    n = 1 << sf
    n_in = count * n + n - 1
    y, cons, prod, st = f.filter(x[:n_in], room)
    assert (cons, prod, st) == lora_ref.count(sf, n_in, room)
    assert y.shape[0] == prod
    return y


# ---- 1. hard and raw decisions ----------------------------------------------

@pytest.mark.parametrize("sf", SFS)
def test_hard_and_raw_bit_equal(gpu, sf, grid_cap):
    n = 1 << sf
    for cfo_on in (False, True):
        cfo = CFO if cfo_on else (0, 0.0)
        x, ids, X = _spectrum(sf, "lo", cfo_on, False)
        # no symbol is left out: the reference alone decides every one
        assert lora_ref.margin_ok(X).all()
        for reduced in (False, True):
            want = lora_ref.hard(X, reduced)
            assert np.array_equal(want, ((ids - 1) % n) // (4 if reduced
                                                           else 1))
            f = gpu.LoraFftDemod(sf, HARD)
            if cfo_on or reduced:
                f.set_frame(*cfo, reduced_rate=reduced)
            for c in COUNTS[sf]:
                for room in (c + 3, c, max(c - 1, 1)):
                    y = _call(f, sf, x, c, room)
                    assert y.dtype == np.uint16
                    assert np.array_equal(y, want[:y.size]), (c, room)
        xr, _, Xr = _spectrum(sf, "lo", cfo_on, True)
        assert lora_ref.margin_ok(Xr).all()
        want = lora_ref.raw(Xr)
        assert np.array_equal(want, (ids - 1) % n)
        f = gpu.LoraFftDemod(sf, RAW)
        if cfo_on:
            f.set_frame(*cfo, reduced_rate=True)   # RAW ignores the rate
        for c in COUNTS[sf]:
            assert np.array_equal(_call(f, sf, xr, c, c + 3), want[:c])


# ---- 2. tie-break and zero energy, exact ------------------------------------

@pytest.mark.parametrize("sf", SFS)
def test_zero_input_pins_last_index_and_none(gpu, sf, grid_cap):
    n = 1 << sf
    z = np.zeros(3 * n, np.complex64)
    f = gpu.LoraFftDemod(sf, HARD)
    assert f.filter(z, 3)[0].tolist() == [n - 2] * 3
    f.set_frame(0, 0.0, reduced_rate=True)
    assert f.filter(z, 3)[0].tolist() == [(n - 2) // 4] * 3
    assert gpu.LoraFftDemod(sf, RAW).filter(z, 3)[0].tolist() == [0xFFFF] * 3


# ---- 3. soft decisions ------------------------------------------------------

@pytest.mark.parametrize("which", ["lo", "hi"])
@pytest.mark.parametrize("sf", SFS)
def test_soft_llrs_within_bound(gpu, sf, which, grid_cap):
    worst = 0.0
    for reduced in (False, True):
        x, ids, X, llr, bound, a_max, da_max = _soft_ref(sf, which, reduced)
        # conditions on the reference alone
        assert lora_ref.margin_ok(X).all()
        assert lora_ref.regime_ok(a_max, da_max).all()
        assert ((a_max >= 709.0) == (which == "hi")).all()
        med = np.median(np.abs(llr[:, :sf]))
        assert bound.max() <= 0.01 * med, (bound.max(), med)
        f = gpu.LoraFftDemod(sf, SOFT)
        if reduced:
            f.set_frame(0, 0.0, reduced_rate=True)
        for c in COUNTS[sf]:
            y = _call(f, sf, x, c, c + 2)
            assert y.dtype == np.float64 and y.shape == (c, 12)
            assert np.isfinite(y).all()
            err = np.abs(y - llr[:c]).max(axis=1)
            assert (err <= bound[:c]).all(), \
                f"worst err/bound {np.max(err / bound[:c]):.3g}"
            assert (y[:, sf:] == 0.0).all()
            if reduced:
                assert (y[:, :2] <= 0.0).all()
            worst = max(worst, float(np.max(err / bound[:c])))
    print(f"lora soft sf {sf} {which} cap={grid_cap}: "
          f"worst err/bound {worst:.3g}")
    assert worst > 0


# ---- 4. counts, chunking, guard ---------------------------------------------

@pytest.mark.parametrize("mode", [HARD, SOFT])
@pytest.mark.parametrize("sf", [5, 8, 12])
def test_chunked_stream_equals_one_shot(gpu, sf, mode, grid_cap):
    n = 1 << sf
    x, _ = _stream(sf, "lo", 0.0)
    k = x.size // n
    assert x.size == k * n + n - 1
    f = gpu.LoraFftDemod(sf, mode)
    whole = _call(f, sf, x, k, k + 4)            # n_out above k
    assert whole.shape[0] == k
    short = _call(f, sf, x, k, max(k - 2, 1))    # n_out below k
    assert np.array_equal(short, whole[:short.shape[0]])
    for per_call in (1, 2, 5):
        # the first call is n/2 + 1 samples short of whole symbols, so
        # every call leaves a partial symbol to carry; with 5 symbols'
        # worth and room for 2 the carried tail is longer than a symbol
        room = 2 if per_call == 5 else per_call + 1
        got, pending, pos = [], x[:0], 0
        first = True
        while True:
            take = per_call * n - (n // 2 + 1 if first else 0)
            first = False
            new = x[pos:pos + take]
            pos += new.size
            pending = np.concatenate([pending, new])
            y, cons, prod, st = f.filter(pending, room)
            assert (cons, prod, st) == lora_ref.count(sf, pending.size, room)
            got.append(y)
            pending = pending[cons:]
            if new.size == 0 and prod == 0:
                break
        got = np.concatenate(got)
        assert got.shape == whole.shape and np.array_equal(got, whole), \
            per_call
        assert pending.size == n - 1


@pytest.mark.parametrize("mode", [HARD, SOFT])
def test_nothing_written_past_produced(gpu, mode, grid_cap):
    sf = 7
    n = 1 << sf
    lib = gpu.lib()
    x, _ = _stream(sf, "lo", 0.0)
    item = 96 if mode == SOFT else 2
    f = gpu.LoraFftDemod(sf, mode)
    want = f.filter(x, 40)[0]
    for n_in, room in ((7 * n + n - 1, 9), (7 * n + n - 1, 5), (n - 1, 4)):
        prod = min(n_in // n, room)
        cap = (room + 2) * item
        host = np.full(cap, 0xA5, np.uint8)
        d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
        assert lib.fsdr_dev_alloc(ctypes.byref(d_in), x.size * 8) == 0
        assert lib.fsdr_dev_alloc(ctypes.byref(d_out), cap) == 0
        try:
            lib.fsdr_memcpy_h2d(d_in, ctypes.c_void_p(x.ctypes.data),
                                x.size * 8)
            lib.fsdr_memcpy_h2d(d_out, ctypes.c_void_p(host.ctypes.data), cap)
            assert f.filter_dev(d_in.value, n_in, d_out.value, room) == \
                lora_ref.count(sf, n_in, room)
            gpu.synchronize()
            back = np.zeros(cap, np.uint8)
            lib.fsdr_memcpy_d2h(ctypes.c_void_p(back.ctypes.data), d_out, cap)
        finally:
            lib.fsdr_dev_free(d_in)
            lib.fsdr_dev_free(d_out)
        assert (back[prod * item:] == 0xA5).all(), (n_in, room)
        assert back[:prod * item].tobytes() == want[:prod].tobytes()


# ---- 5. flowgraph -----------------------------------------------------------

def test_flowgraph_bytes_equal_direct_call(gpu, grid_cap):
    sf = 7
    x, _ = _stream(sf, "lo", 0.0)
    f = gpu.LoraFftDemod(sf, HARD)
    assert f.length == 1 << sf
    direct = f.filter(x, 64)[0]
    assert direct.size == x.size >> sf
    fg = gpu.Flowgraph()
    src = fg.vector_source(x)
    blk = fg.filter(gpu.LoraFftDemod(sf, HARD))
    snk = fg.vector_sink()
    fg.connect(src, blk, snk)
    fg.run()
    got = fg.sink_data(snk, dtype=np.uint16)
    assert got.tobytes() == direct.tobytes()
    assert fg.n_received(snk) == direct.size
