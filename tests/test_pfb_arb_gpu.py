"""PFB arbitrary-rate resampler on the GPU against the literal restatement
of arb_resampler.rs (tests/pfb_arb_ref.py: f32 timing state, float64
filtering and interpolation).

Bar, per output and per component (re, im):
    |got - ref| <= gamma_{tpf+4} * ((1-mu) * sum|h_a||x| + mu * sum|h_b||x|)
with gamma_k = k*u/(1-k*u), u = 2^-24. The tpf-term dot is gamma_{tpf+1}
by the project's convention and the interpolation adds
three roundings; |1-mu| and |mu| stand where mu is negative (rate >
num_filters). Counts and shapes must be exact. Inputs and taps have every
component in +-[0.5, 1)."""
import ctypes
import functools

import numpy as np
import pytest

from pfb_arb_ref import PfbArbResamplerRef, oneshot, random_case

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
POISON = np.complex64(1e6 + 1e6j)


def gamma(k):
    return k * U / (1 - k * U)


def tpf_of(n_taps, nf):
    return -(-n_taps // nf)


def check(got, ref, bounds, tpf, what=""):
    got = np.asarray(got, np.complex128)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    g = gamma(tpf + 4)
    d = got - ref
    ratio = max(float(np.max(np.abs(d.real) / (g * bounds.real))),
                float(np.max(np.abs(d.imag) / (g * bounds.imag))))
    print(f"{what}: worst error / bar = {ratio:.3f} over {ref.size} outputs")
    assert ratio <= 1.0, f"{what}: error {ratio} x the bar"


@functools.lru_cache(maxsize=None)
def cached(rate, nf, n_taps, C, n_in):
    """random_case + its one-call restatement with room for everything,
    computed once per shape and shared; read-only."""
    taps, chans = random_case(rate, nf, n_taps, C, n_in)
    out, bounds, cons, idx = oneshot(rate, nf, taps, chans,
                                     int(n_in * rate) + 64)
    assert cons == n_in
    for a in (taps, chans, out, bounds, idx):
        a.setflags(write=False)
    return taps, chans, out, bounds, idx


def prefix(case, n_in, tpf):
    """The restatement of the first n_in inputs of a cached case: outputs
    are emitted input by input, so it is a prefix."""
    taps, chans, out, bounds, idx = case
    k = int(np.searchsorted(idx, max(0, n_in - tpf)))
    return taps, chans[:, :n_in], out[:, :k], bounds[:, :k]


def raw_call(gpu, rs, buf, in_stride, n_in, out_stride, out_cap, fn="run"):
    """run_dev/stream_dev over a host copy `buf` of C*in_stride items;
    returns (the whole [C, out_stride] output buffer, pre-poisoned,
    consumed, produced)."""
    lib = gpu.lib()
    call = getattr(lib, f"fsdr_pfb_arb_resampler_{fn}_dev")
    buf = np.ascontiguousarray(buf, np.complex64)
    C = rs.n
    out = np.full(C * out_stride, POISON, np.complex64)
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(d_in), buf.size * 8 + 8) == 0
    assert lib.fsdr_dev_alloc(ctypes.byref(d_out), out.size * 8 + 8) == 0
    try:
        lib.fsdr_memcpy_h2d(d_in, ctypes.c_void_p(buf.ctypes.data),
                            buf.size * 8)
        lib.fsdr_memcpy_h2d(d_out, ctypes.c_void_p(out.ctypes.data),
                            out.size * 8)
        cons, prod = ctypes.c_size_t(), ctypes.c_size_t()
        rc = call(rs._h, d_in, in_stride, n_in, d_out, out_stride, out_cap,
                  None, ctypes.byref(cons), ctypes.byref(prod))
        assert rc == 0, lib.fsdr_last_error().decode()
        gpu.synchronize()
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(out.ctypes.data), d_out,
                            out.size * 8)
        return out.reshape(C, out_stride), cons.value, prod.value
    finally:
        lib.fsdr_dev_free(d_in)
        lib.fsdr_dev_free(d_out)


# ---------------- bulk parity -------------------------------------------

BULK = [
    (2.5, 5, 40, 1, 700),
    (2.5, 5, 40, 3, 700),
    (0.7, 32, 125, 2, 900),   # zero-padded partition
    (1.6, 32, 32, 1, 300),    # tpf 1
    (0.3, 5, 25, 1, 2000),    # sparse outputs
    (7.3, 4, 32, 2, 200),     # many outputs per input, negative mu
]


@pytest.fixture(params=[None, "1"], ids=["grid-free", "grid-cap-1"])
def grid_cap(request, monkeypatch):
    """FSDR_FIR_GRID_CAP unset, and at 1 so that one block owns every
    segment of the call (read per launch)."""
    if request.param is None:
        monkeypatch.delenv("FSDR_FIR_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("FSDR_FIR_GRID_CAP", request.param)
    return request.param


@pytest.mark.parametrize("rate,nf,n_taps,C,n_in", BULK)
def test_bulk_parity(gpu, grid_cap, rate, nf, n_taps, C, n_in):
    taps, chans, ref, bounds, _ = cached(rate, nf, n_taps, C, n_in)
    tpf = tpf_of(n_taps, nf)
    rs = gpu.PfbArbResampler(rate, taps, nf, C)
    assert rs.length == n_taps
    got, cons = rs.run(chans)
    assert cons == n_in
    assert (cons, got.shape[1]) == rs.schedule.work(
        tpf, 0, n_in, rs.out_cap_for(n_in))
    check(got, ref, bounds, tpf, f"bulk {rate} nf={nf} C={C}")


SEG = [(2.5, 5, 40, 2), (7.3, 4, 32, 1), (0.7, 32, 125, 1)]


@pytest.mark.parametrize("rate,nf,n_taps,C", SEG)
def test_bulk_parity_around_segment_length(gpu, grid_cap, rate, nf, n_taps,
                                           C):
    """n_in (and the inputs left after the tpf fill pushes) one below, at
    and one above the inputs one block owns per pass (queried, not
    copied), plus two segments and one input; with the grid capped at one
    block, that block loops over every segment."""
    tpf = tpf_of(n_taps, nf)
    R = gpu.PfbArbSchedule(rate, nf).segment_inputs
    assert R > tpf
    sizes = [R - 1, R, R + 1, tpf + R - 1, tpf + R, tpf + R + 1,
             tpf + 2 * R + 1]
    case = cached(rate, nf, n_taps, C, max(sizes))
    rs = gpu.PfbArbResampler(rate, case[0], nf, C)
    assert rs.schedule.segment_inputs == R
    for n_in in sizes:
        taps, chans, ref, bounds = prefix(case, n_in, tpf)
        got, cons = rs.run(chans)
        assert cons == n_in
        check(got, ref, bounds, tpf, f"segment {rate} n_in={n_in}")


def test_run_leaves_streaming_state_alone(gpu):
    rate, nf, n_taps, C, n_in = 2.5, 5, 40, 3, 700
    taps, chans, ref, bounds, _ = cached(rate, nf, n_taps, C, n_in)
    rs = gpu.PfbArbResampler(rate, taps, nf, C)
    a, ca = rs.stream(chans[:, :301])
    rs.run(chans[:, :123])
    b, cb = rs.stream(chans[:, 301:])
    assert (ca, cb) == (301, n_in - 301)
    check(np.concatenate([a, b], axis=1), ref, bounds, 8, "run between")


# ---------------- streaming ---------------------------------------------

def stream_all(gpu, rs, lit, tpf, chans, chunks, caps):
    """Feed `chunks` (then the rest) through stream(); the caller
    re-presents what a call leaves. Every call's consumed/produced must
    equal both the host schedule's and the literal work() pair's."""
    C, T = chans.shape
    outs, off, pushes, it = [], 0, 0, 0
    leftover = np.zeros((C, 0), np.complex64)
    cut_short = 0
    while off < T or leftover.shape[1]:
        take = chunks[it] if it < len(chunks) else 97
        cap = caps[it] if it < len(caps) else None
        it += 1
        buf = np.concatenate([leftover, chans[:, off:off + take]], axis=1)
        off = min(T, off + take)
        n = buf.shape[1]
        out_cap = rs.out_cap_for(n) if cap is None else cap
        out, cons = rs.stream(buf, out_cap)
        assert (cons, out.shape[1]) == rs.schedule.work(tpf, pushes, n,
                                                        out_cap), it
        lo, lc = lit.call(list(buf[0]), out_cap)
        assert (cons, out.shape[1]) == (lc, len(lo)), it
        cut_short += int(cons < n)
        pushes += cons
        outs.append(out)
        leftover = buf[:, cons:]
        assert it < 500
    assert pushes == T
    return np.concatenate(outs, axis=1), cut_short


@pytest.mark.parametrize("rate,nf,n_taps,C,n_in", [
    (2.5, 5, 40, 3, 700), (0.7, 32, 125, 2, 900), (7.3, 4, 32, 2, 200),
    (1.6, 32, 32, 1, 300)])
def test_streaming_equals_bulk(gpu, rate, nf, n_taps, C, n_in):
    """Chunks of 1, tpf-1, tpf, a prime and 0 inputs, calls that end
    inside the fill, and calls whose out_cap cuts them short."""
    taps, chans, ref, bounds, _ = cached(rate, nf, n_taps, C, n_in)
    tpf = tpf_of(n_taps, nf)
    rs = gpu.PfbArbResampler(rate, taps, nf, C)
    lit = PfbArbResamplerRef(rate, taps, nf)
    chunks = [1, 0, tpf - 1, tpf, 1, 13, 0, 40, 40, 1, 31]
    caps = [None] * 7 + [5, int(np.ceil(rate)) - 1, 3, None]
    got, cut_short = stream_all(gpu, rs, lit, tpf, chans, chunks, caps)
    assert cut_short >= 2
    check(got, ref, bounds, tpf, f"stream {rate} nf={nf} C={C}")


# ---------------- layout ------------------------------------------------

@pytest.mark.parametrize("fn", ["run", "stream"])
def test_strides_and_nothing_past_produced(gpu, fn):
    rate, nf, n_taps, C, n_in = 2.5, 5, 40, 3, 700
    taps, chans, ref, bounds, _ = cached(rate, nf, n_taps, C, n_in)
    in_stride, out_stride = n_in + 37, ref.shape[1] + 91
    buf = np.full((C, in_stride), POISON, np.complex64)
    buf[:, :n_in] = chans
    rs = gpu.PfbArbResampler(rate, taps, nf, C)
    out, cons, prod = raw_call(gpu, rs, buf, in_stride, n_in, out_stride,
                               ref.shape[1] + 50, fn)
    assert (cons, prod) == (n_in, ref.shape[1])
    check(out[:, :prod], ref, bounds, 8, f"strides {fn}")
    assert np.all(out[:, prod:] == POISON)
    # out_cap in the way: stops early, writes nothing past produced
    rs = gpu.PfbArbResampler(rate, taps, nf, C)
    out, cons, prod = raw_call(gpu, rs, buf, in_stride, n_in, out_stride,
                               400, fn)
    assert 0 < cons < n_in and 0 < prod <= 400
    check(out[:, :prod], ref[:, :prod], bounds[:, :prod], 8,
          f"strides short {fn}")
    assert np.all(out[:, prod:] == POISON)


def test_stride_smaller_than_span_is_refused(gpu):
    rs = gpu.PfbArbResampler(2.5, np.ones(40, np.float32), 5, 2)
    lib = gpu.lib()
    cons, prod = ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.fsdr_pfb_arb_resampler_run_dev(
        rs._h, None, 10, 11, None, 100, 100, None, ctypes.byref(cons),
        ctypes.byref(prod))
    assert rc == gpu.ERR_INVALID


# ---------------- generic entry points, flowgraph -----------------------

def test_filter_dev_single_channel_and_refusal(gpu):
    rate, nf, n_taps, n_in = 2.5, 5, 40, 700
    taps, chans, ref, bounds, _ = cached(rate, nf, n_taps, 1, n_in)
    rs = gpu.PfbArbResampler(rate, taps, nf)
    out, cons, prod, status = rs.filter(chans[0], rs.out_cap_for(n_in))
    assert (cons, prod, status) == (n_in, ref.shape[1], gpu.BOTH_SUFFICIENT)
    check(out[None, :], ref, bounds, 8, "fsdr_filter_host")
    many = gpu.PfbArbResampler(rate, taps, nf, 2)
    lib = gpu.lib()
    r = gpu._Result()
    rc = lib.fsdr_filter_dev(many._h, None, 0, None, 0, None,
                             ctypes.byref(r))
    assert rc == gpu.ERR_INVALID
    assert b"fsdr_pfb_arb_resampler_run_dev" in lib.fsdr_last_error()


def test_flowgraph_vector_source_arb_vector_sink(gpu):
    rate, nf, n_taps, n_in = 2.5, 5, 40, 700
    taps, chans, ref, bounds, _ = cached(rate, nf, n_taps, 1, n_in)
    fg = gpu.Flowgraph()
    src = fg.vector_source(chans[0])
    arb = fg.filter(gpu.PfbArbResampler(rate, taps, nf))
    snk = fg.vector_sink()
    fg.connect(src, arb, snk)
    fg.run()
    got = fg.sink_data(snk)
    assert fg.n_received(snk) == ref.shape[1]
    check(got[None, :], ref, bounds, 8, "flowgraph")


def test_channelizer_output_feeds_arb_resampler(gpu, oracle_lib):
    """The channelizer's device output buffer (channel-major, stride
    out_cap_per_chan) goes straight into the batched resampler at the
    LoRa shape (rate 2.5, 5 filters). The composition is held to the
    composed references in two links, each at its own bar: the
    channelizer's buffer against its oracle at the channelizer's bar
    (relative l2 1e-4), and the resampler's output against
    the restatement applied to that same buffer read back, at the bar of
    this file."""
    N, n_in, rate, nf = 8, 4096, 2.5, 5
    r = np.random.default_rng(79)
    ctaps = r.uniform(-1, 1, 64).astype(np.float32)
    rtaps, _ = random_case(rate, nf, 40, 1, 1)
    x = (r.uniform(-1, 1, (n_in, 2)) @ [1, 1j]).astype(np.complex64)
    lib = gpu.lib()
    chz = gpu.PfbChannelizer(N, ctaps)
    rs = gpu.PfbArbResampler(rate, rtaps, nf, N)
    cap = n_in // N + 5  # stride > produced
    out_cap = rs.out_cap_for(cap)
    d_x, d_mid, d_out = (ctypes.c_void_p() for _ in range(3))
    for d, items in ((d_x, n_in), (d_mid, N * cap), (d_out, N * out_cap)):
        assert lib.fsdr_dev_alloc(ctypes.byref(d), items * 8) == 0
    try:
        lib.fsdr_memcpy_h2d(d_x, ctypes.c_void_p(x.ctypes.data), n_in * 8)
        ppc = ctypes.c_size_t()
        assert lib.fsdr_pfb_channelizer_run_dev(
            chz._h, d_x, n_in, d_mid, cap, None, ctypes.byref(ppc)) == 0
        T = ppc.value
        assert 0 < T < cap
        cons, prod = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.fsdr_pfb_arb_resampler_run_dev(
            rs._h, d_mid, cap, T, d_out, out_cap, out_cap, None,
            ctypes.byref(cons), ctypes.byref(prod)) == 0, \
            lib.fsdr_last_error().decode()
        gpu.synchronize()
        mid = np.zeros(N * cap, np.complex64)
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(mid.ctypes.data), d_mid,
                            mid.size * 8)
        got = np.zeros(N * out_cap, np.complex64)
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(got.ctypes.data), d_out,
                            got.size * 8)
    finally:
        for d in (d_x, d_mid, d_out):
            lib.fsdr_dev_free(d)
    mid = mid.reshape(N, cap)[:, :T]
    cref = oracle_lib.pfb_channelizer(N, N, ctaps, x, max(1, n_in // N))
    assert cref.shape == mid.shape
    rel = np.linalg.norm(mid - cref) / np.linalg.norm(cref)
    print(f"channelizer link rel l2 {rel:.3e}")
    assert rel <= 1e-4
    ref, bounds, rcons, _ = oneshot(rate, nf, rtaps, mid, out_cap)
    assert (cons.value, prod.value) == (rcons, ref.shape[1])
    got = got.reshape(N, out_cap)[:, :prod.value]
    check(got, ref, bounds, 8, "channelizer -> arb hand-off")
