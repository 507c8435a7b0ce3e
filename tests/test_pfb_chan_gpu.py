"""PFB channelizer on the GPU against the literal float64 restatement of
channelizer.rs (tests/pfb_chan_ref.py), per output step and from step 0.

Bound: relative l2 of a step's N-vector at most 1e-4, the project's FFT
figure; the tpf-term f32 dots add about tpf * 2^-24. A
wrong source sample or a missed hole is O(1/sqrt(tpf)) on the loud random
inputs used here. Each case covers the fill, every start-up step and a few
steady ones, and prints its worst step as `PCH <case> <figure>`.

Streaming output is compared bit for bit with the bulk entry on the same
stream: both go through pfb_chan_dots -> launch_fft -> k_pfb_scatter, whose
per-output arithmetic does not depend on how the steps are split into
launches."""
import ctypes

import numpy as np
import pytest

from pfb_chan_ref import PfbChannelizerRef, cached_oneshot, startup_steps

pytestmark = pytest.mark.gpu

BOUND = 1e-4
FLOOR = 1e-2  # a step's reference norm, before dividing by it

# (N, n_taps, D, steady steps after the start-up ones)
BULK = [(4, 4, 4, 8),            # tpf = 1: no start-up steps
        (4, 16, 4, 8),
        (4, 20, 4, 8),           # odd tpf
        (4, 37, 4, 8),           # padded taps
        (8, 64, 8, 8), (8, 64, 4, 8), (8, 64, 2, 8),
        (4, 12, 1, 8),           # D = 1
        (64, 64 * 3 + 5, 64, 8), (64, 256, 16, 8),
        (1024, 2048, 1024, 3), (4096, 8192, 4096, 3)]  # large-N IFFT
STREAM = [(8, 64, 8), (8, 64, 2), (4, 20, 4), (4, 12, 1)]


def _id(s):
    return "-".join(str(v) for v in s[:3])


def step_figures(got, ref):
    """Relative l2 of every output step's N-vector."""
    assert got.shape == ref.shape
    nrm = np.linalg.norm(ref, axis=0)
    assert nrm.size == 0 or nrm.min() > FLOOR
    return np.linalg.norm(got.astype(np.complex128) - ref, axis=0) / nrm


def check_steps(got, ref, label):
    fig = step_figures(got, ref)
    worst = float(fig.max()) if fig.size else 0.0
    print(f"PCH {label} {worst:.3e}")
    assert worst <= BOUND, (label, int(fig.argmax()), worst)


def textbook(N, taps, D, x, steps):
    """Every step as the steady-state polyphase sum
    fft_buf[b] = sum_j x[pmax(b) - jN] * part[i(b)][j], in float64: what a
    clean shift-register window gives, right from step tpf*N/D - 1 on."""
    tpf = -(-len(taps) // N)
    part = np.zeros(N * tpf)
    part[:len(taps)] = taps
    part = part.reshape(tpf, N).T  # part[i][j] = taps[i + j*N]
    xx = np.asarray(x, np.complex128)
    b = np.arange(N)
    out = np.zeros((N, steps), np.complex128)
    for k in range(steps):
        P = N * tpf + (k + 1) * D
        base = (N - 1 - P) % N
        i = (b - base - 1) % N
        pmax = P - 1 - ((P - 1 - (N - 1 - b)) % N)
        idx = pmax[:, None] - np.arange(tpf)[None, :] * N
        out[:, k] = np.fft.ifft((xx[idx] * part[i]).sum(axis=1)) * N
    return out


class Dev:
    """One raw-ABI call on a pre-poisoned output buffer of N*cap + guard
    slots; returns (out[N, produced], consumed, buffer after, poison)."""
    GUARD = 64

    def __init__(self, gpu):
        self.gpu, self.lib = gpu, gpu.lib()

    def call(self, chz, x, cap, stream=False, seed=1):
        lib, N = self.lib, chz.n
        x = np.ascontiguousarray(x, np.complex64)
        slots = N * cap + self.GUARD
        poison = np.random.default_rng(seed).integers(
            1, 2 ** 63, slots, dtype=np.uint64)
        d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
        assert lib.fsdr_dev_alloc(ctypes.byref(d_in), x.size * 8 + 8) == 0
        assert lib.fsdr_dev_alloc(ctypes.byref(d_out), slots * 8) == 0
        try:
            if x.size:
                lib.fsdr_memcpy_h2d(d_in, ctypes.c_void_p(x.ctypes.data),
                                    x.size * 8)
            lib.fsdr_memcpy_h2d(d_out, ctypes.c_void_p(poison.ctypes.data),
                                slots * 8)
            prod, cons = ctypes.c_size_t(), ctypes.c_size_t(x.size)
            if stream:
                rc = lib.fsdr_pfb_channelizer_stream_dev(
                    chz._h, d_in, x.size, d_out, cap, None,
                    ctypes.byref(prod), ctypes.byref(cons))
            else:
                rc = lib.fsdr_pfb_channelizer_run_dev(
                    chz._h, d_in, x.size, d_out, cap, None,
                    ctypes.byref(prod))
            assert rc == 0, lib.fsdr_last_error().decode()
            self.gpu.synchronize()
            after = np.zeros(slots, np.uint64)
            lib.fsdr_memcpy_d2h(ctypes.c_void_p(after.ctypes.data), d_out,
                                slots * 8)
        finally:
            lib.fsdr_dev_free(d_in)
            lib.fsdr_dev_free(d_out)
        p = prod.value
        assert p <= cap
        body = after[:N * cap].reshape(N, cap)
        keep = poison[:N * cap].reshape(N, cap)
        # every slot outside [c*cap, c*cap + produced) is as it was
        assert np.array_equal(body[:, p:], keep[:, p:])
        assert np.array_equal(after[N * cap:], poison[N * cap:])
        out = np.ascontiguousarray(body[:, :p]).view(np.complex64)
        return out.reshape(N, p), cons.value


def _chz(gpu, N, taps, D):
    return gpu.PfbChannelizer(N, taps, oversample_rate=N / D)


# ---------------- bulk ---------------------------------------------------

@pytest.mark.parametrize("shape", BULK, ids=_id)
def test_bulk_matches_restatement(gpu, shape):
    """Every step, the start-up ones included, against the restatement;
    the start-up steps are NOT the textbook sum (a kernel reading a clean
    shift-register window fails here) and the first steady step is."""
    N, n_taps, D, steady = shape
    taps, x, ref, cons = cached_oneshot(N, n_taps, D, steady)
    n_start = startup_steps(N, n_taps, D)
    assert cons == x.size and ref.shape[1] == n_start + steady
    got = _chz(gpu, N, taps, D).run(x)
    check_steps(got, ref, f"bulk-{_id(shape)}")
    text = textbook(N, taps, D, x, n_start + 1)
    fig = step_figures(got[:, :n_start + 1], text)
    if n_start:
        assert fig[:n_start].min() > 1e-3, (int(fig[:n_start].argmin()),
                                            float(fig[:n_start].min()))
    assert fig[n_start] <= BOUND


@pytest.mark.parametrize("shape", [(8, 64, 4, 8), (4, 20, 4, 8),
                                   (64, 256, 16, 8)], ids=_id)
def test_bulk_fill_boundary_and_out_cap(gpu, shape):
    """n_in = N*tpf, N*tpf + D - 1, N*tpf + D produce 0, 0, 1 steps; an
    out_cap below and above the available steps; nothing else in the
    poisoned buffer changes (checked inside Dev.call)."""
    N, n_taps, D, steady = shape
    taps, x, ref, _ = cached_oneshot(N, n_taps, D, steady)
    tpf = -(-n_taps // N)
    dev, chz = Dev(gpu), _chz(gpu, N, taps, D)
    worst = 0.0
    for n_in, want in ((N * tpf, 0), (N * tpf + D - 1, 0), (N * tpf + D, 1),
                       (N * tpf - 1, 0), (0, 0)):
        got, _ = dev.call(chz, x[:n_in], 5, seed=n_in + 1)
        assert got.shape[1] == want, n_in
        if want:
            worst = max(worst, step_figures(got, ref[:, :want]).max())
    total = ref.shape[1]
    for cap in (1, 3, total - 1, total, total + 7):
        got, _ = dev.call(chz, x, cap, seed=cap)
        assert got.shape[1] == min(cap, total), cap
        worst = max(worst, step_figures(got, ref[:, :got.shape[1]]).max())
    print(f"PCH edge-{_id(shape)} {worst:.3e}")
    assert worst <= BOUND
    # the wrapper's out_cap argument
    assert chz.run(x, out_cap=2).shape == (N, 2)


# ---------------- streaming ----------------------------------------------

def _plans(N, tpf, D, n_total, r):
    """name -> list of (new samples, out_cap or None); the driver repeats
    the last entry until the stream is used up."""
    W = N * tpf
    small = max(1, D - 1)
    return {
        # one sample at a time through the fill and two start-up steps
        "ones": [(1, None)] * (W + 2 * D) + [(n_total, None)],
        # ends inside the fill, exactly at its end, inside the start-up
        # span (leaving a remainder), then the rest
        "edges": [(W - 3, None), (3, None), (D + 1, None), (n_total, None)],
        # chunks smaller than D (D = 1: single samples)
        "small": [(small, None)] * ((W + 4 * D) // small + 1)
        + [(n_total, None)],
        "random": [(int(v), None) for v in r.integers(1, 3 * W + 1, 64)],
        # the capped branch decides consumed
        "cap1": [(3 * D + 1, 1)],
        "cap3": [(5 * D + 2, 3)],
    }


def _drive(dev, chz, ref, x, plan, D):
    """Feed x through chz.stream_dev by `plan`, re-presenting what a call
    leaves; every call's (consumed, produced) must equal the restatement's
    work() sequence, its fill call and first producing call folded into
    one. Returns the concatenated output."""
    N = chz.n
    cols, left, off = [np.zeros((N, 0), np.complex64)], x[:0], 0
    for call in range(4000):
        take, cap = plan[min(call, len(plan) - 1)]
        buf = np.concatenate([left, x[off:off + take]])
        off = min(off + take, x.size)
        if cap is None:
            cap = buf.size // D + 1
        was_filled = ref.all_windows_filled
        want, want_cons = ref.work(buf, cap)
        if ref.all_windows_filled and not was_filled:
            want, more = ref.work(buf[want_cons:], cap)
            want_cons += more
        got, cons = dev.call(chz, buf, cap, stream=True, seed=call + 1)
        assert (cons, got.shape[1]) == (want_cons, want.shape[1]), call
        cols.append(got)
        left = buf[cons:]
        if off >= x.size and got.shape[1] == 0 and left.size < D:
            return np.concatenate(cols, axis=1)
    pytest.fail("stream did not drain")


@pytest.mark.parametrize("plan", ["ones", "edges", "small", "random",
                                  "cap1", "cap3"])
@pytest.mark.parametrize("shape", STREAM, ids=_id)
def test_stream_matches_restatement_and_bulk_bits(gpu, shape, plan):
    N, n_taps, D = shape
    taps, x, ref_out, _ = cached_oneshot(N, n_taps, D, 8)
    tpf = -(-n_taps // N)
    r = np.random.default_rng([N, n_taps, D, 5])
    chz = _chz(gpu, N, taps, D)
    bulk = chz.run(x)
    got = _drive(Dev(gpu), _chz(gpu, N, taps, D),
                 PfbChannelizerRef(N, taps, N / D), x,
                 _plans(N, tpf, D, x.size, r)[plan], D)
    assert got.shape == bulk.shape == ref_out.shape
    check_steps(got, ref_out, f"stream-{plan}-{_id(shape)}")
    assert np.array_equal(got.view(np.uint32), bulk.view(np.uint32))


def test_stream_state_is_per_handle(gpu):
    """A long stream on one handle, then a fresh handle from zero (its
    start-up steps again), then the first handle goes on where it was."""
    N, n_taps, D = 8, 64, 2
    taps, x, ref_out, _ = cached_oneshot(N, n_taps, D, 8)
    r = np.random.default_rng(77)
    from dsp_ref import loud_c64
    long_x = loud_c64(r, 40 * N * 8 + 3)
    a, b = _chz(gpu, N, taps, D), _chz(gpu, N, taps, D)
    whole = a.run(long_x)
    cut = 2500
    a1, c1 = a.stream(long_x[:cut])
    got_b, cb = b.stream(x)
    a2, c2 = a.stream(long_x[c1:])
    assert cb == x.size and c1 + c2 == long_x.size - (long_x.size % D)
    check_steps(got_b, ref_out, "stream-fresh-handle")
    assert np.array_equal(got_b.view(np.uint32),
                          b.run(x).view(np.uint32))
    got_a = np.concatenate([a1, a2], axis=1)
    assert np.array_equal(got_a.view(np.uint32), whole.view(np.uint32))
    # the wrapper's out_cap argument on the streaming entry
    out, cons = _chz(gpu, N, taps, D).stream(x, out_cap=2)
    assert out.shape == (N, 2) and cons == N * 8 + 2 * D
