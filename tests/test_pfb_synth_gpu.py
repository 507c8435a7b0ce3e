"""PFB synthesizer on the GPU against the literal float64 restatement of
synthesizer.rs (tests/pfb_synth_ref.py). Bar: relative l2 <= 1e-4, the
FFT bar of DESIGN.md (c) — the op contains an N-point transform; shapes
and consumed/produced must match exactly. Every case runs on both kernel
paths (FSDR_PFB_SYNTH_FUSED is read at call time)."""
import ctypes

import numpy as np
import pytest

from pfb_synth_ref import (PfbSynthesizerRef, cached_oneshot, random_case,
                           synth_oneshot, tone_energy_fraction,
                           tone_prototype)

pytestmark = pytest.mark.gpu

BAR = 1e-4


@pytest.fixture(params=["1", "0"], ids=["fused", "staged"])
def path(request, monkeypatch):
    monkeypatch.setenv("FSDR_PFB_SYNTH_FUSED", request.param)
    return request.param


def rel_l2(got, ref):
    ref = np.asarray(ref, np.complex128)
    got = np.asarray(got, np.complex128)
    assert got.shape == ref.shape
    if ref.size == 0:
        return 0.0
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def check(got, ref, what=""):
    err = rel_l2(got, ref)
    print(f"{what} rel l2 {err:.3e}")
    assert err <= BAR, f"{what} rel l2 {err} > {BAR}"


def run_dev(gpu, syn, buf, stride, n, out_cap, fn="run"):
    """Raw run_dev/stream_dev over a host copy `buf` of N*stride items."""
    lib = gpu.lib()
    call = getattr(lib, f"fsdr_pfb_synthesizer_{fn}_dev")
    buf = np.ascontiguousarray(buf, np.complex64)
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(d_in), buf.size * 8 + 8) == 0
    assert lib.fsdr_dev_alloc(ctypes.byref(d_out), out_cap * 8 + 8) == 0
    try:
        lib.fsdr_memcpy_h2d(d_in, ctypes.c_void_p(buf.ctypes.data),
                            buf.size * 8)
        cons, prod = ctypes.c_size_t(), ctypes.c_size_t()
        rc = call(syn._h, d_in, stride, n, d_out, out_cap, None,
                  ctypes.byref(cons), ctypes.byref(prod))
        assert rc == 0, lib.fsdr_last_error().decode()
        gpu.synchronize()
        out = np.zeros(prod.value, np.complex64)
        if prod.value:
            lib.fsdr_memcpy_d2h(ctypes.c_void_p(out.ctypes.data), d_out,
                                prod.value * 8)
        return out, cons.value
    finally:
        lib.fsdr_dev_free(d_in)
        lib.fsdr_dev_free(d_out)


# ---------------- bulk parity -------------------------------------------

BULK = [
    (4, 4, 9),         # tpf = 1, no history
    (4, 37, 50),       # zero-padded partition
    (8, 64, 200),      # radix-2 tail
    (64, 512, 100),
    (1024, 4096, 40),  # largest fused shape
    (2048, 4096, 12),  # staged fallback
]


@pytest.mark.parametrize("N,n_taps,T", BULK)
def test_bulk_parity(gpu, path, N, n_taps, T):
    taps, chans, ref, ref_cons = cached_oneshot(N, n_taps, T)
    fusable = gpu.pfb_synthesizer_run_length(N, -(-n_taps // N)) > 0
    assert fusable == (N <= 1024)
    syn = gpu.PfbSynthesizer(N, taps)
    assert syn.length == n_taps
    got, cons = syn.run(chans)
    assert cons == ref_cons and got.size == ref.size
    check(got, ref, f"bulk N={N} taps={n_taps} T={T} {path}")


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("N,n_taps", [(8, 64), (64, 512)])
def test_bulk_parity_around_run_length(gpu, path, N, n_taps, delta):
    """T one below, at and one above the steps one block of the fused
    kernel owns (queried, not copied), so the last block is one step
    short, exactly full, and a second block gets a single step."""
    R = gpu.pfb_synthesizer_run_length(N, n_taps // N)
    assert R > 0
    T = R + delta
    taps, chans, ref, ref_cons = cached_oneshot(N, n_taps, T)
    got, cons = gpu.PfbSynthesizer(N, taps).run(chans)
    assert cons == ref_cons and got.size == ref.size
    check(got, ref, f"run-length N={N} T={T} {path}")


def test_bulk_in_stride_larger_than_t(gpu, path):
    N, n_taps, T, stride = 8, 64, 200, 237
    taps, chans, ref, ref_cons = cached_oneshot(N, n_taps, T)
    buf = np.full((N, stride), 1e6 + 1e6j, np.complex64)  # poison the gap
    buf[:, :T] = chans
    got, cons = run_dev(gpu, gpu.PfbSynthesizer(N, taps), buf, stride, T,
                        (T + 1) * N)
    assert cons == ref_cons and got.size == ref.size
    check(got, ref, f"in_stride {path}")


@pytest.mark.parametrize("N,n_taps,T,out_cap", [
    (8, 64, 200, 8 * 57 + 3), (64, 512, 100, 64 * 30)])
def test_bulk_out_cap_limits_production(gpu, path, N, n_taps, T, out_cap):
    taps, chans = random_case(N, n_taps, T)
    ref, ref_cons = synth_oneshot(N, taps, chans, out_cap)
    assert 0 < ref_cons < T  # production stops mid-input
    got, cons = gpu.PfbSynthesizer(N, taps).run(chans, out_cap)
    assert cons == ref_cons and got.size == ref.size
    assert (cons, got.size) == gpu.pfb_synthesizer_count(
        N, n_taps // N, 0, T, out_cap)
    check(got, ref, f"out_cap {path}")


def test_run_leaves_streaming_state_alone(gpu, path):
    """run() between two stream() calls does not disturb the stream."""
    N, n_taps, T = 8, 64, 60
    taps, chans, ref, _ = cached_oneshot(N, n_taps, T)
    syn = gpu.PfbSynthesizer(N, taps)
    a, ca = syn.stream(chans[:, :25])
    syn.run(chans[:, :40])
    b, cb = syn.stream(chans[:, 25:])
    assert (ca, cb) == (25, T - 25)
    check(np.concatenate([a, b]), ref, f"run-between-streams {path}")


# ---------------- streaming ---------------------------------------------

@pytest.mark.parametrize("N,n_taps", [(8, 64), (64, 300)])
def test_streaming_random_chunks(gpu, path, N, n_taps):
    """Random chunk sizes in [0, 40] steps (0 and 1 forced first) and a
    random out_cap per call; the caller re-presents the unconsumed tail.
    The concatenation equals the one-shot restatement and every call's
    consumed/produced equals fsdr_pfb_synthesizer_count."""
    T = 400
    tpf = -(-n_taps // N)
    taps, chans, ref, _ = cached_oneshot(N, n_taps, T)
    r = np.random.default_rng(N + n_taps)
    syn = gpu.PfbSynthesizer(N, taps)
    outs, off, pushes = [], 0, 0
    leftover = np.zeros((N, 0), np.complex64)
    forced = [0, 1, 0, 1, 3]
    for it in range(400):
        if off >= T and leftover.shape[1] == 0:
            break
        take = forced[it] if it < len(forced) else int(r.integers(0, 41))
        buf = np.concatenate([leftover, chans[:, off:off + take]], axis=1)
        off = min(T, off + take)
        out_cap = int(r.integers(N, 45 * N))
        out, cons = syn.stream(buf, out_cap)
        assert (cons, out.size) == gpu.pfb_synthesizer_count(
            N, tpf, pushes, buf.shape[1], out_cap), (it, pushes)
        pushes += cons
        outs.append(out)
        leftover = buf[:, cons:]
    assert pushes == T
    check(np.concatenate(outs), ref, f"stream N={N} taps={n_taps} {path}")


def test_streaming_call_ends_on_filling_step(gpu, path):
    """Calls that end one before, exactly on and one past the filling
    step (global step tpf-1), then the rest."""
    N, n_taps, T = 8, 64, 60
    tpf = n_taps // N
    taps, chans, ref, _ = cached_oneshot(N, n_taps, T)
    for first in (tpf - 2, tpf - 1, tpf, tpf + 1):
        syn = gpu.PfbSynthesizer(N, taps)
        a, ca = syn.stream(chans[:, :first])
        b, cb = syn.stream(chans[:, first:])
        assert (ca, cb) == (first, T - first)
        assert a.size == max(0, first - (tpf - 1)) * N
        check(np.concatenate([a, b]), ref, f"fill-step first={first} {path}")


# ---------------- tone placement ----------------------------------------

@pytest.mark.parametrize("m", [0, 3, 9, 15])
def test_tone_placement(gpu, path, m):
    """A constant on channel m alone comes out as a tone in bin
    2048*m/16 holding > 0.95 of the energy (the channelizer tone test's
    threshold; the float64 restatement gives > 0.99)."""
    N, tpf = 16, 8
    taps = tone_prototype(N, N * tpf)
    T = tpf - 1 + tpf + 2048 // N
    x = np.zeros((N, T), np.complex64)
    x[m] = 1.0
    out, cons = gpu.PfbSynthesizer(N, taps).run(x)
    assert cons == T
    peak, frac, want = tone_energy_fraction(out, N, tpf, m)
    print(f"tone m={m} peak {peak} frac {frac:.5f} {path}")
    assert peak == want
    assert frac > 0.95


# ---------------- device-resident hand-off ------------------------------

def test_channelizer_output_feeds_synthesizer(gpu, path):
    """The channelizer's device output buffer (channel-major, stride
    out_cap_per_chan) goes straight into run_dev; the result equals the
    restatement applied to the same channelizer output read back."""
    N, n_taps, n_in = 8, 64, 4096
    r = np.random.default_rng(77)
    taps = r.uniform(-1, 1, n_taps).astype(np.float32)
    x = (r.uniform(-1, 1, (n_in, 2)) @ [1, 1j]).astype(np.complex64)
    lib = gpu.lib()
    chz = gpu.PfbChannelizer(N, taps)
    syn = gpu.PfbSynthesizer(N, taps)
    cap = n_in // N + 5  # stride > produced
    d_x, d_mid, d_out = (ctypes.c_void_p() for _ in range(3))
    out_cap = (cap + 1) * N
    for d, items in ((d_x, n_in), (d_mid, N * cap), (d_out, out_cap)):
        assert lib.fsdr_dev_alloc(ctypes.byref(d), items * 8) == 0
    try:
        lib.fsdr_memcpy_h2d(d_x, ctypes.c_void_p(x.ctypes.data), n_in * 8)
        ppc = ctypes.c_size_t()
        assert lib.fsdr_pfb_channelizer_run_dev(
            chz._h, d_x, n_in, d_mid, cap, None, ctypes.byref(ppc)) == 0
        T = ppc.value
        assert 0 < T < cap
        cons, prod = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.fsdr_pfb_synthesizer_run_dev(
            syn._h, d_mid, cap, T, d_out, out_cap, None,
            ctypes.byref(cons), ctypes.byref(prod)) == 0, \
            lib.fsdr_last_error().decode()
        gpu.synchronize()
        mid = np.zeros(N * cap, np.complex64)
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(mid.ctypes.data), d_mid,
                            mid.size * 8)
        got = np.zeros(prod.value, np.complex64)
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(got.ctypes.data), d_out,
                            got.size * 8)
    finally:
        for d in (d_x, d_mid, d_out):
            lib.fsdr_dev_free(d)
    ref, ref_cons = synth_oneshot(N, taps, mid.reshape(N, cap)[:, :T])
    assert cons.value == ref_cons and got.size == ref.size
    check(got, ref, f"hand-off {path}")


def test_generic_entry_points_refuse(gpu):
    syn = gpu.PfbSynthesizer(8, np.ones(16, np.float32))
    with pytest.raises(gpu.FsdrError, match="fsdr_pfb_synthesizer_run_dev"):
        syn.filter(np.zeros(64, np.complex64), 64)
