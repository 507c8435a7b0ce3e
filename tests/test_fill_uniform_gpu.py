"""k_fill_uniform_cf32 against a restatement of its counter-based stream.

The fill is a function of (seed, offset, element index) alone, so numpy
can restate it exactly: integer hashes, then (r >> 8) * 2^-23 - 1, which
is exact in float32. The kernel launches at most 8192 * 256 threads and
strides beyond; a thread stores two pairs per iteration, a grid stride
apart, and one more if a single pair is left. The lengths put the end of
the buffer in each of those places: no full stride (tail store only), a
few pairs past one stride (the two-pair loop runs for a few threads and
the others take the tail), a few past two strides (the loop, then the tail
for a few), each with an odd length, whose last sample comes from another
hash, and once from a nonzero, odd offset.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDE = 8192 * 256  # pairs per grid stride (grid_for's cap x block)
M32 = np.uint64(0xFFFFFFFF)


def lowbias32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def to_unit(r):
    return ((r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23)
            - np.float32(1.0))


def reference(n, seed, offset):
    out = np.zeros(2 * n, np.float32)
    sm = np.uint32(((seed & 0xFFFFFFFF) * 0x9E3779B9 & 0xFFFFFFFF)
                   ^ (seed >> 32))
    i = np.arange(0, n - (n & 1), 2, dtype=np.uint64)
    c64 = np.uint64(0x5D5D5D5D + offset) + i
    c = (c64 & M32).astype(np.uint32) ^ (
        (c64 >> np.uint64(32)).astype(np.uint32) * np.uint32(0x85EBCA6B))
    for k in range(4):
        out[k:4 * i.size:4] = to_unit(
            lowbias32(c * np.uint32(4) + np.uint32(k) + sm))
    if n & 1:
        h = splitmix64(seed ^ ((0x5D5D5D5D + offset + n - 1)
                               & ((1 << 64) - 1)))
        out[-2:] = to_unit(np.array([h & 0xFFFFFFFF, h >> 32], np.uint32))
    return out


@pytest.mark.parametrize("n,seed,offset", [
    (1, 7, 0), (2, 7, 0), (1001, 123, 0),
    (2 * STRIDE + 10, 1000, 0), (2 * STRIDE + 11, 1000, 0),
    (4 * STRIDE + 6, 0x1234567800000005, 0),
    (4 * STRIDE + 7, 7, (1 << 32) - 3),
])
def test_fill_matches_restated_stream(gpu, n, seed, offset):
    with np.errstate(over="ignore"):
        want = reference(n, seed, offset)
    lib = gpu.lib()
    ptr = ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(ptr), n * 8 + 64) == 0
    try:
        guard = np.full(2 * n + 16, np.nan, np.float32)
        lib.fsdr_memcpy_h2d(ptr, ctypes.c_void_p(guard.ctypes.data),
                            guard.nbytes)
        gpu.fill_uniform_dev(ptr.value, n, seed=seed, offset=offset)
        gpu.synchronize()
        got = np.zeros(2 * n + 16, np.float32)
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(got.ctypes.data), ptr,
                            got.nbytes)
    finally:
        lib.fsdr_dev_free(ptr)
    np.testing.assert_array_equal(got[:2 * n], want)
    assert np.isnan(got[2 * n:]).all(), "stored past the end"
