"""Host-side planning of the MovingAvg call (no GPU): the closed-form
frame accounting against the literal work() loop, and the fast path's
first live chunk against the horizon formula, worked out here
independently."""
import ctypes
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib(fsdr):
    lib = fsdr.lib()
    sz, psz = ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)
    lib.fsdr_moving_avg_count.argtypes = [sz, sz, sz, psz, psz, psz]
    lib.fsdr_moving_avg_count.restype = None
    pint = ctypes.POINTER(ctypes.c_int)
    lib.fsdr_moving_avg_plan.argtypes = [sz, ctypes.c_float, ctypes.c_int,
                                         pint, pint]
    lib.fsdr_moving_avg_plan.restype = ctypes.c_int
    return lib


def _count(lib, n_in, n_out, history, i):
    ist, cons, prod = (ctypes.c_size_t(i), ctypes.c_size_t(99),
                       ctypes.c_size_t(99))
    lib.fsdr_moving_avg_count(n_in, n_out, history, ctypes.byref(ist),
                              ctypes.byref(cons), ctypes.byref(prod))
    return cons.value, prod.value, ist.value


def _count_loop(n_in, n_out, history, i):
    """moving_avg.rs work(): consume a frame, emit every history-th."""
    cons = prod = 0
    while cons < n_in and prod < n_out:
        i += 1
        if i == history:
            i = 0
            prod += 1
        cons += 1
    return cons, prod, i


def test_count_matches_loop_exhaustive_small(lib):
    for history in range(1, 8):
        for i in range(history):
            for n_in in range(0, 25):
                for n_out in range(0, 5):
                    assert _count(lib, n_in, n_out, history, i) == \
                        _count_loop(n_in, n_out, history, i), \
                        (n_in, n_out, history, i)


def test_count_matches_loop_random(lib):
    r = np.random.default_rng(20)
    for _ in range(300):
        history = int(r.integers(1, 5000))
        i = int(r.integers(0, history))
        n_in = int(r.integers(0, 20000))
        n_out = int(r.integers(0, 8))
        assert _count(lib, n_in, n_out, history, i) == \
            _count_loop(n_in, n_out, history, i), (n_in, n_out, history, i)


def test_count_bench_shape_and_saturation(lib):
    assert _count(lib, 262143, 1, 262143, 0) == (262143, 1, 0)
    big = 2 ** 64 - 1
    # first emission after big-5 frames, then 5 more frames consumed
    assert _count(lib, big, big, big, 5) == (big, 1, 5)


def _plan(lib, frames, decay, skip=1):
    cf, nch = ctypes.c_int(), ctypes.c_int()
    c0 = lib.fsdr_moving_avg_plan(frames, decay, skip, ctypes.byref(cf),
                                  ctypes.byref(nch))
    return c0, cf.value, nch.value


def _horizon(decay):
    """Smallest H with |om|^H < 2^-160, om = 1 - decay formed in float32;
    None when there is none."""
    om = abs(float(np.float32(1.0) - np.float32(decay)))
    if om == 0.0:
        return 1
    if om >= 1.0:
        return None
    return math.ceil(160.0 * math.log(2.0) / -math.log(om))


@pytest.mark.parametrize("decay", [0.1, 0.5, 1e-2, 1e-4, 0.999, 1.0, 0.0])
@pytest.mark.parametrize("frames", [1, 63, 64, 65, 1052, 1053, 1054, 1116,
                                    1117, 1118, 3000, 65536, 65537, 70000,
                                    262143])
def test_plan_first_live_chunk(lib, frames, decay):
    c0, cf, nch = _plan(lib, frames, decay)
    assert cf >= 64 and 1 <= nch <= 1024 and nch * cf >= frames
    assert _plan(lib, frames, decay, skip=0) == (0, cf, nch)
    h = _horizon(decay)

    def age(c):  # frames between the end of chunk c and the emission
        return frames - min((c + 1) * cf, frames)

    if h is None:
        assert c0 == 0
        return
    # the weight the device gives a chunk of age h is exactly zero
    om = np.float32(1.0) - np.float32(decay)
    assert np.power(om, np.float32(h), dtype=np.float32) == 0.0
    assert 0 <= c0 <= nch - 1
    assert age(c0) < h                   # c0 is inside the horizon
    assert c0 == 0 or age(c0 - 1) >= h   # and the chunk before it is not


def test_plan_bench_shape(lib):
    # 262143 frames, decay 0.1: cf 256, 1024 chunks, H = 1053 -> 5 live
    assert _plan(lib, 262143, 0.1) == (1019, 256, 1024)
    assert _plan(lib, 3000, 0.1) == (30, 64, 47)
    assert _plan(lib, 3000, 1.0) == (46, 64, 47)
