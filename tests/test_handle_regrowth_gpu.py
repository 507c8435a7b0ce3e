"""A live handle's device buffers grow between calls and the results stay
right: the host-path staging buffers of a Fir, and the chunk-partials
scratch of MovingAvg's fast path. Tolerances are the ones
test_gpu_parity.py uses for the same blocks.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def assert_close(got, ref, tol):
    ref = np.asarray(ref)
    got = np.asarray(got)
    assert got.shape == ref.shape
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= tol * scale, f"max err {err} > {tol}*{scale}"


def test_fir_staging_grows_and_is_kept(gpu, oracle_lib):
    """filter() stages n_in and n_out items on the device: 64, then 4096
    (both buffers are replaced), then 64 again (the large ones are kept)."""
    r = np.random.default_rng(5)
    taps = r.uniform(-1, 1, 5).astype(np.float32)
    f = gpu.Fir(taps)
    for n_in in (64, 4096, 64):
        x = (r.uniform(-1, 1, (n_in, 2)) @ [1, 1j]).astype(np.complex64)
        got, c, p, s = f.filter(x, n_in)
        ref, co, po, so = oracle_lib.fir_cf32(taps, x, n_in)
        assert (c, p, s) == (co, po, so)
        assert_close(got, ref, 1e-5)


def test_moving_avg_partials_grow(gpu, oracle_lib):
    """The chunked fast path keeps one partial per 64-frame chunk and
    channel: 64 frames need one chunk, the 4096 that follow need 64, so
    the scratch is replaced between the calls; a 64-frame call after that
    fits the larger one. The second call ends on the emission."""
    r = np.random.default_rng(6)
    w, d, history = 4, 0.1, 64 + 4096
    f = gpu.MovingAvg(w, d, history)
    avg, i = None, 0
    for frames, emitted in ((64, 0), (4096, 1), (64, 0)):
        x = r.uniform(-1, 1, frames * w).astype(np.float32)
        got, c, p, s = f.filter(x, w)
        ref, co, po, avg, i = oracle_lib.moving_avg(w, d, history, x, w,
                                                    avg=avg, i_state=i)
        assert (c, p) == (co, po) == (frames * w, emitted * w)
        assert_close(got[:p], ref[:po], 1e-4)
    # the state after the last, non-emitting call: flush it with the rest
    # of the history and compare the emission
    x = r.uniform(-1, 1, (history - 64) * w).astype(np.float32)
    got, c, p, s = f.filter(x, w)
    ref, co, po, avg, i = oracle_lib.moving_avg(w, d, history, x, w, avg=avg,
                                                i_state=i)
    assert (c, p) == (co, po) == ((history - 64) * w, w)
    assert_close(got[:p], ref[:po], 1e-4)
