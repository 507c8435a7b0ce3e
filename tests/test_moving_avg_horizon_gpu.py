"""MovingAvg single-emission fast path: chunks older than the EMA's frame
horizon (weight exactly 0.0f) are skipped. The skip must not change a bit
of the emitted spectrum (FSDR_MOVAVG_SKIP=0 computes every chunk), and
the result still matches the oracle at the fast path's usual tolerance."""
import numpy as np
import pytest

from test_gpu_parity import assert_close, rng

pytestmark = pytest.mark.gpu

TOL = 1e-4  # test_moving_avg_single_emission_fast_path's tolerance
HORIZON_09 = 1053  # ceil(160 ln2 / -ln 0.9): frames that can weigh in

# (width, decay, frames): fast-path chunking is cf = 64 frames per chunk,
# capped at 1024 chunks (then cf grows).
CASES = [
    pytest.param(16, 0.1, 3000, id="w16-vec4-47chunks-30skipped"),
    pytest.param(6, 0.1, 3000, id="w6-scalar-branch"),
    pytest.param(4, 0.1, 70000, id="w4-chunk-cap-cf69"),
    pytest.param(16, 1e-4, 3000, id="long-horizon-nothing-skipped"),
    pytest.param(16, 1.0, 3000, id="om-zero-last-chunk-only"),
    pytest.param(6, 1.0, 3000, id="om-zero-scalar"),
]


def _input(seed, w, frames, plant):
    x = rng(seed).uniform(-1, 1, frames * w).astype(np.float32)
    if plant:
        bad = np.array([np.inf, np.nan, 3e38, -np.inf, -3e38], np.float32)
        r = rng(seed + 1)
        dead_frames = max(frames - 2 * HORIZON_09, 1)
        live_from = frames - min(frames, 150)
        dead = r.integers(0, dead_frames * w, 40)
        live = r.integers(live_from * w, frames * w, 12)
        x[dead] = bad[np.arange(dead.size) % bad.size]
        x[live] = bad[np.arange(live.size) % bad.size]
        # both sides of the skip boundary at decay 0.1: the last frames
        # before the horizon (last skipped chunk) and the first inside it
        edge = frames - HORIZON_09
        if edge > 70:
            near = r.integers((edge - 70) * w, (edge + 70) * w, 24)
            x[near] = bad[np.arange(near.size) % bad.size]
            x[(edge - 1) * w] = 3e38
            x[edge * w] = -3e38
        x[0] = np.nan          # first frame of the first (skipped) chunk
        x[-1] = np.inf         # last bin of the last frame
        x[-w] = 3e38           # first bin of the last frame
    return x


def _run(gpu, monkeypatch, skip, w, d, history, blocks):
    """One MovingAvg over `blocks` (one filter() call each); returns the
    list of (out, consumed, produced)."""
    if skip:
        monkeypatch.delenv("FSDR_MOVAVG_SKIP", raising=False)
    else:
        monkeypatch.setenv("FSDR_MOVAVG_SKIP", "0")
    f = gpu.MovingAvg(w, d, history)
    res = []
    for x in blocks:
        out, c, p, _ = f.filter(x, w)
        res.append((out.copy(), c, p))
    return res


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("plant", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("w,d,frames", CASES)
def test_horizon_skip_is_bit_exact(gpu, oracle_lib, monkeypatch, w, d,
                                   frames, plant):
    x = _input(frames + w, w, frames, plant)
    (got, c, p), = _run(gpu, monkeypatch, True, w, d, frames, [x])
    (full, c0, p0), = _run(gpu, monkeypatch, False, w, d, frames, [x])
    ref, co, po, _, _ = oracle_lib.moving_avg(w, d, frames, x, w)
    assert (c, p) == (co, po) == (c0, p0) and p == w
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(full))
    assert_close(got, ref, TOL)


@pytest.mark.parametrize("w", [16, 6], ids=["vec4", "scalar"])
def test_horizon_skip_state_carry(gpu, oracle_lib, monkeypatch, w):
    """history = 2*frames: the first call emits nothing and leaves only
    the avg state behind, the second call emits. The state written by a
    call that skipped chunks must carry."""
    d, frames = 0.1, 3000
    x1 = _input(71 + w, w, frames, True)
    x2 = _input(73 + w, w, frames, True)
    # the second block's own frames would hide the carried state (its
    # weight there is 0.9^3000 = 0); a third, short block keeps it visible
    x3 = _input(79 + w, w, 20, False)
    hist = 2 * frames
    a = _run(gpu, monkeypatch, True, w, d, hist, [x1, x2])
    b = _run(gpu, monkeypatch, False, w, d, hist, [x1, x2])
    assert a[0][1:] == b[0][1:] == (frames * w, 0)
    assert a[1][1:] == b[1][1:] == (frames * w, w)
    assert np.array_equal(_bits(a[1][0]), _bits(b[1][0]))
    _, _, po, avg, i = oracle_lib.moving_avg(w, d, hist, x1, w)
    assert po == 0
    ref, _, _, _, _ = oracle_lib.moving_avg(w, d, hist, x2, w, avg=avg,
                                            i_state=i)
    assert_close(a[1][0], ref, TOL)

    # short history after a long skipped call: avg from call 1 weighs in
    hist = frames + 20
    a = _run(gpu, monkeypatch, True, w, d, hist, [x1, x3])
    b = _run(gpu, monkeypatch, False, w, d, hist, [x1, x3])
    assert a[0][2] == b[0][2] == 0 and a[1][2] == b[1][2] == w
    assert np.array_equal(_bits(a[1][0]), _bits(b[1][0]))
    _, _, _, avg, i = oracle_lib.moving_avg(w, d, hist, x1, w)
    ref, _, _, _, _ = oracle_lib.moving_avg(w, d, hist, x3, w, avg=avg,
                                            i_state=i)
    assert_close(a[1][0], ref, TOL)
    assert float(np.abs(ref).max()) > 0.0
