"""PFB channelizer, host side (no GPU): the closed form of the start-up
windows (what the product's start-up kernel and its exported map use)
pinned against the literal WindowBuffer, the literal restatement pinned on
its own, and the oracle against the restatement from output step 0."""
import numpy as np
import pytest

from pfb_chan_ref import PfbChannelizerRef, chan_oneshot, startup_steps
from pfb_synth_ref import WindowBuffer, partition_filter_taps

# (N, n_taps, D): the shapes the start-up defect was measured on, the
# last one (tpf = 1) having no start-up steps
TABLE = [(4, 16, 4), (4, 20, 4), (8, 64, 8), (8, 64, 4), (8, 64, 2),
         (4, 37, 4), (4, 12, 1), (8, 8, 8)]
EXTRA = [(4, 9, 2), (8, 17, 1)]


def window_src(L, q, w):
    """Push ordinal (0 = first fill push) that slice position w, 0 =
    oldest, of a window holds after L fill pushes and q more; -1 = hole."""
    if q >= L:
        return q + w
    x = (q + w) % L
    if x < q:
        return L + x
    if (x + L) % 2 == 0:
        return (x + L) // 2
    if x % 2 == 0:
        return x // 2
    return -1


def _case(N, n_taps, D, steady=6, seed=11):
    r = np.random.default_rng([seed, N, n_taps, D])
    tpf = -(-n_taps // N)
    steps = tpf * N // D - 1 + steady
    taps = r.uniform(-1, 1, n_taps)
    n = N * tpf + steps * D
    x = r.uniform(-1, 1, n) + 1j * r.uniform(-1, 1, n)
    return taps, x, tpf, steps


def _closed_form(N, taps, D, x, steps, src):
    """Every output step from window position -> push ordinal map `src`;
    the sums run in the restatement's order (oldest first)."""
    part, L = partition_filter_taps(taps, N)
    out = np.zeros((N, steps), np.complex128)
    for k in range(steps):
        P = N * L + (k + 1) * D
        base = (N - 1 - P) % N
        fb = np.zeros(N, np.complex128)
        for b in range(N):
            i = (b - base - 1) % N
            q = (P + b) // N - L
            acc = 0.0 + 0.0j
            for w in range(L):
                m = src(L, q, w)
                s = x[(N - 1 - b) + m * N] if m >= 0 else 0.0
                acc = acc + s * part[i][L - 1 - w]
            fb[b] = acc
        out[:, k] = np.fft.ifft(fb) * N
    return out


@pytest.mark.parametrize("L", range(1, 14))
def test_window_src_against_literal_window_buffer(L, fsdr):
    """L fill pushes then q in 0..L+1 ordinary ones into
    WindowBuffer::new(L, false): the slice is what window_src says, and
    the product's exported map says the same."""
    for q in range(L + 2):
        wb = WindowBuffer(L, False)
        for m in range(L + q):
            wb.push(m + 1)  # ordinal + 1, 0 = hole
        got = [int(v.real) - 1 for v in wb.get_as_slice()]
        want = [window_src(L, q, w) for w in range(L)]
        assert got == want, (L, q)
        assert list(fsdr.pfb_channelizer_window_map(L, q)) == want, (L, q)


@pytest.mark.parametrize("N,n_taps,D", TABLE + EXTRA)
def test_closed_form_end_to_end(N, n_taps, D):
    """The closed form reproduces the restatement on every step; both are
    float64 sums in the same order, so to a few ulp of O(tpf) values."""
    taps, x, tpf, steps = _case(N, n_taps, D)
    ref, cons = chan_oneshot(N, taps, x, N / D)
    assert ref.shape == (N, steps) and cons == x.size
    got = _closed_form(N, taps, D, x, steps, window_src)
    assert np.abs(got - ref).max() <= 1e-12


@pytest.mark.parametrize("N,n_taps,D", TABLE)
def test_restatement_textbook_form(N, n_taps, D):
    """Steady steps equal fft_buf[b] = sum_j x[pmax(b) - jN] part[i(b)][j];
    the tpf*N/D - 1 start-up steps differ from it by more than 1e-3.
    (Not on EXTRA: with n_taps = 9 most sub-filters end in a zero pad,
    which hides the one slot the last start-up step has wrong.)"""
    taps, x, tpf, steps = _case(N, n_taps, D)
    ref, _ = chan_oneshot(N, taps, x, N / D)
    text = _closed_form(N, taps, D, x, steps, lambda L, q, w: q + w)
    n_start = startup_steps(N, n_taps, D)
    assert n_start == (0 if tpf == 1 else tpf * N // D - 1)
    assert np.abs(ref[:, n_start:] - text[:, n_start:]).max() < 1e-12
    for k in range(n_start):
        assert np.abs(ref[:, k] - text[:, k]).max() > 1e-3, k


def test_restatement_call_structure():
    """The fill call never produces; later calls produce
    min(out_cap, n // D) and consume D per step; chunked replay equals
    the one-shot."""
    N, n_taps, D = 8, 64, 2
    taps, x, tpf, steps = _case(N, n_taps, D)
    one, _ = chan_oneshot(N, taps, x, N / D)
    ref = PfbChannelizerRef(N, taps, N / D)
    out, cons = ref.work(x[:10], 100)
    assert (out.shape[1], cons) == (0, 10)
    out, cons = ref.work(x[10:N * tpf + 7], 100)
    assert (out.shape[1], cons) == (0, N * tpf - 10)
    assert ref.all_windows_filled
    pos, cols = N * tpf, []
    for n, cap in [(1, 5), (7, 2), (7, 5), (40, 3), (x.size, 1000)]:
        out, cons = ref.work(x[pos:pos + n], cap)
        avail = min(n, x.size - pos)
        assert out.shape[1] == min(cap, avail // D)
        assert cons == out.shape[1] * D
        pos += cons
        cols.append(out)
    got = np.concatenate(cols, axis=1)
    assert got.shape == one.shape
    assert np.array_equal(got, one)


def test_restatement_linearity():
    N, n_taps, D = 8, 37, 4
    taps, a, tpf, steps = _case(N, n_taps, D)
    _, b, _, _ = _case(N, n_taps, D, seed=12)
    oa, _ = chan_oneshot(N, taps, a, N / D)
    ob, _ = chan_oneshot(N, taps, b, N / D)
    oab, _ = chan_oneshot(N, taps, 2.0 * a - 3.0j * b, N / D)
    assert np.abs(oab - (2.0 * oa - 3.0j * ob)).max() < 1e-11


@pytest.mark.parametrize("N,n_taps,D", TABLE)
def test_oracle_matches_restatement_from_step_0(oracle_lib, N, n_taps, D):
    """Per output step, relative l2 of the N-vector at most 1e-5, start-up
    steps included."""
    from dsp_ref import loud_c64
    r = np.random.default_rng([21, N, n_taps, D])
    tpf = -(-n_taps // N)
    steps = tpf * N // D - 1 + 8
    taps = r.uniform(-1, 1, n_taps).astype(np.float32)
    x = loud_c64(r, N * tpf + steps * D)
    ref, _ = chan_oneshot(N, taps, x, N / D)
    got = oracle_lib.pfb_channelizer(N, D, taps, x, steps + 3)
    assert got.shape == ref.shape == (N, steps)
    for k in range(steps):
        nrm = np.linalg.norm(ref[:, k])
        assert nrm > 1e-2, k
        assert np.linalg.norm(got[:, k] - ref[:, k]) / nrm <= 1e-5, k
