"""PFB synthesizer, host side (no GPU): the consumed/produced planning
against the literal restatement of synthesizer.rs work(), the constructor
constraints, and the restatement pinned on its own."""
import ctypes

import numpy as np
import pytest

from pfb_synth_ref import (PfbSynthesizerRef, synth_oneshot, tone_prototype,
                           tone_energy_fraction)


def _ref_counts(N, n_taps, calls):
    """(consumed, produced) per call of one restatement instance; the
    sample values do not matter for the counts."""
    ref = PfbSynthesizerRef(N, np.ones(n_taps))
    res = []
    for n, cap in calls:
        out, cons = ref.work([np.zeros(n, np.complex128)] * N, cap)
        res.append((cons, out.size))
    return res


def test_count_matches_restatement_random_sequences(fsdr):
    r = np.random.default_rng(0x5E17)
    n_seq = 2400
    for _ in range(n_seq):
        N = int(r.choice([4, 8]))
        n_taps = int(r.integers(N, 5 * N))
        tpf = -(-n_taps // N)
        calls = [(int(r.integers(0, 9)), int(r.integers(N, 6 * N)))
                 for _ in range(4)]
        pushes = 0
        for (n, cap), want in zip(calls, _ref_counts(N, n_taps, calls)):
            got = fsdr.pfb_synthesizer_count(N, tpf, pushes, n, cap)
            assert got == want, (N, n_taps, calls, pushes, n, cap)
            pushes += got[0]


@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("tpf", [1, 2, 5])
def test_count_explicit_out_caps(fsdr, N, tpf):
    """out_cap in {N, N+1, 2N, 2N+1} — either side of both strict
    comparisons — from every fill level."""
    n_taps = N * tpf
    for cap in (N, N + 1, 2 * N, 2 * N + 1):
        for first in range(0, tpf + 3):
            for n in (0, 1, 2, 7):
                calls = [(first, 6 * N), (n, cap)]
                want = _ref_counts(N, n_taps, calls)
                p = fsdr.pfb_synthesizer_count(N, tpf, 0, first, 6 * N)
                assert p == want[0]
                got = fsdr.pfb_synthesizer_count(N, tpf, p[0], n, cap)
                assert got == want[1], (cap, first, n)


@pytest.mark.parametrize("N,tpf", [(4, 1), (4, 3), (8, 4)])
def test_count_deviation_out_cap_below_n(fsdr, N, tpf):
    """Filling step with fewer than N free slots: the reference panics
    (restatement raises); the ABI stops in front of that step."""
    n_taps = N * tpf
    for cap in range(0, N):
        for pushes in range(0, tpf):
            n = tpf - pushes + 2  # reaches the filling step
            ref = PfbSynthesizerRef(N, np.ones(n_taps))
            ref.work([np.zeros(pushes, np.complex128)] * N, 6 * N)
            with pytest.raises(IndexError):
                ref.work([np.zeros(n, np.complex128)] * N, cap)
            assert fsdr.pfb_synthesizer_count(N, tpf, pushes, n, cap) == (
                tpf - 1 - pushes, 0)
        # windows already filled: the loop condition alone stops it
        ref = PfbSynthesizerRef(N, np.ones(n_taps))
        ref.work([np.zeros(tpf + 1, np.complex128)] * N, 6 * N)
        out, cons = ref.work([np.zeros(5, np.complex128)] * N, cap)
        assert (cons, out.size) == (0, 0)
        assert fsdr.pfb_synthesizer_count(N, tpf, tpf + 1, 5, cap) == (0, 0)


@pytest.mark.parametrize("N,n_taps,null_taps", [
    (2, 32, False), (6, 32, False), (8192, 16384, False), (8, 7, False),
    (8, 32, True)])
def test_constructor_rejects(fsdr, N, n_taps, null_taps):
    lib = fsdr.lib()
    taps = np.ones(max(n_taps, 1), np.float32)
    p = None if null_taps else taps.ctypes.data_as(
        ctypes.POINTER(ctypes.c_float))
    assert not lib.fsdr_pfb_synthesizer_create(N, p, n_taps)
    err = lib.fsdr_last_error().decode()
    assert err and "pfb synthesizer" in err
    if not null_taps:  # the class always passes a tap array
        with pytest.raises(fsdr.FsdrError, match="pfb synthesizer"):
            fsdr.PfbSynthesizer(N, taps[:n_taps])


def test_run_length_query(fsdr):
    """Host-only: a positive run length where the fused kernel applies,
    0 where only the staged path does."""
    for N in (4, 8, 64, 1024):
        assert fsdr.pfb_synthesizer_run_length(N, 4) > 0
    assert fsdr.pfb_synthesizer_run_length(2048, 2) == 0
    assert fsdr.pfb_synthesizer_run_length(1024, 64) == 0  # LDS budget


def test_symbols_exported(fsdr):
    lib = fsdr.lib()
    for s in ("fsdr_pfb_synthesizer_create", "fsdr_pfb_synthesizer_count",
              "fsdr_pfb_synthesizer_run_length",
              "fsdr_pfb_synthesizer_run_dev",
              "fsdr_pfb_synthesizer_stream_dev"):
        assert s in fsdr.exported_symbols()
        assert getattr(lib, s)


# ---------------- the restatement, pinned on its own -------------------

@pytest.mark.parametrize("n_taps,tpf", [(11, 3), (16, 4), (4, 1)])
def test_restatement_direct_formula(n_taps, tpf):
    """Steady state: out[(t-(tpf-1))*N + c] = sum_j taps[c+j*N] *
    v[t-j][c], from emitted step tpf on. The first tpf emitted steps
    come from WindowBuffer's start-up order (next test) and differ."""
    N, T = 4, 14
    r = np.random.default_rng(3)
    taps = r.uniform(-1, 1, n_taps)
    x = r.uniform(-1, 1, (N, T)) + 1j * r.uniform(-1, 1, (N, T))
    out, cons = synth_oneshot(N, taps, x)
    v = np.fft.ifft(x, axis=0) * N  # v[c][t]
    pt = np.zeros(N * tpf)
    pt[:n_taps] = taps
    want = np.array([sum(pt[c + j * N] * v[c, t - j] for j in range(tpf))
                     for t in range(tpf - 1, T) for c in range(N)])
    assert cons == T and out.shape == want.shape
    skip = 0 if tpf == 1 else tpf * N
    assert np.abs(out[skip:] - want[skip:]).max() < 1e-12
    if tpf > 1:
        assert np.abs(out[:skip] - want[:skip]).max() > 1e-3


@pytest.mark.parametrize("L", range(1, 14))
def test_restatement_startup_window_order(L):
    """WindowBuffer::new(L, false) puts fill-phase push k at position
    2k mod L (window_buffer.rs:24-31), so the windows of the first L
    emitted steps are a shuffle with holes. Pins the closed form the
    product's start-up kernel uses: window position w of emitted step e
    is slot x = (e+w) mod L, holding frame L+x if x < e, else the last
    fill push k with 2k = x (mod L), else nothing."""
    from pfb_synth_ref import WindowBuffer
    wb = WindowBuffer(L, False)
    for k in range(L - 1):
        wb.push(k + 1)  # frame id + 1, 0 = hole
    for e in range(L + 2):
        wb.push(L - 1 + e + 1)
        got = [int(v.real) - 1 for v in wb.get_as_slice()]
        want = []
        for w in range(L):
            x = (e + w) % L
            if e >= L:
                want.append(e + w)  # steady state: oldest -> newest
            elif x < e:
                want.append(L + x)
            elif (x + L) % 2 == 0:
                want.append((x + L) // 2)
            elif x % 2 == 0:
                want.append(x // 2)
            else:
                want.append(-1)
        assert got == want, (L, e)


def test_restatement_linearity():
    N, n_taps, T = 8, 37, 30
    r = np.random.default_rng(5)
    taps = r.uniform(-1, 1, n_taps)
    a = r.uniform(-1, 1, (N, T)) + 1j * r.uniform(-1, 1, (N, T))
    b = r.uniform(-1, 1, (N, T)) + 1j * r.uniform(-1, 1, (N, T))
    oa, _ = synth_oneshot(N, taps, a)
    ob, _ = synth_oneshot(N, taps, b)
    oab, _ = synth_oneshot(N, taps, 2.0 * a - 3.0j * b)
    assert np.abs(oab - (2.0 * oa - 3.0j * ob)).max() < 1e-11


@pytest.mark.parametrize("m", [0, 3, 9, 15])
def test_restatement_tone_placement(m):
    """A constant on channel m comes out as a tone in bin 2048*m/16."""
    N, tpf = 16, 8
    taps = tone_prototype(N, N * tpf)
    T = tpf - 1 + tpf + 2048 // N
    x = np.zeros((N, T), np.complex128)
    x[m] = 1.0
    out, _ = synth_oneshot(N, taps, x)
    peak, frac, want = tone_energy_fraction(out, N, tpf, m)
    assert peak == want
    assert frac > 0.99
