"""Host-only parts of the PFB arbitrary-rate resampler against the literal
restatement of arb_resampler.rs (tests/pfb_arb_ref.py): the checkpointed
timing schedule (records and counts exact, mu bit for bit), the start-up
window shuffle, the per-call consumed/produced arithmetic and the
constructor checks. No GPU, no compute kernels."""
import copy
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from pfb_arb_ref import (PfbArbResamplerRef, records_arrays, startup_window,
                         timing_records)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "pfb_arb_schedule.npz")

CASES = [(2.5, 5), (1.6, 32), (1.5, 5), (48000 / 44100, 5), (0.3, 5),
         (7.3, 4)]
LONG = 20000


@functools.lru_cache(maxsize=None)
def schedule(fsdr, rate, nf):
    return fsdr.PfbArbSchedule(rate, nf)


@functools.lru_cache(maxsize=None)
def literal(fsdr, rate, nf):
    """The literal walk from input 0, once per case: at least 3 periods
    where the cycle is short, LONG inputs otherwise."""
    s = schedule(fsdr, rate, nf)
    n = s.preperiod + 3 * s.period
    n = max(n, 200) if n <= LONG else LONG
    _, recs = timing_records(rate, nf, 0, n)
    arrs = records_arrays(recs)
    for a in arrs:
        a.setflags(write=False)
    return n, arrs


def same_records(got, want, what):
    for name, g, w in zip(("in_index", "base_index", "boundary", "mu"), got,
                          want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name == "mu":  # bit for bit
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("rate,nf", CASES)
def test_records_and_counts_equal_literal_walk(fsdr, rate, nf):
    s = schedule(fsdr, rate, nf)
    n, lit = literal(fsdr, rate, nf)
    q = s.checkpoint_spacing
    assert q > 2 and n > q + 1
    for start in (0, q // 2, q - 1, q, q + 1):
        k = int(np.searchsorted(lit[0], start))
        got = s.records(start, n - start)
        same_records(got, [a[k:] for a in lit], f"start {start}")
        assert s.count(start, n - start) == lit[0].size - k
        for m in (0, 1, q - 1, q, (n - start) // 2):
            k2 = int(np.searchsorted(lit[0], start + m))
            assert s.count(start, m) == k2 - k, (start, m)
    assert s.count(0, 0) == 0


@pytest.mark.parametrize("rate,nf", [(2.5, 5), (1.6, 32), (1.5, 5),
                                     (1.6, 5), (0.75, 7)])
def test_reported_cycle_is_a_cycle_of_the_literal_walk(fsdr, rate, nf):
    """Short cycles (the long ones are in the golden test): the literal
    walk from the reported preperiod and from preperiod + period yields
    identical records (shifted by the period), and the outputs per period
    agree."""
    s = schedule(fsdr, rate, nf)
    rho, lam = s.preperiod, s.period
    span = min(lam, 300)
    assert rho + lam + span <= LONG
    ref, a = timing_records(rate, nf, rho, span)
    assert ref.inputs_seen == rho + span
    _, mid = timing_records(rate, nf, rho + span, lam - span, start=ref)
    _, b = timing_records(rate, nf, rho + lam, span, start=ref)
    assert len(a) + len(mid) == s.outputs_per_period
    a, b = records_arrays(a), records_arrays(b)
    assert np.array_equal(a[0] + np.uint64(lam), b[0])
    same_records(a[1:], b[1:], "one period apart")
    same_records(s.records(rho, span), a, "abi at rho")
    same_records(s.records(rho + lam, span), b, "abi at rho+lam")
    # and far past the table
    far = rho + 1000003 * lam
    c = s.records(far, span)
    assert np.array_equal(c[0] - np.uint64(far - rho), a[0])
    same_records(c[1:], a[1:], "abi far out")
    assert s.count(rho, far - rho) == 1000003 * s.outputs_per_period


def test_long_cycles_equal_golden_walk(fsdr):
    """Positions on both sides of rho and rho+lam and beyond rho+2*lam,
    against the literal walk stored by golden/generate_pfb_arb.py."""
    g = np.load(GOLDEN)
    span = int(g["span"])
    seen_wrap = 0
    for ci in range(int(g["n_cases"])):
        rate, nf = float(g[f"c{ci}_rate"]), int(g[f"c{ci}_nf"])
        s = schedule(fsdr, rate, nf)
        pos, cum = g[f"c{ci}_pos"], g[f"c{ci}_cum"]
        assert pos.size >= 8
        seen_wrap += int(pos.max() > s.preperiod + 2 * s.period)
        for k, (p, c) in enumerate(zip(pos, cum)):
            p = int(p)
            assert s.count(0, p) == int(c), (rate, nf, p)
            want = [g[f"c{ci}_p{k}_{f}"] for f in ("idx", "base", "bnd",
                                                   "mu")]
            same_records(s.records(p, span), want, f"{rate} {nf} @ {p}")
    assert seen_wrap == int(g["n_cases"])


@pytest.mark.parametrize("tpf", range(1, 10))
def test_startup_shuffle_closed_form(fsdr, tpf):
    assert np.array_equal(fsdr.pfb_arb_startup_map(tpf), startup_window(tpf))


WORK = [(2.5, 5, 8), (0.3, 5, 3), (7.3, 4, 2), (1.0, 1, 1)]


@pytest.mark.parametrize("rate,nf,tpf", WORK)
def test_work_equals_literal_work(fsdr, rate, nf, tpf):
    """consumed/produced of one call for a grid of (pushes, n_in,
    out_cap), including out_cap < ceil(rate) and n_in < tpf. Where the
    reference would index past out_cap the product stops earlier (the
    documented guard); that must never happen with the reference's own n
    here, so it is asserted not to."""
    s = schedule(fsdr, rate, nf)
    taps = np.ones(nf * tpf, np.float32)
    x = list(np.arange(1, 200).astype(np.complex128))
    cr = math.ceil(np.float32(rate))
    for pushes in (0, 1, tpf - 1, tpf, tpf + 1, tpf + 64, 101):
        if pushes < 0:
            continue
        base = PfbArbResamplerRef(rate, taps, nf)
        fed = 0
        while fed < pushes:  # chunked: a call may stop at the fill
            _, c = base.call(x[fed:pushes], 10 ** 6)
            assert c > 0
            fed += c
        for n_in in (0, 1, tpf - 1, tpf, tpf + 1, 37):
            for out_cap in (0, 1, cr - 1, cr, 7, 50, 1000):
                ref = copy.deepcopy(base)
                out, cons = ref.call(x[pushes:pushes + n_in], out_cap)
                assert len(out) <= out_cap
                got = s.work(tpf, pushes, n_in, out_cap)
                assert got == (cons, len(out)), (pushes, n_in, out_cap)


def test_out_cap_guard_stops_at_the_largest_prefix_that_fits(fsdr):
    """The guard itself, reached through a position where the reference's
    n = out_cap/rate inputs yield more than out_cap outputs, if the
    schedule has one; else only the invariant produced <= out_cap."""
    for rate, nf in ((2.5, 5), (7.3, 4), (1.6, 32)):
        s = schedule(fsdr, rate, nf)
        for pushes in range(1, 60):
            for out_cap in range(0, 40):
                cons, prod = s.work(1, pushes, 64, out_cap)
                assert prod <= out_cap
                lim = int(np.float32(out_cap) / np.float32(rate))
                assert cons <= min(64, lim)
                assert prod == s.count(pushes - 1, cons)
                if cons < min(64, lim):  # cut short: one more would not fit
                    assert s.count(pushes - 1, cons + 1) > out_cap


def test_constructor_violations_return_null(fsdr):
    lib = fsdr.lib()
    taps = np.ones(8, np.float32)
    p = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for args, msg in (((0.0, p, 8, 4, 1), b"rate must be greater than zero"),
                      ((-1.5, p, 8, 4, 1), b"rate must be greater than zero"),
                      ((float("nan"), p, 8, 4, 1), b"greater than zero"),
                      ((1.5, p, 3, 4, 1), b"at least num_filters"),
                      ((1.5, p, 8, 0, 1), b"filter banks must be greater"),
                      ((1.5, p, 8, 4, 0), b"num_channels")):
        assert not lib.fsdr_pfb_arb_resampler_create(*args)
        assert msg in lib.fsdr_last_error(), (args, lib.fsdr_last_error())


def test_schedule_create_errors(fsdr):
    for rate, nf, code in ((0.0, 5, fsdr.ERR_INVALID),
                           (2.5, 0, fsdr.ERR_INVALID),
                           (float("inf"), 5, fsdr.ERR_UNSUPPORTED),
                           (1e9, 5, fsdr.ERR_UNSUPPORTED),
                           (1e-9, 64, fsdr.ERR_UNSUPPORTED)):
        with pytest.raises(fsdr.FsdrError) as e:
            fsdr.PfbArbSchedule(rate, nf)
        assert e.value.code == code, (rate, nf)
    s = fsdr.PfbArbSchedule(2.5, 5)
    assert (s.preperiod + s.period) <= 2 ** 25
    assert s.segment_inputs > 0 and s.checkpoint_spacing > 0
