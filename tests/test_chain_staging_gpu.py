"""Staging loader of the ws chain kernel: interior tiles (every staged
sample below n_in) load unguarded, boundary tiles keep the per-sample
guard. The switch between the two is a comparison against n_in, so the
test moves n_in one sample at a time across tile 2's threshold and asks
for the same bits every time.

Set-up: the stream of R.chain_input(nt1, nt2, 5*1024) sits in a device
buffer that is 8192 samples longer; the slack is NaN, and before each run
so is every stream sample from n_in on, so a tile that takes the unguarded
path even one group too early puts NaN into the output instead of reading
past an allocation. out_cap = mag_cap = 3 tiles fixes prod at
3072 whatever n_in is. The baseline run gets the minimal input for 3072
outputs (its last tile is a boundary tile) and is checked against the f64
reference at the chain tolerance of test_kernel_variants_gpu (rel-l2 <
2e-4 per frame). Every other run sees more input; the extra samples lie
past the last output's filter window, so spectra and |X|^2 must equal the
baseline bit for bit.

The reference is the first three frames of R.chain_case(nt1, nt2, 1024)
(prod 5*1024): chain_case draws taps and input from a generator keyed by
prod, so its prod=3072 case is another stream; test_minimal_stream_case
runs that one on its own.
"""
import ctypes

import numpy as np
import pytest

import dsp_ref as R

pytestmark = pytest.mark.gpu

TILE = 1024
PROD = 3 * TILE
SLACK = 8192
LIVE = 4 * PROD  # n_in > LIVE in every run; samples below it are left alone
CASES = {80: (127, 127), 20: (8, 8)}  # fused MFMA K -> (nt1, nt2)
KNOBS = ("FSDR_FIR_GRID_CAP", "FSDR_CHAIN_WS", "FSDR_CHAIN_ALLPHASE",
         "FSDR_CHAIN_FUSED", "FSDR_CHAIN_FFTFUSE", "FSDR_CHAIN_BLOCK512",
         "FSDR_CHAIN_OCC8", "FSDR_CHAIN_STAGGER")


def sweep_range(kk):
    """Every n_in around tile 2's interior threshold: the tile stages
    groups 2*1024 .. 2*1024 + 1024+K+9 of 4 samples."""
    return range((2 * TILE + TILE + kk + 9) * 4 - 8,
                 (2 * TILE + 1280) * 4 + 8 + 1)


def five(kk):
    r = sweep_range(kk)
    thr = (2 * TILE + TILE + kk + 9) * 4  # first n_in with tile 2 interior
    return (r[0], thr - 1, thr, thr + 1, r[-1])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Rig:
    """One chain, its NaN-padded device input and NaN-primed outputs."""

    def __init__(self, gpu, kk, t1, t2, x):
        self.gpu, self.lib, self.ptrs = gpu, gpu.lib(), []
        self.d_in = self.alloc((x.size + SLACK) * 8)
        assert (self.d_in & 15) == 0  # the ws route needs a 16 B base
        self.x = np.concatenate(
            [x, np.full(SLACK, np.nan + 1j * np.nan, np.complex64)])
        self.put(self.d_in, self.x)
        self.d_out, self.d_mag = self.alloc(PROD * 8), self.alloc(PROD * 4)
        self.chain = gpu.Chain(t1, t2, 4, 1024)
        assert self.chain.variant() == kk

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.lib.fsdr_dev_alloc(ctypes.byref(p), nbytes) == 0
        self.ptrs.append(p)
        return p.value

    def put(self, addr, arr):
        arr = np.ascontiguousarray(arr)
        assert self.lib.fsdr_memcpy_h2d(ctypes.c_void_p(addr),
                                        ctypes.c_void_p(arr.ctypes.data),
                                        arr.nbytes) == 0

    def get(self, addr, dtype):
        self.gpu.synchronize()
        out = np.zeros(PROD, dtype)
        assert self.lib.fsdr_memcpy_d2h(ctypes.c_void_p(out.ctypes.data),
                                        ctypes.c_void_p(addr),
                                        out.nbytes) == 0
        return out

    def run(self, n_in, want_out=True, want_mag=True):
        """(spectra or None, |X|^2 or None) of one run over n_in samples;
        every sample of the buffer from n_in on is NaN during the run."""
        tail = self.x[LIVE:].copy()
        tail[n_in - LIVE:] = np.nan + 1j * np.nan
        self.put(self.d_in + LIVE * 8, tail)
        self.put(self.d_out, np.full(PROD, np.nan, np.complex64))
        self.put(self.d_mag, np.full(PROD, np.nan, np.float32))
        counts = self.chain.run_dev(
            self.d_in, n_in, self.d_out if want_out else 0,
            PROD if want_out else 0, self.d_mag if want_mag else 0,
            PROD if want_mag else 0)
        assert counts == (4 * PROD, PROD)
        return (self.get(self.d_out, np.complex64) if want_out else None,
                self.get(self.d_mag, np.float32) if want_mag else None)

    def close(self):
        self.gpu.synchronize()
        for p in self.ptrs:
            self.lib.fsdr_dev_free(p)


@pytest.fixture
def cap(monkeypatch):
    """cap(None | "1"): clear every chain launch knob, set the grid cap."""
    def set_(value):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if value is not None:
            monkeypatch.setenv("FSDR_FIR_GRID_CAP", value)
    set_(None)
    return set_


@pytest.fixture(params=sorted(CASES, reverse=True))
def rig(request, gpu, cap):
    """(kk, Rig, baseline spectra, baseline |X|^2); the baseline is
    checked against the f64 reference here, once per K."""
    kk = request.param
    nt1, nt2 = CASES[kk]
    t1, t2, x, ref = R.chain_case(nt1, nt2, 1024)
    t1b, t2b, xb = R.chain_input(nt1, nt2, 5 * TILE)
    assert (np.array_equal(xb, x) and np.array_equal(t1b, t1)
            and np.array_equal(t2b, t2))  # the same stream
    r = Rig(gpu, kk, t1, t2, x)
    try:
        n_min = 4 * PROD + nt1 + nt2 - 2 + 3
        spec, mag = r.run(n_min)
        rel = R.rel_l2_per_frame(spec, ref[:PROD], 1024)
        print(f"chain staging K{kk} baseline rel-l2 per frame {rel}")
        assert float(rel.max()) < 2e-4
        want = spec.real.astype(np.float64) ** 2 + spec.imag.astype(
            np.float64) ** 2
        assert np.all(np.abs(mag - want) <= 1e-6 * want)
        yield kk, r, spec, mag
    finally:
        r.close()


def same_bits(got, base, what):
    np.testing.assert_array_equal(bits(got), bits(base), err_msg=what)


def test_sweep_one_block(rig, cap):
    """One block owns the three tiles and prefetches tile 2, boundary or
    interior according to n_in, from tile 1's interior iteration."""
    kk, r, spec0, mag0 = rig
    cap("1")
    for n_in in sweep_range(kk):
        spec, mag = r.run(n_in)
        same_bits(spec, spec0, f"spectra, n_in={n_in}")
        same_bits(mag, mag0, f"|X|^2, n_in={n_in}")


def test_five_points_three_blocks(rig, cap):
    """Cap unset: each tile has a block of its own, so the boundary or
    interior choice for tile 2 falls to a prologue load."""
    kk, r, spec0, mag0 = rig
    for n_in in five(kk):
        spec, mag = r.run(n_in)
        same_bits(spec, spec0, f"spectra, n_in={n_in}")
        same_bits(mag, mag0, f"|X|^2, n_in={n_in}")


@pytest.mark.parametrize("grid_cap", ["1", None])
def test_output_combinations(rig, cap, grid_cap):
    """d_out only and d_mag only against the baseline's both."""
    kk, r, spec0, mag0 = rig
    cap(grid_cap)
    for n_in in five(kk):
        spec, none = r.run(n_in, want_mag=False)
        assert none is None
        same_bits(spec, spec0, f"d_out only, n_in={n_in}")
        none, mag = r.run(n_in, want_out=False)
        assert none is None
        same_bits(mag, mag0, f"d_mag only, n_in={n_in}")


@pytest.mark.parametrize("kk", sorted(CASES, reverse=True))
def test_minimal_stream_case(gpu, cap, kk):
    """R.chain_case(..., prod=3072) as it stands: its own stream, exactly
    the minimal input, NaN behind it."""
    nt1, nt2 = CASES[kk]
    t1, t2, x, ref = R.chain_case(nt1, nt2, 1024, PROD)
    assert x.size == 4 * PROD + nt1 + nt2 - 2 + 3
    r = Rig(gpu, kk, t1, t2, x)
    try:
        for grid_cap in ("1", None):
            cap(grid_cap)
            spec, mag = r.run(x.size)
            rel = float(R.rel_l2_per_frame(spec, ref, 1024).max())
            print(f"chain staging K{kk} prod=3072 cap={grid_cap} {rel:.3e}")
            assert rel < 2e-4
            assert not np.isnan(mag).any()
    finally:
        r.close()
