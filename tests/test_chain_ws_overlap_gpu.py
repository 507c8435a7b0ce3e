"""The ws chain kernel's software pipeline at every depth, every K.

k_decim4_fft_mfma_ws_tpl runs tile t's FFT stages inside tile t+1's MFMA
windows and stores tile t's spectrum in iteration t+2. Each block runs its own
prologue and epilogue, so what a run exercises depends on how many tiles a
block owns: one tile is prologue and epilogue only, two add one loop
iteration with a previous tile, the first held store needs three and the
steady state more than three. So: fft_len 1024, every tap pair of
dsp_ref.CHAIN_TAP_PAIRS (all five K), outputs of exactly 1, 2, 3 and 5
tiles, FSDR_FIR_GRID_CAP unset, 1 and 3, spectrum + |X|^2 and |X|^2 alone
(out null: the held-store path differs).

Inputs: dsp_ref.chain_case gives exactly the samples that `prod` outputs
need, which ends inside the last tile's staging range (a tile stages
4 * (1024 + K + 8) + 3 samples), so that tile takes the guarded boundary
loader and the ones before it the straight-line one. test_interior_tiles
adds the other end: two tiles more input than the output capacity lets the
chain produce, every tile interior.

Reference and bound are those of tests/test_kernel_variants_gpu.py for
this route: dsp_ref's float64 chain, per-frame relative l2 < 2e-4, |X|^2
within 1e-6 of the spectrum's own; capped runs equal the uncapped run bit
for bit.
"""
import ctypes

import numpy as np
import pytest

import dsp_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("FSDR_FIR_GRID_CAP", "FSDR_CHAIN_WS", "FSDR_CHAIN_ALLPHASE",
         "FSDR_CHAIN_FUSED", "FSDR_CHAIN_FFTFUSE", "FSDR_CHAIN_BLOCK512",
         "FSDR_CHAIN_OCC8", "FSDR_CHAIN_STAGGER")
CAPS = (None, "1", "3")
TILES = (1, 2, 3, 5)


@pytest.fixture
def cap(monkeypatch):
    def set_(value):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if value is not None:
            monkeypatch.setenv("FSDR_FIR_GRID_CAP", value)
    set_(None)
    return set_


@pytest.fixture
def dev(gpu):
    """alloc(nbytes) -> device address; put/get copy; all freed after."""
    lib = gpu.lib()
    ptrs = []

    class Dev:
        def alloc(self, nbytes):
            p = ctypes.c_void_p()
            assert lib.fsdr_dev_alloc(ctypes.byref(p), max(8, nbytes)) == 0
            ptrs.append(p)
            return p.value

        def put(self, addr, arr):
            arr = np.ascontiguousarray(arr)
            assert lib.fsdr_memcpy_h2d(ctypes.c_void_p(addr),
                                       ctypes.c_void_p(arr.ctypes.data),
                                       arr.nbytes) == 0

        def get(self, addr, dtype, n):
            out = np.zeros(n, dtype)
            gpu.synchronize()
            assert lib.fsdr_memcpy_d2h(ctypes.c_void_p(out.ctypes.data),
                                       ctypes.c_void_p(addr),
                                       out.nbytes) == 0
            return out

    yield Dev()
    gpu.synchronize()
    for p in ptrs:
        lib.fsdr_dev_free(p)


def assert_mag(mag, spec):
    want = spec.real.astype(np.float64) ** 2 + spec.imag.astype(
        np.float64) ** 2
    assert np.all(np.abs(mag - want) <= 1e-6 * want)


def run_ws(gpu, dev, cap, kk, t1, t2, x, prod, ref):
    """Both output modes at every cap against ref; returns nothing."""
    d_in = dev.alloc(x.nbytes)
    assert (d_in & 15) == 0  # an 8-byte-odd base would take halves
    d_out, d_mag = dev.alloc(prod * 8), dev.alloc(prod * 4)
    dev.put(d_in, x)
    base = None
    for c in CAPS:
        cap(c)
        ch = gpu.Chain(t1, t2, 4, 1024)
        assert ch.variant() == kk
        dev.put(d_out, np.full(prod, np.nan, np.complex64))
        dev.put(d_mag, np.full(prod, np.nan, np.float32))
        assert ch.run_dev(d_in, x.size, d_out, prod, d_mag, prod) == (
            4 * prod, prod)
        spec = dev.get(d_out, np.complex64, prod)
        mag = dev.get(d_mag, np.float32, prod)
        dev.put(d_mag, np.full(prod, np.nan, np.float32))
        assert ch.run_dev(d_in, x.size, 0, 0, d_mag, prod) == (4 * prod,
                                                               prod)
        mag_only = dev.get(d_mag, np.float32, prod)
        if base is None:
            base = (spec, mag)
            rel = float(R.rel_l2_per_frame(spec, ref, 1024).max())
            print(f"WSO K{kk} prod{prod} {rel:.3e}")
            assert rel < 2e-4
            assert_mag(mag, spec)
        else:
            np.testing.assert_array_equal(
                spec, base[0], err_msg=f"FSDR_FIR_GRID_CAP={c} changed bits")
            np.testing.assert_array_equal(
                mag, base[1], err_msg=f"FSDR_FIR_GRID_CAP={c} changed bits")
        np.testing.assert_array_equal(
            mag_only, base[1], err_msg=f"out null, cap {c}: |X|^2 differs")


@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("kk", sorted(R.CHAIN_TAP_PAIRS))
def test_pipeline_depths(gpu, dev, cap, kk, tiles):
    nt1, nt2 = R.CHAIN_TAP_PAIRS[kk]
    prod = tiles * 1024
    t1, t2, x, ref = R.chain_case(nt1, nt2, 1024, prod)
    # the input ends inside the last tile's staging range
    assert 4 * prod < x.size < 4 * (prod + kk + 8) + 3
    run_ws(gpu, dev, cap, kk, t1, t2, x, prod, ref)


@pytest.mark.parametrize("kk", sorted(R.CHAIN_TAP_PAIRS))
def test_interior_tiles(gpu, dev, cap, kk):
    """Input for five tiles, room for three: no tile meets the end."""
    nt1, nt2 = R.CHAIN_TAP_PAIRS[kk]
    t1, t2, x, ref = R.chain_case(nt1, nt2, 1024, 5 * 1024)
    prod = 3 * 1024
    assert x.size >= 4 * (prod + kk + 8) + 3
    run_ws(gpu, dev, cap, kk, t1, t2, x, prod, ref[:prod])
