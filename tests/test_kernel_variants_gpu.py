"""Every kernel variant and template instantiation, with blocks that own
more than one tile, against the float64 references of tests/dsp_ref.py.

The default launches give each block one tile at test sizes, so the
persistent tile loops (restage barriers, prefetch into registers, the ws
chain kernel's whole software pipeline) only iterate when the grid is
capped. Every case here produces 3 full tiles plus a partial one and runs
with FSDR_FIR_GRID_CAP unset, 1 (one block owns all four tiles) and 3
(block 0 owns tiles 0 and 3):

  * the unset-cap output is compared with dsp_ref: per output and
    component within the derived fp32 bound for FIR-class kernels, per
    frame relative l2 for FFT (1e-4, DESIGN.md section c) and chain (2e-4,
    the chain fuzz figure), 5e-4 for XlatingFir (its fast __sincosf is
    unmeasured);
  * every capped output must be bit-identical to the unset-cap output of
    the same kernel: tile arithmetic does not depend on the owning block.

Counts (consumed, produced, status) come from the KAT-pinned oracle.
Which instantiation a handle selects is read back through
fsdr_filter_variant / fsdr_chain_variant and checked against a restatement
of the selector, so a case list that stops covering a switch table fails.

Each test prints its figure ("KVC family case figure"); the worst per
family is in profiles/kernel_variant_coverage.txt.
"""
import ctypes

import numpy as np
import pytest

import dsp_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("FSDR_FIR_GRID_CAP", "FSDR_FIR_MFMA", "FSDR_FIR_MFMA32",
         "FSDR_DECIM_MFMA", "FSDR_RESAMP_TILED", "FSDR_XLATING_TILED",
         "FSDR_CHAIN_WS", "FSDR_CHAIN_ALLPHASE", "FSDR_CHAIN_FUSED",
         "FSDR_CHAIN_FFTFUSE", "FSDR_CHAIN_BLOCK512", "FSDR_CHAIN_OCC8",
         "FSDR_CHAIN_STAGGER", "FSDR_FFT_FPB_BASE")
CAPS = (None, "1", "3")
FFT_CAPS = (None, "1", "2")

# the switch tables of the launch sites
FIR_KK = (32, 64, 96, 144, 272, 528)        # K >= n_taps + 15
FIR_KK32 = (48, 96, 160, 288, 544)          # K >= n_taps + 31
FIR_TP = (17, 33, 65, 129, 257, 513)        # TP >= n_taps
DECIM_KK = (20, 32, 48, 80, 144)            # K >= ceil(n_taps/4) + 15
DECIM_TP = (8, 16, 32, 64, 128)             # 4 TP >= n_taps


def _first(table, need):
    return next((k for k in table if k >= need), 0)


def fir_variant(n_taps):
    return (_first(FIR_KK, n_taps + 15), _first(FIR_KK32, n_taps + 31),
            _first(FIR_TP, n_taps))


def decim4_variant(n_taps):
    if n_taps > 512:
        return (0, 0, 0)
    return (_first(DECIM_KK, (n_taps + 3) // 4 + 15), 0,
            _first(DECIM_TP, (n_taps + 3) // 4))


@pytest.fixture
def knobs(monkeypatch):
    """set(**env): clear every launch knob, then set the given ones."""
    def set_(cap=None, **env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        if cap is not None:
            monkeypatch.setenv("FSDR_FIR_GRID_CAP", cap)
    set_()
    return set_


def report(family, case, figure):
    print(f"KVC {family} {case} {figure:.3e}")


def run_caps(knobs, env, run, caps=CAPS):
    """run() at every cap; returns the unset-cap result after asserting
    that each capped one equals it bit for bit."""
    base = None
    for cap in caps:
        knobs(cap=cap, **env)
        got = run()
        if cap is None:
            base = got
            continue
        for b, g in zip(base, got):
            if isinstance(b, np.ndarray):
                np.testing.assert_array_equal(
                    g, b, err_msg=f"FSDR_FIR_GRID_CAP={cap} changed bits")
            else:
                assert g == b, f"FSDR_FIR_GRID_CAP={cap}: {g} != {b}"
    return base


def check_fir_class(family, case, got, counts, oracle_counts, ref, a_re,
                    a_im, n_terms, complex_taps=False):
    assert tuple(counts) == tuple(oracle_counts)
    assert got.size == ref.size
    ratio = R.fir_err_ratio(got, ref, a_re, a_im, n_terms, complex_taps)
    report(family, case, ratio)
    assert ratio <= 1.0, f"{family} {case}: err / bound = {ratio}"


# ---------------- FIR cf32 ----------------------------------------------

FIR_VARIANTS = {"mfma": {}, "mfma32": {"FSDR_FIR_MFMA32": "1"},
                "scalar": {"FSDR_FIR_MFMA": "0"}}


@pytest.mark.parametrize("variant", FIR_VARIANTS)
@pytest.mark.parametrize("n_taps", R.FIR_TAPS)
def test_fir_cf32(gpu, oracle_lib, knobs, n_taps, variant):
    taps, x, ref, a_re, a_im = R.fir_case(n_taps)
    f = gpu.Fir(taps)
    assert f.variant() == fir_variant(n_taps)
    if n_taps >= 514:  # past every template: the untemplated k_fir_cf32
        assert f.variant() == (0, 0, 0)
    got, *counts = run_caps(knobs, FIR_VARIANTS[variant],
                            lambda: f.filter(x, R.N_OUT_1024))
    _, *oc = oracle_lib.fir_cf32(taps, x, R.N_OUT_1024)
    check_fir_class(f"fir_cf32/{variant}", n_taps, got, counts, oc, ref,
                    a_re, a_im, n_taps)


def test_fir_cf32_case_list_covers_switch_tables(gpu):
    seen = [gpu.Fir(R.fir_case(t)[0]).variant() for t in R.FIR_TAPS]
    assert {v[0] for v in seen} - {0} == set(FIR_KK)
    assert {v[1] for v in seen} - {0} == set(FIR_KK32)
    assert {v[2] for v in seen} - {0} == set(FIR_TP)
    assert (0, 0, 0) in seen  # k_fir_cf32
    # both sides of every template boundary select different kernels
    for lo in (17, 49, 81, 129, 257, 513):
        assert fir_variant(lo)[0] != fir_variant(lo + 1)[0]
        assert lo in R.FIR_TAPS and lo + 1 in R.FIR_TAPS


# ---------------- decimating FIR ----------------------------------------

DECIM_VARIANTS = {"mfma": {}, "scalar": {"FSDR_DECIM_MFMA": "0"}}


@pytest.mark.parametrize("variant", DECIM_VARIANTS)
@pytest.mark.parametrize("n_taps", R.DECIM4_TAPS)
def test_decim4(gpu, oracle_lib, knobs, n_taps, variant):
    taps, x, ref, a_re, a_im = R.decim_case(4, n_taps)
    f = gpu.DecimFir(4, taps)
    assert f.variant() == decim4_variant(n_taps)
    got, *counts = run_caps(knobs, DECIM_VARIANTS[variant],
                            lambda: f.filter(x, R.N_OUT_1024))
    _, *oc = oracle_lib.decim_fir_cf32(4, taps, x, R.N_OUT_1024)
    check_fir_class(f"decim4/{variant}", n_taps, got, counts, oc, ref,
                    a_re, a_im, n_taps)


@pytest.mark.parametrize("decim,n_taps", R.DECIM_GENERIC)
def test_decim_generic(gpu, oracle_lib, knobs, decim, n_taps):
    """Grid-stride kernel without a tile loop: no cap runs."""
    taps, x, ref, a_re, a_im = R.decim_case(decim, n_taps)
    f = gpu.DecimFir(decim, taps)
    assert f.variant() == (0, 0, 0)
    got, *counts = f.filter(x, R.N_OUT_1024)
    _, *oc = oracle_lib.decim_fir_cf32(decim, taps, x, R.N_OUT_1024)
    check_fir_class("decim_generic", f"D{decim}", got, counts, oc, ref,
                    a_re, a_im, n_taps)


def test_decim4_case_list_covers_switch_tables(gpu):
    seen = [gpu.DecimFir(4, R.decim_case(4, t)[0]).variant()
            for t in R.DECIM4_TAPS]
    assert {v[0] for v in seen} - {0} == set(DECIM_KK)
    assert {v[2] for v in seen} - {0} == set(DECIM_TP)
    assert (0, 0, 0) in seen  # k_fir_decim4_cf32
    for t in R.DECIM4_TAPS:
        assert (decim4_variant(t) == (0, 0, 0)) == (t >= 513)


# ---------------- polyphase resampler ------------------------------------

def _plane_floats(elems):
    e = elems - 1
    return (e + ((e >> 4) << 1) + 4) & ~3


def resamp_tiled_lds(interp, decim, n_taps):
    span = 511 * decim // interp + n_taps // interp + 2
    return (2 * _plane_floats(span) + n_taps) * 4


def _resamp(gpu, oracle_lib, knobs, env, interp, decim, n_taps, family,
            caps=CAPS):
    taps, x, ref, a_re, a_im = R.resamp_case(interp, decim, n_taps)
    f = gpu.Resampler(interp, decim, taps)
    got, *counts = run_caps(knobs, env, lambda: f.filter(x, R.N_OUT_512),
                            caps)
    _, *oc = oracle_lib.resamp_cf32(interp, decim, taps, x, R.N_OUT_512)
    check_fir_class(family, f"{interp}:{decim}x{n_taps}", got, counts, oc,
                    ref, a_re, a_im, n_taps // interp)
    return f


@pytest.mark.parametrize("interp,decim,n_taps", R.RESAMP_CASES)
def test_resamp_tiled(gpu, oracle_lib, knobs, interp, decim, n_taps):
    assert resamp_tiled_lds(interp, decim, n_taps) <= 64 * 1024
    f = _resamp(gpu, oracle_lib, knobs, {}, interp, decim, n_taps,
                "resamp/tiled")
    assert f.variant() == (0, 0, 0)


@pytest.mark.parametrize("n_taps", R.RESAMP_1TO4_TAPS)
def test_resamp_1to4_mfma_route(gpu, oracle_lib, knobs, n_taps):
    """1:4 runs the MFMA decim kernel through an input pointer rebased by
    -3; the host path stages the input at the start of its allocation."""
    f = _resamp(gpu, oracle_lib, knobs, {}, 1, 4, n_taps, "resamp/1to4mfma")
    # 513 taps has no sub-filter and takes the tiled kernel by itself
    assert f.variant() == decim4_variant(n_taps)


@pytest.mark.parametrize("n_taps", R.RESAMP_1TO4_TAPS)
def test_resamp_1to4_tiled_route(gpu, oracle_lib, knobs, n_taps):
    assert resamp_tiled_lds(1, 4, n_taps) <= 64 * 1024
    _resamp(gpu, oracle_lib, knobs, {"FSDR_DECIM_MFMA": "0"}, 1, 4, n_taps,
            "resamp/1to4tiled")


def test_resamp_1to4_covers_decim_switch_table(gpu):
    seen = {gpu.Resampler(1, 4, R.resamp_case(1, 4, t)[0]).variant()[0]
            for t in R.RESAMP_1TO4_TAPS}
    assert seen - {0} == set(DECIM_KK)


def test_resamp_naive_by_lds_need(gpu, oracle_lib, knobs):
    """D/I >= 32: the tiled span needs more than 64 KiB of LDS, so the
    launch takes k_resamp_cf32 (grid-stride, no tile loop) by itself."""
    interp, decim, n_taps = R.RESAMP_NAIVE
    assert resamp_tiled_lds(interp, decim, n_taps) > 64 * 1024
    _resamp(gpu, oracle_lib, knobs, {}, interp, decim, n_taps,
            "resamp/naive", caps=(None,))


def test_resamp_naive_by_knob(gpu, oracle_lib, knobs):
    _resamp(gpu, oracle_lib, knobs, {"FSDR_RESAMP_TILED": "0"}, 5, 3, 40,
            "resamp/naive", caps=(None,))


# ---------------- complex-tap and real FIR -------------------------------

@pytest.mark.parametrize("n_taps", R.FIRCC_TAPS)
def test_fir_ccf32(gpu, oracle_lib, knobs, n_taps):
    taps, x, ref, a_re, a_im = R.fircc_case(n_taps)
    f = gpu.FirCC(taps)
    got, *counts = run_caps(knobs, {}, lambda: f.filter(x, R.N_OUT_1024))
    _, *oc = oracle_lib.fir_ccf32(taps, x, R.N_OUT_1024)
    check_fir_class("fir_ccf32", n_taps, got, counts, oc, ref, a_re, a_im,
                    n_taps, complex_taps=True)


@pytest.mark.parametrize("n_taps", R.FIRF32_TAPS)
def test_fir_f32(gpu, oracle_lib, knobs, n_taps):
    taps, x, ref, a_re, a_im = R.firf32_case(n_taps)
    f = gpu.FirF32(taps)
    got, *counts = run_caps(knobs, {}, lambda: f.filter(x, R.N_OUT_1024))
    _, *oc = oracle_lib.fir_f32(taps, x, R.N_OUT_1024)
    check_fir_class("fir_f32", n_taps, got, counts, oc, ref, a_re, a_im,
                    n_taps)


# ---------------- XlatingFir ---------------------------------------------

def xlating_tiled_lds(decim, n_taps):
    span = 511 * decim + n_taps + 2
    return (2 * _plane_floats(span) + 2 * n_taps) * 4


@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "naive"])
@pytest.mark.parametrize("n_taps", R.XLATING_TAPS)
@pytest.mark.parametrize("decim", R.XLATING_DECIMS)
def test_xlating(gpu, oracle_lib, knobs, decim, n_taps, tiled):
    """Two consecutive calls on one handle: the second starts at phase
    index k0 = produced of the first (the carried rotator phase). The
    5e-4 is test_xlating_fir_parity's: the kernels use the fast __sincosf,
    whose error is unmeasured; a single wrong product is >= 0.25."""
    taps, x, y0, y1, _, _ = R.xlating_case(decim, n_taps)
    fits = xlating_tiled_lds(decim, n_taps) <= 64 * 1024
    assert fits == (decim != 32)  # D = 32 falls back by itself
    env = {} if tiled else {"FSDR_XLATING_TILED": "0"}

    def run():
        f = gpu.XlatingFir(taps, decim, R.XLATING_OFFSET, R.XLATING_FS)
        g0, *c0 = f.filter(x, R.N_OUT_512)
        g1, *c1 = f.filter(x, R.N_OUT_512)
        return g0, g1, tuple(c0), tuple(c1)

    caps = CAPS if (tiled and fits) else (None,)
    g0, g1, c0, c1 = run_caps(knobs, env, run, caps)
    bpf, _ = R.xlating_params(taps, decim, R.XLATING_OFFSET, R.XLATING_FS)
    _, *oc = oracle_lib.decim_fir_ccf32(decim, bpf, x, R.N_OUT_512)
    assert c0 == c1 == tuple(oc)
    worst = 0.0
    for g, y in ((g0, y0), (g1, y1)):
        assert g.size == y.size
        worst = max(worst, float(np.abs(g - y).max())
                    / max(1.0, float(np.abs(y).max())))
    report("xlating/" + ("tiled" if tiled and fits else "naive"),
           f"D{decim}x{n_taps}", worst)
    assert worst <= 5e-4


# ---------------- device-buffer helpers ----------------------------------

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

        def get(self, addr, dtype, count):
            gpu.synchronize()
            out = np.zeros(count, dtype)
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


# ---------------- FFT ------------------------------------------------------

def _fft_bulk(gpu, dev, knobs, n, inverse, shift, norm):
    x, ref = R.fft_case(n, inverse, shift, norm)
    frames = x.size // n
    assert frames == 3 * R.fft_fpb(n) + 1
    d_in, d_out = dev.alloc(x.nbytes), dev.alloc(x.nbytes)
    d_mag = dev.alloc(x.size * 4)
    dev.put(d_in, x)
    f = gpu.Fft(n, inverse, shift, norm)

    def run():
        # poison the outputs so a frame that is not written shows
        dev.put(d_out, np.full(x.size, np.nan, np.complex64))
        dev.put(d_mag, np.full(x.size, np.nan, np.float32))
        f.bulk_dev(d_in, d_out, frames, d_mag)
        return (dev.get(d_out, np.complex64, x.size),
                dev.get(d_mag, np.float32, x.size))

    spec, mag = run_caps(knobs, {}, run, FFT_CAPS)
    rel = float(R.rel_l2_per_frame(spec, ref, n).max())
    mode = f"n{n}" + ("i" if inverse else "") + ("s" if shift else "") + (
        "n" if norm is not None else "")
    report("fft_bulk", mode, rel)
    assert rel < 1e-4
    assert_mag(mag, spec)


@pytest.mark.parametrize("n", R.FFT_LENS)
def test_fft_bulk_forward(gpu, dev, knobs, n):
    _fft_bulk(gpu, dev, knobs, n, False, False, None)


@pytest.mark.parametrize("inverse,shift,norm", R.FFT_MODES)
@pytest.mark.parametrize("n", R.FFT_ODD_LOG2)
def test_fft_bulk_modes_odd_log2(gpu, dev, knobs, n, inverse, shift, norm):
    """Odd log2 lengths end in the radix-2 stage, the only user of the
    inverse twiddle conjugation in cmul_tw."""
    _fft_bulk(gpu, dev, knobs, n, inverse, shift, norm)


@pytest.mark.parametrize("n,frames", [(4, 1), (4, 33), (4096, 1),
                                      (4096, 33)])
def test_fft_filter_dev_quantum(gpu, oracle_lib, dev, knobs, n, frames):
    """fsdr_filter_dev at the shortest and longest length: one frame, and
    33 frames against the 32-frame quantum."""
    x, ref = R.fft_case(n, frames=frames)
    d_in, d_out = dev.alloc(x.nbytes), dev.alloc(x.nbytes)
    dev.put(d_in, x)
    dev.put(d_out, np.full(x.size, np.nan, np.complex64))
    f = gpu.Fft(n)
    c, p, s = f.filter_dev(d_in, x.size, d_out, x.size)
    _, m = oracle_lib.fft_block(n, x, x.size)
    assert c == p == m == min(frames, 32) * n
    assert s == gpu.BOTH_SUFFICIENT
    got = dev.get(d_out, np.complex64, x.size)
    rel = float(R.rel_l2_per_frame(got[:m], ref[:m], n).max())
    report("fft_filter_dev", f"n{n}x{frames}", rel)
    assert rel < 1e-4
    assert np.all(np.isnan(got[m:].real))  # nothing past the quantum


# ---------------- fused chain ----------------------------------------------

CHAIN_ROUTES = {
    "ws": {},
    "ap": {"FSDR_CHAIN_WS": "0"},
    "halves": {"FSDR_CHAIN_WS": "0", "FSDR_CHAIN_ALLPHASE": "0"},
}


def _chain(gpu, oracle_lib, dev, knobs, kk, fft_len, env, name,
           prod=R.CHAIN_PROD, unaligned=False, expect_kk=None):
    nt1, nt2 = R.CHAIN_TAP_PAIRS[kk]
    t1, t2, x, ref = R.chain_case(nt1, nt2, fft_len, prod)
    off = 8 if unaligned else 0  # one sample: 8-byte-odd base
    d_in = dev.alloc(x.nbytes + off) + off
    assert (d_in & 15) == off
    d_out, d_mag = dev.alloc(prod * 8), dev.alloc(prod * 4)
    dev.put(d_in, x)

    def run():
        # FSDR_CHAIN_FUSED is read at create
        ch = gpu.Chain(t1, t2, 4, fft_len)
        assert ch.variant() == (kk if expect_kk is None else expect_kk)
        dev.put(d_out, np.full(prod, np.nan, np.complex64))
        dev.put(d_mag, np.full(prod, np.nan, np.float32))
        counts = ch.run_dev(d_in, x.size, d_out, prod, d_mag, prod)
        return (dev.get(d_out, np.complex64, prod),
                dev.get(d_mag, np.float32, prod), counts)

    spec, mag, counts = run_caps(knobs, env, run)
    _, consumed = oracle_lib.chain_cf32(t1, t2, 4, fft_len, x,
                                        capture=False)
    assert counts == (consumed, prod)
    rel = float(R.rel_l2_per_frame(spec, ref, fft_len).max())
    report(f"chain/{name}", f"K{kk}L{fft_len}", rel)
    assert rel < 2e-4
    assert_mag(mag, spec)


@pytest.mark.parametrize("fft_len", R.CHAIN_FFT_LENS)
@pytest.mark.parametrize("kk", sorted(R.CHAIN_TAP_PAIRS))
def test_chain_default_route(gpu, oracle_lib, dev, knobs, kk, fft_len):
    """ws at 1024, ap below: every K x L of the default route."""
    _chain(gpu, oracle_lib, dev, knobs, kk, fft_len, {},
           "ws" if fft_len == 1024 else "ap")


def test_chain_partial_last_tile(gpu, oracle_lib, dev, knobs):
    """70 frames of 64: 4 full tiles and 6 frames of a fifth."""
    _chain(gpu, oracle_lib, dev, knobs, 80, 64, {}, "ap", prod=70 * 64)


@pytest.mark.parametrize("route", ["ap", "halves"])
@pytest.mark.parametrize("kk", sorted(R.CHAIN_TAP_PAIRS))
def test_chain_1024_routes(gpu, oracle_lib, dev, knobs, kk, route):
    _chain(gpu, oracle_lib, dev, knobs, kk, 1024, CHAIN_ROUTES[route],
           route)


@pytest.mark.parametrize("kk", sorted(R.CHAIN_TAP_PAIRS))
def test_chain_1024_unaligned_input(gpu, oracle_lib, dev, knobs, kk):
    """An 8-byte-odd input base (the ring-carry case) takes the halves
    kernel without any knob."""
    _chain(gpu, oracle_lib, dev, knobs, kk, 1024, {}, "halves_unaligned",
           unaligned=True)


def test_chain_block512(gpu, oracle_lib, dev, knobs):
    """512-thread kernel, 2048-output tiles: 8192 outputs are 4 of them."""
    _chain(gpu, oracle_lib, dev, knobs, 80, 1024,
           {"FSDR_CHAIN_BLOCK512": "1"}, "block512", prod=8 * 1024)


def test_chain_occ8(gpu, oracle_lib, dev, knobs):
    _chain(gpu, oracle_lib, dev, knobs, 80, 1024,
           {"FSDR_CHAIN_WS": "0", "FSDR_CHAIN_ALLPHASE": "0",
            "FSDR_CHAIN_OCC8": "1"}, "occ8")


def test_chain_fft_unfused(gpu, oracle_lib, dev, knobs):
    """Fused filter through the Filter-level MFMA decim kernel, then the
    Stockham kernel."""
    _chain(gpu, oracle_lib, dev, knobs, 80, 1024,
           {"FSDR_CHAIN_FFTFUSE": "0"}, "fftfuse0")


def test_chain_two_stage(gpu, oracle_lib, dev, knobs):
    _chain(gpu, oracle_lib, dev, knobs, 80, 1024,
           {"FSDR_CHAIN_FUSED": "0"}, "fused0", expect_kk=0)


def test_chain_ws_output_combinations(gpu, oracle_lib, dev, knobs):
    """One block owning all five tiles, with both outputs, |X|^2 only and
    neither (NullSink)."""
    nt1, nt2 = R.CHAIN_TAP_PAIRS[80]
    t1, t2, x, ref = R.chain_case(nt1, nt2, 1024)
    prod = R.CHAIN_PROD
    d_in = dev.alloc(x.nbytes)
    d_out, d_mag = dev.alloc(prod * 8), dev.alloc(prod * 4)
    dev.put(d_in, x)
    knobs(cap="1")
    ch = gpu.Chain(t1, t2, 4, 1024)
    assert ch.variant() == 80
    _, consumed = oracle_lib.chain_cf32(t1, t2, 4, 1024, x, capture=False)

    dev.put(d_mag, np.full(prod, np.nan, np.float32))
    assert ch.run_dev(d_in, x.size, d_out, prod, d_mag, prod) == (consumed,
                                                                  prod)
    spec = dev.get(d_out, np.complex64, prod)
    mag_both = dev.get(d_mag, np.float32, prod)
    assert float(R.rel_l2_per_frame(spec, ref, 1024).max()) < 2e-4
    assert_mag(mag_both, spec)

    dev.put(d_mag, np.full(prod, np.nan, np.float32))
    assert ch.run_dev(d_in, x.size, 0, 0, d_mag, prod) == (consumed, prod)
    mag_only = dev.get(d_mag, np.float32, prod)
    assert_mag(mag_only, spec)
    np.testing.assert_array_equal(mag_only, mag_both)

    assert ch.run_dev(d_in, x.size) == (consumed, prod)
    gpu.synchronize()
