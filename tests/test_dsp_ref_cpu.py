"""Keeps tests/dsp_ref.py and its error bound honest without a GPU: on
every case list of test_kernel_variants_gpu.py the KAT-pinned fp32 oracle
must agree with the float64 reference within the derived bound (FIR
class) or the project's 1e-4 relative l2 (FFT, chain). A reference that
indexed a tap or a sample wrongly would be off by >= 0.25 per output on
these inputs."""
import numpy as np
import pytest

import dsp_ref as R


def _check_fir_class(got, counts, ref, a_re, a_im, n_taps, produced,
                     complex_taps=False):
    c, p, s = counts
    assert p == produced == ref.size
    ratio = R.fir_err_ratio(got, ref, a_re, a_im, n_taps, complex_taps)
    assert ratio <= 1.0, f"oracle err / bound = {ratio}"
    return ratio


def test_variant_diagnostics_reject_null_handles(fsdr):
    """fsdr_filter_variant / fsdr_chain_variant are host-only: a null
    handle is an argument error with nothing written, GPU or not."""
    import ctypes
    lib = fsdr.lib()
    kk = ctypes.c_int(-7)
    assert lib.fsdr_filter_variant(None, ctypes.byref(kk), None,
                                   None) == fsdr.ERR_INVALID
    assert lib.fsdr_chain_variant(None, ctypes.byref(kk)) == fsdr.ERR_INVALID
    assert kk.value == -7


def test_gamma_and_bound_scale():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6)
    # the figure the loud-input argument rests on: at 600 taps the bound
    # cannot exceed gamma_601 * 600 (|h|,|x| < 1) = 2.2e-2, and a single
    # product is >= 0.25
    assert R.gamma(601) * 600 < 0.25 / 10


def test_loud_inputs_are_loud():
    taps, x, *_ = R.fir_case(130)
    assert np.abs(taps).min() >= 0.5 and np.abs(taps).max() < 1.0
    for part in (x.real, x.imag):
        assert np.abs(part).min() >= 0.5 and np.abs(part).max() < 1.0


def test_reference_sees_a_single_wrong_product():
    """Dropping one product of one output is far outside the bound."""
    taps, x, ref, a_re, a_im = R.fir_case(600)
    bad = ref.copy()
    bad[1500] -= x[1500 + 7] * float(taps[600 - 1 - 7])
    assert R.fir_err_ratio(bad, ref, a_re, a_im, 600) > 10


@pytest.mark.parametrize("n_taps", R.FIR_TAPS)
def test_fir_oracle_within_bound(oracle_lib, n_taps):
    taps, x, ref, a_re, a_im = R.fir_case(n_taps)
    got, *counts = oracle_lib.fir_cf32(taps, x, R.N_OUT_1024)
    _check_fir_class(got, counts, ref, a_re, a_im, n_taps, R.N_OUT_1024)


@pytest.mark.parametrize("decim,n_taps",
                         [(4, t) for t in R.DECIM4_TAPS]
                         + list(R.DECIM_GENERIC))
def test_decim_oracle_within_bound(oracle_lib, decim, n_taps):
    taps, x, ref, a_re, a_im = R.decim_case(decim, n_taps)
    got, *counts = oracle_lib.decim_fir_cf32(decim, taps, x, R.N_OUT_1024)
    _check_fir_class(got, counts, ref, a_re, a_im, n_taps, R.N_OUT_1024)


@pytest.mark.parametrize("interp,decim,n_taps",
                         list(R.RESAMP_CASES)
                         + [(1, 4, t) for t in R.RESAMP_1TO4_TAPS]
                         + [R.RESAMP_NAIVE])
def test_resamp_oracle_within_bound(oracle_lib, interp, decim, n_taps):
    taps, x, ref, a_re, a_im = R.resamp_case(interp, decim, n_taps)
    got, *counts = oracle_lib.resamp_cf32(interp, decim, taps, x,
                                          R.N_OUT_512)
    _check_fir_class(got, counts, ref, a_re, a_im, n_taps // interp,
                     (R.N_OUT_512 // interp) * interp)
    assert ref.size > 3 * 512  # the last tile exists and is partial
    assert ref.size % 512 != 0


@pytest.mark.parametrize("n_taps", R.FIRCC_TAPS)
def test_fircc_oracle_within_bound(oracle_lib, n_taps):
    taps, x, ref, a_re, a_im = R.fircc_case(n_taps)
    got, *counts = oracle_lib.fir_ccf32(taps, x, R.N_OUT_1024)
    _check_fir_class(got, counts, ref, a_re, a_im, n_taps, R.N_OUT_1024,
                     complex_taps=True)


@pytest.mark.parametrize("n_taps", R.FIRF32_TAPS)
def test_firf32_oracle_within_bound(oracle_lib, n_taps):
    taps, x, ref, a_re, a_im = R.firf32_case(n_taps)
    got, *counts = oracle_lib.fir_f32(taps, x, R.N_OUT_1024)
    _check_fir_class(got, counts, ref, a_re, a_im, n_taps, R.N_OUT_1024)


@pytest.mark.parametrize("n_taps", R.XLATING_TAPS)
@pytest.mark.parametrize("decim", R.XLATING_DECIMS)
def test_xlating_oracle_composition(oracle_lib, decim, n_taps):
    """The oracle has no XlatingFir; its parts (complex-tap decimating
    FIR, iterated rotator) compose to one. The FIR part obeys the derived
    bound; the rotated result the 5e-4 of test_xlating_fir_parity, which
    covers the iterated rotator's drift."""
    taps, x, y0, y1, y_fir, a = R.xlating_case(decim, n_taps)
    bpf, theta = R.xlating_params(taps, decim, R.XLATING_OFFSET,
                                  R.XLATING_FS)
    got, *counts = oracle_lib.decim_fir_ccf32(decim, bpf, x, R.N_OUT_512)
    _check_fir_class(got, counts, y_fir, a, a, n_taps, R.N_OUT_512,
                     complex_taps=True)
    rot0, phase = oracle_lib.rotator(float(theta), got)
    rot1, _ = oracle_lib.rotator(float(theta), got, phase=phase)
    for rot, y in ((rot0, y0), (rot1, y1)):
        assert np.abs(rot - y).max() <= 5e-4 * max(1.0, np.abs(y).max())
    # a phase index off by one is visible at that tolerance
    k = np.arange(y_fir.size)
    off = y_fir * np.exp(1j * float(theta) * (k + 2))
    assert np.abs(off - y0).max() > 100 * 5e-4 * max(1.0, np.abs(y0).max())


def _oracle_fft(oracle_lib, n, x, inverse, shift, norm):
    """oracle.fft_block keeps the block's 32-frame quantum; feed it in
    quanta."""
    parts = []
    for at in range(0, x.size, 32 * n):
        seg = x[at:at + 32 * n]
        out, m = oracle_lib.fft_block(n, seg, seg.size, inverse, shift, norm)
        assert m == seg.size
        parts.append(out)
    return np.concatenate(parts)


@pytest.mark.parametrize("n", R.FFT_LENS)
def test_fft_oracle_forward(oracle_lib, n):
    x, ref = R.fft_case(n)
    got = _oracle_fft(oracle_lib, n, x, False, False, None)
    assert R.rel_l2_per_frame(got, ref, n).max() < 1e-4


@pytest.mark.parametrize("inverse,shift,norm", R.FFT_MODES)
@pytest.mark.parametrize("n", R.FFT_ODD_LOG2)
def test_fft_oracle_modes(oracle_lib, n, inverse, shift, norm):
    x, ref = R.fft_case(n, inverse, shift, norm)
    got = _oracle_fft(oracle_lib, n, x, inverse, shift, norm)
    assert R.rel_l2_per_frame(got, ref, n).max() < 1e-4


@pytest.mark.parametrize("n,frames", [(4, 1), (4, 33), (4096, 1),
                                      (4096, 33)])
def test_fft_oracle_quantum(oracle_lib, n, frames):
    """The fsdr_filter_dev shapes: the block transforms at most 32 frames
    per call."""
    x, ref = R.fft_case(n, frames=frames)
    got, m = oracle_lib.fft_block(n, x, x.size)
    assert m == min(frames, 32) * n
    assert R.rel_l2_per_frame(got, ref[:m], n).max() < 1e-4


@pytest.mark.parametrize("fft_len", R.CHAIN_FFT_LENS)
@pytest.mark.parametrize("kk", sorted(R.CHAIN_TAP_PAIRS))
def test_chain_oracle(oracle_lib, kk, fft_len):
    nt1, nt2 = R.CHAIN_TAP_PAIRS[kk]
    t1, t2, x, ref = R.chain_case(nt1, nt2, fft_len)
    got, consumed = oracle_lib.chain_cf32(t1, t2, 4, fft_len, x)
    assert got.size == ref.size == R.CHAIN_PROD
    assert consumed == 4 * R.CHAIN_PROD
    assert R.rel_l2_per_frame(got, ref, fft_len).max() < 1e-4


@pytest.mark.parametrize("prod,fft_len", [(70 * 64, 64), (8 * 1024, 1024)])
def test_chain_oracle_other_lengths(oracle_lib, prod, fft_len):
    """70 frames of 64 (partial last tile) and the 8-tile BLOCK512 shape."""
    nt1, nt2 = R.CHAIN_TAP_PAIRS[80]
    t1, t2, x, ref = R.chain_case(nt1, nt2, fft_len, prod)
    got, consumed = oracle_lib.chain_cf32(t1, t2, 4, fft_len, x)
    assert got.size == ref.size == prod and consumed == 4 * prod
    assert R.rel_l2_per_frame(got, ref, fft_len).max() < 1e-4
    assert np.array_equal(R.chain(t1, t2, 4, fft_len, x), ref)
