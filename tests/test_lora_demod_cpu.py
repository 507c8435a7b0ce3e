"""CPU checks of the LoRa FFT demodulator's host side against
tests/lora_ref.py: the downchirp table, the ln I0 evaluator the kernel
runs, the call accounting and the constructor's validation. No GPU."""
import numpy as np
import pytest

import lora_ref

ULP1 = float(np.finfo(np.float32).eps)      # one ulp of 1.0 in float32


@pytest.mark.parametrize("sf", [5, 7, 12])
@pytest.mark.parametrize("cfo", [(0, 0.0), (3, 0.25), (-2, -0.4)])
def test_downchirp_matches_reference(fsdr, sf, cfo):
    got = fsdr.lora_downchirp(sf, *cfo)
    want = lora_ref.downchirp(sf, *cfo)
    assert got.dtype == np.complex64 and got.shape == (1 << sf,)
    # the float32 phase arithmetic is identical; sinf/cosf may differ
    d = got.astype(np.complex128) - want.astype(np.complex128)
    worst = max(np.abs(d.real).max(), np.abs(d.imag).max())
    print(f"sf {sf} cfo {cfo}: worst component diff {worst / ULP1:.2f} ulp")
    assert worst <= 2 * ULP1
    assert np.abs(np.abs(got.astype(np.complex128)) - 1.0).max() <= 2 * ULP1


def test_downchirp_is_the_dechirp_of_symbol_zero():
    # what the table is for: build_upchirp(id, sf, 1, false) is the chirp
    # of (id - 1) mod N, the table its conjugate for id = 0, so the product
    # is a tone in bin id and the hard decision is (id - 1) mod N
    for sf in (5, 8):
        n = 1 << sf
        for sym in (0, 1, n // 2, n - 1):
            X = lora_ref.spectrum(lora_ref.upchirp(sym, sf),
                                  lora_ref.downchirp(sf))
            assert lora_ref.raw(X)[0] == sym
            assert lora_ref.hard(X, False)[0] == (sym - 1) % n
            assert lora_ref.hard(X, True)[0] == ((sym - 1) % n) // 4


def test_log_i0_matches_reference_series(fsdr):
    x = np.concatenate([[0.0, 1e-8, 708.999],
                        np.linspace(0.0, 708.999, 2001),
                        np.linspace(19.0, 21.0, 201),       # the seam
                        np.geomspace(1e-6, 700.0, 300)])
    want = lora_ref.log_i0_series(x)
    got = np.array([fsdr.lora_log_i0(v) for v in x])
    rel = np.abs(got - want) / (1.0 + want)
    print(f"ln I0: {x.size} points, worst |d|/(1+lnI0) {rel.max():.3g} "
          f"at x={x[np.argmax(rel)]:.6g}")
    assert np.isfinite(got).all()
    assert (rel <= 1e-12).all()
    assert fsdr.lora_log_i0(0.0) == 0.0


@pytest.mark.parametrize("sf", [5, 12])
def test_count_matches_reference(fsdr, sf):
    n = 1 << sf
    for n_in in (0, n - 1, n, n + 1, 3 * n - 1, 3 * n):
        for n_out in (0, 1, 2, 3, 4):
            assert fsdr.lora_demod_count(sf, n_in, n_out) == \
                lora_ref.count(sf, n_in, n_out), (n_in, n_out)
    # the rule itself
    assert lora_ref.count(sf, 3 * n - 1, 4) == \
        (2 * n, 2, lora_ref.INSUFFICIENT_INPUT)
    assert lora_ref.count(sf, 3 * n, 2) == \
        (2 * n, 2, lora_ref.INSUFFICIENT_OUTPUT)
    assert lora_ref.count(sf, 3 * n, 3) == \
        (3 * n, 3, lora_ref.BOTH_SUFFICIENT)


@pytest.mark.parametrize("sf,mode", [(4, 1), (13, 1), (7, 3), (7, -1)])
def test_create_validation(fsdr, sf, mode):
    lib = fsdr.lib()
    assert lib.fsdr_lora_demod_create(sf, mode) is None
    msg = lib.fsdr_last_error().decode()
    assert ("sf" in msg) if sf != 7 else ("mode" in msg), msg
    with pytest.raises(fsdr.FsdrError):
        fsdr.LoraFftDemod(sf, mode)


def test_host_only_entry_points_reject_bad_sf(fsdr):
    for sf in (4, 13):
        with pytest.raises(fsdr.FsdrError):
            fsdr.lora_downchirp(sf)
        with pytest.raises(fsdr.FsdrError):
            fsdr.lora_demod_count(sf, 10, 10)


def test_reference_soft_properties():
    # the restated LLR branch on a clean symbol: the signs are the Gray
    # bits of the symbol, entries sf..11 are 0, and with the reduced rate
    # the two most significant LLRs cannot be positive
    sf = 7
    x, ids = lora_ref.stream(sf, 12, 2.0, 5)
    X = lora_ref.spectrum(x, lora_ref.downchirp(sf))
    for reduced in (False, True):
        llr, bound, a_max, da_max = lora_ref.soft(X, sf, reduced)
        s = ((ids - 1) % (1 << sf)) // (4 if reduced else 1)
        g = s ^ (s >> 1)
        bits = (g[:, None] >> (sf - 1 - np.arange(sf))[None, :]) & 1
        assert ((llr[:, :sf] > 0) == bits.astype(bool)).all()
        assert (llr[:, sf:] == 0).all()
        if reduced:
            assert (llr[:, :2] <= 0).all()
        assert (bound > 0).all() and (a_max > 0).all()
