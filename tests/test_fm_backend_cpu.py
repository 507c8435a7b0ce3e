"""FM receiver back end, the parts that need no GPU: the multirate tap
designer against the oracle, the float64 reference (tests/fm_ref.py)
against the oracle's fp32 resampler, the reference's signed-zero first
samples and input margins, and the constructor checks the ABI makes
before it looks for a device."""
import ctypes

import numpy as np
import pytest

import dsp_ref as R
import fm_ref as F

F32P = ctypes.POINTER(ctypes.c_float)


def _err(fsdr):
    return fsdr.lib().fsdr_last_error().decode()


@pytest.mark.parametrize("interp,decim,half",
                         [(3, 2, 6), (6, 25, 12), (1, 5, 12), (1, 1, 12)])
def test_kaiser_multirate_matches_oracle(fsdr, oracle_lib, interp, decim,
                                         half):
    tp = fsdr.kaiser_multirate(interp, decim, half, 1e-4)
    to = oracle_lib.kaiser_multirate_f32(interp, decim, half, 1e-4)
    assert tp.size == to.size
    np.testing.assert_array_equal(tp, to)


def test_kaiser_multirate_defaults_and_query(fsdr):
    # half_len = 12, max_ripple = 1e-4: 2 * 12 * interp taps (basic.rs:431)
    assert fsdr.kaiser_multirate(6, 25).size == 144
    np.testing.assert_array_equal(fsdr.kaiser_multirate(6, 25),
                                  fsdr.kaiser_multirate(6, 25, 12, 1e-4))
    lib = fsdr.lib()
    # query with NULL, and a short buffer is left alone
    assert lib.fsdr_firdes_kaiser_multirate_f32(3, 2, 6, 1e-4, None, 0) == 36
    buf = np.full(4, 7.0, np.float32)
    assert lib.fsdr_firdes_kaiser_multirate_f32(
        3, 2, 6, 1e-4, buf.ctypes.data_as(F32P), 4) == 36
    assert np.all(buf == 7.0)


@pytest.mark.parametrize("args", [(0, 2, 6), (3, 0, 6), (3, 2, 0)])
def test_kaiser_multirate_rejects_what_the_reference_asserts(fsdr, args):
    # basic.rs:418-423
    lib = fsdr.lib()
    assert lib.fsdr_firdes_kaiser_multirate_f32(*args, 1e-4, None, 0) == 0
    assert "greater than 0" in _err(fsdr)
    with pytest.raises(fsdr.FsdrError):
        fsdr.kaiser_multirate(*args)


@pytest.mark.parametrize("seed", F.ED_SEEDS)
def test_input_margins(seed):
    """The float64 reference keeps every demodulated value >= 0.3 rad
    from 0 and >= 0.34 rad from the +-pi cut (past the stream's first
    sample, whose neighbour is the zero `last`)."""
    x, d = F.demod_case(seed, F.ED_N)
    assert np.abs(x).min() >= 0.5 - 1e-6 and np.abs(x).max() < 1.0 + 1e-6
    assert np.abs(d[1:]).min() >= 0.3
    assert (np.pi - np.abs(d[1:])).min() >= 0.34


def test_reference_sees_a_wrong_neighbour():
    x, d = F.demod_case(0, 4096)
    # x[i-2] in place of x[i-1], a missing conj, swapped atan2 arguments
    p2 = np.concatenate(([0, 0], x[:-2])).astype(np.complex128)
    xx = x.astype(np.complex128)
    for wrong in (np.angle(xx * np.conj(p2)),
                  np.angle(xx * np.concatenate(([0], xx[:-1]))),
                  np.arctan2((xx * np.conj(np.concatenate(([0], xx[:-1]))))
                             .real,
                             (xx * np.conj(np.concatenate(([0], xx[:-1]))))
                             .imag)):
        bad = np.abs(wrong[2:] - d[2:])
        bad = np.minimum(bad, 2 * np.pi - bad)
        assert np.median(bad) > 0.3 and bad.max() > 1e4 * F.E_D


@pytest.mark.parametrize("x0,want,neg", [
    (0.6 + 0.7j, 0.0, False), (0.6 - 0.7j, 0.0, True),
    (-0.6 + 0.7j, 0.0, False), (-0.6 - 0.7j, np.pi, False)])
def test_reference_first_sample_signed_zeros(x0, want, neg):
    """main.rs:99-101 with last = 0+0i: conj is (+0, -0), and the product
    written by components gives +0, -0, +0, pi by the quadrant of x[0]."""
    d = F.demod(np.array([x0], np.complex64))
    assert d.shape == (1,) and d[0] == want
    assert bool(np.signbit(d[0])) == neg
    # a carried neighbour is used as given
    d2 = F.demod(np.array([x0], np.complex64), last=1.0 + 0j)
    assert d2[0] == pytest.approx(np.angle(complex(np.complex64(x0))))


@pytest.mark.parametrize("interp,decim,n_taps",
                         [(1, 5, 22), (1, 4, 128), (3, 2, 6), (6, 25, 144),
                          (2, 7, 10)])
def test_chain_reference_vs_oracle(oracle_lib, interp, decim, n_taps):
    """fm_ref.chain against the oracle's fp32 PolyphaseResamplingFir on
    the demodulated stream rounded to fp32. Bound: dsp_ref's
    gamma(tpp+1) * a for the fp32 dot product, plus u * a because the
    oracle's summands are fl(d), each off from d by at most u |d|."""
    taps = R.loud_f32(np.random.default_rng([9, interp, decim, n_taps]),
                      n_taps)
    x = F.fm_input(5, 3000)
    d32 = F.demod(x).astype(np.float32)
    got, cons, prod, status = oracle_lib.resamp_f32(interp, decim, taps,
                                                    d32, 10 ** 6)
    assert prod > 0 and status == 0
    ref, a, h1 = F.chain(interp, decim, taps, x, prod)
    err = np.abs(got.astype(np.float64) - ref)
    bound = R.gamma(n_taps // interp + 1) * a + R.U * a
    assert np.all(err <= bound), (err / bound).max()
    # the chain bound of the GPU tests contains this one
    assert np.all(F.chain_bound(n_taps, interp, a, h1) >= bound)
    assert np.all(h1 >= 0.5 * (n_taps // interp))


def _taps7():
    t = np.ones(7, np.float32)
    return t, t.ctypes.data_as(F32P)


@pytest.mark.parametrize("create", ["fsdr_resamp_f32_create",
                                    "fsdr_fm_demod_resamp_create"])
def test_constructors_reject_before_the_device_check(fsdr, create):
    """polyphase_resampling_fir.rs:54-56: n_taps % interp. Decided before
    the GPU is looked for, so the message names the argument."""
    fn = getattr(fsdr.lib(), create)
    keep, p = _taps7()
    assert not fn(3, 2, p, 7)
    assert "interp" in _err(fsdr)
    for bad in ((0, 2, p, 6), (3, 0, p, 6), (3, 2, p, 0), (3, 2, None, 6)):
        assert not fn(*bad)
        assert "invalid resampler parameters" in _err(fsdr)


def test_valid_creates_depend_on_the_device_alone(fsdr):
    """Valid arguments: a handle where a device exists, else NULL with
    the no-device message (no CPU fallback)."""
    keep, p = _taps7()
    lib = fsdr.lib()
    have = fsdr.device_count() > 0
    for make in (lambda: lib.fsdr_resamp_f32_create(1, 2, p, 7),
                 lambda: lib.fsdr_fm_demod_resamp_create(1, 2, p, 7),
                 lambda: lib.fsdr_quad_demod_create()):
        h = make()
        if have:
            assert h
            lib.fsdr_filter_destroy(ctypes.c_void_p(h))
        else:
            assert not h and "no HIP device" in _err(fsdr)
    assert lib.fsdr_fm_demod_resamp_fused(None) == 0
