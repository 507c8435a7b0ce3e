"""Plain float64 references of the FIR-class, FFT and chain operations,
shared by test_dsp_ref_cpu.py and test_kernel_variants_gpu.py. numpy only,
nothing from oracle/: the oracle accumulates in fp32 like the kernels do,
so it cannot tell a kernel's rounding from a kernel's mistake. The CPU
test pins the oracle against these references, the GPU test the kernels.

Every FIR-class function returns (y, a_re, a_im): the complex128 (or
float64) result and the per-output magnitude sums of its dot products,
  real taps     a_re[k] = sum_t |h_t| |Re x_t|,  a_im likewise
  complex taps  a_re[k] = a_im[k] = sum_t (|h_re|+|h_im|) (|x_re|+|x_im|)

Error bound (derived, not tuned). An fp32 dot product of T terms, in any
summation order, with or without fma or an f32 MFMA, has
|err| <= gamma_T * a[k], gamma_n = n u / (1 - n u), u = 2^-24 (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5: the
bound holds for every order of evaluation). Zero padding adds exact
terms. One more u covers the comparison against values rounded to fp32,
so the tests use gamma_{T+1}; a complex-tap component is a 2T-term dot
product, gamma_{2T+1}. Asserted per output and per component.

Loud inputs: every tap and every sample component is +-uniform[0.5, 1),
so one dropped, duplicated or shifted product moves an output by at least
0.25, ~20x above the bound's maximum (1.3e-2 at 600 taps).
"""
import functools

import numpy as np

U = 2.0 ** -24

# One tile = 1024 outputs (FIR, decim, chain, fir_f32, fir_ccf32) or 512
# (resampler, xlating). Three full tiles and a partial one.
N_OUT_1024 = 3 * 1024 + 37
N_OUT_512 = 3 * 512 + 37

FIR_TAPS = (1, 17, 18, 33, 34, 49, 50, 65, 66, 81, 82, 129, 130, 257, 258,
            513, 514, 600, 1025)
DECIM4_TAPS = (1, 2, 3, 5, 6, 7, 20, 21, 32, 33, 64, 65, 68, 69, 128, 129,
               132, 133, 256, 257, 260, 261, 512, 513, 1000)
DECIM_GENERIC = ((2, 33), (3, 33), (8, 33))
RESAMP_CASES = ((3, 2, 6), (2, 1, 2), (1, 3, 2), (5, 3, 40), (4, 7, 48),
                (7, 1, 70))
RESAMP_1TO4_TAPS = (4, 20, 21, 68, 69, 132, 133, 260, 261, 512, 513)
RESAMP_NAIVE = (1, 32, 32)  # tiled LDS need > 64 KiB
FIRCC_TAPS = (1, 2, 64, 127, 300)
FIRF32_TAPS = (1, 2, 64, 127, 300)
XLATING_DECIMS = (2, 3, 4, 5, 32)
XLATING_TAPS = (1, 63, 64, 200)
XLATING_OFFSET, XLATING_FS = 12_000.0, 1_000_000.0
FFT_LENS = (4, 8, 16, 32, 128, 512, 2048, 4096)
FFT_ODD_LOG2 = (8, 32, 128, 512, 2048)
# (inverse, fft_shift, normalize) beyond the plain forward transform
FFT_MODES = ((True, False, None), (False, True, None), (True, True, None),
             (False, False, 0.37))
CHAIN_TAP_PAIRS = {20: (8, 8), 32: (30, 30), 48: (60, 60), 80: (127, 127),
                   144: (250, 250)}  # fused MFMA K -> (nt1, nt2)
CHAIN_FFT_LENS = (64, 128, 256, 512, 1024)
CHAIN_PROD = 5 * 1024


def gamma(n):
    return n * U / (1.0 - n * U)


def fir_bound(n_taps, a, complex_taps=False):
    """Largest fp32 error of one output component with magnitude sum a."""
    return gamma((2 * n_taps if complex_taps else n_taps) + 1) * a


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def loud(r, shape):
    return r.uniform(0.5, 1.0, shape) * r.choice([-1.0, 1.0], shape)


def loud_f32(r, n):
    return loud(r, n).astype(np.float32)


def loud_c64(r, n):
    return (loud(r, (n, 2)) @ [1, 1j]).astype(np.complex64)


def _widen(a):
    a = np.asarray(a)
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def _mag(a):
    """|re| + |im| of complex a, |a| of real a."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return np.abs(a.real) + np.abs(a.imag)
    return np.abs(a).astype(np.float64)


def fir(taps, x):
    """y[k] = sum_t x[k+t] h[T-1-t] for every full window."""
    h, xx = _widen(taps), _widen(x)
    # np.convolve(x, h, 'valid')[k] = sum_j x[k+T-1-j] h[j]; t = T-1-j
    y = np.convolve(xx, h, "valid")
    if np.iscomplexobj(h):
        a = np.convolve(_mag(xx), _mag(h), "valid")
        return y, a, a
    ah = np.abs(h)
    if np.iscomplexobj(xx):
        return (y, np.convolve(np.abs(xx.real), ah, "valid"),
                np.convolve(np.abs(xx.imag), ah, "valid"))
    return y, np.convolve(np.abs(xx), ah, "valid"), np.zeros(y.size)


def decim_fir(decim, taps, x):
    """y[k] = sum_t x[D-1+kD+t] h[T-1-t]."""
    return tuple(v[decim - 1::decim] for v in fir(taps, x))


def resamp(interp, decim, taps, x, produced):
    """y[k] = sum_t x[kD//I + t] h[I(T/I - t - 1) + (kD)%I], k < produced."""
    h, xx = _widen(taps), _widen(x)
    tpp = h.size // interp
    k = np.arange(produced)
    bank = (k * decim) % interp
    start = (k * decim) // interp
    t = np.arange(tpp)
    win = xx[start[:, None] + t[None, :]]
    hh = h[interp * (tpp - t[None, :] - 1) + bank[:, None]]
    y = (win * hh).sum(axis=1)
    ah = np.abs(hh)
    return (y, (np.abs(win.real) * ah).sum(axis=1),
            (np.abs(win.imag) * ah).sum(axis=1))


def xlating_params(taps, decim, offset, fs):
    """Band-pass taps (complex64) and rotator increment (float32), formed
    in float32 in the order fsdr_xlating_fir_cf32_create uses."""
    taps = np.asarray(taps, np.float32)
    tau = np.float32(6.2831853071795864769)
    i = np.arange(taps.size, dtype=np.float32)
    ang = i * tau * np.float32(offset) / np.float32(fs)
    bpf = np.empty(taps.size, np.complex64)
    bpf.real = np.cos(ang) * taps
    bpf.imag = np.sin(ang) * taps
    theta = -tau * np.float32(offset) * np.float32(decim) / np.float32(fs)
    return bpf, np.float32(theta)


def xlating(taps, decim, offset, fs, x, k0=0):
    """Decimating FIR with the band-pass taps in complex128, output k
    times exp(i theta (k0+k+1)). Returns (y, y_fir, a): the rotated and
    the unrotated result and the magnitude sums of the latter."""
    bpf, theta = xlating_params(taps, decim, offset, fs)
    y_fir, a, _ = decim_fir(decim, bpf, x)
    k = np.arange(y_fir.size, dtype=np.float64)
    return y_fir * np.exp(1j * float(theta) * (k0 + k + 1)), y_fir, a


def fft(x, n, inverse=False, shift=False, norm=None):
    """Per-frame transform with the Fft block's conventions: unnormalized
    in both directions, input halves swapped when inverse and shift, output
    halves when forward and shift, then the optional factor."""
    f = _widen(x).reshape(-1, n).astype(np.complex128)
    if inverse and shift:
        f = np.roll(f, -(n // 2), axis=1)
    f = np.fft.ifft(f, axis=1) * n if inverse else np.fft.fft(f, axis=1)
    if not inverse and shift:
        f = np.roll(f, -(n // 2), axis=1)
    if norm is not None:
        f = f * float(np.float32(norm))
    return f.reshape(-1)


def chain(taps1, taps2, decim, fft_len, x):
    """Fir(taps1) -> DecimatingFir(decim, taps2) -> forward fft_len DFT per
    full frame, everything in float64."""
    y1, _, _ = fir(taps1, x)
    y2, _, _ = decim_fir(decim, taps2, y1)
    frames = y2.size // fft_len
    return fft(y2[:frames * fft_len], fft_len)


def rel_l2_per_frame(got, ref, n):
    g = np.asarray(got, np.complex128).reshape(-1, n)
    r = np.asarray(ref, np.complex128).reshape(-1, n)
    return np.linalg.norm(g - r, axis=1) / np.linalg.norm(r, axis=1)


def fir_err_ratio(got, ref, a_re, a_im, n_taps, complex_taps=False):
    """max over outputs and components of |got - ref| / bound; the test
    asserts <= 1. Components whose bound is 0 must be exact."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    worst = 0.0
    parts = [(got.real, ref.real, a_re)]
    if np.iscomplexobj(ref):
        parts.append((got.imag, ref.imag, a_im))
    for g, r, a in parts:
        err = np.abs(g.astype(np.float64) - r)
        b = fir_bound(n_taps, a, complex_taps)
        assert np.all(err[b == 0] == 0)
        if np.any(b > 0):
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    return worst


# ---- shared cases: inputs and their reference, computed once per shape ----

def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def fir_case(n_taps):
    r = _rng(1, n_taps)
    taps = loud_f32(r, n_taps)
    x = loud_c64(r, N_OUT_1024 + n_taps - 1)
    return _freeze(taps, x, *fir(taps, x))


@functools.lru_cache(maxsize=None)
def decim_case(decim, n_taps):
    r = _rng(2, decim, n_taps)
    taps = loud_f32(r, n_taps)
    x = loud_c64(r, decim * N_OUT_1024 + n_taps - 1)
    return _freeze(taps, x, *decim_fir(decim, taps, x))


@functools.lru_cache(maxsize=None)
def resamp_case(interp, decim, n_taps):
    """The block emits multiples of interp: produced is N_OUT_512 rounded
    down to one, still three full tiles and a partial one."""
    r = _rng(3, interp, decim, n_taps)
    taps = loud_f32(r, n_taps)
    produced = (N_OUT_512 // interp) * interp
    n_in = (N_OUT_512 * decim + interp) // interp + n_taps // interp + 2
    x = loud_c64(r, n_in)
    return _freeze(taps, x, *resamp(interp, decim, taps, x, produced))


@functools.lru_cache(maxsize=None)
def fircc_case(n_taps):
    r = _rng(4, n_taps)
    taps = loud_c64(r, n_taps)
    x = loud_c64(r, N_OUT_1024 + n_taps - 1)
    return _freeze(taps, x, *fir(taps, x))


@functools.lru_cache(maxsize=None)
def firf32_case(n_taps):
    r = _rng(5, n_taps)
    taps = loud_f32(r, n_taps)
    x = loud_f32(r, N_OUT_1024 + n_taps - 1)
    return _freeze(taps, x, *fir(taps, x))


@functools.lru_cache(maxsize=None)
def xlating_case(decim, n_taps):
    """(taps, x, y_first_call, y_second_call, y_fir, a): the same span fed
    twice, the second call starting at phase index k0 = produced."""
    r = _rng(6, decim, n_taps)
    taps = loud_f32(r, n_taps)
    x = loud_c64(r, decim * N_OUT_512 + n_taps - 1)
    y0, y_fir, a = xlating(taps, decim, XLATING_OFFSET, XLATING_FS, x)
    y1, _, _ = xlating(taps, decim, XLATING_OFFSET, XLATING_FS, x,
                       k0=y0.size)
    return _freeze(taps, x, y0, y1, y_fir, a)


def fft_fpb(n):
    return min(16, max(1, 1024 // n))


@functools.lru_cache(maxsize=None)
def fft_input(n, frames):
    (x,) = _freeze(loud_c64(_rng(7, n, frames), n * frames))
    return x


@functools.lru_cache(maxsize=None)
def fft_case(n, inverse=False, shift=False, norm=None, frames=None):
    frames = 3 * fft_fpb(n) + 1 if frames is None else frames
    x = fft_input(n, frames)
    return _freeze(x, fft(x, n, inverse, shift, norm))


@functools.lru_cache(maxsize=None)
def chain_input(nt1, nt2, prod):
    """Taps and exactly the input that yields `prod` decimated samples
    (plus 3 that the decimator must leave)."""
    r = _rng(8, nt1, nt2, prod)
    t1, t2 = loud_f32(r, nt1), loud_f32(r, nt2)
    x = loud_c64(r, 4 * prod + nt1 + nt2 - 2 + 3)
    return _freeze(t1, t2, x)


@functools.lru_cache(maxsize=None)
def _chain_y2(nt1, nt2, prod):
    t1, t2, x = chain_input(nt1, nt2, prod)
    y1, _, _ = fir(t1, x)
    y2, _, _ = decim_fir(4, t2, y1)
    assert y2.size == prod
    return y2


@functools.lru_cache(maxsize=None)
def chain_case(nt1, nt2, fft_len, prod=CHAIN_PROD):
    """(t1, t2, x, spectra); prod must be a multiple of fft_len."""
    assert prod % fft_len == 0
    t1, t2, x = chain_input(nt1, nt2, prod)
    (ref,) = _freeze(fft(_chain_y2(nt1, nt2, prod), fft_len))
    return t1, t2, x, ref
