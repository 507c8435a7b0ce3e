"""Plain float64 references of the FM receiver back end: the quadrature
demodulator (examples/fm-receiver/src/main.rs:99-104) and the demod >
resamp2 chain (main.rs:121-129). numpy only, nothing from oracle/. Shared
by test_fm_backend_cpu.py, test_fm_backend_gpu.py and
tools/fm_backend_bench.py.

Inputs (fm_input): Complex32 of magnitude [0.5, 1) whose successive phase
steps are +-uniform[0.3, 2.8] rad. Every demodulated value is then at
least 0.3 rad from 0 and pi - 2.8 > 0.34 rad from the +-pi cut, so a wrong
neighbour, a missing conj or swapped atan2 arguments moves an output by
O(0.3) and no wrap handling is needed. Taps are dsp_ref.loud, so one lost
product moves an output by >= 0.5 * 0.3.

Error bound of the chain, per output k (derived, not tuned):
  |y_gpu - y_ref| <= gamma(tpp+1) * sum_t |h||d|  +  E_D * sum_t |h|
The first term is dsp_ref's bound of the fp32 dot product on the fp32
values the kernel actually sums; the second carries each summand's own
error |d_gpu - d_f64| <= E_D through the taps (second-order terms are
below 1e-13 here). E_D is the one number that cannot be derived on paper:
the f32 product x*conj(p) adds an angle error of a few u = 2^-24, but the
atan2f term is the device math library's. It was measured once with
tools/fm_backend_bench.py over fm_input(s, ED_N) for s in ED_SEEDS through
the staged QuadDemod kernel (profiles/fm_backend.txt: max |d_gpu - d_f64|
= 3.325e-07) and is set to 4x that, rounded up to a power of two; it has
to stay <= 1e-5, four orders of magnitude under a logic error.
"""
import functools

import numpy as np

import dsp_ref

E_D = 2.0 ** -19
assert E_D <= 1e-5

ED_SEEDS = (0, 1, 2, 3)
ED_N = 1 << 16

STEP_MIN, STEP_MAX = 0.3, 2.8


def fm_input(seed, n):
    """(x complex64, read-only) — see the module docstring."""
    r = np.random.default_rng([0xF3, int(seed), int(n)])
    step = r.uniform(STEP_MIN, STEP_MAX, n) * r.choice([-1.0, 1.0], n)
    phase = r.uniform(-np.pi, np.pi) + np.cumsum(step)
    mag = r.uniform(0.5, 1.0, n)
    x = (mag * np.exp(1j * phase)).astype(np.complex64)
    x.setflags(write=False)
    return x


def demod(x, last=0j):
    """d[i] = arg(x[i] * conj(x[i-1])), x[-1] = last, in float64. The
    product is written out by components the way num_complex's Mul does
    (b = conj(p) = (p.re, -p.im); re = a.re*b.re - a.im*b.im, im =
    a.re*b.im + a.im*b.re) so the signed zeros of the first sample of a
    stream (last = 0+0i, b = (+0, -0)) reach atan2 as in the reference."""
    x = np.asarray(x)
    a_re = x.real.astype(np.float64)
    a_im = x.imag.astype(np.float64)
    p_re = np.concatenate(([np.float64(complex(last).real)], a_re[:-1]))
    p_im = np.concatenate(([np.float64(complex(last).imag)], a_im[:-1]))
    b_re, b_im = p_re, -p_im
    re = a_re * b_re - a_im * b_im
    im = a_re * b_im + a_im * b_re
    return np.arctan2(im, re)[: x.size]


def chain(interp, decim, taps, x, produced, last=0j):
    """(y, a, h1): demod then dsp_ref.resamp, the magnitude sums
    a[k] = sum_t |h||d| and the tap sums h1[k] = sum_t |h| of output k."""
    d = demod(x, last)
    y, a, _ = dsp_ref.resamp(interp, decim, taps, d, produced)
    _, h1, _ = dsp_ref.resamp(interp, decim, taps, np.ones(d.size),
                              produced)
    return y, a, h1


def chain_bound(n_taps, interp, a, h1):
    return dsp_ref.gamma(n_taps // interp + 1) * a + E_D * h1


@functools.lru_cache(maxsize=None)
def demod_case(seed, n):
    x = fm_input(seed, n)
    d = demod(x)
    d.setflags(write=False)
    return x, d
