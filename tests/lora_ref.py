"""Float64 numpy restatement of the LoRa FFT demodulator's arithmetic, the
reference of tests/test_lora_demod_{cpu,gpu}.py. Lines cited are the
reference's examples/lora/src/{fft_demod,utils}.rs.

The demodulator takes one symbol of N = 2^sf samples, multiplies it by a
downchirp table, takes the N-point forward FFT and |X|^2, and reduces over
the bins (raw argmax, hard symbol, soft LLRs). Everything here that the
GPU is compared with starts from

    X_ref = f64 DFT of the f32 product sample * downchirp,

so the budget below is about the kernel's FFT and what follows it.

Error budget
------------
The project's FFT tolerance (DESIGN.md, section c) is, per symbol,

    ||X_gpu - X_ref||_2 <= 1e-4 * ||X_ref||_2 =: E.

With d_n = |X_gpu,n| - |X_ref,n|:

 * per bin |d_n| <= |X_gpu,n - X_ref,n| <= ||X_gpu - X_ref||_2 <= E;
 * for a sum S = sum_{n in B} |X_n|^2 over any set of bins B,
   dS = sum 2 |X_n| d_n + d_n^2 <= 2 ||X|| ||d|| + ||d||^2 <= 2 ||X|| E + E^2
   (Cauchy-Schwarz), so the signal sum and the noise sum of compute_llrs
   (fft_demod.rs:132-144) each move by at most dS;
 * hard decisions: the argmax is the same on both sides wherever the two
   largest |X_ref,n| differ by more than 2E (`margin_ok`);
 * soft, not clipped: a_n = K |X_n| with K = sqrt(ps N) / pn, ps = sig / N,
   pn = noise / (N - 3). To first order K moves by the relative amount
   rho = dS / (2 sig) + dS / noise, so da_n <= K E + a_n rho. ll_n =
   ln I0(a_n) and d ln I0 / da = I1 / I0 < 1, so dll_n <= da_n;
 * soft, clipped (some a_n >= 709): ll_n = N |X_n|^2, so
   dll_n <= N (2 |X_n| E + E^2);
 * an LLR is a difference of two maxima over bins, each of which moves by
   at most max_n dll_n: |dLLR| <= 2 max_n dll_n.

The f32 rounding of |X|^2 (2^-23 relative) and of ln I0 (1e-12, checked on
the CPU) are four and eight orders below the 1e-4 of E and are not added.
Both sides take the same branch where |709 - max_n a_n| > max_n da_n
(`regime_ok`).
"""
import numpy as np

F32 = np.float32
MAX_SF = 12
RAW, HARD, SOFT = 0, 1, 2
INSUFFICIENT_INPUT, INSUFFICIENT_OUTPUT, BOTH_SUFFICIENT = 0, 1, 2
FFT_TOL = 1e-4


def symbols_per_block(sf):
    """Symbols one block of the kernel holds (kernel layout)."""
    n = 1 << sf
    return 1 if n >= 1024 else min(16, 1024 // n)


# ---- chirps (utils.rs:884-914, 1053-1057; fft_demod.rs:280-283, 384-398) ----

def upchirp(sym_id, sf, preamble=False):
    """build_upchirp(id, sf, 1, preamble): float32 arithmetic in the
    reference's operation order."""
    n = 1 << sf
    if not preamble:
        sym_id = (sym_id - 1) % n           # my_modulo(id - 1, n)
    n_fold = n - sym_id
    nf = F32(n)
    two_pi = F32(2.0) * F32(np.pi)
    j = np.arange(n)
    t = j.astype(F32) / F32(1.0)
    off = np.where(j < n_fold, F32(0.5), F32(1.5)).astype(F32)
    quad = (t * t) / (F32(2.0) * nf)
    lin = (F32(sym_id) / nf - off) * t
    ph = two_pi * (quad + lin)
    assert ph.dtype == F32
    return (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64)


def downchirp(sf, cfo_int=0, cfo_frac=0.0, preamble=False):
    """The table of the demodulator: conj(upchirp(0)) in float64, rotated by
    e^{-2 pi i (cfo_int + cfo_frac) / N * j}, rounded to float32.
    preamble=True is the RAW table (build_ref_chirps)."""
    n = 1 << sf
    base = np.conj(upchirp(0, sf, preamble).astype(np.complex128))
    th = -2.0 * np.pi * (float(cfo_int) + cfo_frac) / float(n) * np.arange(n)
    return (base * (np.cos(th) + 1j * np.sin(th))).astype(np.complex64)


# ---- ln I0 by the reference's series (fft_demod.rs:9-23) --------------------

def log_i0_series(x):
    """ln(bessel_I0(x)) with the reference's loop, vectorized: every
    element keeps adding terms until its own sum stops changing.

    One deliberate difference: the reference forms addend * base / j^2
    left to right, and for x above ~706 the product addend * base passes
    1.8e308 although the term itself does not, so its sum becomes inf and
    the loop stops there (the `!sum.is_finite()` exit). The same series
    with the term formed as addend * (base / j^2) stays finite up to 709,
    which is what an evaluator can be held to; below ~706 the two differ
    by an ulp per term."""
    x = np.atleast_1d(np.asarray(x, np.float64))
    base = x * x / 4.0
    addend = np.ones_like(x)
    total = np.ones_like(x)
    live = np.ones(x.shape, bool)
    j = 1
    while live.any():
        addend = np.where(live, addend * (base / float(j * j)), addend)
        new = total + addend
        live &= new != total
        total = np.where(live, new, total)
        j += 1
    return np.log(total)


# ---- counts (decimating_fir.rs:71-78 with D = N and one tap) ----------------

def count(sf, n_in, n_out):
    n = 1 << sf
    can = n_in // n
    if can > n_out:
        prod, st = n_out, INSUFFICIENT_OUTPUT
    elif can == n_out:
        prod, st = n_out, BOTH_SUFFICIENT
    else:
        prod, st = can, INSUFFICIENT_INPUT
    return prod * n, prod, st


# ---- the spectrum and the three reductions ----------------------------------

def spectrum(x, table):
    """X_ref[s, n]: float64 DFT of the float32 product, whole symbols."""
    n = table.size
    k = x.size // n
    prod = (np.asarray(x[:k * n], np.complex64).reshape(k, n)
            * table[None, :].astype(np.complex64)).astype(np.complex64)
    return np.fft.fft(prod.astype(np.complex128), axis=1)


def budget(X):
    """E per symbol."""
    return FFT_TOL * np.linalg.norm(X, axis=1)


def argmax_last(mag):
    """max_by(total_cmp): the last of equal maxima (utils.rs:1101-1119)."""
    n = mag.shape[1]
    return n - 1 - np.argmax(mag[:, ::-1], axis=1)


def margin_ok(X):
    """True per symbol where the two largest |X| differ by more than 2E."""
    a = np.sort(np.abs(X), axis=1)
    return (a[:, -1] - a[:, -2]) > 2.0 * budget(X)


def raw(X):
    """get_symbol_val (utils.rs:1059-1078); None is 0xFFFF."""
    mag = np.abs(X) ** 2
    idx = argmax_last(mag)
    return np.where(mag.sum(axis=1) == 0.0, 0xFFFF, idx).astype(np.uint16)


def hard(X, reduced):
    """fft_demod.rs:115-120, 238-248."""
    n = X.shape[1]
    idx = argmax_last(np.abs(X) ** 2)
    return (((idx - 1) % n) // (4 if reduced else 1)).astype(np.uint16)


def gray_symbols(sf, reduced):
    """s of fft_demod.rs:192-194 for every bin."""
    n = 1 << sf
    s = ((np.arange(n) - 1) % n) // (4 if reduced else 1)
    return s ^ (s >> 1)


def soft(X, sf, reduced):
    """compute_llrs, max-log branch (fft_demod.rs:126-208), in float64.
    Returns (llr [k, 12], bound [k], a_max [k], da_max [k]): the LLRs, the
    bound on |LLR_gpu - LLR_ref| derived above, and the largest Bessel
    argument with the largest da_n, for `regime_ok`."""
    k, n = X.shape
    assert n == 1 << sf
    absx = np.abs(X)
    mag = absx ** 2
    idx = argmax_last(mag)
    i = np.arange(n)[None, :]
    is_sig = (np.abs(i - idx[:, None]) % (n - 1)) < 2
    sig = np.where(is_sig, mag, 0.0).sum(axis=1)
    noise = np.where(is_sig, 0.0, mag).sum(axis=1)
    ps = sig / n
    pn = noise / (n - 3)
    magn = mag * n
    a = (np.sqrt(ps) / pn)[:, None] * np.sqrt(magn)
    clip = (a >= 709.0).any(axis=1)
    ll = np.where(clip[:, None], magn, 0.0)
    if (~clip).any():
        ll[~clip] = log_i0_series(a[~clip])
    s = gray_symbols(sf, reduced)
    llr = np.zeros((k, MAX_SF))
    for bit in range(sf):
        one = ((s >> bit) & 1).astype(bool)
        # both maxima start at 0; with the reduced rate no s has its two
        # top bits set and max_x1 stays 0
        m1 = np.maximum(ll[:, one].max(axis=1), 0.0) if one.any() else 0.0
        m0 = np.maximum(ll[:, ~one].max(axis=1), 0.0)
        llr[:, sf - 1 - bit] = m1 - m0
    # the bound
    E = budget(X)
    normx = np.linalg.norm(X, axis=1)
    dS = 2.0 * normx * E + E * E
    K = np.sqrt(ps * n) / pn
    rho = dS / (2.0 * sig) + dS / noise
    da = K[:, None] * E[:, None] + a * rho[:, None]
    dll_bessel = da.max(axis=1)
    dll_clip = (n * (2.0 * absx * E[:, None] + (E * E)[:, None])).max(axis=1)
    bound = 2.0 * np.where(clip, dll_clip, dll_bessel)
    return llr, bound, a.max(axis=1), da.max(axis=1)


def regime_ok(a_max, da_max):
    return np.abs(709.0 - a_max) > da_max


# ---- test streams -----------------------------------------------------------

def stream(sf, n_sym, snr_lin, seed, cfo=0.0):
    """(x complex64, ids): n_sym random symbols on the reference's upchirp,
    rotated by e^{+2 pi i cfo / N * j} over the stream, plus complex Gaussian
    noise of variance 1/snr_lin per sample."""
    n = 1 << sf
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n, n_sym)
    x = np.concatenate([upchirp(int(s), sf) for s in ids]).astype(
        np.complex128)
    if cfo:
        x = x * np.exp(2j * np.pi * cfo / n * np.arange(x.size))
    sd = np.sqrt(0.5 / snr_lin)
    x = x + sd * (rng.standard_normal(x.size)
                  + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64), ids
