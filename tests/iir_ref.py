"""References for the IIR filter (futuredsp iir.rs:79-178), numpy only:
the literal serial loop, its call accounting, the test filters, a numpy
restatement of the kernels' blocked decomposition, and the error bound the
CPU and GPU tests assert.

Recurrence. y[k] = sum_j b[j] x[k+nb-1-j] + sum_j a[j] y[k-1-j], with
y[-1-j] = memory[j]. The first n_a inputs of a stream fill `memory` and
are ordinary inputs as well (iir.rs:102-118).

Error bound (derived, not tuned). Each output is one sum of n_b + n_a
products, M[k] = sum_j |b[j]||x[k+nb-1-j]| + sum_j |a[j]||y[k-1-j]| its
magnitude sum. An fp32 evaluation of that sum in any order has error at
most gamma_c M[k] for c operations on the longest path (DESIGN.md §c,
Higham eq. 3.5), and an error e[k] made at output k reaches output n
multiplied by g[n-k], g the impulse response of the feedback alone
(g[0] = 1, g[k] = sum_j a[j] g[k-1-j]). So

    |err[n]| <= gamma_c * sum_{k<=n} |g[n-k]| M[k],  gamma_c = c u/(1 - c u).

The constant c.
  serial f32 loop: c = n_b + n_a, the sum itself.
  kernels: the longest chain of rounded operations that ends in an output,
  with a fused multiply-add as one rounding (kernel_c below):
    n_b + n_a      the chunk's own sum from zero state;
    (n_a + 1) * d  the scan levels on the longest path to the chunk's
                   incoming state. One level is p[q] += sum_r M[q][r] o[r]:
                   n_a fused multiply-adds into the state element, and one
                   more rounding for the table entry M[q][r], rounded to
                   f32 once. d is counted by walking the scan: a seeding
                   (by the state entering the tile, or the pass) is one
                   level on lane 0; at distance 2^k every lane c >= 2^k
                   gets 1 + the longer of its own and lane c - 2^k's path.
                   In a tile (256 chunks) that is 9; across tiles it
                   depends on the tile states present (3 states: 2);
    n_a + 2        the correction sum_q H[i][q] s[q] (n_a fused
                   multiply-adds, one rounding for the table entry) and
                   its addition to the zero-state output.
The tests require c <= 128 for every case they run.
"""
import numpy as np

U = 2.0 ** -24

INSUFFICIENT_INPUT = 0
INSUFFICIENT_OUTPUT = 1
BOTH_SUFFICIENT = 2


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the test filters, taps rounded to f32 --------------------------------

def _a_from_poles(poles):
    poles = np.asarray(poles, np.complex128)
    poly = np.poly(np.concatenate([poles, poles.conj()])).real
    return (-poly[1:]).astype(np.float32)


def _loud_taps(n, seed):
    r = np.random.default_rng([0x11F, seed])
    return (r.uniform(0.5, 1.0, n) * r.choice([-1.0, 1.0], n)).astype(
        np.float32)


P_DEEMPH = np.float32(np.exp(-1.0 / 3.6))

FILTERS = {
    "D": (np.array([P_DEEMPH], np.float32),
          np.array([np.float32(1.0) - P_DEEMPH], np.float32)),
    "B": (np.array([1.5610, -0.6414], np.float32),
          np.array([0.0201, 0.0402, 0.0201], np.float32)),
    "Q": (_a_from_poles([0.9 * np.exp(0.4j), 0.8 * np.exp(1.2j)]),
          np.array([0.1, 0.2, 0.3, 0.2, 0.1], np.float32)),
    "O": (_a_from_poles([0.95 * np.exp(0.2j), 0.9 * np.exp(0.7j),
                         0.85 * np.exp(1.5j), 0.7 * np.exp(2.5j)]),
          np.array([0.3, -0.2, 0.1], np.float32)),
    "F": (np.zeros(0, np.float32), _loud_taps(33, 1)),
    "W": (np.array([0.5], np.float32), _loud_taps(64, 2)),
}

# every table entry 0 or +-1; with inputs in {-1, 0, 1} all arithmetic is
# on small integers, so every association gives the same bits
EXACT = {
    "I": (np.array([1], np.float32), np.array([1], np.float32)),
    "A": (np.array([-1], np.float32), np.array([1, 1], np.float32)),
    "T": (np.array([0, 1], np.float32), np.array([1], np.float32)),
    "E": (np.array([0, 0, 0, 0, 0, 0, 0, 1], np.float32),
          np.array([1, -1], np.float32)),
}


def exact_input(n, seed):
    return np.random.default_rng([0xE8AC7, seed]).integers(
        -1, 2, n).astype(np.float32)


def exact_closed_form(name, x):
    """All outputs of exact filter `name` on a fresh stream x (float64),
    len(x) - (n_b - 1) of them, in closed numpy form."""
    x = np.asarray(x, np.float64)
    if name == "I":     # y[k] = x[k] + y[k-1], y[-1] = x[0]
        return np.cumsum(x) + x[0]
    if name == "A":     # y[k] = x[k+1] + x[k] - y[k-1], y[-1] = x[0]
        f = x[1:] + x[:-1]
        s = np.where(np.arange(f.size) % 2 == 0, 1.0, -1.0)
        return s * (np.cumsum(s * f) - x[0])
    if name == "T":     # y[k] = x[k] + y[k-2], y[-1] = x[0], y[-2] = x[1]
        y = np.empty(x.size)
        y[0::2] = np.cumsum(x[0::2]) + x[1]
        y[1::2] = np.cumsum(x[1::2]) + x[0]
        return y
    if name == "E":     # y[k] = x[k+1] - x[k] + y[k-8], y[-1-j] = x[j]
        f = x[1:] - x[:-1]
        y = np.empty(f.size)
        for r in range(8):
            y[r::8] = np.cumsum(f[r::8]) + x[7 - r]
        return y
    raise KeyError(name)


# ---- iir.rs:79-178 ----------------------------------------------------------

def count(n_a, n_b, filled, n_in, n_out):
    """(filled_after, consumed, produced, status): steps 1-3 alone."""
    idle = BOTH_SUFFICIENT if n_out == 0 else INSUFFICIENT_INPUT
    if n_in == 0:
        return filled, 0, 0, idle
    m, pushes = filled, 0
    while m < n_a:
        if n_in <= m:
            return m, 0, 0, idle
        m += 1
        pushes += 1
    if pushes == n_in:
        return m, 0, 0, idle
    n = 0
    while n + n_b - 1 < n_in and n < n_out:
        n += 1
    if n == n_in and n == n_out:
        st = BOTH_SUFFICIENT
    elif n < n_in:
        st = INSUFFICIENT_OUTPUT
    else:
        st = INSUFFICIENT_INPUT
    return m, n, n, st


def serial(a, b, x, n_out, dtype, memory=None):
    """One filter() call, the loop of iir.rs:134-164 with the fill in front,
    every operation rounded to `dtype` in the order written. `memory` is
    the list the call starts with (None = a fresh filter). Returns
    (outputs, consumed, produced, status, memory after)."""
    dt = np.dtype(dtype).type
    a = [dt(v) for v in np.asarray(a, np.float32)]
    b = [dt(v) for v in np.asarray(b, np.float32)]
    x = np.asarray(x, np.float32).astype(dt)
    mem = [dt(v) for v in (memory if memory is not None else [])]
    filled, n, _, st = count(len(a), len(b), len(mem), x.size, n_out)
    mem += [x[k] for k in range(len(mem), filled)]
    if n == 0:
        return np.zeros(0, dt), 0, 0, st, mem
    nb = len(b)
    # the b part of every output, in the loop's own order (it does not
    # depend on the feedback, so it vectorises across outputs)
    acc = np.zeros(n, dt)
    for j in range(nb):
        acc = acc + b[j] * x[nb - 1 - j: nb - 1 - j + n]
    y = np.zeros(n, dt)
    for k in range(n):
        o = acc[k]
        for q in range(len(a)):
            o = o + a[q] * mem[q]
        if mem:
            mem = [o] + mem[:-1]
        y[k] = o
    return y, n, n, st, mem


def impulse(a, n):
    a = np.asarray(a, np.float64)
    g = np.zeros(n)
    if n:
        g[0] = 1.0
    for k in range(1, n):
        for j in range(min(a.size, k)):
            g[k] += a[j] * g[k - 1 - j]
    return g


def bound_sum(a, b, x, y_ref, memory=None):
    """Per output of y_ref (float64, computed from x and `memory`):
    sum_{k<=n} |g[n-k]| M[k]."""
    g = np.abs(impulse(a, len(y_ref)))
    a = np.abs(np.asarray(a, np.float64))
    b = np.abs(np.asarray(b, np.float64))
    x = np.abs(np.asarray(x, np.float64))
    n = len(y_ref)
    nb, na = b.size, a.size
    mem = np.abs(np.asarray(
        memory if memory is not None else x[:na], np.float64))
    yy = np.concatenate([mem[::-1], np.abs(np.asarray(y_ref, np.float64))])
    M = np.zeros(n)
    for j in range(nb):
        M += b[j] * x[nb - 1 - j: nb - 1 - j + n]
    for j in range(na):         # y[k-1-j] sits at yy[na + k - 1 - j]
        M += a[j] * yy[na - 1 - j: na - 1 - j + n]
    return np.convolve(g, M)[:n]


def bound(a, b, x, y_ref, c, memory=None):
    return gamma(c) * bound_sum(a, b, x, y_ref, memory)


def scan_depth(states, lanes, carried=0):
    """Levels on the longest path through one pass of the doubling scan
    over `states` <= `lanes` states, lane 0 seeded by a state that has
    been through `carried` levels."""
    d = [0] * states
    d[0] = carried + 1
    k = 1
    while k < lanes:
        prev = list(d)
        for c in range(k, states):
            d[c] = max(prev[c], prev[c - k]) + 1
        k *= 2
    return max(d)


def kernel_c(n_a, n_b, n_out, info):
    """The kernels' operation-path constant for a call of n_out outputs
    (module docstring). info = plan.info()."""
    L, chunks, tile, per_pass = info
    if n_a == 0:
        return n_b
    states = -(-n_out // tile) - 1      # tile states the scan combines
    depth = 0
    while states > 0:
        here = min(states, per_pass)
        depth = scan_depth(here, per_pass, depth)
        states -= here
    depth = scan_depth(chunks, chunks, depth)
    return n_b + n_a + (n_a + 1) * depth + n_a + 2


# ---- the kernels' decomposition, restated in float64 -----------------------

def _scan(p, pw):
    """Inclusive doubling scan along axis -2 of p [..., 2^len(pw), n_a]:
    P_c = sum_{k<=c} B^(c-k) p_k with pw[d] = B^(2^d)."""
    k = 1
    for m in pw:
        q = p.copy()
        q[..., k:, :] += p[..., :-k, :] @ m.T
        p = q
        k *= 2
    return p


def blocked(a, b, x, n, memory, tables, info, fault=None):
    """n outputs from `memory` the way the kernels form them, in float64
    from the plan's tables alone: chunks from zero state, chunk end states
    scanned over a tile, tile end states scanned over the call, and the
    correction H s per chunk. `fault` plants one mistake: 'drop' zeroes
    one chunk's incoming state, 'hrow' reads H one row off, 'swap'
    exchanges the first two state elements in the correction."""
    H, pc, pt = (np.asarray(t, np.float64) for t in tables)
    L, C, tile, P = info
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    x = np.asarray(x, np.float64)
    na, nb = a.size, b.size
    n_tiles = -(-n // tile)
    fir = np.zeros(n_tiles * tile)
    for j in range(nb):
        fir[:n] += b[j] * x[nb - 1 - j: nb - 1 - j + n]
    z = fir.reshape(n_tiles, C, L).copy()
    for i in range(L):
        for q in range(min(na, i)):
            z[:, :, i] += a[q] * z[:, :, i - 1 - q]
    if na == 0:
        return z.reshape(-1)[:n]
    v = z[:, :, L - 1 - np.arange(na)]              # chunk end states
    T = _scan(v, pc)[:, -1, :]                      # tile end states
    S = np.zeros((n_tiles, na))                     # state entering a tile
    S[0] = carry = np.asarray(memory, np.float64)
    for base in range(0, n_tiles - 1, P):
        m = min(P, n_tiles - 1 - base)
        p = np.zeros((P, na))
        p[:m] = T[base: base + m]
        p[0] += pt[0] @ carry
        p = _scan(p, pt)
        S[base + 1: base + 1 + m] = p[:m]
        carry = p[-1]
    pp = v.copy()
    pp[:, 0, :] += S @ pc[0].T
    pp = _scan(pp, pc)
    s = np.concatenate([S[:, None, :], pp[:, :-1, :]], axis=1)
    if fault == "drop":
        s[min(1, n_tiles - 1), C // 2] = 0.0
    elif fault == "hrow":
        H = np.roll(H, 1, axis=0)
    elif fault == "swap":
        s = s[..., [1, 0] + list(range(2, na))]
    elif fault is not None:
        raise KeyError(fault)
    y = z + np.einsum("tcq,iq->tci", s, H)
    return y.reshape(-1)[:n]


# ---- the cases tests/test_iir_gpu.py runs ----------------------------------

def value_counts(n_a, info):
    """Produced counts of the value test: one output, a call shorter than
    the memory, around a chunk, around a tile, several tiles with a
    partial chunk at the end."""
    L, _, tile, _ = info
    ns = [1, L - 1, L + 1, tile - 1, tile, tile + 1, 2 * tile + 1,
          3 * tile + L + 1]
    return ns + ([n_a] if n_a else [])


def value_stream(name, info):
    """(x, y_ref float64, bound_sum) of filter `name` over the longest
    value case; shorter cases are prefixes."""
    from dsp_ref import _rng, loud_f32
    a, b = FILTERS[name]
    n = max(value_counts(a.size, info))
    x = loud_f32(_rng(0x11A, ord(name)), n + b.size - 1 + 5)
    y = serial(a, b, x, n, np.float64)[0]
    return x, y, bound_sum(a, b, x, y)


def stream_len(info):
    return 3 * info[2] + 7
