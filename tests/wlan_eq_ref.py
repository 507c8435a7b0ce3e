"""numpy restatement of the reference WLAN FrameEqualizer, for tests only.

Equalizer (examples/wlan/src/frame_equalizer.rs:27-62, 234-331) in f64, and
in f32 with the reference's own operation order (every product, sum and
quotient rounded to f32, the SNR sums accumulated carrier by carrier).
Demapper and mapper tables (lib.rs:66-218), the SIGNAL field encode
(mapper.rs:23-69) and the carrier layout (mapper.rs:108-132). The bit
pipeline (encode, decode, SIGNAL parse) is tests/wlan_ref.py.

Test signals: a frequency-domain channel (complex gain per carrier from a
few random taps, a common phase that drifts per symbol, white noise at a
stated SNR) applied to mapped symbols, and a time-domain transmitter (short
and long preamble, 16-sample prefix, 80 samples per symbol).

Error model used by the GPU test. The f32 restatement differs from f64 by
E_ref (worst |z32 - z64| / max(1, |z64|) over a case's symbols): a chain of
atan2, sincos, a complex product and a complex quotient, each operation
rounded once. The device runs the same chain with atan2f, sincosf and a
division that are each a few ulp where numpy's are below one, and contracts
products and sums to FMA, so its error is bounded by K * E_ref with K = 8.
snr_db: signal and noise are sums of 52 non-negative f32 terms, each term
with relative error <= 4 eps (two subtractions or additions, two squares,
one sum), a sum of n non-negative terms in any order adds <= (n-1) eps, the
derotation enters |h -+ s|^2 with <= 8 eps relative to |h|^2 + |s|^2, which
is signal + noise over 2. With eps = 2^-24 the quotient signal/noise is off
by at most (2*(4 + 51) + 8*(1 + signal/noise)) eps relatively; at the 35 dB
ceiling of these tests (signal/noise < 6400) that is 3.1e-3, or 0.0135 dB
worst case. The bound is a worst case over adversarial rounding; the errors
are independent and two orders smaller in practice, and SNR_TOL_DB = 1e-3
is what the tests assert (measured: the f32 restatement and the device are
both within 3.3e-5 dB of f64, profiles/wlan_equalize.txt)."""
import functools

import numpy as np

import wlan_ref

DELTA = 1e-3
K_DEVICE = 8
SNR_TOL_DB = 1e-3

PILOTS = (11, 25, 39, 53)
DATA_CARRIERS = np.array([m for m in range(6, 59)
                          if m not in (11, 25, 32, 39, 53)])
USED = np.array([m for m in range(6, 59) if m != 32])

# IEEE 802.11-2012 eq. 18-8: L(-26..26) on carriers 6..58
_L = "++--++-+-++++++--++-+-++++0+--++-+-+-----++--+-+-++++"
LONG = np.zeros(64)
LONG[6:59] = [{"+": 1.0, "-": -1.0, "0": 0.0}[c] for c in _L]

# eq. 18-6: S(-26..26) * sqrt(13/6), nonzero on every fourth carrier
_S = {-24: 1, -20: -1, -16: 1, -12: -1, -8: -1, -4: 1,
      4: -1, 8: -1, 12: 1, 16: 1, 20: 1, 24: 1}
SHORT = np.zeros(64, np.complex128)
for _k, _v in _S.items():
    SHORT[_k + 32] = _v * (1 + 1j) * np.sqrt(13.0 / 6.0)


def polarity(n=127):
    """lib.rs:365: 1 - 2*bit of the x^7+x^4+1 scrambler seeded with ones."""
    out, state = np.zeros(n, np.int64), 0x7F
    for i in range(n):
        fb = ((state >> 6) ^ (state >> 3)) & 1
        state = ((state << 1) & 0x7E) | fb
        out[i] = 1 - 2 * fb
    return out


POLARITY = polarity()

L16 = np.float32(0.31622776601683794)
L64 = np.float32(0.1543033499620919)
D16 = np.float32(0.6324555320336759)


def constellation(n_bpsc):
    """Modulation::map tables, lib.rs:66-175, as complex64 (f32 products)."""
    i = np.arange(1 << n_bpsc)
    if n_bpsc == 1:
        re, im = 2.0 * i - 1, 0.0 * i
    elif n_bpsc == 2:
        lv = np.float32(np.sqrt(0.5))
        re, im = lv * (2 * (i & 1) - 1), lv * (2 * (i >> 1 & 1) - 1)
    elif n_bpsc == 4:
        mag = lambda b: np.where(b, 1, 3).astype(np.float32) * L16
        re = mag(i >> 1 & 1) * (2 * (i & 1) - 1)
        im = mag(i >> 3 & 1) * (2 * (i >> 2 & 1) - 1)
    else:
        mag = lambda b: np.array([7, 1, 5, 3], np.float32)[b] * L64
        re = mag(i >> 1 & 3) * (2 * (i & 1) - 1)
        im = mag(i >> 4 & 3) * (2 * (i >> 3 & 1) - 1)
    return (np.asarray(re, np.float32)
            + 1j * np.asarray(im, np.float32)).astype(np.complex64)


def thresholds(n_bpsc):
    """The values demap compares an axis against, as f32."""
    if n_bpsc <= 2:
        return np.array([0.0], np.float32)
    if n_bpsc == 4:
        return np.array([-D16, 0.0, D16], np.float32)
    t = [np.float32(k) * L64 for k in (2.0, 4.0, 6.0)]
    return np.array([-t[2], -t[1], -t[0], 0.0, t[0], t[1], t[2]], np.float32)


def demap(n_bpsc, z):
    """Modulation::demap, lib.rs:177-218, on the f32 values of z."""
    z = np.asarray(z, np.complex64)
    re, im = z.real, z.imag
    if n_bpsc == 1:
        return (re > 0).astype(np.uint8)
    if n_bpsc == 2:
        return (2 * (im > 0) + (re > 0)).astype(np.uint8)
    are, aim = np.abs(re), np.abs(im)
    if n_bpsc == 4:
        return ((re > 0) | (are < D16) << 1 | (im > 0) << 2
                | (aim < D16) << 3).astype(np.uint8)
    l2, l4, l6 = (np.float32(k) * L64 for k in (2.0, 4.0, 6.0))
    return ((re > 0) | (are < l4) << 1 | ((are < l6) & (are > l2)) << 2
            | (im > 0) << 3 | (aim < l4) << 4
            | ((aim < l6) & (aim > l2)) << 5).astype(np.uint8)


def near_threshold(n_bpsc, z, delta=DELTA):
    """True where an axis demap looks at lies within delta of a threshold."""
    z = np.asarray(z, np.complex128)
    t = thresholds(n_bpsc).astype(np.float64)
    near = np.abs(z.real[:, None] - t).min(1) < delta
    if n_bpsc > 1:
        near |= np.abs(z.imag[:, None] - t).min(1) < delta
    return near


# ---- transmitter ---------------------------------------------------------------

def signal_indices(mcs, psdu):
    """mapper.rs:23-69: the 48 BPSK indices of the SIGNAL symbol."""
    return encode_signal_bits(wlan_ref.signal_bits(mcs, psdu))


def encode_signal_bits(bits):
    """mapper.rs:51-68 on any 24 bits: rate-1/2 code, interleave."""
    enc = np.zeros(48, np.uint8)
    state = 0
    for i, b in enumerate(bits):
        state = ((state << 1) & 0x7E) | int(b)
        enc[2 * i] = bin(state & 0o155).count("1") & 1
        enc[2 * i + 1] = bin(state & 0o117).count("1") & 1
    out = np.zeros(48, np.uint8)
    out[wlan_ref.INTERLEAVER_PATTERN] = enc
    return out


def map_symbol(n_bpsc, idx48, index):
    """Mapper::map, mapper.rs:108-132: 64 carriers of one symbol."""
    out = np.zeros(64, np.complex128)
    p = POLARITY[index % 127]
    out[[11, 25, 39]] = p
    out[53] = -p
    out[DATA_CARRIERS] = constellation(n_bpsc)[idx48]
    return out


def frame_carriers(mcs, psdu_bytes, seed=1):
    """(2 + 1 + n_symbols, 64) carriers of a frame: LONG twice, SIGNAL,
    data; and the frame's data indices."""
    n_bpsc = wlan_ref.MCS[mcs][0]
    idx = wlan_ref.encode(mcs, psdu_bytes, seed=seed)
    rows = [LONG.astype(np.complex128), LONG.astype(np.complex128),
            map_symbol(1, signal_indices(mcs, len(psdu_bytes)), 0)]
    for j, s in enumerate(idx.reshape(-1, 48)):
        rows.append(map_symbol(n_bpsc, s, j + 1))
    return np.array(rows), idx


def custom_frame(signal_bits, n_bpsc, n_data, rng):
    """Carriers of a frame whose SIGNAL field carries `signal_bits` (any 24
    bits) followed by n_data symbols of random indices; and those indices."""
    idx = rng.integers(0, 1 << n_bpsc, 48 * n_data).astype(np.uint8)
    rows = [LONG.astype(np.complex128), LONG.astype(np.complex128),
            map_symbol(1, encode_signal_bits(signal_bits), 0)]
    for j, s in enumerate(idx.reshape(-1, 48)):
        rows.append(map_symbol(n_bpsc, s, j + 1))
    return np.array(rows), idx


def to_bins(carriers):
    """Carrier m -> FFT bin (m + 32) % 64, frame_equalizer.rs:234-237."""
    return np.roll(carriers, 32, axis=-1)


def channel(carriers, rng, snr_db, n_taps=4, scale=3.7, drift=0.02):
    """Per-carrier gain from n_taps random taps (decaying, times `scale`), a
    random common phase plus `drift` rad per symbol, white noise snr_db
    below the mean received power of the used carriers. Returns cf32 in
    FFT-bin order, flattened."""
    taps = (rng.normal(size=n_taps) + 1j * rng.normal(size=n_taps)) \
        * 0.5 ** np.arange(n_taps)
    taps *= scale / np.linalg.norm(taps)
    m = np.arange(64) - 32
    gain = (taps * np.exp(-2j * np.pi * np.outer(m, np.arange(n_taps)) / 64)
            ).sum(1)
    phase = rng.uniform(-np.pi, np.pi) + drift * np.arange(len(carriers))
    rx = carriers * gain * np.exp(1j * phase)[:, None]
    power = np.mean(np.abs(rx[:, USED]) ** 2)
    sigma = np.sqrt(power / 10 ** (snr_db / 10) / 2)
    rx = rx + sigma * (rng.normal(size=rx.shape)
                       + 1j * rng.normal(size=rx.shape))
    return to_bins(rx).astype(np.complex64).reshape(-1)


def tx_samples(mcs, psdu_bytes, seed=1):
    """Time-domain frame: 160 samples of short preamble, 32-sample guard and
    the long symbol twice, then 16-sample prefix + 64 samples per symbol.
    Unit mean power over the data symbols' used carriers."""
    carriers, _ = frame_carriers(mcs, psdu_bytes, seed)
    t = np.fft.ifft(to_bins(carriers), axis=1) * (64 / np.sqrt(52.0))
    short = np.fft.ifft(to_bins(SHORT)) * (64 / np.sqrt(52.0))
    parts = [np.tile(short, 3)[:160], t[0][-32:], t[0], t[1]]
    for row in t[2:]:
        parts += [row[-16:], row]
    return np.concatenate(parts)


# ---- equalizer -----------------------------------------------------------------

def _cx(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def _derotate(s, psum, dtype):
    """s * from_polar(1, -arg(psum)), every operation rounded to dtype."""
    beta = np.arctan2(dtype(psum.imag), dtype(psum.real))
    c, sn = np.cos(-beta), np.sin(-beta)
    re, im = s.real.astype(dtype), s.imag.astype(dtype)
    return ((re * c - im * sn) + 1j * (re * sn + im * c)).astype(_cx(dtype))


def _pilots_training(s):
    return ((s[11] - s[25]) + s[39]) + s[53]


def _pilots_data(s, p):
    p = s.real.dtype.type(p)
    return ((s[11] * p + s[39] * p) + s[25] * p) + s[53] * -p


def _cdiv(a, b, dtype):
    """num-complex: (a * conj(b)) / |b|^2, componentwise."""
    ar, ai = a.real.astype(dtype), a.imag.astype(dtype)
    br, bi = b.real.astype(dtype), b.imag.astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = br * br + bi * bi
        return ((ar * br + ai * bi) / n
                + 1j * ((ai * br - ar * bi) / n)).astype(_cx(dtype))


def equalize(spec, dtype=np.float64):
    """One frame. spec: its symbols in FFT-bin order, (n_avail, 64) or flat.
    Returns a dict: found, mcs, psdu_size, n_symbols, n_copied, snr_db, idx
    (48*n_copied uint8), z (as many complex), sig_idx, sig_z."""
    cx = _cx(dtype)
    sym = to_bins(np.asarray(spec).reshape(-1, 64)).astype(cx)
    res = dict(found=False, mcs=0, psdu_size=0, n_symbols=0, n_copied=0,
               snr_db=0.0, idx=np.zeros(0, np.uint8), z=np.zeros(0, cx))
    if len(sym) < 2:
        return res
    h = _derotate(sym[0], _pilots_training(sym[0]), dtype)
    s = _derotate(sym[1], _pilots_training(sym[1]), dtype)
    signal = noise = dtype(0)
    for i in USED:          # sequential, as frame_equalizer.rs:35-44
        d, e = h[i] - s[i], h[i] + s[i]
        noise = noise + (d.real * d.real + d.imag * d.imag)
        signal = signal + (e.real * e.real + e.imag * e.imag)
    h = h.copy()
    h[USED] = (h[USED] + s[USED]) * (0.5 * LONG[USED]).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        res["snr_db"] = float(dtype(10) * np.log10(signal / noise / dtype(2)))
    if len(sym) < 3:
        return res
    sig = _derotate(sym[2], _pilots_data(sym[2], POLARITY[0]), dtype)
    res["sig_z"] = _cdiv(sig[DATA_CARRIERS], h[DATA_CARRIERS], dtype)
    res["sig_idx"] = demap(1, res["sig_z"])
    dec = wlan_ref.decode(0, 0, res["sig_idx"])[1]
    parsed = wlan_ref.signal_field(np.unpackbits(dec)[:24])
    if parsed is None:
        return res
    mcs, psdu = parsed
    n_bpsc = wlan_ref.MCS[mcs][0]
    n_sym = wlan_ref.frame_param(mcs, psdu)[0]
    n_copied = min(n_sym, len(sym) - 3)
    zs = []
    for j in range(n_copied):
        v = sym[3 + j]
        v = _derotate(v, _pilots_data(v, POLARITY[(j + 1) % 127]), dtype)
        zs.append(_cdiv(v[DATA_CARRIERS], h[DATA_CARRIERS], dtype))
    z = np.concatenate(zs) if zs else np.zeros(0, cx)
    res.update(found=True, mcs=mcs, psdu_size=psdu, n_symbols=n_sym,
               n_copied=n_copied, z=z, idx=demap(n_bpsc, z))
    return res


def e_ref(z32, z64):
    """Worst f32-restatement error relative to max(1, |z|)."""
    z64 = np.asarray(z64, np.complex128)
    return float(np.max(np.abs(np.asarray(z32, np.complex128) - z64)
                        / np.maximum(1.0, np.abs(z64))))


# ---- shared cases --------------------------------------------------------------

PARITY_PSDU = (30, 36, 40, 60, 60, 100, 104, 104)   # 11 .. 4 data symbols
PARITY_SNR = (12, 12, 15, 15, 22, 22, 30, 30)
PARITY_SEED = 1265


def psdu_bytes(mcs, psdu, seed):
    rng = np.random.default_rng(seed)
    return wlan_ref.with_fcs(rng.integers(0, 256, psdu - 4, np.uint8).tobytes())


@functools.lru_cache(maxsize=None)
def case(mcs, psdu, snr_db, seed=PARITY_SEED):
    """One frame through the frequency-domain channel: dict with data
    (bytes), tx_idx, spec (flat cf32, read-only), r64 and r32 (equalize in
    f64 and f32), e_ref, near (mask of data symbols within DELTA of a
    threshold in f64)."""
    data = psdu_bytes(mcs, psdu, seed + mcs)
    carriers, tx_idx = frame_carriers(mcs, data)
    rng = np.random.default_rng([seed, mcs, psdu])
    spec = channel(carriers, rng, snr_db)
    spec.setflags(write=False)
    r64, r32 = equalize(spec, np.float64), equalize(spec, np.float32)
    c = dict(mcs=mcs, psdu=psdu, data=data, tx_idx=tx_idx, spec=spec,
             r64=r64, r32=r32)
    if r64["found"] and r32["found"] and r32["z"].size == r64["z"].size:
        c["e_ref"] = e_ref(r32["z"], r64["z"])
        c["near"] = near_threshold(wlan_ref.MCS[r64["mcs"]][0], r64["z"])
    return c


def parity_cases():
    return [case(m, PARITY_PSDU[m], PARITY_SNR[m]) for m in range(8)]


# ---- samples to bytes ----------------------------------------------------------

SAMPLE_FRAMES = ((2, 60), (5, 100))   # Qpsk_1_2, Qam16_3_4


@functools.lru_cache(maxsize=None)
def sample_stream(snr_db=30.0, gap=600, tail=160, seed=4321):
    """(iq cf32, [psdu bytes]) of SAMPLE_FRAMES at unit power: 80 zeros (the
    metric chain's warm-up is then 0/0, which triggers nothing), frame,
    `gap` samples, frame, `tail` samples; white noise snr_db below the
    frames everywhere behind the zeros."""
    rng = np.random.default_rng(seed)
    data = [psdu_bytes(m, p, seed + m) for m, p in SAMPLE_FRAMES]
    tx = [tx_samples(m, d) for (m, _), d in zip(SAMPLE_FRAMES, data)]
    sig = np.concatenate([np.zeros(80), tx[0], np.zeros(gap), tx[1],
                          np.zeros(tail)]).astype(np.complex128)
    sigma = np.sqrt(10 ** (-snr_db / 10) / 2)
    sig[80:] += sigma * (rng.normal(size=sig.size - 80)
                         + 1j * rng.normal(size=sig.size - 80))
    iq = sig.astype(np.complex64)
    iq.setflags(write=False)
    return iq, data


def frame_spans_walk(tags, frames, n_samples):
    """The SyncLong rule, walked literally (sync_long.rs:136-178): per tag,
    Sync needs SEARCH_WINDOW + 128 = 448 samples before the next tag, emits
    128 items from the correlator offset, then Copy emits 64 items for every
    80 samples it still has."""
    spans, produced, j = [], 0, 0
    for t in range(len(tags)):
        start = tags[t][0]
        end = tags[t + 1][0] if t + 1 < len(tags) else n_samples
        if end - start < 448:
            continue
        first = produced
        cur = start + frames[j][0]
        j += 1
        cur += 128
        produced += 128
        while cur + 80 <= end:
            cur += 80
            produced += 64
        spans.append((first, (produced - first) // 64))
    return spans
