"""numpy restatement of the reference WLAN bit pipeline, for tests only.

Encoder (examples/wlan/src/encoder.rs:23-131): bits, scramble, K=7
convolutional code, puncture, interleave, split into constellation indices.
Decoder (decoder.rs:47-115 and viterbi_decoder.rs:48-528): index bits,
deinterleave, depuncture, the hard-decision Viterbi with its byte-wide
paths shifted as 16-bit pairs, sliding traceback, descramble, CRC-32.
Signal field parse: frame_equalizer.rs:10-13, 121-175.

The arrays keep the reference's own layout (64-entry metric and path arrays,
updated in two halves of 16) so that the GPU kernel's state-per-lane form is
checked against something written differently.

Tail rule: the reference's `depunctured` array is never cleared between
frames and is read 76..164 entries past the frame's own bits. Here every
frame is decoded as a freshly constructed decoder would: those entries are 0
(bit value 0, not an erasure), for any frame size. At rates 3/4 and 2/3 the
scrambled pad bits followed by this tail are no codeword and the traceback
is short, so for some scrambler seeds the last PSDU byte decodes wrong even
without channel errors (Qam64_3_4, 104 bytes, seed 5); seed 1, the
reference encoder's first, round-trips at every size tested.
"""
import zlib

import numpy as np

# (n_bpsc, n_cbps, n_dbps, depuncture pattern, n_traceback) — lib.rs:234-282,
# viterbi_decoder.rs:68-78
MCS = (
    (1, 48, 24, (1, 1), 5),                 # Bpsk_1_2
    (1, 48, 36, (1, 1, 1, 0, 0, 1), 10),    # Bpsk_3_4
    (2, 96, 48, (1, 1), 5),                 # Qpsk_1_2
    (2, 96, 72, (1, 1, 1, 0, 0, 1), 10),    # Qpsk_3_4
    (4, 192, 96, (1, 1), 5),                # Qam16_1_2
    (4, 192, 144, (1, 1, 1, 0, 0, 1), 10),  # Qam16_3_4
    (6, 288, 192, (1, 1, 1, 0), 9),         # Qam64_2_3
    (6, 288, 216, (1, 1, 1, 0, 0, 1), 10),  # Qam64_3_4
)
N_MCS = len(MCS)
MAX_PSDU_SIZE = 1528
MAX_SYM = 511
CRC_RESIDUE = 558161692

INTERLEAVER_PATTERN = np.array(
    [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 33, 36, 39, 42, 45, 1, 4, 7, 10,
     13, 16, 19, 22, 25, 28, 31, 34, 37, 40, 43, 46, 2, 5, 8, 11, 14, 17, 20,
     23, 26, 29, 32, 35, 38, 41, 44, 47])

# rate bits (LSB first) -> mcs, frame_equalizer.rs:161-169
SIGNAL_RATES = {11: 0, 15: 1, 10: 2, 14: 3, 9: 4, 13: 5, 8: 6, 12: 7}


def frame_param(mcs, psdu):
    """(n_symbols, n_data_bits, n_pad) — lib.rs:324-343."""
    n_dbps = MCS[mcs][2]
    bits = 16 + 8 * psdu + 6
    n_symbols = bits // n_dbps + (bits % n_dbps != 0)
    n_data_bits = n_symbols * n_dbps
    return n_symbols, n_data_bits, n_data_bits - bits


def n_decoded_bytes(mcs, psdu):
    return (frame_param(mcs, psdu)[1] + 7) // 8


def deinterleave_map(mcs):
    """m with deinterleaved[m[k]] = rx_bits[k] inside one symbol
    (decoder.rs:50-64; the encoder uses the same m the other way round)."""
    n_bpsc, n_cbps = MCS[mcs][:2]
    s = max(n_bpsc // 2, 1)
    j = np.arange(n_cbps)
    first = s * (j // s) + ((j + (16 * j // n_cbps)) % s)
    second = 16 * j - (n_cbps - 1) * (16 * j // n_cbps)
    return second[first]


# ---- encoder -----------------------------------------------------------------

def encode(mcs, psdu_bytes, seed=1):
    """Constellation indices (uint8, 48 per symbol) of one frame."""
    n_bpsc, n_cbps, _, pattern, _ = MCS[mcs]
    data = np.frombuffer(bytes(psdu_bytes), np.uint8)
    n_sym, n_data_bits, n_pad = frame_param(mcs, data.size)
    bits = np.zeros(n_data_bits, np.uint8)
    bits[16:16 + 8 * data.size] = np.unpackbits(data, bitorder="little")
    scrambled = np.zeros(n_data_bits, np.uint8)
    state = seed
    for i in range(n_data_bits):
        fb = ((state >> 6) ^ (state >> 3)) & 1
        scrambled[i] = fb ^ bits[i]
        state = ((state << 1) & 0x7E) | fb
    off = n_data_bits - n_pad - 6
    scrambled[off:off + 6] = 0
    encoded = np.zeros(2 * n_data_bits, np.uint8)
    state = 0
    for i in range(n_data_bits):
        state = ((state << 1) & 0x7E) | int(scrambled[i])
        encoded[2 * i] = bin(state & 0o155).count("1") & 1
        encoded[2 * i + 1] = bin(state & 0o117).count("1") & 1
    if len(pattern) == 2:
        punctured = encoded
    else:
        keep = np.array(pattern, bool)[np.arange(encoded.size) % len(pattern)]
        punctured = encoded[keep]
    assert punctured.size == n_sym * n_cbps
    m = deinterleave_map(mcs)
    inter = punctured.reshape(n_sym, n_cbps)[:, m].reshape(-1)
    weights = (1 << np.arange(n_bpsc)).astype(np.uint8)
    return (inter.reshape(-1, n_bpsc) * weights).sum(1).astype(np.uint8)


def with_fcs(payload):
    """payload + its CRC-32, little-endian: a PSDU whose check passes."""
    payload = bytes(payload)
    return payload + zlib.crc32(payload).to_bytes(4, "little")


def flip_coded_bits(mcs, syms, fraction, rng):
    """Flips about `fraction` of the frame's coded bits (at least one)."""
    n_bpsc = MCS[mcs][0]
    out = np.array(syms, np.uint8)
    n = out.size * n_bpsc
    pick = rng.choice(n, max(1, int(round(fraction * n))), replace=False)
    np.bitwise_xor.at(out, pick // n_bpsc,
                      (1 << (pick % n_bpsc)).astype(np.uint8))
    return out


# ---- decoder -----------------------------------------------------------------

def rx_bits(mcs, syms):
    """decoder.rs:69-76: bit k < n_bpsc of index i -> rx_bits[i*n_bpsc+k]."""
    n_bpsc = MCS[mcs][0]
    syms = np.asarray(syms, np.uint8)
    return ((syms[:, None] >> np.arange(n_bpsc)) & 1).astype(np.uint8) \
        .reshape(-1)


def deinterleave(mcs, bits):
    n_cbps = MCS[mcs][1]
    out = np.zeros_like(bits)
    b = bits.reshape(-1, n_cbps)
    out.reshape(-1, n_cbps)[:, deinterleave_map(mcs)] = b
    return out


def depuncture(mcs, n_symbols, in_bits, out):
    """viterbi_decoder.rs:81-107 into `out` (left as it is elsewhere).
    Returns the number of entries written."""
    _, n_cbps, _, pattern, n_traceback = MCS[mcs]
    if n_traceback == 5:
        out[:in_bits.size] = in_bits
        return in_bits.size
    count = 0
    for i in range(n_symbols):
        for k in range(n_cbps):
            while pattern[count % len(pattern)] == 0:
                out[count] = 2
                count += 1
            out[count] = in_bits[i * n_cbps + k]
            count += 1
            while pattern[count % len(pattern)] == 0:
                out[count] = 2
                count += 1
    return count


def depunctured_length(mcs, psdu):
    """Entries the decoder reads: 16*(n_traceback + n_bytes) - 4."""
    return 16 * (MCS[mcs][4] + n_decoded_bytes(mcs, psdu)) - 4


def _branchtab():
    j = np.arange(32)
    par = lambda v: np.array([bin(int(x)).count("1") & 1 for x in v])
    return par((2 * j) & 0x6D), par((2 * j) & 0x4F)


_BT0, _BT1 = _branchtab()


class Viterbi:
    """viterbi_decoder.rs, one frame per instance (reset() at :48-79)."""

    def __init__(self, n_traceback):
        self.n_traceback = n_traceback
        self.store_pos = 0
        self.metric = np.zeros(64, np.int64)
        self.path = np.zeros(64, np.int64)
        self.ppresult = np.zeros((24, 64), np.int64)
        self.max_metric = 0

    def _butterfly(self, s0, s1):
        """One trellis step, viterbi_decoder.rs:143-282."""
        metric0, path0 = self.metric, self.path
        metric1 = np.zeros(64, np.int64)
        path1 = np.zeros(64, np.int64)
        for i in range(2):
            a = slice(i * 16, i * 16 + 16)
            b = slice((i + 2) * 16, (i + 2) * 16 + 16)
            if s0 == 2:
                metsvm = _BT1[a] ^ s1
                metsv = 1 - metsvm
            elif s1 == 2:
                metsvm = _BT0[a] ^ s0
                metsv = 1 - metsvm
            else:
                metsvm = (_BT0[a] ^ s0) + (_BT1[a] ^ s1)
                metsv = 2 - metsvm
            m0 = metric0[a] + metsv
            m1 = metric0[b] + metsvm
            m2 = metric0[a] + metsvm
            m3 = metric0[b] + metsv
            d0 = m0 > m1
            d1 = m2 > m3
            surv0 = np.where(d0, m0, m1)
            surv1 = np.where(d1, m2, m3)
            shift = []
            for sl in (a, b):
                p = path0[sl]
                w = ((p[0::2] | (p[1::2] << 8)) << 1) & 0xFFFF
                sh = np.zeros(16, np.int64)
                sh[0::2] = w & 0xFF
                sh[1::2] = w >> 8
                shift.append(sh)
            shift0, shift1 = shift[0], (shift[1] + 1) & 0xFF
            tmp0 = np.where(d0, shift0, shift1)
            tmp1 = np.where(d1, shift0, shift1)
            lo = 2 * i * 16
            hi = (2 * i + 1) * 16
            metric1[lo:lo + 16:2] = surv0[:8]
            metric1[lo + 1:lo + 16:2] = surv1[:8]
            metric1[hi:hi + 16:2] = surv0[8:]
            metric1[hi + 1:hi + 16:2] = surv1[8:]
            path1[lo:lo + 16:2] = tmp0[:8]
            path1[lo + 1:lo + 16:2] = tmp1[:8]
            path1[hi:hi + 16:2] = tmp0[8:]
            path1[hi + 1:hi + 16:2] = tmp1[8:]
        self.metric, self.path = metric1, path1
        self.max_metric = max(self.max_metric, int(metric1.max()))

    def butterfly2(self, symbols):
        self._butterfly(int(symbols[0]), int(symbols[1]))
        self._butterfly(int(symbols[2]), int(symbols[3]))

    def get_output(self):
        """viterbi_decoder.rs:435-484."""
        nt = self.n_traceback
        self.store_pos = (self.store_pos + 1) % nt
        self.ppresult[self.store_pos] = self.path
        mm = self.metric
        beststate = int(np.argmax(mm))   # first maximum = strict '>' scan
        minmetric = int(mm.min())
        pos = self.store_pos
        for _ in range(nt - 1):
            beststate = int(self.ppresult[pos][beststate]) >> 2
            pos = (pos + nt - 1) % nt
        self.path = np.zeros(64, np.int64)
        self.metric = mm - minmetric
        return int(self.ppresult[pos][beststate])


def viterbi(mcs, n_data_bits, depunctured):
    """decode() at viterbi_decoder.rs:486-528 -> (bytes, max metric)."""
    nt = MCS[mcs][4]
    v = Viterbi(nt)
    out = []
    in_count = out_count = n_decoded = 0
    while n_decoded < n_data_bits:
        if in_count % 4 == 0:
            v.butterfly2(depunctured[in_count:in_count + 4])
            if in_count > 0 and in_count % 16 == 8:
                c = v.get_output()
                if out_count >= nt:
                    out.append(c)
                    n_decoded += 8
                out_count += 1
        in_count += 1
    return np.array(out, np.uint8), v.max_metric


def descramble(dec_bytes, psdu):
    """decoder.rs:92-115 on the MSB-first decoded bytes."""
    bits = np.unpackbits(dec_bytes)
    out = np.zeros(psdu + 2, np.uint8)
    state = 0
    for i in range(7):
        if bits[i]:
            state |= 1 << (6 - i)
    out[0] = state
    for i in range(7, psdu * 8 + 16):
        fb = ((state >> 6) ^ (state >> 3)) & 1
        out[i // 8] |= (fb ^ int(bits[i])) << (i % 8)
        state = ((state << 1) & 0x7E) | fb
    return out


def decode(mcs, psdu, syms):
    """(out_bytes, dec_bytes, crc_ok, max_metric) of one frame."""
    n_sym, n_data_bits, _ = frame_param(mcs, psdu)
    syms = np.asarray(syms, np.uint8)
    assert syms.size == 48 * n_sym
    dep = np.zeros(depunctured_length(mcs, psdu) + 16, np.uint8)
    depuncture(mcs, n_sym, deinterleave(mcs, rx_bits(mcs, syms)), dep)
    dec, mx = viterbi(mcs, n_data_bits, dep)
    assert dec.size == (n_data_bits + 7) // 8
    out = descramble(dec, psdu)
    crc_ok = zlib.crc32(out[2:psdu + 2].tobytes()) == CRC_RESIDUE
    return out, dec, crc_ok, mx


def source_map(mcs, n_symbols, count):
    """For depunctured index p < count: 8*byte + bit of the index byte the
    value comes from, -1 for an erasure, -2 past the frame (reads 0). Built
    by pushing labels through rx_bits/deinterleave/depuncture."""
    n_bpsc = MCS[mcs][0]
    n = 48 * n_symbols
    labels = (8 * np.arange(n)[:, None] + np.arange(n_bpsc)).reshape(-1)
    out = np.full(max(count, 2 * labels.size + 16), -2, np.int64)
    marked = np.full(out.size, 0, np.int64)
    used = depuncture(mcs, n_symbols, deinterleave(mcs, labels), out)
    # erasures were written as the value 2: find them by a second pass
    depuncture(mcs, n_symbols, np.full(labels.size, 7, np.int64), marked)
    out[:used][marked[:used] == 2] = -1
    return out[:count]


def signal_field(bits24):
    """(mcs, psdu) or None — frame_equalizer.rs:142-174."""
    b = [int(x) > 0 for x in bits24]
    r = sum(1 << i for i in range(4) if b[i])
    length = sum(1 << (i - 5) for i in range(5, 17) if b[i])
    parity = sum(b[:17]) & 1
    if parity != b[17] or r not in SIGNAL_RATES:
        return None
    return SIGNAL_RATES[r], length


def signal_bits(mcs, psdu):
    """The 24 SIGNAL bits a transmitter sends for (mcs, psdu)."""
    inv = {v: k for k, v in SIGNAL_RATES.items()}
    b = np.zeros(24, np.uint8)
    for i in range(4):
        b[i] = (inv[mcs] >> i) & 1
    for i in range(12):
        b[5 + i] = (psdu >> i) & 1
    b[17] = b[:17].sum() & 1
    return b
