#!/usr/bin/env python3
"""WLAN frame decoding in the shape of the reference's Decoder block
(examples/wlan/src/decoder.rs): a batch of frames of mixed MCS and length
goes through bits -> deinterleave -> depuncture -> Viterbi -> descramble ->
CRC-32 in one kernel, one frame per wavefront (futuresdr_amd.WlanDecoder).

The input is synthesized the way the reference's Encoder does it
(encoder.rs:23-131): payload + FCS, scramble, K=7 convolutional code,
puncture, interleave, split into constellation indices. A few coded bits of
every frame are then flipped; the decoder corrects them. The SIGNAL field
of each frame is coded as one BPSK 1/2 symbol and decoded by the same kernel
as a frame of (mcs 0, psdu 0), then parsed with wlan_signal_field.

Run on a box with an MI355X:  python examples/wlan_decode.py [n_frames]
"""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import futuresdr_amd as fa  # noqa: E402

NAMES = ("Bpsk_1_2", "Bpsk_3_4", "Qpsk_1_2", "Qpsk_3_4", "Qam16_1_2",
         "Qam16_3_4", "Qam64_2_3", "Qam64_3_4")
N_BPSC = (1, 1, 2, 2, 4, 4, 6, 6)
PATTERN = ((1, 1), (1, 1, 1, 0, 0, 1), (1, 1), (1, 1, 1, 0, 0, 1), (1, 1),
           (1, 1, 1, 0, 0, 1), (1, 1, 1, 0), (1, 1, 1, 0, 0, 1))
RATE_BITS = (11, 15, 10, 14, 9, 13, 8, 12)   # SIGNAL bits 0..3, LSB first


def conv_encode(bits):
    out = np.zeros(2 * bits.size, np.uint8)
    state = 0
    for i, b in enumerate(bits):
        state = ((state << 1) & 0x7E) | int(b)
        out[2 * i] = bin(state & 0o155).count("1") & 1
        out[2 * i + 1] = bin(state & 0o117).count("1") & 1
    return out


def encode(mcs, psdu, seed):
    """Constellation indices (48 per symbol) of one frame."""
    n_sym, n_bits, n_pad = fa.wlan_frame_param(mcs, len(psdu))
    bits = np.zeros(n_bits, np.uint8)
    bits[16:16 + 8 * len(psdu)] = np.unpackbits(
        np.frombuffer(psdu, np.uint8), bitorder="little")
    state = seed
    for i in range(n_bits):
        fb = ((state >> 6) ^ (state >> 3)) & 1
        bits[i] ^= fb
        state = ((state << 1) & 0x7E) | fb
    tail = n_bits - n_pad - 6
    bits[tail:tail + 6] = 0
    coded = conv_encode(bits)
    pat = np.array(PATTERN[mcs], bool)
    coded = coded[pat[np.arange(coded.size) % pat.size]]
    m = fa.wlan_deinterleave_map(mcs)
    inter = coded.reshape(n_sym, m.size)[:, m].reshape(-1, N_BPSC[mcs])
    return (inter << np.arange(N_BPSC[mcs])).sum(1).astype(np.uint8)


def signal_symbol(mcs, length):
    bits = np.zeros(24, np.uint8)
    bits[:4] = [(RATE_BITS[mcs] >> i) & 1 for i in range(4)]
    bits[5:17] = [(length >> i) & 1 for i in range(12)]
    bits[17] = bits[:17].sum() & 1
    return conv_encode(bits)[fa.wlan_deinterleave_map(0)]


def main():
    if fa.device_count() < 1:
        raise SystemExit("needs a HIP device (MI355X)")
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    rng = np.random.default_rng(5)
    frames, signals, payloads = [], [], []
    for i in range(n_frames):
        mcs = i % 8
        payload = rng.integers(0, 256, int(rng.integers(20, 300)),
                               dtype=np.uint8).tobytes()
        psdu = payload + zlib.crc32(payload).to_bytes(4, "little")
        syms = encode(mcs, psdu, seed=1)
        n_flip = 1 + syms.size * N_BPSC[mcs] // 400
        where = rng.choice(syms.size, n_flip, replace=False)
        syms[where] ^= (1 << rng.integers(0, N_BPSC[mcs], n_flip)) \
            .astype(np.uint8)
        frames.append((mcs, len(psdu), syms))
        signals.append((0, 0, signal_symbol(mcs, len(psdu))))
        payloads.append(payload)

    dec = fa.WlanDecoder()
    heads = dec.decode(signals, raw=True)
    bodies = dec.decode(frames)
    good = 0
    for i, ((mcs, n, syms), (_, _, raw), (out, crc_ok)) in \
            enumerate(zip(frames, heads, bodies)):
        field = fa.wlan_signal_field(np.unpackbits(raw))
        match = out[2:n - 2].tobytes() == payloads[i]
        good += match and crc_ok and field == (mcs, n)
        print(f"frame {i}: SIGNAL {field}  {NAMES[mcs]:9s} psdu {n:3d}, "
              f"{syms.size // 48:2d} symbols: payload "
              f"{'matches' if match else 'DIFFERS'}, crc_ok {crc_ok}")
    print(f"{good} of {n_frames} frames recovered")


if __name__ == "__main__":
    main()
