#!/usr/bin/env python3
"""WLAN reception from samples to checked bytes, in the shape of the
reference's receiver (examples/wlan/src/bin/rx.rs:60-110): autocorrelation
metric chain -> SyncShort -> SyncLong -> 64-point FFT -> FrameEqualizer ->
Decoder. The equalizer (futuresdr_amd.WlanEqualizer) estimates the channel
from the two long-training symbols, removes every symbol's pilot phase,
decodes the SIGNAL field to learn modulation and length, and demaps the data
carriers; fa.wlan_receive then hands its indices to the frame decoder on the
device.

Two frames are synthesized as samples the way a transmitter does it: bits as
in examples/wlan_decode.py, constellation mapping and pilots (mapper.rs:
108-132), short and long preamble, 64-point IFFT with a 16-sample prefix;
white noise 30 dB below the frames, a gap of noise between them.

Run on a box with an MI355X:  python examples/wlan_rx.py
"""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import futuresdr_amd as fa  # noqa: E402
from wlan_decode import N_BPSC, NAMES, encode, signal_symbol  # noqa: E402

# IEEE 802.11 long and short training sequences on carriers 6..58
LONG = "++--++-+-++++++--++-+-++++0+--++-+-+-----++--+-+-++++"
SHORT = {-24: 1, -20: -1, -16: 1, -12: -1, -8: -1, -4: 1,
         4: -1, 8: -1, 12: 1, 16: 1, 20: 1, 24: 1}


def constellation(n_bpsc):
    """Modulation::map (lib.rs:66-175): the point of every index."""
    i = np.arange(1 << n_bpsc)
    if n_bpsc == 1:
        return (2.0 * i - 1).astype(np.complex128)
    half = n_bpsc // 2
    levels = {1: [1], 2: [3, 1], 3: [7, 1, 5, 3]}[half]
    norm = {1: np.sqrt(2), 2: np.sqrt(10), 3: np.sqrt(42)}[half]

    def axis(b):
        mag = np.array(levels)[(b >> 1) & (len(levels) - 1)]
        return mag * (2 * (b & 1) - 1) / norm

    return axis(i & ((1 << half) - 1)) + 1j * axis(i >> half)


def transmit(mcs, psdu):
    """Samples of one frame, unit power on the used carriers."""
    cm = fa.wlan_carrier_map()
    data = cm >= 0
    idx = encode(mcs, psdu, seed=1).reshape(-1, 48)
    pol = fa.wlan_pilot_polarity(len(idx) + 1).astype(np.float64)
    rows = np.zeros((3 + len(idx), 64), np.complex128)
    rows[0, 6:59] = rows[1, 6:59] = [{"+": 1, "-": -1, "0": 0}[c]
                                     for c in LONG]
    rows[2:, [11, 25, 39]] = pol[:, None]
    rows[2:, 53] = -pol
    rows[2, data] = constellation(1)[signal_symbol(mcs, len(psdu))][cm[data]]
    rows[3:, data] = constellation(N_BPSC[mcs])[idx][:, cm[data]]
    short = np.zeros(64, np.complex128)
    for k, v in SHORT.items():
        short[k + 32] = v * (1 + 1j) * np.sqrt(13 / 6)
    scale = 64 / np.sqrt(52)
    t = np.fft.ifft(np.roll(rows, 32, axis=1), axis=1) * scale
    s = np.fft.ifft(np.roll(short, 32)) * scale
    parts = [np.tile(s, 3)[:160], t[0][-32:], t[0], t[1]]
    for row in t[2:]:
        parts += [row[-16:], row]
    return np.concatenate(parts)


def main():
    if fa.device_count() < 1:
        raise SystemExit("needs a HIP device (MI355X)")
    rng = np.random.default_rng(9)
    plan = ((2, 60), (5, 100))            # Qpsk_1_2, Qam16_3_4
    payloads = [rng.integers(0, 256, n - 4, dtype=np.uint8).tobytes()
                for _, n in plan]
    psdus = [p + zlib.crc32(p).to_bytes(4, "little") for p in payloads]
    tx = [transmit(mcs, psdu) for (mcs, _), psdu in zip(plan, psdus)]
    # 80 zeros first: the metric's warm-up is then 0/0 and triggers nothing
    sig = np.concatenate([np.zeros(80), tx[0], np.zeros(600), tx[1],
                          np.zeros(160)])
    sigma = np.sqrt(10 ** (-30 / 10) / 2)
    sig[80:] += sigma * (rng.normal(size=sig.size - 80)
                         + 1j * rng.normal(size=sig.size - 80))
    sig = sig.astype(np.complex64)
    n = sig.size

    # rx.rs:60-96: delay 16, a*conj(b), sliding sums, |.|/power
    delayed = np.concatenate([np.zeros(16, np.complex64), sig[:-16]])
    abs48 = fa.wlan_moving_sum_host(fa.cmul_conj_host(sig, delayed), 48)[:n]
    mag, _, _, _ = fa.Mag2().filter(sig, n)
    power = fa.wlan_moving_sum_host(mag.astype(np.float32), 64)[:n]
    cor = fa.divide_mag_host(abs48, power)
    rx = fa.WlanRx()
    frame_samples, tags = rx.sync_short(delayed, abs48, cor)
    symbols, frames = rx.sync_long(frame_samples, tags)
    spans = fa.wlan_frame_spans(tags, frames, frame_samples.size)
    fft = fa.Fft(64)
    outs, off = [], 0
    while off < symbols.size:
        y, c, p, _ = fft.filter(symbols[off:], symbols.size - off)
        if p == 0:
            break
        outs.append(y)
        off += c
    spec = np.concatenate(outs)

    good = 0
    for i, (info, psdu, crc_ok) in enumerate(fa.wlan_receive(spec, spans)):
        if not info.found:
            print(f"frame {i}: SIGNAL field not decoded, snr "
                  f"{info.snr_db:.1f} dB")
            continue
        match = psdu is not None and i < len(psdus) and \
            psdu.tobytes() == psdus[i]
        good += match and crc_ok
        print(f"frame {i}: snr {info.snr_db:5.1f} dB  {NAMES[info.mcs]:9s} "
              f"psdu {info.psdu_size:3d}, {info.n_copied} of "
              f"{info.n_symbols} symbols: payload "
              f"{'matches' if match else 'DIFFERS'}, crc_ok {crc_ok}")
    print(f"{good} of {len(plan)} frames recovered")


if __name__ == "__main__":
    main()
