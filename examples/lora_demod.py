#!/usr/bin/env python3
"""LoRa symbol demodulation in the shape of the reference's FftDemod
(examples/lora/src/fft_demod.rs): every symbol of N = 2^sf samples is
dechirped, transformed and reduced to a hard decision or to sf LLRs in one
kernel (futuresdr_amd.LoraFftDemod).

The input is synthesized: a few hundred random symbols with the
reference's build_upchirp(id, sf, 1, false) formula (utils.rs:884-914)
plus white Gaussian noise. build_upchirp(id, ..., false) is the chirp of
(id - 1) mod N, and the demodulator's "-1" shift (fft_demod.rs:242-246)
makes the hard decision (id - 1) mod N as well, so that is the symbol the
decisions are counted against. The LLRs come MSB first over the Gray code
of that symbol (fft_demod.rs:192-207): a positive LLR says the bit is 1.

Run on a box with an MI355X:  python examples/lora_demod.py [sf] [snr_db]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import futuresdr_amd as fa  # noqa: E402


def upchirp(sym_id, sf):
    """build_upchirp(id, sf, 1, false) in float32, as the reference."""
    n = 1 << sf
    f32 = np.float32
    sym_id = (sym_id - 1) % n
    j = np.arange(n)
    t = j.astype(f32)
    off = np.where(j < n - sym_id, f32(0.5), f32(1.5)).astype(f32)
    ph = (f32(2.0) * f32(np.pi)) * ((t * t) / (f32(2.0) * f32(n))
                                    + (f32(sym_id) / f32(n) - off) * t)
    return (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64)


def main():
    if fa.device_count() < 1:
        raise SystemExit("needs a HIP device (MI355X)")
    sf = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    snr_db = float(sys.argv[2]) if len(sys.argv) > 2 else -8.0
    n, n_sym = 1 << sf, 300
    rng = np.random.default_rng(7)
    ids = rng.integers(0, n, n_sym)
    x = np.concatenate([upchirp(int(s), sf) for s in ids])
    sd = np.sqrt(0.5 / 10.0 ** (snr_db / 10.0))
    x = (x + sd * (rng.standard_normal(x.size)
                   + 1j * rng.standard_normal(x.size))).astype(np.complex64)
    sent = (ids - 1) % n

    hard, cons, prod, _ = fa.LoraFftDemod(sf, fa.LORA_HARD).filter(x, n_sym)
    assert (cons, prod) == (x.size, n_sym)
    print(f"sf {sf}, {n_sym} symbols at {snr_db:+.1f} dB per sample: "
          f"{int(np.count_nonzero(hard != sent))} symbol errors (hard)")

    llr, _, prod, _ = fa.LoraFftDemod(sf, fa.LORA_SOFT).filter(x, n_sym)
    gray = sent ^ (sent >> 1)
    bits = (gray[:, None] >> (sf - 1 - np.arange(sf))[None, :]) & 1
    agree = (llr[:, :sf] > 0) == bits.astype(bool)
    print(f"LLR signs agree with the Gray bits on {int(agree.sum())} of "
          f"{agree.size} bits; entries {sf}..11 are "
          f"{'all 0' if not llr[:, sf:].any() else 'NOT all 0'}; "
          f"median |LLR| {np.median(np.abs(llr[:, :sf])):.3g}")


if __name__ == "__main__":
    main()
