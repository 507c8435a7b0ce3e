#!/usr/bin/env python3
"""Multi-channel receiver front end in the shape of the reference's LoRa
example (examples/lora/src/bin/rx_all_channels_eu.rs:109-143): a PFB
channelizer, then on EVERY channel a PFB arbitrary-rate resampler at rate
2.5 with 5 filters.

    x -> PfbChannelizer(N) -> [N channel streams, device-resident]
      -> PfbArbResampler(2.5, taps, 5, num_channels=N) -> N streams at 2.5x

The reference adds one resampler block per channel; here the N channels run
in lockstep through one batched call that reads the channelizer's
channel-major output buffer as it is (stride out_cap_per_chan). A tone
placed inside one channel must come out of that channel's resampled stream
at 1/2.5 of its channel-rate frequency; the script prints where it lands.
What follows per channel in the reference, fft_demod's dechirp + FFT +
argmax/LLR on whole symbols, is examples/lora_demod.py.

Run on a box with an MI355X:  python examples/lora_frontend.py
"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import futuresdr_amd as fa  # noqa: E402

RATE, NUM_FILTERS = 2.5, 5


def main():
    if fa.device_count() < 1:
        raise SystemExit("needs a HIP device (MI355X)")
    lib = fa.lib()
    N, n_in = 8, 1 << 18
    chan, f_chan = 3, 0.04  # tone: channel 3, 0.04 cycles/sample there
    ctaps = fa.kaiser_lowpass(1.0 / (2 * N), 0.05, 1e-3)
    # interpolation low-pass over the 5-phase bank, passband gain 5
    rtaps = NUM_FILTERS * fa.lowpass_kaiser_n(
        NUM_FILTERS * 8, 6.0, 0.5 / NUM_FILTERS)
    t = np.arange(n_in)
    x = np.exp(2j * np.pi * (chan + f_chan) / N * t).astype(np.complex64)

    chz = fa.PfbChannelizer(N, ctaps)
    rs = fa.PfbArbResampler(RATE, rtaps, NUM_FILTERS, num_channels=N)
    cap = n_in // N
    out_cap = rs.out_cap_for(cap)
    d_x, d_mid, d_y = (ctypes.c_void_p() for _ in range(3))
    for d, items in ((d_x, n_in), (d_mid, N * cap), (d_y, N * out_cap)):
        assert lib.fsdr_dev_alloc(ctypes.byref(d), items * 8) == 0
    try:
        lib.fsdr_memcpy_h2d(d_x, ctypes.c_void_p(x.ctypes.data), n_in * 8)
        ppc, cons, prod = (ctypes.c_size_t() for _ in range(3))
        assert lib.fsdr_pfb_channelizer_run_dev(
            chz._h, d_x, n_in, d_mid, cap, None, ctypes.byref(ppc)) == 0
        # device-resident hand-off: d_mid, stride cap, ppc items per channel
        assert lib.fsdr_pfb_arb_resampler_run_dev(
            rs._h, d_mid, cap, ppc.value, d_y, out_cap, out_cap, None,
            ctypes.byref(cons), ctypes.byref(prod)) == 0, \
            lib.fsdr_last_error().decode()
        fa.synchronize()
        y = np.zeros(N * out_cap, np.complex64)
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(y.ctypes.data), d_y, y.size * 8)
    finally:
        for d in (d_x, d_mid, d_y):
            lib.fsdr_dev_free(d)
    y = y.reshape(N, out_cap)[:, :prod.value]

    s = rs.schedule
    print(f"{N} channels x {ppc.value} items in, {cons.value} consumed, "
          f"{prod.value} out per channel (rate {RATE}); schedule period "
          f"{s.period} inputs / {s.outputs_per_period} outputs")
    energy = (np.abs(y[:, 256:]) ** 2).sum(axis=1)
    nfft = 1 << 14
    spec = np.abs(np.fft.fft(y[chan, 256:256 + nfft])) ** 2
    peak = int(np.argmax(spec))
    peak_f = (peak if peak < nfft // 2 else peak - nfft) / nfft
    print(f"energy share of channel {chan}: {energy[chan] / energy.sum():.4f}")
    print(f"tone at {f_chan} cycles/sample in the channel -> peak at "
          f"{peak_f:.5f} after resampling (expected {f_chan / RATE:.5f}), "
          f"holding {spec[peak] / spec.sum():.4f} of that channel's energy")


if __name__ == "__main__":
    main()
