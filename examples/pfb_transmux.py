#!/usr/bin/env python3
"""PFB transmultiplexer: channelize -> synthesize on the GPU with the
channel streams staying in device memory in between.

    x -> PfbChannelizer(N) -> [N channel streams, device-resident]
      -> PfbSynthesizer(N) -> y

The channelizer writes channel-major rows with stride out_cap_per_chan;
the synthesizer reads exactly that layout, so the buffer is handed over
as it is. Prints the reconstruction error of y against x after aligning
delay and complex gain (least squares). Asserts nothing: how close a
maximally decimated bank gets depends on the prototype.

Run on a box with an MI355X:  python examples/pfb_transmux.py
"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import futuresdr_amd as fa  # noqa: E402


def prototype(n_chan, taps_per_chan, beta=8.0):
    n = n_chan * taps_per_chan
    k = np.arange(n) - (n - 1) / 2.0
    h = np.sinc(k / n_chan) * np.kaiser(n, beta)
    return (h / h.sum()).astype(np.float32)


def aligned_error(x, y, max_delay):
    """Best (delay, relative l2 error) of y ~ g * x delayed, g complex."""
    best = (0, np.inf)
    for d in range(max_delay + 1):
        n = min(x.size, y.size - d)
        if n <= 0:
            break
        a, b = x[:n].astype(np.complex128), y[d:d + n].astype(np.complex128)
        g = np.vdot(a, b) / np.vdot(a, a)
        err = np.linalg.norm(b - g * a) / np.linalg.norm(b)
        if err < best[1]:
            best = (d, float(err))
    return best


def main():
    if fa.device_count() < 1:
        raise SystemExit("needs a HIP device (MI355X)")
    lib = fa.lib()
    N, tpc, n_in = 16, 8, 1 << 16
    taps = prototype(N, tpc)
    t = np.arange(n_in)
    x = (0.6 * np.exp(2j * np.pi * 0.012 * t)          # inside channel 0
         + 0.3 * np.exp(2j * np.pi * (3 / N + 0.004) * t)  # channel 3
         ).astype(np.complex64)

    chz = fa.PfbChannelizer(N, taps)
    syn = fa.PfbSynthesizer(N, taps * N)  # interpolation gain N
    cap = n_in // N
    d_x, d_mid, d_y = (ctypes.c_void_p() for _ in range(3))
    for d, items in ((d_x, n_in), (d_mid, N * cap), (d_y, n_in + N)):
        assert lib.fsdr_dev_alloc(ctypes.byref(d), items * 8) == 0
    try:
        lib.fsdr_memcpy_h2d(d_x, ctypes.c_void_p(x.ctypes.data), n_in * 8)
        ppc, cons, prod = (ctypes.c_size_t() for _ in range(3))
        assert lib.fsdr_pfb_channelizer_run_dev(
            chz._h, d_x, n_in, d_mid, cap, None, ctypes.byref(ppc)) == 0
        # device-resident hand-off: d_mid, stride cap, ppc steps per channel
        assert lib.fsdr_pfb_synthesizer_run_dev(
            syn._h, d_mid, cap, ppc.value, d_y, n_in + N, None,
            ctypes.byref(cons), ctypes.byref(prod)) == 0, \
            lib.fsdr_last_error().decode()
        fa.synchronize()
        y = np.zeros(prod.value, np.complex64)
        lib.fsdr_memcpy_d2h(ctypes.c_void_p(y.ctypes.data), d_y, y.size * 8)
    finally:
        for d in (d_x, d_mid, d_y):
            lib.fsdr_dev_free(d)

    skip = 2 * N * tpc  # both banks' start-up
    delay, err = aligned_error(x[skip:skip + 8192], y[skip:], 4 * N * tpc)
    print(f"channels {N}, {taps.size} taps: {ppc.value} steps per channel "
          f"through the device buffer, {prod.value} samples synthesized")
    print(f"reconstruction: best delay {delay} samples, "
          f"relative l2 error {err:.3e}")


if __name__ == "__main__":
    main()
