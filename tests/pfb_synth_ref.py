"""Literal float64 restatement of the reference PfbSynthesizer, shared by
test_pfb_synth_cpu.py and test_pfb_synth_gpu.py (oracle/ is frozen, so it
lives with the tests). Each part is a step-by-step transcription of the
reference source it cites, NOT the closed form the product uses:

  partition_filter_taps   src/blocks/pfb/utilities.rs:5-25
  WindowBuffer            src/blocks/pfb/window_buffer.rs:11-44
  FirFilter core          crates/futuredsp/src/fir.rs:69-90
  PfbSynthesizer          src/blocks/pfb/synthesizer.rs:59-71, 86-118
"""
import functools
import math

import numpy as np


def partition_filter_taps(taps, n_filters):
    """utilities.rs:5-25 -> (list of tap arrays, taps_per_filter)."""
    taps = np.asarray(taps, np.float64)
    taps_per_filter = math.ceil(len(taps) / n_filters)          # :10
    filters = []
    for i in range(n_filters):                                  # :11
        pad = taps_per_filter - math.ceil((len(taps) - i) / n_filters)  # :12
        taps_tmp = list(taps[i::n_filters]) + [0.0] * pad       # :13-20
        assert len(taps_tmp) == taps_per_filter                 # :21
        filters.append(np.array(taps_tmp, np.float64))
    return filters, taps_per_filter


class WindowBuffer:
    """window_buffer.rs:11-44."""

    def __init__(self, buffer_len, pad_start):                  # :13-20
        self.buffer_len = buffer_len
        self.circular_buffer = np.zeros(buffer_len * 2, np.complex128)
        self.start_idx = 0
        self.num_samples_missing = 0 if pad_start else buffer_len

    def push(self, sample):                                     # :23-32
        at = (self.start_idx - self.num_samples_missing) % self.buffer_len
        self.circular_buffer[at] = sample
        self.circular_buffer[at + self.buffer_len] = sample
        self.num_samples_missing = max(self.num_samples_missing - 1, 0)
        self.start_idx = (self.start_idx + 1) % self.buffer_len

    def get_as_slice(self):                                     # :35-39
        assert self.num_samples_missing == 0
        return self.circular_buffer[
            self.start_idx:self.start_idx + self.buffer_len]

    def filled(self):                                           # :41-43
        return self.num_samples_missing == 0


def fir_filter_one(taps, window):
    """FirFilter::filter into a 1-item output — fir.rs:69-90: the sum
    over t of window[t] * taps[num_taps-1-t]."""
    num_taps = len(taps)
    assert len(window) + 1 - num_taps >= 1                      # :69
    acc = 0.0 + 0.0j
    for t in range(num_taps):                                   # :79-85
        acc = acc + window[t] * taps[num_taps - 1 - t]
    return acc


class PfbSynthesizerRef:
    """synthesizer.rs:59-71 (new) and :86-118 (work)."""

    def __init__(self, num_channels, taps):
        self.num_channels = num_channels
        self.fir_filters, filter_length = partition_filter_taps(
            taps, num_channels)                                 # :60
        self.taps_per_filter = filter_length
        self.window_buf = [WindowBuffer(filter_length, False)
                           for _ in range(num_channels)]        # :68
        self.all_windows_filled = False                         # :69

    def work(self, inputs, out_cap):
        """inputs: one sequence per channel; returns (out, consumed).
        Raises IndexError where the reference slice out[produced..
        produced+1] would panic (:111)."""
        n_items_to_consume = min(len(x) for x in inputs)        # :88
        n_items_to_produce = out_cap                            # :89
        out = np.zeros(out_cap, np.complex128)
        consumed_per_channel = 0
        produced = 0
        while (n_items_to_consume - consumed_per_channel > 0
               and (n_items_to_produce - produced > self.num_channels
                    or not self.all_windows_filled)):           # :93-94
            fft_buf = np.array([x[consumed_per_channel] for x in inputs],
                               np.complex128)                   # :97-99
            consumed_per_channel += 1                           # :100
            # :102 rustfft Inverse: unnormalized, e^{+2 pi i m c / N}
            fft_buf = np.fft.ifft(fft_buf) * self.num_channels
            for window, fir, spun in zip(self.window_buf, self.fir_filters,
                                         fft_buf):              # :103-108
                window.push(spun)                               # :109
                if window.filled():                             # :110
                    if produced + 1 > out_cap:
                        raise IndexError("out[produced..produced+1]")
                    out[produced] = fir_filter_one(
                        fir, window.get_as_slice())             # :111
                    produced += 1                               # :112
            if not self.all_windows_filled:                     # :115-117
                self.all_windows_filled = all(
                    w.filled() for w in self.window_buf)
        return out[:produced], consumed_per_channel


def synth_oneshot(num_channels, taps, chans, out_cap=None):
    """One work() call from a fresh block; (out complex128, consumed)."""
    chans = np.asarray(chans)
    if out_cap is None:
        out_cap = (chans.shape[1] + 1) * num_channels
    return PfbSynthesizerRef(num_channels, taps).work(list(chans), out_cap)


def random_case(num_channels, n_taps, steps, seed=None):
    """Seeded taps (f32) and channel rows (complex64) for a shape."""
    r = np.random.default_rng(
        seed if seed is not None
        else num_channels * 100003 + n_taps * 101 + steps)
    taps = r.uniform(-1, 1, n_taps).astype(np.float32)
    chans = (r.uniform(-1, 1, (num_channels, steps, 2)) @ [1, 1j]).astype(
        np.complex64)
    return taps, chans


@functools.lru_cache(maxsize=None)
def cached_oneshot(num_channels, n_taps, steps):
    """random_case + its one-shot restatement, computed once per shape
    and shared by every test (and both kernel paths) that needs it."""
    taps, chans = random_case(num_channels, n_taps, steps)
    out, consumed = synth_oneshot(num_channels, taps, chans)
    for a in (taps, chans, out):
        a.setflags(write=False)
    return taps, chans, out, consumed


def tone_prototype(num_channels=16, n_taps=128, beta=8.0):
    """sinc(k/N) * kaiser(n_taps, beta), k centred on the filter."""
    k = np.arange(n_taps) - (n_taps - 1) / 2.0
    return (np.sinc(k / num_channels) * np.kaiser(n_taps, beta)).astype(
        np.float32)


def tone_energy_fraction(out, num_channels, taps_per_filter, m, nfft=2048):
    """Drop N*tpf outputs, FFT the next nfft: (peak bin, its share of the
    energy, expected bin)."""
    seg = np.asarray(out)[num_channels * taps_per_filter:][:nfft]
    assert seg.size == nfft
    e = np.abs(np.fft.fft(seg)) ** 2
    peak = int(np.argmax(e))
    return peak, float(e[peak] / e.sum()), nfft * m // num_channels
