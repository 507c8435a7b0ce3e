"""Literal float64 restatement of the reference PfbChannelizer, shared by
test_pfb_chan_cpu.py and test_pfb_chan_gpu.py. A step-by-step transcription
of the reference source it cites, NOT the closed form the product and the
oracle use (that form is pinned against this file in test_pfb_chan_cpu.py):

  partition_filter_taps   src/blocks/pfb/utilities.rs:5-25      } from
  WindowBuffer            src/blocks/pfb/window_buffer.rs:11-44 } pfb_synth_
  FirFilter core          crates/futuredsp/src/fir.rs:69-90     } ref
  PfbChannelizer          src/blocks/pfb/channelizer.rs:90-122 (new),
                          :126-133 (decrement_base_index), :142-212 (work)

One point where this file follows the product ABI and the oracle rather
than the letter of the source: the call that completes the window fill
returns at :179 without a consume() of the samples it pushed, so a
scheduler would present them again. Here, as in the ABI, the fill samples
count as consumed; everything else is line by line.
"""
import functools

import numpy as np

from pfb_synth_ref import WindowBuffer, fir_filter_one, partition_filter_taps


class PfbChannelizerRef:
    """channelizer.rs:90-122 (new) and :142-212 (work)."""

    def __init__(self, num_channels, taps, oversample_rate=1.0):
        assert num_channels > 2                                 # :92-95
        assert len(taps) >= num_channels                        # :96-99
        assert (oversample_rate != 0.
                and num_channels % oversample_rate == 0.)       # :100-103
        self.num_channels = num_channels
        self.decimation_factor = int(num_channels / oversample_rate)  # :105
        self.fir_filters, filter_semi_length = partition_filter_taps(
            taps, num_channels)                                 # :106
        self.taps_per_filter = filter_semi_length
        self.fft_buf = np.zeros(num_channels, np.complex128)    # :115
        self.window_buf = [WindowBuffer(filter_semi_length, False)
                           for _ in range(num_channels)]        # :117
        self.base_index = num_channels - 1                      # :118
        self.all_windows_filled = False                         # :119

    def decrement_base_index(self):                             # :126-133
        self.base_index = (self.num_channels - 1 if self.base_index == 0
                           else self.base_index - 1)

    def work(self, input, out_cap):
        """One work() call over `input` with out_cap free slots per
        output; returns (out[N, produced] complex128, consumed)."""
        n_items_to_consume = len(input)                         # :149
        n_items_to_produce_per_channel = min(
            out_cap, n_items_to_consume // self.decimation_factor)  # :152-155
        none = np.zeros((self.num_channels, 0), np.complex128)
        if not self.all_windows_filled:                         # :157
            consumed = 0
            while not all(w.filled() for w in self.window_buf):  # :160
                if consumed == n_items_to_consume:              # :161-167
                    return none, consumed
                self.window_buf[self.base_index].push(input[consumed])  # :168
                self.decrement_base_index()                     # :169
                consumed += 1                                   # :170
            self.all_windows_filled = True                      # :173
            return none, consumed                               # :179
        out = np.zeros((self.num_channels, n_items_to_produce_per_channel),
                       np.complex128)
        for output_sample_index in range(
                n_items_to_produce_per_channel):                # :182
            for j in range(self.decimation_factor):             # :184
                self.window_buf[self.base_index].push(
                    input[output_sample_index * self.decimation_factor
                          + j])                                 # :186-187
                self.decrement_base_index()                     # :188
            for i in range(self.num_channels):                  # :191
                buffer_index = ((self.base_index + i + 1)
                                % self.num_channels)            # :193
                self.fft_buf[buffer_index] = fir_filter_one(
                    self.fir_filters[i],
                    self.window_buf[buffer_index].get_as_slice())  # :195-198
            # :201 rustfft Inverse: unnormalized, e^{+2 pi i m c / N}
            self.fft_buf = np.fft.ifft(self.fft_buf) * self.num_channels
            for channel_index in range(self.num_channels):      # :204-206
                out[channel_index, output_sample_index] = (
                    self.fft_buf[channel_index])
        return out, (n_items_to_produce_per_channel
                     * self.decimation_factor)                  # :209-210


def chan_oneshot(num_channels, taps, x, oversample_rate=1.0, out_cap=None):
    """A fresh block fed all of x: the fill call, then one producing call
    on what the fill left. Returns (out[N, produced], consumed)."""
    ref = PfbChannelizerRef(num_channels, taps, oversample_rate)
    x = np.asarray(x)
    none, consumed = ref.work(x, 0)
    if not ref.all_windows_filled:
        return none, consumed
    rest = x[consumed:]
    if out_cap is None:
        out_cap = len(rest) // ref.decimation_factor
    out, more = ref.work(rest, out_cap)
    return out, consumed + more


def startup_steps(num_channels, n_taps, decim):
    """Leading output steps that still see a shuffled window: step k is
    steady once (k+1)*D >= tpf*N."""
    tpf = -(-n_taps // num_channels)
    return 0 if tpf == 1 else tpf * num_channels // decim - 1


def random_case(num_channels, n_taps, decim, steady=8, seed=None):
    """Seeded taps (f32) and a loud complex64 input covering the fill,
    every start-up step and `steady` steps after them."""
    from dsp_ref import loud_c64
    tpf = -(-n_taps // num_channels)
    steps = tpf * num_channels // decim - 1 + steady
    r = np.random.default_rng(
        seed if seed is not None
        else num_channels * 100003 + n_taps * 101 + decim)
    taps = r.uniform(-1, 1, n_taps).astype(np.float32)
    x = loud_c64(r, num_channels * tpf + steps * decim)
    return taps, x


@functools.lru_cache(maxsize=None)
def cached_oneshot(num_channels, n_taps, decim, steady=8):
    """random_case + its one-shot restatement, computed once per shape and
    shared read-only by every test that needs it."""
    taps, x = random_case(num_channels, n_taps, decim, steady)
    out, consumed = chan_oneshot(num_channels, taps, x,
                                 num_channels / decim)
    for a in (taps, x, out):
        a.setflags(write=False)
    return taps, x, out, consumed
