"""Literal restatement of the reference PfbArbResampler, shared by
test_pfb_arb_cpu.py, test_pfb_arb_gpu.py and tests/golden/generate_pfb_arb.py.
A step-by-step transcription of src/blocks/pfb/arb_resampler.rs, NOT the
checkpointed schedule the product uses:

  new                   arb_resampler.rs:90-127
  update_timing_state   :132-140
  consume_single        :142-188
  work                  :193-231

The timing state is held in np.float32 scalars, one numpy op per reference
op (numpy rounds each to nearest, as Rust does); filtering and the
interpolation are in float64. WindowBuffer, partition_filter_taps and
fir_filter_one come from pfb_synth_ref.py.
"""
import math

import numpy as np

from pfb_synth_ref import WindowBuffer, fir_filter_one, partition_filter_taps

F32 = np.float32
INTERPOLATE, BOUNDARY = 0, 1


def _abs_dot(taps, window):
    """(sum |h||re x|, sum |h||im x|) of fir_filter_one's terms: the
    magnitude the rounding-error bar of the GPU tests scales with."""
    num_taps = len(taps)
    w = np.asarray(window[:num_taps])
    h = np.abs(taps[::-1])
    return complex(float(np.sum(h * np.abs(w.real))),
                   float(np.sum(h * np.abs(w.imag))))


class PfbArbResamplerRef:
    """taps=None gives the timing state machine alone (no samples)."""

    def __init__(self, rate, taps, num_filters):                # :90-127
        rate = F32(rate)
        assert rate > 0.0                                       # :92-95
        if taps is not None:
            assert len(taps) >= num_filters                     # :96-99
        assert num_filters != 0                                 # :100-103
        if taps is not None:
            self.fir_filters, filter_length = partition_filter_taps(
                taps, num_filters)                              # :105
            self.window_buf = WindowBuffer(filter_length, False)  # :114
            self.taps_per_filter = filter_length
        else:
            self.fir_filters = self.window_buf = None
        self.min_items = math.ceil(rate)                        # :108
        self.num_filters = num_filters
        self.rate = rate
        self.delay = F32(1.0) / rate                            # :116
        self.buff = [0j, 0j]
        self.abs_buff = [0j, 0j]
        self.state = INTERPOLATE
        self.tau = F32(0.0)
        self.bf = F32(0.0)
        self.base_index = 0
        self.mu = F32(0.0)
        self.inputs_seen = 0    # consume_single calls so far
        self.records = []       # (input, base_index, boundary, mu)
        self.bounds = []        # per output: |.| sums for the error bar

    def timing_state(self):
        """The state in front of an input, as the cycle detection sees it."""
        return (self.tau.tobytes(), self.base_index, self.mu.tobytes(),
                self.state)

    def update_timing_state(self):                              # :132-140
        self.tau = self.tau + self.delay                        # :134
        self.bf = self.tau * F32(self.num_filters)              # :136
        fl = np.floor(self.bf)
        # `as usize` saturates: negative and NaN give 0
        self.base_index = int(fl) if fl > 0 else 0              # :138
        self.mu = self.bf - F32(self.base_index)                # :139
        assert self.tau.dtype == F32 and self.mu.dtype == F32

    def _filter(self, f, slot):
        if self.fir_filters is None:
            return
        w = self.window_buf.get_as_slice()
        self.buff[slot] = fir_filter_one(self.fir_filters[f], w)
        self.abs_buff[slot] = _abs_dot(self.fir_filters[f], w)

    def _emit(self, out_buf, boundary):
        mu = float(self.mu)
        out_buf.append((1.0 - mu) * self.buff[0] + mu * self.buff[1])
        self.records.append((self.inputs_seen, self.base_index, boundary,
                             self.mu))
        if self.fir_filters is not None:
            a, b = self.abs_buff
            self.bounds.append(abs(1.0 - mu) * a + abs(mu) * b)

    def consume_single(self, sample, out_buf):                  # :142-188
        if self.window_buf is not None:
            self.window_buf.push(sample)                        # :143
        produced = 0
        while self.base_index < self.num_filters:               # :145
            if self.state == BOUNDARY:                          # :147
                self._filter(0, 1)                              # :149-150
                self._emit(out_buf, 1)                          # :152
                produced += 1
                self.update_timing_state()                      # :154
                self.state = INTERPOLATE                        # :155
            else:
                self._filter(self.base_index, 0)                # :159-160
                if self.base_index == self.num_filters - 1:     # :164
                    self.state = BOUNDARY                       # :166
                    self.base_index = self.num_filters          # :169
                else:
                    self._filter(self.base_index + 1, 1)        # :173-174
                    self._emit(out_buf, 0)                      # :176
                    produced += 1
                    self.update_timing_state()                  # :178
        self.tau = self.tau - F32(1.0)                          # :184
        self.bf = self.bf - F32(self.num_filters)               # :185
        self.base_index -= self.num_filters                     # :186
        self.inputs_seen += 1
        return produced

    def work(self, inputs, out_cap):                            # :193-231
        """One work() call; returns (outputs list, consumed). Raises
        IndexError where out[produced] would be out of range."""
        ninput_items = len(inputs)
        if not self.window_buf.filled():                        # :202
            consumed = 0
            while not self.window_buf.filled() and consumed < ninput_items:
                self.window_buf.push(inputs[consumed])          # :205
                consumed += 1
            return [], consumed                                 # :208-214
        noutput_items = out_cap
        nitem_to_process = min(
            ninput_items, int(F32(noutput_items) / self.rate))  # :218
        out = []
        for sample in inputs[:nitem_to_process]:                # :221
            self.consume_single(sample, out)                    # :222
            if len(out) > out_cap:
                raise IndexError("out[produced..]")
        return out, nitem_to_process                            # :224-225

    def call(self, inputs, out_cap):
        """What one product call restates: the fill work() (if the window
        is not filled), then one processing work() on what remains."""
        consumed = 0
        if not self.window_buf.filled():
            _, consumed = self.work(inputs, out_cap)
            if not self.window_buf.filled() or consumed == len(inputs):
                return [], consumed
        out, c = self.work(inputs[consumed:], out_cap)
        return out, consumed + c


def timing_records(rate, num_filters, first_input, n_inputs, start=None):
    """Walk the timing state alone from input 0 (or continue `start`);
    returns (ref, records of inputs [first_input, first_input+n_inputs))."""
    ref = start or PfbArbResamplerRef(rate, None, num_filters)
    sink = []
    while ref.inputs_seen < first_input:
        ref.consume_single(None, sink)
    ref.records = []
    for _ in range(n_inputs):
        ref.consume_single(None, sink)
    return ref, list(ref.records)


def records_arrays(records):
    """records -> (in_index u64, base_index u32, boundary u8, mu f32)."""
    idx = np.array([r[0] for r in records], np.uint64)
    base = np.array([r[1] for r in records], np.uint32)
    bnd = np.array([r[2] for r in records], np.uint8)
    mu = np.array([r[3] for r in records], np.float32)
    return idx, base, bnd, mu


def startup_window(tpf):
    """Slot -> fill push index (or -1) of the literal WindowBuffer after
    tpf pushes, read back through get_as_slice()."""
    w = WindowBuffer(tpf, False)
    for k in range(tpf):
        w.push(complex(k + 1, 0))
    assert w.filled()
    return np.array([int(round(v.real)) - 1 for v in w.get_as_slice()],
                    np.int64)


def random_case(rate, num_filters, n_taps, channels, n_in, seed=None):
    """Seeded taps (f32) and channel rows (complex64), every component in
    +-[0.5, 1) as in DESIGN.md (c)."""
    r = np.random.default_rng(
        seed if seed is not None
        else int(rate * 1000) * 7919 + num_filters * 101 + n_taps * 13
        + channels * 3 + n_in)

    def pm(shape):
        return r.uniform(0.5, 1.0, shape) * r.choice([-1.0, 1.0], shape)

    taps = pm(n_taps).astype(np.float32)
    chans = (pm((channels, n_in)) + 1j * pm((channels, n_in))).astype(
        np.complex64)
    return taps, chans


def oneshot(rate, num_filters, taps, chans, out_cap):
    """One call() from a fresh block per channel row. Returns (out
    [C, produced] complex128, bounds [C, produced] complex128 holding the
    per-component magnitude sums, consumed, and per output the index of
    the input that emitted it, counted after the fill)."""
    outs, bnds, cons, idx = [], [], None, None
    for row in np.asarray(chans).reshape(len(chans), -1):
        ref = PfbArbResamplerRef(rate, taps, num_filters)
        out, c = ref.call(list(row), out_cap)
        assert cons is None or cons == c
        cons = c
        outs.append(np.array(out, np.complex128))
        bnds.append(np.array(ref.bounds, np.complex128))
        idx = np.array([r[0] for r in ref.records], np.int64)
    return (np.array(outs).reshape(len(outs), -1),
            np.array(bnds).reshape(len(bnds), -1), cons, idx)
