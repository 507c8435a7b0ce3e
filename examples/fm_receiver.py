#!/usr/bin/env python3
"""FM receiver (the reference's examples/fm-receiver flowgraph,
src/main.rs:92-129) on a synthesized signal: an FM-modulated audio tone
at 1 MS/s, its carrier offset from the tuned frequency.

    shift (rotator) > resamp1 6/25 (1 MS/s -> 240 kS/s)
                    > demod + resamp2 1/5 (-> 48 kS/s), one fused block
                    [> de-emphasis, a one-pole IIR at 48 kS/s]
                    > vector sink

The source and the audio sink are left out. The de-emphasis filter the
reference wishes for (main.rs:117) is off by default; receive(x,
deemph_tau=75e-6) appends it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import futuresdr_amd as fa  # noqa: E402

FS = 1_000_000.0         # input rate
OFFSET = 100_000.0       # carrier above the tuned frequency, Hz
AUDIO_TONE = 1_000.0     # modulating tone, Hz
DEVIATION = 25_000.0     # peak frequency deviation, Hz
INTERP, DECIM = 6, 25    # resamp1: FS -> 240 kS/s
AUDIO_MULT = 5           # resamp2: 240 kS/s -> 48 kS/s
AUDIO_RATE = FS * INTERP / DECIM / AUDIO_MULT


def synthesize(n):
    t = np.arange(n) / FS
    phase = (2 * np.pi * OFFSET * t
             - DEVIATION / AUDIO_TONE * np.cos(2 * np.pi * AUDIO_TONE * t))
    return np.exp(1j * phase).astype(np.complex64)


def deemph_taps(tau):
    """(a, b) of y[k] = (1-p) x[k] + p y[k-1], p = exp(-1/(rate*tau))."""
    p = np.float32(np.exp(-1.0 / (AUDIO_RATE * tau)))
    return [p], [np.float32(1.0) - p]


def receive(x, deemph_tau=None):
    """The flowgraph above; returns the 48 kS/s audio (float32)."""
    shifted, _ = fa.rotator_host(x, -2 * np.pi * OFFSET / FS)
    if_rate = FS * INTERP / DECIM
    audio_taps = fa.kaiser_lowpass(2e3 / if_rate, 10e3 / if_rate, 0.1)
    fg = fa.Flowgraph()
    src = fg.vector_source(shifted)
    resamp1 = fg.filter(fa.Resampler(INTERP, DECIM,
                                     fa.kaiser_multirate(INTERP, DECIM)))
    back = fg.filter(fa.FmDemodResampler(1, AUDIO_MULT, audio_taps))
    snk = fg.vector_sink()
    blocks = [src, resamp1, back]
    if deemph_tau is not None:
        blocks.append(fg.filter(fa.Iir(*deemph_taps(deemph_tau))))
    fg.connect(*blocks, snk)
    fg.run()
    return fg.sink_data(snk, np.float32)


def tone_bin(audio):
    """(peak bin, expected bin, bins) of the Hann-windowed audio spectrum."""
    a = audio.astype(np.float64)
    spec = np.abs(np.fft.rfft((a - a.mean()) * np.hanning(a.size)))
    return (int(spec.argmax()), int(round(AUDIO_TONE / AUDIO_RATE * a.size)),
            spec.size)


def main():
    if fa.device_count() < 1:
        raise SystemExit("needs a HIP device (MI355X)")
    audio = receive(synthesize(1 << 20))
    peak, want, bins = tone_bin(audio)
    hz = AUDIO_RATE / audio.size
    print(f"audio samples: {audio.size} at {AUDIO_RATE:.0f} S/s")
    print(f"recovered tone: bin {peak} of {bins} = {peak * hz:.1f} Hz "
          f"(expected bin {want} = {AUDIO_TONE:.1f} Hz)")
    # past the filters' start-up; a sine's amplitude is sqrt(2) * rms
    amp = np.sqrt(2.0) * audio[200:].astype(np.float64).std()
    print(f"tone amplitude: {amp:.4f} rad/sample (expected "
          f"{2 * np.pi * DEVIATION / (FS * INTERP / DECIM):.4f} times the "
          "audio filter's gain at the tone, designed to 0.1 ripple)")


if __name__ == "__main__":
    main()
