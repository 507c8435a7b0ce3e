#!/usr/bin/env python3
"""Standalone rooflines for the off-metric-path kernels (VERDICT weak-3):
XlatingFir (tiled), FirCC (WLAN correlator shape + bulk), resampler
shapes, the standalone FFT kernel, and the PFB synthesizer (fused and
staged path per shape, plus the channelizer at the same shape for
context). Prints TF/s or GB/s vs peak. --synth runs the PFB synthesizer
part only, --arb the PFB arbitrary-rate resampler part only, --iir the IIR
filter part only, --lora the LoRa FFT demodulator part only, --wlan-decode
the WLAN frame decoder part only, --wlan-eq the WLAN frame equalizer part
only."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import futuresdr_amd as fa  # noqa: E402

PEAK_TF = 157.3
PEAK_HBM = 8.0  # TB/s


def timeit(fn, reps=10, warm=3):
    st = torch.cuda.current_stream()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pfb_synth_lines(lib, st, d_in, d_out, S, rounds=5):
    """Synthesizer at N in {16, 256, 1024}, tpf = 8, ~S output samples:
    `rounds` interleaved timings of the fused and the staged path
    (FSDR_PFB_SYNTH_FUSED is read per call), median and range of each,
    and the achieved share of HBM peak at the op's floor of 16 B per
    output sample (8 in, 8 out)."""
    sz = ctypes.c_size_t
    for N in (16, 256, 1024):
        tpf = 8
        taps = fa.lowpass_kaiser_n(N * tpf, 8.0, 0.5 / N)
        syn = fa.PfbSynthesizer(N, taps)
        T = S // N
        cons, prod = sz(), sz()

        def run():
            rc = lib.fsdr_pfb_synthesizer_run_dev(
                syn._h, d_in, T, T, d_out, S, ctypes.c_void_p(st.cuda_stream),
                ctypes.byref(cons), ctypes.byref(prod))
            assert rc == 0, lib.fsdr_last_error().decode()

        ms = {"fused": [], "staged": []}
        for _ in range(rounds):
            for name, knob in (("fused", "1"), ("staged", "0")):
                os.environ["FSDR_PFB_SYNTH_FUSED"] = knob
                ms[name].append(timeit(run, reps=5, warm=2))
        os.environ.pop("FSDR_PFB_SYNTH_FUSED", None)
        assert cons.value == T and prod.value == (T - tpf + 1) * N
        for name in ("fused", "staged"):
            v = sorted(ms[name])
            med = v[len(v) // 2]
            tbs = prod.value * 16 / (med * 1e-3) / 1e12
            print(f"pfb_synth(N={N},tpf={tpf}) {name:6s}: {med:7.3f} ms "
                  f"median of {rounds} [{v[0]:.3f}..{v[-1]:.3f}]  "
                  f"{tbs:5.2f} TB/s at 16 B/sample "
                  f"({tbs / PEAK_HBM:.3f} of HBM peak)")
        chz = fa.PfbChannelizer(N, taps)
        ppc = sz()
        v = sorted(timeit(lambda: lib.fsdr_pfb_channelizer_run_dev(
            chz._h, d_in, S, d_out, T, ctypes.c_void_p(st.cuda_stream),
            ctypes.byref(ppc)), reps=5, warm=2) for _ in range(rounds))
        tbs = ppc.value * N * 16 / (v[len(v) // 2] * 1e-3) / 1e12
        print(f"pfb_channelizer(N={N},taps={N * tpf}) context: "
              f"{v[len(v) // 2]:7.3f} ms median [{v[0]:.3f}..{v[-1]:.3f}]  "
              f"{tbs:5.2f} TB/s at 16 B/sample")


def pfb_arb_lines(lib, st, d_in, S, rounds=5):
    """PFB arb resampler, S input samples in all per shape: the LoRa shape
    (rate 2.5, 5 filters, tpf 8) over 64 channels in lockstep, and rate 0.7
    with 32 filters (tpf 8) on one long channel; for context the rational
    Resampler(5, 2) with as many taps on the same S samples. `rounds`
    timings of each, interleaved; median, range and the share of HBM peak
    at the op's floor of 8 + 8*rate bytes per input sample. Also the
    create-time schedule walk of the longest cycle found so far."""
    import time
    sz = ctypes.c_size_t
    stream = ctypes.c_void_p(st.cuda_stream)
    legs = []
    out_items = int(S * 2.5 * 1.001) + 4096
    d_out = ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(d_out), out_items * 8) == 0
    for rate, nf, C in ((2.5, 5, 64), (0.7, 32, 1)):
        taps = fa.lowpass_kaiser_n(nf * 8, 8.0, 0.5 / nf)
        rs = fa.PfbArbResampler(rate, taps, nf, C)
        T = S // C
        cap = rs.out_cap_for(T)
        assert C * cap <= out_items
        cons, prod = sz(), sz()

        def run(rs=rs, T=T, cap=cap, cons=cons, prod=prod):
            rc = lib.fsdr_pfb_arb_resampler_run_dev(
                rs._h, d_in, T, T, d_out, cap, cap, stream,
                ctypes.byref(cons), ctypes.byref(prod))
            assert rc == 0, lib.fsdr_last_error().decode()

        legs.append((f"pfb_arb(rate={rate},nf={nf},tpf=8,C={C},"
                     f"T=2^{T.bit_length() - 1})", run, rate,
                     lambda c=cons, p=prod, T=T: (c.value, p.value, T), rs))
    rtaps = fa.lowpass_kaiser_n(40, 8.0, 0.1)
    rr = fa.Resampler(5, 2, rtaps)
    legs.append(("resampler(5,2,taps=40) context",
                 lambda: rr.filter_dev(d_in.value, S, d_out.value, out_items,
                                       stream=st.cuda_stream), 2.5, None, rr))
    ms = [[] for _ in legs]
    for _ in range(rounds):
        for k, leg in enumerate(legs):
            ms[k].append(timeit(leg[1], reps=5, warm=2))
    for k, (name, _, rate, counts, _) in enumerate(legs):
        v = sorted(ms[k])
        med = v[len(v) // 2]
        tbs = S * (8 + 8 * rate) / (med * 1e-3) / 1e12
        extra = ""
        if counts:
            c, p, T = counts()
            assert c == T
            extra = f"  produced/chan {p}"
        print(f"{name}: {med:7.3f} ms median of {rounds} "
              f"[{v[0]:.3f}..{v[-1]:.3f}]  {tbs:5.2f} TB/s at "
              f"{8 + 8 * rate:.1f} B/input ({tbs / PEAK_HBM:.3f} of HBM "
              f"peak){extra}")
    lib.fsdr_dev_free(d_out)
    for rate, nf in ((0.9371897, 2), (2.5, 5)):
        t0 = time.perf_counter()
        s = fa.PfbArbSchedule(rate, nf)
        dt = time.perf_counter() - t0
        print(f"pfb_arb schedule create(rate={rate},nf={nf}): {dt:.3f} s on "
              f"one host core, preperiod {s.preperiod} period {s.period} "
              f"inputs, one 24-byte checkpoint every {s.checkpoint_spacing}: "
              f"{-(-(s.preperiod + s.period) // s.checkpoint_spacing) * 24 / 1e6:.2f} MB")


def iir_lines(lib, st, d_in, d_out, S, rounds=5):
    """IIR filter over S device-resident f32 samples in one call: the
    de-emphasis one-pole (D), a biquad (B) and an order-8 filter (O) of
    tests/iir_ref.py; for context a device-to-device copy of the same
    8 B/sample and FirF32 with as many taps as the biquad has feed-forward
    taps. `rounds` timings of each (5 back-to-back calls after 2 warm-up
    calls), the legs interleaved; median, range, and the rate against the
    op's floor of 8 B/sample and against the 12 B/sample the three-launch
    design moves (the input is read twice)."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..",
                                    "tests"))
    import iir_ref
    legs = []
    for name in ("D", "B", "O"):
        a, b = iir_ref.FILTERS[name]
        f = fa.Iir(a, b)
        legs.append((f"iir {name} (n_a={a.size}, n_b={b.size})",
                     lambda f=f: f.filter_dev(d_in.value, S, d_out.value, S,
                                              stream=st.cuda_stream), f))
    fir = fa.FirF32(iir_ref.FILTERS["B"][1])
    legs.append(("fir_f32(3 taps) context",
                 lambda: fir.filter_dev(d_in.value, S, d_out.value, S,
                                        stream=st.cuda_stream), fir))
    src = torch.empty(S, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    legs.append(("d2d copy, 8 B/sample", lambda: dst.copy_(src), None))
    ms = [[] for _ in legs]
    for _ in range(rounds):
        for k, leg in enumerate(legs):
            ms[k].append(timeit(leg[1], reps=5, warm=2))
    copy_med = sorted(ms[-1])[rounds // 2]
    for k, (name, _, _) in enumerate(legs):
        v = sorted(ms[k])
        med = v[len(v) // 2]
        tbs = S * 8 / (med * 1e-3) / 1e12
        line = (f"{name:26s}: {med:7.3f} ms median of {rounds} "
                f"[{v[0]:.3f}..{v[-1]:.3f}]  {tbs:5.2f} TB/s at 8 B/sample "
                f"({tbs / PEAK_HBM:.3f} of HBM peak), "
                f"{med / copy_med:.2f}x the copy")
        if name.startswith("iir"):
            line += f"; {tbs * 1.5:5.2f} TB/s of the 12 B/sample moved"
        print(line)


def lora_symbols(sf, S, snr_lin, seed):
    """S device-resident samples of random LoRa symbols (the chirp of a
    random id per symbol, phase formed in float64) plus complex Gaussian
    noise of variance 1/snr_lin."""
    n = 1 << sf
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(0, n, (S // n, 1), generator=g,
                        device="cuda").to(torch.float64)
    t = torch.arange(n, device="cuda", dtype=torch.float64)[None, :]
    ph = (t * t / (2.0 * n) + (ids / n - 0.5) * t) % 1.0
    ph = (ph * (2.0 * np.pi)).to(torch.float32).reshape(-1)
    del ids, t
    x = torch.polar(torch.ones_like(ph), ph)
    del ph
    sd = float(np.sqrt(0.5 / snr_lin))
    x += sd * torch.view_as_complex(
        torch.randn(S, 2, generator=g, device="cuda", dtype=torch.float32))
    return x


def lora_lines(lib, st, d_out, S, rounds=5):
    """LoRa FFT demodulator over S device-resident samples of whole symbols
    in one call, sf 7, 9 and 12: the fused HARD call, the fused SOFT call
    in its ln I0 branch (largest Bessel argument near 300) and in its
    clipped branch (near 3000), against what the library composes the same
    arithmetic from today, of which only the Stockham FFT with its |X|^2
    output is timed (the dechirp product before it and the reduction after
    it would come on top), and a device-to-device copy of the same 8
    B/sample. `rounds` timings of each (5 back-to-back calls after 2
    warm-up calls), the legs interleaved; median and range, the rate at the
    op's floor of 8 B/sample, and the ratio to the FFT + |X|^2 call."""
    d_mag = ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(d_mag), S * 4) == 0
    dst = torch.empty(S, dtype=torch.complex64, device="cuda")
    for sf in (7, 9, 12):
        n = 1 << sf
        k = S // n
        lo = lora_symbols(sf, S, 300.0 / n, seed=sf)
        hi = lora_symbols(sf, S, 3000.0 / n, seed=100 + sf)
        hard = fa.LoraFftDemod(sf, fa.LORA_HARD)
        soft = fa.LoraFftDemod(sf, fa.LORA_SOFT)
        fft = fa.Fft(n)
        s = st.cuda_stream
        legs = [
            ("HARD", lambda: hard.filter_dev(lo.data_ptr(), S, d_out.value,
                                             k, stream=s)),
            ("SOFT ln I0", lambda: soft.filter_dev(lo.data_ptr(), S,
                                                   d_out.value, k, stream=s)),
            ("SOFT clipped", lambda: soft.filter_dev(hi.data_ptr(), S,
                                                     d_out.value, k,
                                                     stream=s)),
            ("fft + |X|^2", lambda: fft.bulk_dev(lo.data_ptr(), d_out.value,
                                                 k, d_mag=d_mag.value,
                                                 stream=s)),
            ("d2d copy", lambda: dst.copy_(lo)),
        ]
        ms = [[] for _ in legs]
        for _ in range(rounds):
            for i, leg in enumerate(legs):
                ms[i].append(timeit(leg[1], reps=5, warm=2))
        fft_med = sorted(ms[3])[rounds // 2]
        for i, (name, _) in enumerate(legs):
            v = sorted(ms[i])
            med = v[len(v) // 2]
            tbs = S * 8 / (med * 1e-3) / 1e12
            print(f"sf {sf:2d} {name:13s}: {med:7.3f} ms median of {rounds} "
                  f"[{v[0]:.3f}..{v[-1]:.3f}]  {tbs:5.2f} TB/s at 8 B/sample "
                  f"({tbs / PEAK_HBM:.3f} of HBM peak), "
                  f"{med / fft_med:.2f}x fft + |X|^2")
        del lo, hi
    lib.fsdr_dev_free(d_mag)


def wlan_decode_lines(lib, st, rounds=5):
    """WLAN frame decoder over device-resident batches of equal frames:
    Bpsk_1_2 and Qam64_3_4, psdu 100 and 1500, batches of 1, 256, 4096 and
    16384 frames, plus a sweep over powers of two at Bpsk_1_2 / psdu 100 to
    find where the time per call stops being flat. The index bytes are
    uniformly random (the kernel's work does not depend on the data). One
    timing is one fsdr_wlan_decode_dev call between two events (descriptor
    upload included); 2 warm-up calls, then `rounds` timings; median and
    range, frames/s, decoded Mbit/s (n_data_bits per frame) and trellis
    steps/s (8 per output byte, n_traceback bytes of run-in, 2 less at the
    start)."""
    traceback = {0: 5, 7: 10}
    dec = fa.WlanDecoder()
    g = torch.Generator(device="cuda").manual_seed(11)

    def run(mcs, psdu, batch):
        n_sym, n_bits, _ = fa.wlan_frame_param(mcs, psdu)
        n_bytes = (n_bits + 7) // 8
        steps = 8 * (traceback[mcs] + n_bytes) - 2
        syms = torch.randint(0, 256, (batch * 48 * n_sym,), generator=g,
                             device="cuda", dtype=torch.uint8)
        out = torch.empty(batch * (psdu + 2), dtype=torch.uint8,
                          device="cuda")
        crc = torch.empty(batch, dtype=torch.uint8, device="cuda")
        descs = dec._descs([(mcs, psdu, i * 48 * n_sym, i * (psdu + 2), 0)
                            for i in range(batch)])

        def call():
            rc = lib.fsdr_wlan_decode_dev(dec._h, syms.data_ptr(), descs,
                                          batch, out.data_ptr(), None,
                                          crc.data_ptr(), st.cuda_stream)
            assert rc == 0, lib.fsdr_last_error()

        v = sorted(timeit(call, reps=1, warm=2) for _ in range(rounds))
        med = v[len(v) // 2]
        name = {0: "Bpsk_1_2", 7: "Qam64_3_4"}[mcs]
        print(f"{name:9s} psdu {psdu:4d} x {batch:5d}: {med:8.3f} ms median "
              f"of {rounds} [{v[0]:.3f}..{v[-1]:.3f}]  "
              f"{batch / med * 1e3:11.0f} frames/s  "
              f"{batch * n_bits / med / 1e3:9.1f} Mbit/s decoded  "
              f"{batch * steps / med / 1e6:8.2f} G trellis steps/s")
        return med

    for mcs in (0, 7):
        for psdu in (100, 1500):
            for batch in (1, 256, 4096, 16384):
                run(mcs, psdu, batch)
    print("sweep, Bpsk_1_2 psdu 100:")
    for k in range(0, 15):
        run(0, 100, 1 << k)


def wlan_eq_frame(mcs, psdu, n_data, rng):
    """Spectra (FFT-bin order, cf32) of one frame with n_data data symbols
    behind a flat unit channel: the long-training sequence twice, the SIGNAL
    symbol for (mcs, psdu), then pilots of the right polarity and uniformly
    random values on the data carriers (the kernel's work does not depend
    on them)."""
    cm = fa.wlan_carrier_map()
    data = cm >= 0
    long_seq = np.zeros(64)
    long_seq[6:59] = [{"+": 1.0, "-": -1.0, "0": 0.0}[c] for c in
                      "++--++-+-++++++--++-+-++++0+--++-+-+-----++--+-+-++++"]
    rate = {0: 11, 1: 15, 2: 10, 3: 14, 4: 9, 5: 13, 6: 8, 7: 12}[mcs]
    bits = np.zeros(24, np.int64)
    bits[:4] = (rate >> np.arange(4)) & 1
    bits[5:17] = (psdu >> np.arange(12)) & 1
    bits[17] = bits[:17].sum() & 1
    coded, state = np.zeros(48, np.int64), 0
    for i, b in enumerate(bits):
        state = ((state << 1) & 0x7E) | int(b)
        coded[2 * i] = bin(state & 0o155).count("1") & 1
        coded[2 * i + 1] = bin(state & 0o117).count("1") & 1
    sig = np.zeros(48, np.int64)
    i = np.arange(48)
    sig[3 * (i % 16) + i // 16] = coded
    pol = fa.wlan_pilot_polarity(n_data + 1).astype(np.float64)
    rows = np.zeros((3 + n_data, 64), np.complex128)
    rows[0] = rows[1] = long_seq
    rows[2:, [11, 25, 39]] = pol[:, None]
    rows[2:, 53] = -pol
    rows[2, data] = 2.0 * sig[cm[data]] - 1.0
    rows[3:, data] = rng.uniform(-1, 1, (n_data, 48)) \
        + 1j * rng.uniform(-1, 1, (n_data, 48))
    return np.roll(rows, 32, axis=1).astype(np.complex64).reshape(-1)


def wlan_eq_lines(lib, st, rounds=5):
    """WLAN frame equalizer over device-resident batches of equal frames:
    Bpsk_1_2 and Qam64_3_4 at 4 data symbols and at the longest frame below
    250 data symbols that the SIGNAL field can announce (250 at Bpsk_1_2;
    152 at Qam64_3_4, psdu 4095), 16384 frames and a single frame. One timing
    is one fsdr_wlan_equalize_dev call between two events (both descriptor
    uploads, k_wlan_eq_head, the SIGNAL decode and k_wlan_eq_data; d_eq
    NULL); 2 warm-up calls, then `rounds` timings; median and range, and the
    share of the HBM floor of 560 B per data symbol (512 in, 48 out) at
    PEAK_HBM."""
    eq = fa.WlanEqualizer()
    rng = np.random.default_rng(12)

    def run(mcs, n_data, batch):
        psdu = max(p for p in range(4096)
                   if fa.wlan_frame_param(mcs, p)[0] == n_data)
        frame = wlan_eq_frame(mcs, psdu, n_data, rng)
        spec = torch.from_numpy(frame).cuda().repeat(batch)
        idx = torch.empty(batch * 48 * n_data, dtype=torch.uint8,
                          device="cuda")
        info = torch.zeros(batch * 24, dtype=torch.uint8, device="cuda")
        descs = eq._descs([(i * frame.size, 3 + n_data, i * 48 * n_data, 0)
                           for i in range(batch)])

        def call():
            rc = lib.fsdr_wlan_equalize_dev(eq._h, spec.data_ptr(), descs,
                                            batch, idx.data_ptr(), None,
                                            info.data_ptr(), st.cuda_stream)
            assert rc == 0, lib.fsdr_last_error()

        v = sorted(timeit(call, reps=1, warm=2) for _ in range(rounds))
        rec = info.cpu().numpy().view(fa.WLAN_EQ_INFO_DTYPE)
        assert (rec["found"] == 1).all() and (rec["mcs"] == mcs).all() and \
            (rec["psdu_size"] == psdu).all() and \
            (rec["n_copied"] == n_data).all(), rec[:2]
        med = v[len(v) // 2]
        floor = batch * n_data * 560 / (med * 1e-3) / 1e12
        name = {0: "Bpsk_1_2", 7: "Qam64_3_4"}[mcs]
        print(f"{name:9s} {n_data:3d} data symbols (psdu {psdu:4d}) x "
              f"{batch:5d}: {med:8.3f} ms median of {rounds} "
              f"[{v[0]:.3f}..{v[-1]:.3f}]  "
              f"{batch * n_data / med / 1e3:8.2f} M symbols/s  "
              f"{floor:6.3f} TB/s = {100 * floor / PEAK_HBM:5.1f} % of the "
              f"HBM floor")

    for mcs, long_n in ((0, 250), (7, 152)):
        for n_data in (4, long_n):
            for batch in (1, 16384):
                run(mcs, n_data, batch)


def main():
    lib = fa.lib()
    fa.set_device(0)
    st = torch.cuda.current_stream()
    if "--wlan-eq" in sys.argv[1:]:
        wlan_eq_lines(lib, st)
        return
    if "--wlan-decode" in sys.argv[1:]:
        wlan_decode_lines(lib, st)
        return
    S = 1 << 26
    d_in = ctypes.c_void_p()
    d_out = ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(d_in), S * 8) == 0
    assert lib.fsdr_dev_alloc(ctypes.byref(d_out), S * 8) == 0
    fa.fill_uniform_dev(d_in.value, S, seed=5, stream=st.cuda_stream)

    if {"--synth", "--arb", "--iir", "--lora"} & set(sys.argv[1:]):
        if "--lora" in sys.argv[1:]:
            lora_lines(lib, st, d_out, S)
        if "--iir" in sys.argv[1:]:
            iir_lines(lib, st, d_in, d_out, S)
        if "--synth" in sys.argv[1:]:
            pfb_synth_lines(lib, st, d_in, d_out, S)
        if "--arb" in sys.argv[1:]:
            pfb_arb_lines(lib, st, d_in, S)
        lib.fsdr_dev_free(d_in)
        lib.fsdr_dev_free(d_out)
        return

    # XlatingFir: 127 taps, decim 4 (the FM front-end shape)
    taps = fa.lowpass_kaiser_n(127, fa.kaiser_beta(1e-4), 0.1)
    xl = fa.XlatingFir(taps, 4, 0.25, 1.0)
    ms = timeit(lambda: xl.filter_dev(d_in.value, S, d_out.value, S,
                                      stream=st.cuda_stream))
    prod = (S + 1 - 127) // 4
    # complex taps x complex samples: 8 flops/tap + rotator ~10
    tf = prod * (127 * 8 + 10) / (ms * 1e-3) / 1e12
    print(f"xlating_fir(127,D4) tiled: {ms:7.3f} ms  {tf:6.1f} TF/s "
          f"({tf / PEAK_TF:.3f} of fp32 peak)")

    # FirCC bulk (complex taps, D=1) — WLAN correlator math at scale
    ltf = np.exp(2j * np.pi * np.arange(64) / 7).astype(np.complex64)
    fcc = fa.FirCC(np.conj(ltf[::-1]))
    ms = timeit(lambda: fcc.filter_dev(d_in.value, S, d_out.value, S,
                                       stream=st.cuda_stream))
    prod = S + 1 - 64
    tf = prod * 64 * 8 / (ms * 1e-3) / 1e12
    print(f"fir_ccf32(64) bulk:        {ms:7.3f} ms  {tf:6.1f} TF/s "
          f"({tf / PEAK_TF:.3f} of fp32 peak)")

    # standalone FFT kernel (bulk 1024-pt)
    fft = fa.Fft(1024)
    frames = S // 1024
    ms = timeit(lambda: fft.bulk_dev(d_in.value, d_out.value, frames,
                                     stream=st.cuda_stream))
    gb = frames * 1024 * 16 / 1e9  # in+out
    tbs = gb / (ms * 1e-3) / 1e3
    flops = frames * 5 * 1024 * 10
    tf = flops / (ms * 1e-3) / 1e12
    print(f"fft_stockham(1024) bulk:   {ms:7.3f} ms  {tbs:6.2f} TB/s HBM "
          f"({tbs / PEAK_HBM:.3f} of peak), {tf:5.1f} TF/s")

    pfb_synth_lines(lib, st, d_in, d_out, S)
    pfb_arb_lines(lib, st, d_in, S)

    lib.fsdr_dev_free(d_in)
    lib.fsdr_dev_free(d_out)


if __name__ == "__main__":
    main()
