#!/usr/bin/env python3
"""FM back end: the demodulator's measured error and the fused kernel's
timing, written to profiles/fm_backend.txt (or --out).

1. max |d_gpu - d_f64| of the staged QuadDemod kernel over the inputs of
   tests/fm_ref.py (fm_input(s, ED_N), s in ED_SEEDS) against fm_ref.demod.
   fm_ref.E_D is 4x this figure rounded up to a power of two.
2. FmDemodResampler(1, 5, 22 taps) over 2^26 device-resident Complex32
   samples: the fused kernel, the FSDR_FM_FUSED=0 path (demod into scratch,
   then the f32 resampler kernel), and for each a device-to-device copy
   whose read + write traffic equals the bytes that path moves per call
   (fused 8 + 4/M per input sample, staged 8 + 4 + 4 + 4/M). HIP events
   around CALLS back-to-back calls after WARM warm-up calls = one timing;
   REPS timings per leg, the legs interleaved; median [min..max].
"""
import argparse
import ctypes
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import fm_ref as F  # noqa: E402
import futuresdr_amd as fa  # noqa: E402

N = 1 << 26
L, M, T = 1, 5, 22
WARM, CALLS, REPS = 2, 5, 5


def demod_error():
    worst = 0.0
    lines = []
    for s in F.ED_SEEDS:
        x, ref = F.demod_case(s, F.ED_N)
        got = fa.QuadDemod().filter(x, x.size)[0]
        err = float(np.abs(got.astype(np.float64) - ref).max())
        lines.append(f"  seed {s}: n = {x.size}, max |d_gpu - d_f64| = "
                     f"{err:.3e}")
        worst = max(worst, err)
    e_d = 2.0 ** math.ceil(math.log2(4 * worst))
    lines.append(f"  max over seeds {worst:.3e}; 4x rounded up to a power "
                 f"of two: E_D = 2^{int(math.log2(e_d))} = {e_d:.3e} "
                 f"({'<=' if e_d <= 1e-5 else 'ABOVE'} 1e-5)")
    return lines


def timed(st, fn):
    for _ in range(WARM):
        fn()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(CALLS):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


def timing():
    lib = fa.lib()
    st = torch.cuda.current_stream()
    taps = fa.kaiser_lowpass(2e3 / 240e3, 10e3 / 240e3, 0.1)
    assert taps.size == T
    n_out = N // M
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.fsdr_dev_alloc(ctypes.byref(d_in), N * 8) == 0
    assert lib.fsdr_dev_alloc(ctypes.byref(d_out), n_out * 4) == 0
    fa.fill_uniform_dev(d_in.value, N, seed=3, stream=st.cuda_stream)
    moved = {"fused": N * 8 + n_out * 4, "staged": N * 16 + n_out * 4}
    handles, fused_flag = {}, {}
    for name, env in (("fused", None), ("staged", "0")):
        os.environ.pop("FSDR_FM_FUSED", None)
        if env is not None:
            os.environ["FSDR_FM_FUSED"] = env
        handles[name] = fa.FmDemodResampler(L, M, taps)
        fused_flag[name] = handles[name].fused
    assert fused_flag == {"fused": True, "staged": False}
    src = torch.empty(moved["staged"] // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    produced = {}

    def run(name):
        def fn():
            os.environ.pop("FSDR_FM_FUSED", None)
            if name == "staged":
                os.environ["FSDR_FM_FUSED"] = "0"
            _, produced[name], _ = handles[name].filter_dev(
                d_in.value, N, d_out.value, n_out, stream=st.cuda_stream)
        return fn

    def copy(name):
        k = moved[name] // 2
        return lambda: dst[:k].copy_(src[:k])

    legs = [("fused", run("fused")), ("copy of fused bytes", copy("fused")),
            ("staged", run("staged")),
            ("copy of staged bytes", copy("staged"))]
    ms = {name: [] for name, _ in legs}
    for _ in range(REPS):
        for name, fn in legs:
            ms[name].append(timed(st, fn))
    os.environ.pop("FSDR_FM_FUSED", None)
    lib.fsdr_dev_free(d_in)
    lib.fsdr_dev_free(d_out)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"  {N} input samples, ({L},{M},{T}); produced "
             f"{produced['fused']} (fused), {produced['staged']} (staged)",
             "  leg                    median ms  [min..max]        "
             "GSample/s  bytes moved  of copy rate"]
    for name, _ in legs:
        path = name.split()[-2] if name.startswith("copy") else name
        rate = N / (med[name] * 1e-3) / 1e9
        frac = (f"{med['copy of ' + path + ' bytes'] / med[name]:.3f}"
                if not name.startswith("copy") else "-")
        lines.append(f"  {name:22s} {med[name]:8.4f}   [{min(ms[name]):.4f}.."
                     f"{max(ms[name]):.4f}]  {rate:9.2f}  "
                     f"{moved[path] / 1e6:9.1f} MB  {frac}")
    lines.append(f"  fused / staged time: {med['fused'] / med['staged']:.3f}"
                 f" (bytes moved: {moved['fused'] / moved['staged']:.3f})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "fm_backend.txt"))
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if fa.device_count() < 1:
        raise SystemExit("needs a HIP device (MI355X)")
    fa.set_device(0)
    text = ["FM back end: QuadDemod error and fused-kernel timing, 1x MI355X",
            "", "QuadDemod (staged kernel) against the float64 reference:"]
    text += demod_error()
    if not args.skip_timing:
        text += ["", "Timing (tools/fm_backend_bench.py):"] + timing()
    out = "\n".join(text) + "\n"
    print(out, end="")
    with open(args.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
