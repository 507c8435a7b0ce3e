"""Generate tests/golden/pfb_arb_schedule.npz: the PfbArbResampler timing
schedule far into the stream, where a Python walk inside a test is too
slow. The generator is the literal walk of tests/pfb_arb_ref.py (np.float32
scalars, one op per reference op) from input 0, run once; it knows nothing
of the product's checkpoints or cycle detection.

For each (rate, num_filters) it stores, at about ten stream positions, the
cumulative output count and the per-output records of the next 64 inputs.
The positions sit on both sides of where the timing state's preperiod rho
ends and where its first period rho+lam ends, and beyond rho+2*lam; rho and
lam below are the figures of the cycle search recorded in DESIGN.md, used
here only to choose where to look.

Run: python tests/golden/generate_pfb_arb.py   (a few minutes)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from pfb_arb_ref import PfbArbResamplerRef, records_arrays  # noqa: E402

SPAN = 64
CASES = [  # rate, num_filters, rho, lam
    (0.7, 5, 0, 5991863),
    (0.3, 5, 8388611, 10),
    (3.14159265, 32, 0, 2409827),
]


def positions(rho, lam):
    p = {0, 63, rho + 1, rho + lam - 65, rho + lam - 1, rho + lam,
         rho + lam + 1, rho + lam + 1000, rho + 2 * lam - 1,
         rho + 2 * lam + 7}
    if rho > 65:
        p |= {rho - 65, rho - 1, rho}
    return sorted(x for x in p if x >= 0)


def main():
    out = {}
    for ci, (rate, nf, rho, lam) in enumerate(CASES):
        pos = positions(rho, lam)
        ref = PfbArbResamplerRef(rate, None, nf)
        sink = []
        cum = 0
        cum_at, keep = {}, []
        pos_set = set(pos)
        last = pos[-1] + SPAN
        wi = 0  # first window that has not ended yet
        while ref.inputs_seen < last:
            i = ref.inputs_seen
            if i in pos_set:
                cum_at[i] = cum
            ref.records = []
            cum += ref.consume_single(None, sink)
            sink.clear()
            while wi < len(pos) and i >= pos[wi] + SPAN:
                wi += 1
            if wi < len(pos) and i >= pos[wi]:
                keep.extend(ref.records)
        cums = [cum_at[p] for p in pos]
        recs = [[r for r in keep if p <= r[0] < p + SPAN] for p in pos]
        out[f"c{ci}_rate"] = np.float32(rate)
        out[f"c{ci}_nf"] = np.int64(nf)
        out[f"c{ci}_pos"] = np.array(pos, np.uint64)
        out[f"c{ci}_cum"] = np.array(cums, np.uint64)
        for k, r in enumerate(recs):
            idx, base, bnd, mu = records_arrays(r)
            out[f"c{ci}_p{k}_idx"] = idx
            out[f"c{ci}_p{k}_base"] = base
            out[f"c{ci}_p{k}_bnd"] = bnd
            out[f"c{ci}_p{k}_mu"] = mu
        print(f"rate {rate} nf {nf}: {len(pos)} positions, "
              f"walked {last} inputs", flush=True)
    out["n_cases"] = np.int64(len(CASES))
    out["span"] = np.int64(SPAN)
    np.savez_compressed(os.path.join(HERE, "pfb_arb_schedule.npz"), **out)


if __name__ == "__main__":
    main()
