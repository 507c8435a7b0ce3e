#!/usr/bin/env python3
"""Compare two device-assembly builds of the module kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S \
        futuresdr_amd/csrc/futuresdr_hip.hip -o new.s
    python tools/isa_diff.py old.s new.s [name-filter-regex]

Per kernel symbol: `identical` (same instruction lines once comments and
directives are dropped), `same-multiset` (same length and the same count
of every mnemonic) or `differs` with the mnemonic count deltas, then the
kernel-descriptor fields that decide occupancy, old -> new. Exit status 1
if any kernel is not identical.
"""
import collections
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size",
          "private_segment_fixed_size")


def kernels(path):
    """{symbol: (instruction lines, descriptor fields)}"""
    lines = open(path).read().split("\n")
    desc = {}
    for n, l in enumerate(lines):
        if l.startswith("\t.amdhsa_kernel "):
            end = lines.index("\t.end_amdhsa_kernel", n)
            desc[l.split()[1]] = {
                m.group(1): int(m.group(2)) for x in lines[n:end]
                for m in [re.match(r"\s+\.amdhsa_(\w+) (\d+)$", x)] if m}
    out = {}
    for n, l in enumerate(lines):
        m = re.match(r"(\w+):", l)
        name = m.group(1) if m else None
        if name in desc and name not in out:
            end = n
            while not lines[end].startswith(".Lfunc_end"):
                end += 1
            # branch targets carry the function's index in the module,
            # which moves with the instantiation order: keep the block only
            body = [re.sub(r"\.LBB\d+_", ".LBB_",
                           re.sub(r"\s*;.*$", "", x)).strip()
                    for x in lines[n:end]]
            out[name] = ([x for x in body if x and not x.startswith(".")
                          and not x.endswith(":")], desc[name])
    return out


def mnemonics(ins):
    return collections.Counter(x.split()[0] for x in ins)


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    want = re.compile(sys.argv[3] if len(sys.argv) > 3 else "")
    worst = 0
    for name in sorted(set(old) | set(new)):
        if not want.search(name):
            continue
        if name not in old or name not in new:
            print(f"{name}: only in {'new' if name in new else 'old'}")
            worst = 1
            continue
        (a, da), (b, db) = old[name], new[name]
        if a == b:
            verdict = "identical"
        else:
            worst = 1
            ma, mb = mnemonics(a), mnemonics(b)
            if len(a) == len(b) and ma == mb:
                verdict = "same-multiset"
            else:
                delta = {k: mb[k] - ma[k] for k in sorted(set(ma) | set(mb))
                         if mb[k] != ma[k]}
                verdict = (f"differs ({len(a)} -> {len(b)} instructions) " +
                           " ".join(f"{k}{v:+d}" for k, v in delta.items()))
        fields = " ".join(f"{k.split('_segment')[0].replace('next_free_', '')}"
                          f"={da.get(k)}->{db.get(k)}" for k in FIELDS)
        print(f"{name}: {verdict} [{fields}]")
    return worst


if __name__ == "__main__":
    sys.exit(main())
