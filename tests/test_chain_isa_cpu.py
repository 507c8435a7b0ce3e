"""gfx950 ISA of the ws and ap chain kernels' tile loop, at every K.

The staging loads of a tile are meant to be one overlapped HBM round trip
under the previous tile's MFMAs. Whether they are is decided by where the
compiler puts its vmcnt waits, which no numerical test sees, so this
reads the device assembly (one device-only -S compile for the module,
~10 s; skipped where hipcc is absent):

- the tile loop holds a run of ten global_load_dwordx4 with no wait on
  vmcnt between the first and the tenth (ws and ap);
- ws: no global_load between the loop's first and last v_mfma (in-order
  VMEM return would let it drain the staging loads inside an MFMA window);
- ws: no vmcnt wait between the loop's last global_store ahead of the
  staging loads and the first of them (it would drain the output stores);
- ws: no scratch, and VGPR+AGPR <= 168, i.e. still 3 blocks per CU.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "futuresdr_amd", "csrc", "futuresdr_hip.hip")
KS = (20, 32, 48, 80, 144)
KERNEL = re.compile(r"^(_Z\d+k_decim4_fft_mfma_(ws|ap)_tplILi(\d+)EEv\w*):")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{(kind, K): (instructions of the tile loop, kernel descriptor)}"""
    hipcc = shutil.which("hipcc") or shutil.which(
        "hipcc", path="/opt/rocm/bin")
    if not hipcc:
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / "chain.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "--cuda-device-only", "-S", SRC, "-o", out], check=True,
                   stderr=subprocess.DEVNULL)
    with open(out) as f:
        lines = f.read().split("\n")
    found = {}
    i = 0
    while i < len(lines):
        m = KERNEL.match(lines[i])
        if m:
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            found[(m.group(2), int(m.group(3)))] = (
                tile_loop(lines[i:j]), descriptor(lines, m.group(1)))
            i = j
        i += 1
    return found


def tile_loop(body):
    """Instructions of the widest backward-branch span that holds MFMAs."""
    at = {m.group(1): n for n, l in enumerate(body)
          for m in [LABEL.match(l)] if m}
    best = None
    for n, l in enumerate(body):
        m = BRANCH.match(l)
        t = at.get(m.group(1)) if m else None
        if t is not None and t < n and any("v_mfma" in x
                                           for x in body[t:n]):
            if best is None or n - t > best[1] - best[0]:
                best = (t, n)
    assert best, "no loop with MFMAs"
    return [l.strip() for l in body[best[0]:best[1] + 1]
            if l.startswith("\t") and not l.strip().startswith((".", ";"))]


def descriptor(lines, name):
    k = lines.index("\t.amdhsa_kernel " + name)
    end = lines.index("\t.end_amdhsa_kernel", k)
    return {m.group(1): int(m.group(2)) for l in lines[k:end]
            for m in [re.match(r"\s+\.amdhsa_(\w+) (\d+)$", l)] if m}


def is_vm_wait(ins):
    return ins.startswith("s_waitcnt") and "vmcnt" in ins


@pytest.mark.parametrize("kk", KS)
@pytest.mark.parametrize("kind", ["ws", "ap"])
def test_ten_staging_loads_back_to_back(asm, kind, kk):
    loop, _ = asm[(kind, kk)]
    best = run = 0
    for ins in loop:
        if ins.startswith("global_load_dwordx4"):
            run += 1
            best = max(best, run)
        elif is_vm_wait(ins):
            run = 0
    assert best >= 10, f"longest wait-free run of 16 B loads: {best}"


@pytest.mark.parametrize("kk", KS)
def test_ws_no_global_load_among_mfmas(asm, kk):
    loop, _ = asm[("ws", kk)]
    mf = [n for n, ins in enumerate(loop) if ins.startswith("v_mfma")]
    assert len(mf) == 2 * kk  # 4 phases x K/4 steps x (re, im)
    inside = [ins for ins in loop[mf[0]:mf[-1]]
              if ins.startswith("global_load")]
    assert not inside, inside


@pytest.mark.parametrize("kk", KS)
def test_ws_stores_not_drained_ahead_of_staging_loads(asm, kk):
    """The previous tile's output stores are issued just ahead of the
    staging loads; a vmcnt wait between the two would drain them."""
    loop, _ = asm[("ws", kk)]
    first = run = None
    for n, ins in enumerate(loop):  # first load of the run of ten
        if ins.startswith("global_load_dwordx4"):
            first, run = (n, 1) if not run else (first, run + 1)
            if run == 10:
                break
        elif is_vm_wait(ins):
            run = None
    assert run == 10
    stores = [n for n, ins in enumerate(loop[:first])
              if ins.startswith("global_store")]
    assert stores, "no output store ahead of the staging loads"
    waits = [ins for ins in loop[stores[-1]:first] if is_vm_wait(ins)]
    assert not waits, waits


@pytest.mark.parametrize("kk", KS)
def test_ws_resources(asm, kk):
    _, desc = asm[("ws", kk)]
    assert desc["private_segment_fixed_size"] == 0
    # gfx950 has one register file: next_free_vgpr counts VGPR + AGPR
    assert desc["next_free_vgpr"] <= 168, desc["next_free_vgpr"]
