"""The WLAN frame equalizer without a device: the host-only helpers (which
are the kernel's own demap, carrier map and polarity functions) against
tests/wlan_eq_ref.py, the ABI, wlan_frame_spans, and the numbers the GPU
test's conditions rest on, taken from the reference alone: the f32
restatement's error against f64 (E_ref), the share of data symbols within
DELTA of a decision threshold, and that the f64 reference followed by
wlan_ref.decode recovers every test frame."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import wlan_eq_ref as R
import wlan_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCS = range(wlan_ref.N_MCS)


# ---- 1. demap ------------------------------------------------------------------

@pytest.mark.parametrize("mcs", MCS)
def test_demap_inverts_the_mapper(fsdr, mcs):
    n_bpsc = wlan_ref.MCS[mcs][0]
    pts = R.constellation(n_bpsc)
    assert len(set(pts.tolist())) == 1 << n_bpsc
    assert np.array_equal(R.demap(n_bpsc, pts), np.arange(1 << n_bpsc))
    assert np.array_equal(fsdr.wlan_demap(mcs, pts), np.arange(1 << n_bpsc))


@pytest.mark.parametrize("mcs", MCS)
def test_demap_at_the_thresholds(fsdr, mcs):
    """At, just below and just above every threshold on one axis, crossed
    with the same values and a few ordinary ones on the other."""
    n_bpsc = wlan_ref.MCS[mcs][0]
    t = R.thresholds(n_bpsc)
    edge = np.concatenate([t, np.nextafter(t, np.float32(-9)),
                           np.nextafter(t, np.float32(9)),
                           np.float32([-0.0, 0.05, -0.3, 0.7, -1.2, 8.9])])
    z = (edge[:, None] + 1j * edge[None, :]).astype(np.complex64).reshape(-1)
    got = fsdr.wlan_demap(mcs, z)
    assert np.array_equal(got, R.demap(n_bpsc, z))
    assert got.max() < 1 << n_bpsc
    # the strict comparisons: a value on a threshold is on its far side
    assert fsdr.wlan_demap(mcs, np.complex64([0]))[0] == \
        {1: 0, 2: 0, 4: 10, 6: 18}[n_bpsc]


@pytest.mark.parametrize("mcs", MCS)
def test_demap_nan_gives_zero(fsdr, mcs):
    nan = np.float32(np.nan)
    z = np.array([complex(nan, nan)] * 3, np.complex64)
    assert fsdr.wlan_demap(mcs, z).tolist() == [0, 0, 0]
    assert R.demap(wlan_ref.MCS[mcs][0], z).tolist() == [0, 0, 0]


def test_demap_rejects(fsdr):
    with pytest.raises(fsdr.FsdrError):
        fsdr.wlan_demap(8, np.zeros(1, np.complex64))
    assert fsdr.wlan_demap(3, np.zeros(0, np.complex64)).size == 0


# ---- 2. polarity, carrier map --------------------------------------------------

def test_pilot_polarity(fsdr):
    want = R.POLARITY[np.arange(300) % 127]
    assert np.array_equal(fsdr.wlan_pilot_polarity(300), want)
    assert np.array_equal(fsdr.wlan_pilot_polarity(140, first=120),
                          R.POLARITY[np.arange(120, 260) % 127])
    # 802.11 p_0.. = 1, 1, 1, 1, -1, -1, -1, 1, and a balanced m-sequence
    assert want[:8].tolist() == [1, 1, 1, 1, -1, -1, -1, 1]
    assert int((R.POLARITY == -1).sum()) == 64


def test_carrier_map(fsdr):
    cm = fsdr.wlan_carrier_map()
    assert np.array_equal(np.flatnonzero(cm >= 0), R.DATA_CARRIERS)
    assert np.array_equal(cm[R.DATA_CARRIERS], np.arange(48))
    assert R.DATA_CARRIERS.size == 48
    for m in (0, 5, 11, 25, 32, 39, 53, 59, 63):
        assert cm[m] == -1


# ---- 3. ABI --------------------------------------------------------------------

ABI_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "futuresdr_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(fsdr_wlan_eq_frame),
           offsetof(fsdr_wlan_eq_frame, sym_off),
           offsetof(fsdr_wlan_eq_frame, n_avail),
           offsetof(fsdr_wlan_eq_frame, idx_off),
           offsetof(fsdr_wlan_eq_frame, eq_off));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(fsdr_wlan_eq_info),
           offsetof(fsdr_wlan_eq_info, found), offsetof(fsdr_wlan_eq_info, mcs),
           offsetof(fsdr_wlan_eq_info, psdu_size),
           offsetof(fsdr_wlan_eq_info, n_symbols),
           offsetof(fsdr_wlan_eq_info, n_copied),
           offsetof(fsdr_wlan_eq_info, snr_db));
    return 0;
}
"""


def test_struct_layout(fsdr, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler for the layout program")
    src = tmp_path / "abi.c"
    src.write_text(ABI_PROGRAM)
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True,
                           text=True).stdout.split("\n")
    F, I = fsdr._WlanEqFrame, fsdr._WlanEqInfo
    assert [int(x) for x in lines[0].split()] == [
        ctypes.sizeof(F), F.sym_off.offset, F.n_avail.offset,
        F.idx_off.offset, F.eq_off.offset]
    assert [int(x) for x in lines[1].split()] == [
        ctypes.sizeof(I), I.found.offset, I.mcs.offset, I.psdu_size.offset,
        I.n_symbols.offset, I.n_copied.offset, I.snr_db.offset]
    assert ctypes.sizeof(I) == 24 == fsdr.WLAN_EQ_INFO_DTYPE.itemsize
    assert [fsdr.WLAN_EQ_INFO_DTYPE.fields[n][1] for n, _ in I._fields_] == \
        [getattr(I, n).offset for n, _ in I._fields_]


def test_create_and_validation_need_no_device(fsdr):
    lib = fsdr.lib()
    e = fsdr.WlanEqualizer()
    dummy = ctypes.c_void_p(64)   # never dereferenced: validation comes first
    arr = e._descs([(0, 5, 0, 0)])
    dev, host = lib.fsdr_wlan_equalize_dev, lib.fsdr_wlan_equalize_host
    # n_frames == 0 is a successful no-op, with or without pointers
    assert dev(e._h, None, None, 0, None, None, None, None) == fsdr.OK
    assert host(e._h, None, None, 0, None, None, None) == fsdr.OK
    assert dev(e._h, dummy, arr, 0, dummy, dummy, dummy, None) == fsdr.OK
    for args in ((None, dummy, arr, 1, dummy, None, dummy),
                 (e._h, dummy, None, 1, dummy, None, dummy),
                 (e._h, None, arr, 1, dummy, None, dummy),
                 (e._h, dummy, arr, 1, None, None, dummy),
                 (e._h, dummy, arr, 1, dummy, dummy, None)):
        assert dev(*args, None) == fsdr.ERR_INVALID
        assert "null" in lib.fsdr_last_error().decode()
        assert host(*args) == fsdr.ERR_INVALID
        assert "null" in lib.fsdr_last_error().decode()
    lib.fsdr_wlan_equalizer_destroy(None)      # destroying NULL is allowed
    assert lib.fsdr_wlan_demap(0, None, 1, dummy) == fsdr.ERR_INVALID
    assert lib.fsdr_wlan_pilot_polarity(0, 1, None) == fsdr.ERR_INVALID
    assert lib.fsdr_wlan_carrier_map(None) == fsdr.ERR_INVALID
    del e


def test_python_equalize_checks_shapes(fsdr):
    e = fsdr.WlanEqualizer()
    assert e.equalize(np.zeros(64, np.complex64), []) == []
    with pytest.raises(fsdr.FsdrError, match="outside"):
        e.equalize(np.zeros(3 * 64, np.complex64), [(0, 4)])
    with pytest.raises(fsdr.FsdrError, match="outside"):
        fsdr.wlan_receive(np.zeros(3 * 64, np.complex64), [(64, 3)])
    assert fsdr.wlan_receive(np.zeros(64, np.complex64), []) == []


# ---- 4. wlan_frame_spans -------------------------------------------------------

def test_frame_spans(fsdr):
    """3 tags, the second too close to the third (447 samples): it yields no
    frame and no items; the last frame runs to the end of the samples."""
    tags = [(10, 0.0), (2000, 0.0), (2447, 0.0)]
    frames = [(170, 0.0), (133, 0.0)]
    n = 2447 + 133 + 128 + 80 * 7 + 79
    want = R.frame_spans_walk(tags, frames, n)
    assert want == [(0, 2 + (2000 - 10 - 170 - 128) // 80),
                    (128 + 64 * 21, 2 + 7)]
    assert fsdr.wlan_frame_spans(tags, frames, n) == want
    # one sample more and the last frame has another symbol
    assert fsdr.wlan_frame_spans(tags, frames, n + 1)[1] == (want[1][0], 10)
    # exactly 448 samples are enough
    tags[1] = (1999, 0.0)
    got = fsdr.wlan_frame_spans(tags, frames + [(150, 0.0)], n)
    assert got == R.frame_spans_walk(tags, frames + [(150, 0.0)], n)
    assert len(got) == 3
    assert fsdr.wlan_frame_spans([], [], 1000) == []


# ---- 5. what the GPU test's conditions rest on -----------------------------------

def test_parity_cases_reference_only():
    """Per MCS: SIGNAL parses in f64 and f32, both give the same indices,
    E_ref is of f32 size so that K * E_ref * max(1, |z|) stays below DELTA,
    at most 1 % of the symbols lie within DELTA of a threshold (0.42 % in the
    Qam64_2_3 frame, none elsewhere, for the committed seed), snr_db agrees
    to SNR_TOL_DB, and the f64 indices decode to the transmitted PSDU."""
    shares = []
    for c in R.parity_cases():
        r64, r32 = c["r64"], c["r32"]
        n_sym = wlan_ref.frame_param(c["mcs"], c["psdu"])[0]
        assert 4 <= n_sym <= 11
        for r in (r64, r32):
            assert (r["found"], r["mcs"], r["psdu_size"], r["n_symbols"],
                    r["n_copied"]) == (True, c["mcs"], c["psdu"], n_sym, n_sym)
        print(c["mcs"], "E_ref %.3g" % c["e_ref"], "near %.4f"
              % c["near"].mean(), "snr %.4f %.4f"
              % (r64["snr_db"], r32["snr_db"]), "max|z| %.2f"
              % np.abs(r64["z"]).max())
        assert 0 < c["e_ref"] < 64 * 2.0 ** -24
        bound = R.K_DEVICE * c["e_ref"] * np.maximum(1, np.abs(r64["z"]))
        assert bound.max() < R.DELTA
        assert c["near"].mean() <= 0.01
        shares.append(round(100 * c["near"].mean(), 2))
        assert np.array_equal(r32["idx"], r64["idx"])
        assert abs(r32["snr_db"] - r64["snr_db"]) < R.SNR_TOL_DB
        out, _, crc_ok, _ = wlan_ref.decode(c["mcs"], c["psdu"], r64["idx"])
        assert crc_ok and out[2:].tobytes() == c["data"]
    assert shares == [0, 0, 0, 0, 0, 0, 0.42, 0]
    # the channel does something: some frames arrive with wrong indices
    assert any((c["r64"]["idx"] != c["tx_idx"]).any()
               for c in R.parity_cases())


def test_polarity_wrap_case_reference_only():
    c = R.case(0, 400, 12)
    assert c["r64"]["n_symbols"] == 135 and c["r64"]["found"]
    assert np.array_equal(c["r32"]["idx"], c["r64"]["idx"])
    assert c["near"].mean() <= 0.01
    assert c["r64"]["idx"].size == 48 * 135 > 48 * 127


def test_equalizer_restatement_on_a_clean_frame():
    """No noise, flat channel: z is the mapped constellation point."""
    data = R.psdu_bytes(6, 50, 5)
    carriers, tx_idx = R.frame_carriers(6, data)
    spec = R.to_bins(carriers * (0.3 - 0.4j)).astype(np.complex64)
    for dtype in (np.float64, np.float32):
        r = R.equalize(spec, dtype)
        assert r["found"] and (r["mcs"], r["psdu_size"]) == (6, 50)
        assert np.array_equal(r["idx"], tx_idx)
        assert np.abs(r["z"] - R.constellation(6)[tx_idx]).max() < 1e-5
    assert R.equalize(spec[:2])["snr_db"] > 100 and \
        not R.equalize(spec[:2])["found"]
    assert R.equalize(spec[:1])["snr_db"] == 0.0


def test_samples_reference_only():
    """The synthesized sample stream locks in the numpy front end of
    tests/test_wlan_rx_gpu.py and decodes through the f64 equalizer."""
    import test_wlan_rx_gpu as T
    import futuresdr_amd as fa
    iq, data = R.sample_stream()
    long_taps = np.load(T.FIXTURE)["long_taps"]
    delayed, abs48, cor = T.metric_chain_numpy(iq)
    fs, tags = T.sync_short_oracle(delayed, abs48, cor)
    sy, frames = T.sync_long_oracle(fs, tags, long_taps)
    assert len(tags) == 2 and len(frames) == 2
    spans = fa.wlan_frame_spans(tags, frames, fs.size)
    assert spans == R.frame_spans_walk(tags, frames, fs.size)
    assert sum(64 * n for _, n in spans) == sy.size
    spec = np.fft.fft(sy.astype(np.complex128).reshape(-1, 64), axis=1) \
        .astype(np.complex64).reshape(-1)
    for (so, na), d, (mcs, psdu) in zip(spans, data, R.SAMPLE_FRAMES):
        r = R.equalize(spec[so:so + 64 * na])
        assert (r["found"], r["mcs"], r["psdu_size"]) == (True, mcs, psdu)
        assert r["n_copied"] == r["n_symbols"]
        out, _, crc_ok, _ = wlan_ref.decode(mcs, psdu, r["idx"])
        assert crc_ok and out[2:].tobytes() == d
