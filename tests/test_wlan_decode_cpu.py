"""The WLAN frame decoder without a GPU: tests/wlan_ref.py round-trips its
own encoder for every MCS, and the library's host-only helpers (frame
parameters, the index map the kernel stages with, the SIGNAL parse) equal
wlan_ref's. Handle creation and argument validation need no device."""
import ctypes
import functools

import numpy as np
import pytest

import wlan_ref

MCS = range(wlan_ref.N_MCS)


@functools.lru_cache(maxsize=None)
def _roundtrip(mcs, n_payload):
    rng = np.random.default_rng(100 * mcs + n_payload)
    psdu = wlan_ref.with_fcs(rng.integers(0, 256, n_payload, dtype=np.uint8)
                             .tobytes())
    # seed 1 is the reference encoder's first (encoder.rs:161)
    syms = wlan_ref.encode(mcs, psdu, seed=1)
    return psdu, syms, wlan_ref.decode(mcs, len(psdu), syms)


# ---- 1. the reference restatement --------------------------------------------

@pytest.mark.parametrize("mcs", MCS)
@pytest.mark.parametrize("n_payload", (1, 10, 37, 100))
def test_reference_round_trips(mcs, n_payload):
    psdu, syms, (out, dec, crc_ok, max_metric) = _roundtrip(mcs, n_payload)
    n_sym, n_data_bits, _ = wlan_ref.frame_param(mcs, len(psdu))
    assert syms.size == 48 * n_sym
    assert syms.max() < (1 << wlan_ref.MCS[mcs][0])
    assert out.size == len(psdu) + 2
    assert out[2:].tobytes() == psdu
    assert crc_ok
    assert out[0] & 0x7F and out[1] == 0 and not out[0] >> 7  # SERVICE
    assert dec.size == (n_data_bits + 7) // 8
    assert max_metric <= 255   # the reference's u8 metrics never wrap


def test_reference_reads_its_stated_tail():
    """The decoder reads 16*(T + n_bytes) - 4 depunctured values: 16*T - 4
    more than the frame has (76, 140 or 156), and 8 more again where
    n_data_bits is no multiple of 8 (n_dbps 36)."""
    seen = set()
    for mcs in MCS:
        n_cbps, pattern = wlan_ref.MCS[mcs][1], wlan_ref.MCS[mcs][3]
        for psdu in (0, 1, 5, 41, 104, 777, 1528):
            n_sym = wlan_ref.frame_param(mcs, psdu)[0]
            own = n_sym * n_cbps * len(pattern) // sum(pattern)
            seen.add(wlan_ref.depunctured_length(mcs, psdu) - own)
    assert seen == {76, 140, 156, 164}


# ---- 2. host-only helpers against the reference ------------------------------

@pytest.mark.parametrize("mcs", MCS)
def test_frame_param(fsdr, mcs):
    for psdu in (0, 1, 2, 13, 100, 1000, 1527, 1528, 4095):
        assert fsdr.wlan_frame_param(mcs, psdu) == \
            wlan_ref.frame_param(mcs, psdu), psdu
    assert fsdr.wlan_frame_param(0, 1528)[0] == 511
    assert fsdr.wlan_frame_param(7, 1528)[0] == 57
    assert fsdr.wlan_frame_param(1, 1)[1] == 36


def test_frame_param_rejects(fsdr):
    for mcs, psdu in ((8, 10), (255, 0), (0, 4096)):
        with pytest.raises(fsdr.FsdrError):
            fsdr.wlan_frame_param(mcs, psdu)
    assert "wlan" in fsdr.lib().fsdr_last_error().decode()


@pytest.mark.parametrize("mcs", MCS)
def test_deinterleave_map(fsdr, mcs):
    want = wlan_ref.deinterleave_map(mcs)
    assert sorted(want) == list(range(wlan_ref.MCS[mcs][1]))
    assert np.array_equal(fsdr.wlan_deinterleave_map(mcs), want)


def test_signal_interleaver_is_inverse_bpsk_map():
    """INTERLEAVER_PATTERN[i] = 3*(i%16) + i/16 undoes the BPSK map, so the
    SIGNAL decode is a decode of (mcs 0, psdu 0)."""
    i = np.arange(48)
    assert np.array_equal(wlan_ref.INTERLEAVER_PATTERN, 3 * (i % 16) + i // 16)
    m = wlan_ref.deinterleave_map(0)
    assert np.array_equal(m[wlan_ref.INTERLEAVER_PATTERN], i)


@pytest.mark.parametrize("mcs", MCS)
def test_depuncture_map(fsdr, mcs):
    """The kernel's closed-form source of every depunctured value equals
    labels pushed through the reference's bits -> deinterleave -> depuncture,
    up to the last index the decoder reads; beyond the frame it is -2."""
    for psdu in (0, 1, 41, 1528):
        n_sym = wlan_ref.frame_param(mcs, psdu)[0]
        count = wlan_ref.depunctured_length(mcs, psdu)
        want = wlan_ref.source_map(mcs, n_sym, count)
        got = fsdr.wlan_depuncture_map(mcs, n_sym, count)
        assert np.array_equal(got, want), psdu
        assert (got[-75:] == -2).all()
        # a window over the frame's end
        first = int(np.argmax(want == -2)) - 20
        assert first > 0 and (want[first:first + 20] != -2).all()
        assert np.array_equal(
            fsdr.wlan_depuncture_map(mcs, n_sym, 60, first=first),
            want[first:first + 60])
    if len(wlan_ref.MCS[mcs][3]) > 2:
        assert (want == -1).any()
    else:
        assert not (want == -1).any()


def test_signal_field(fsdr):
    for mcs in MCS:
        for psdu in (0, 1, 1528, 4095):
            b = wlan_ref.signal_bits(mcs, psdu)
            assert wlan_ref.signal_field(b) == (mcs, psdu)
            assert fsdr.wlan_signal_field(b) == (mcs, psdu)
            # values above 1 count as set bits, as `> 0` in the reference
            assert fsdr.wlan_signal_field(b * 7) == (mcs, psdu)
            bad = b.copy()
            bad[17] ^= 1                      # parity
            assert wlan_ref.signal_field(bad) is None
            assert fsdr.wlan_signal_field(bad) is None
            bad = b.copy()
            bad[9] ^= 1                       # a length bit: parity again
            assert fsdr.wlan_signal_field(bad) is None
    # every 4-bit rate, parity made right: 8 known, 8 unknown
    known = 0
    for r in range(16):
        b = np.zeros(24, np.uint8)
        b[:4] = [(r >> i) & 1 for i in range(4)]
        b[5] = 1
        b[4] = 1                              # the reserved bit is not parsed
        b[17] = b[:17].sum() & 1
        want = wlan_ref.signal_field(b)
        assert fsdr.wlan_signal_field(b) == want
        known += want is not None
    assert known == 8
    with pytest.raises(fsdr.FsdrError):
        fsdr.wlan_signal_field(np.zeros(23, np.uint8))


def test_signal_field_from_reference_decode():
    """The SIGNAL path end to end in the reference: encode 24 bits as one
    BPSK 1/2 symbol, decode as (mcs 0, psdu 0), parse."""
    for mcs, psdu in ((0, 100), (7, 1528), (5, 1)):
        bits = wlan_ref.signal_bits(mcs, psdu)
        enc = np.zeros(48, np.uint8)
        state = 0
        for i, b in enumerate(bits):          # encoder.rs:51-59, no scrambler
            state = ((state << 1) & 0x7E) | int(b)
            enc[2 * i] = bin(state & 0o155).count("1") & 1
            enc[2 * i + 1] = bin(state & 0o117).count("1") & 1
        syms = enc[wlan_ref.deinterleave_map(0)]
        dec = wlan_ref.decode(0, 0, syms)[1]
        assert dec.size == 3
        assert wlan_ref.signal_field(np.unpackbits(dec)) == (mcs, psdu)


# ---- 3. handle and argument validation ---------------------------------------

def _frames(fsdr, *fr):
    arr = fsdr.WlanDecoder._descs(list(fr))
    return arr, len(fr)


def test_create_and_validation_need_no_device(fsdr):
    lib = fsdr.lib()
    d = fsdr.WlanDecoder()
    dummy = ctypes.c_void_p(64)   # never dereferenced: validation comes first
    for bad, word in (((8, 10, 0, 0, 0), "mcs"),
                      ((0, 1529, 0, 0, 0), "psdu"),
                      ((0xFFFFFFFF, 0, 0, 0, 0), "mcs")):
        arr, n = _frames(fsdr, (0, 10, 0, 0, 0), bad)
        for rc in (lib.fsdr_wlan_decode_dev(d._h, dummy, arr, n, dummy, None,
                                            dummy, None),
                   lib.fsdr_wlan_decode_host(d._h, dummy, arr, n, dummy, None,
                                             dummy)):
            assert rc == fsdr.ERR_INVALID
            assert word in lib.fsdr_last_error().decode()
    # n_frames == 0 is a successful no-op, with or without pointers
    assert lib.fsdr_wlan_decode_dev(d._h, None, None, 0, None, None, None,
                                    None) == fsdr.OK
    assert lib.fsdr_wlan_decode_host(d._h, None, None, 0, None, None,
                                     None) == fsdr.OK
    assert d.decode([]) == []
    # NULL handle, NULL frame array, NULL buffers
    arr, n = _frames(fsdr, (0, 10, 0, 0, 0))
    assert lib.fsdr_wlan_decode_dev(None, dummy, arr, n, dummy, None, dummy,
                                    None) == fsdr.ERR_INVALID
    assert lib.fsdr_wlan_decode_dev(d._h, dummy, None, n, dummy, None, dummy,
                                    None) == fsdr.ERR_INVALID
    assert lib.fsdr_wlan_decode_dev(d._h, None, arr, n, dummy, None, dummy,
                                    None) == fsdr.ERR_INVALID
    assert lib.fsdr_wlan_decode_dev(d._h, dummy, arr, n, dummy, None, None,
                                    None) == fsdr.ERR_INVALID
    lib.fsdr_wlan_decoder_destroy(None)        # destroying NULL is allowed


def test_largest_frames_pass_validation(fsdr):
    """psdu 1528 is legal at every MCS (511 symbols at Bpsk_1_2), so the
    symbol limit never rejects what the size limit admits; without a device
    a valid batch fails loudly instead of falling back."""
    for mcs in MCS:
        assert fsdr.wlan_frame_param(mcs, 1528)[0] <= wlan_ref.MAX_SYM
    if fsdr.device_count() > 0:
        return
    d = fsdr.WlanDecoder()
    with pytest.raises(fsdr.FsdrError, match="no HIP device"):
        d.decode([(0, 0, np.zeros(48, np.uint8))])


def test_python_decode_checks_shapes(fsdr):
    d = fsdr.WlanDecoder()
    with pytest.raises(fsdr.FsdrError, match="indices"):
        d.decode([(0, 0, np.zeros(47, np.uint8))])
    with pytest.raises(fsdr.FsdrError, match="mcs"):
        d.decode([(8, 0, np.zeros(48, np.uint8))])
    with pytest.raises(fsdr.FsdrError, match="psdu"):
        d.decode([(0, 1529, np.zeros(48, np.uint8))])
