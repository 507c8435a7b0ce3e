"""The WLAN frame decoder on the GPU against tests/wlan_ref.py. Everything is
integer arithmetic, so every comparison is exact equality of out_bytes, the
raw decoded bytes and crc_ok. Shapes: every MCS at psdu 0 (the SIGNAL shape
at mcs 0), 1 (n_data_bits 36 at Bpsk_3_4, no multiple of 8), 5, 41 and 104;
psdu 1528 at Bpsk_1_2 (511 symbols, 192 staging chunks of 64 values) and
Qam64_3_4; batches of 1, 3, 64 and 257 frames (257 leaves a block of four
waves partly empty). FSDR_FIR_GRID_CAP=1 makes one block walk every frame, 3
gives the blocks an uneven share. Reference results are cached."""
import ctypes
import functools

import numpy as np
import pytest

import wlan_ref

pytestmark = pytest.mark.gpu

MCS = range(wlan_ref.N_MCS)
KINDS = ("clean", "flip1", "flip5", "random", "zeros")
CANARY = 0xA5


@pytest.fixture(params=[None, "1", "3"], ids=["cap-", "cap1", "cap3"])
def grid_cap(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("FSDR_FIR_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("FSDR_FIR_GRID_CAP", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _frame(mcs, psdu, kind="clean"):
    """(syms, out, dec, crc_ok) of one frame, read-only."""
    seed = 1000 * mcs + psdu
    rng = np.random.default_rng(seed)
    n_sym = wlan_ref.frame_param(mcs, psdu)[0]
    if kind == "zeros":
        syms = np.zeros(48 * n_sym, np.uint8)
    elif kind == "random":
        # garbage above n_bpsc too: maximises metric ties (strict '>' and
        # first-maximum rules) and checks that the high bits are ignored
        syms = rng.integers(0, 256, 48 * n_sym, dtype=np.uint8)
    else:
        body = rng.integers(0, 256, max(psdu - 4, 0), dtype=np.uint8)
        data = wlan_ref.with_fcs(body.tobytes()) if psdu >= 4 \
            else bytes(rng.integers(0, 256, psdu, dtype=np.uint8))
        # clean frames use the reference encoder's first seed, with which
        # the round trip holds (wlan_ref docstring); the others vary it
        syms = wlan_ref.encode(mcs, data,
                               seed=1 if kind == "clean" else 1 + seed % 127)
        if kind != "clean":
            syms = wlan_ref.flip_coded_bits(
                mcs, syms, 0.01 if kind == "flip1" else 0.05, rng)
    out, dec, crc_ok, _ = wlan_ref.decode(mcs, psdu, syms)
    for a in (syms, out, dec):
        a.setflags(write=False)
    return syms, out, dec, crc_ok


def _check(got, want):
    """got: WlanDecoder.decode(raw=True); want: [_frame(...)]."""
    assert len(got) == len(want)
    for i, ((out, crc_ok, dec), (_, w_out, w_dec, w_crc)) in \
            enumerate(zip(got, want)):
        assert np.array_equal(dec, w_dec), (i, "raw decoded bytes")
        assert np.array_equal(out, w_out), (i, "out_bytes")
        assert crc_ok == w_crc, (i, "crc_ok")


def _decode(dec, keys):
    want = [_frame(*k) for k in keys]
    got = dec.decode([(k[0], k[1], w[0]) for k, w in zip(keys, want)],
                     raw=True)
    _check(got, want)
    return got


# ---- 1. single frames ----------------------------------------------------------

@pytest.mark.parametrize("mcs", MCS)
def test_single_frames(gpu, mcs):
    d = gpu.WlanDecoder()
    for psdu in (0, 1, 5, 41, 104):
        (out, crc_ok, dec), = _decode(d, [(mcs, psdu)])
        assert crc_ok == (psdu >= 4)
        assert out.size == psdu + 2
        assert dec.size == (wlan_ref.frame_param(mcs, psdu)[1] + 7) // 8
    assert wlan_ref.frame_param(1, 1)[1] == 36
    assert wlan_ref.frame_param(0, 0)[1] == 24


@pytest.mark.parametrize("mcs", (0, 7))
def test_longest_frame(gpu, mcs):
    """psdu 1528: where the reference itself would run off its array."""
    assert wlan_ref.frame_param(mcs, 1528)[0] == (511, 57)[mcs == 7]
    (out, crc_ok, dec), = _decode(gpu.WlanDecoder(), [(mcs, 1528)])
    assert out.size == 1530


# ---- 2. corruption ----------------------------------------------------------------

@pytest.mark.parametrize("mcs", MCS)
def test_corrupted_input(gpu, mcs):
    d = gpu.WlanDecoder()
    for kind in KINDS:
        (out, crc_ok, dec), = _decode(d, [(mcs, 61, kind)])
        if kind == "clean":
            assert crc_ok
        # 5 % flips break the punctured rates and are corrected at rate 1/2;
        # either way the result is the reference's
        if kind in ("random", "zeros"):
            assert not crc_ok


# ---- 3. batches -------------------------------------------------------------------

POOL = tuple((mcs, psdu, kind)
             for mcs in MCS
             for psdu, kind in ((0, "clean"), (1, "clean"), (5, "flip1"),
                                (23, "clean"), (41, "random"), (61, "flip5"),
                                (104, "clean")))


def _batch(n, order):
    rng = np.random.default_rng(n)
    keys = [POOL[i] for i in rng.integers(0, len(POOL), n)]
    if n >= 3:
        keys[n // 2] = (0, 104, "clean")    # 37 symbols: the longest
        keys[0] = (7, 0, "clean")           # 1 symbol
    work = lambda k: wlan_ref.n_decoded_bytes(k[0], k[1])
    if order == "ascending":
        keys.sort(key=work)
    elif order == "descending":
        keys.sort(key=work, reverse=True)
    return keys


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
@pytest.mark.parametrize("n", (1, 3, 64, 257))
def test_batches(gpu, n, order, grid_cap):
    keys = _batch(n, order)
    if n >= 64:
        assert len({k[0] for k in keys}) == 8
    _decode(gpu.WlanDecoder(), keys)


# ---- 4. no stale state ------------------------------------------------------------

def test_no_stale_state(gpu):
    d = gpu.WlanDecoder()
    _decode(d, [(5, 104)])
    _decode(d, [(0, 0)])                       # long, then short
    keys = _batch(64, "shuffled")
    first = _decode(d, keys)
    second = _decode(d, keys)                  # the same batch twice
    fresh = _decode(gpu.WlanDecoder(), keys)
    for a, b, c in zip(first, second, fresh):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    _decode(d, [(0, 0)])                       # shrinking again
    _decode(d, _batch(257, "descending"))      # growing the descriptors


# ---- 5. canaries, NULL d_dec_bytes, streams ---------------------------------------

def _layout(keys, gap):
    """Frame descriptors with `gap` canary bytes before every range."""
    descs, so, oo, do = [], 0, gap, gap
    for mcs, psdu, *_ in keys:
        ns, nd, _ = wlan_ref.frame_param(mcs, psdu)
        descs.append((mcs, psdu, so, oo, do))
        so += 48 * ns
        oo += psdu + 2 + gap
        do += (nd + 7) // 8 + gap
    return descs, so, oo, do


def _check_spans(keys, descs, out, dec, crc):
    want_out = np.full(out.size, CANARY, np.uint8)
    want_dec = np.full(dec.size, CANARY, np.uint8) if dec is not None else None
    for i, (k, (_, psdu, _, oo, do)) in enumerate(zip(keys, descs)):
        _, w_out, w_dec, w_crc = _frame(*k)
        want_out[oo:oo + psdu + 2] = w_out
        if dec is not None:
            want_dec[do:do + w_dec.size] = w_dec
        assert crc[i] == w_crc, i
    assert np.array_equal(out, want_out)        # values and canaries
    if dec is not None:
        assert np.array_equal(dec, want_dec)
    assert crc[len(keys):].tolist() == [CANARY] * (crc.size - len(keys))


CANARY_KEYS = ((1, 1, "clean"), (6, 61, "flip1"), (0, 104, "clean"),
               (7, 0, "clean"), (3, 41, "random"), (4, 23, "clean"))


@pytest.mark.parametrize("with_dec", (True, False))
def test_host_path_leaves_canaries(gpu, with_dec):
    lib = gpu.lib()
    descs, so, oo, do = _layout(CANARY_KEYS, 5)
    syms = np.concatenate([_frame(*k)[0] for k in CANARY_KEYS])
    out = np.full(oo, CANARY, np.uint8)
    dec = np.full(do, CANARY, np.uint8) if with_dec else None
    crc = np.full(len(descs) + 3, CANARY, np.uint8)
    d = gpu.WlanDecoder()
    rc = lib.fsdr_wlan_decode_host(
        d._h, syms.ctypes.data, d._descs(descs), len(descs), out.ctypes.data,
        dec.ctypes.data if with_dec else None, crc.ctypes.data)
    assert rc == gpu.OK, lib.fsdr_last_error()
    _check_spans(CANARY_KEYS, descs, out, dec, crc)


@pytest.mark.parametrize("with_dec", (True, False))
@pytest.mark.parametrize("own_stream", (False, True))
def test_dev_path_canaries_and_stream(gpu, with_dec, own_stream):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("torch.cuda not available on GPU box")
    descs, so, oo, do = _layout(CANARY_KEYS, 3)
    syms = np.concatenate([_frame(*k)[0] for k in CANARY_KEYS])
    stream = torch.cuda.Stream() if own_stream \
        else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        t_syms = torch.from_numpy(syms).cuda()
        t_out = torch.full((oo,), CANARY, dtype=torch.uint8, device="cuda")
        t_dec = torch.full((do,), CANARY, dtype=torch.uint8, device="cuda")
        t_crc = torch.full((len(descs) + 3,), CANARY, dtype=torch.uint8,
                           device="cuda")
        d = gpu.WlanDecoder()
        frames = list(descs)
        d.decode_dev(t_syms.data_ptr(), frames, t_out.data_ptr(),
                     t_crc.data_ptr(),
                     d_dec_bytes=t_dec.data_ptr() if with_dec else None,
                     stream=stream.cuda_stream)
        frames.clear()            # the host array is the caller's on return
    stream.synchronize()
    dec = t_dec.cpu().numpy()
    if not with_dec:
        assert (dec == CANARY).all()
    _check_spans(CANARY_KEYS, descs, t_out.cpu().numpy(),
                 dec if with_dec else None, t_crc.cpu().numpy())


def test_signal_field_decode(gpu):
    """The SIGNAL shape end to end: 24 bits coded as one BPSK 1/2 symbol,
    decoded as (mcs 0, psdu 0), parsed by wlan_signal_field."""
    d = gpu.WlanDecoder()
    for mcs, psdu in ((0, 100), (7, 1528), (5, 1)):
        bits = wlan_ref.signal_bits(mcs, psdu)
        enc = np.zeros(48, np.uint8)
        state = 0
        for i, b in enumerate(bits):
            state = ((state << 1) & 0x7E) | int(b)
            enc[2 * i] = bin(state & 0o155).count("1") & 1
            enc[2 * i + 1] = bin(state & 0o117).count("1") & 1
        syms = enc[wlan_ref.deinterleave_map(0)]
        (out, crc_ok, dec), = d.decode([(0, 0, syms)], raw=True)
        assert np.array_equal(dec, wlan_ref.decode(0, 0, syms)[1])
        assert gpu.wlan_signal_field(np.unpackbits(dec)) == (mcs, psdu)
