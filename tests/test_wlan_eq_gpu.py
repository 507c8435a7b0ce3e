"""The WLAN frame equalizer on the GPU against tests/wlan_eq_ref.py.

Equalized symbols are compared with the f64 reference under the bound
K * E_ref * max(1, |z|): E_ref is the error of the reference's own f32
restatement on the same frame, K = wlan_eq_ref.K_DEVICE (reasoning in that
module's docstring; the measured worst ratio is printed and recorded in
profiles/wlan_equalize.txt). Indices must equal the f64 reference's wherever
the f64 value is farther than DELTA from a decision threshold; at most 1 %
of a frame's symbols may be exempt, which tests/test_wlan_eq_cpu.py asserts
on the reference alone. Info fields are exact, snr_db within SNR_TOL_DB.
Reference results are cached in wlan_eq_ref.case and never modified."""

import numpy as np
import pytest

import wlan_eq_ref as R
import wlan_ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SENTINEL = np.complex64(1234.5 - 6789.0j)


@pytest.fixture(params=[None, "1"], ids=["cap-", "cap1"])
def grid_cap(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("FSDR_FIR_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("FSDR_FIR_GRID_CAP", request.param)
    return request.param


def _reference(spec):
    """(r64, E_ref, near) of one frame's spectra, from the reference alone."""
    r64, r32 = R.equalize(spec, np.float64), R.equalize(spec, np.float32)
    if not r64["found"] or r64["z"].size == 0:
        return r64, 0.0, np.zeros(0, bool)
    assert r32["z"].size == r64["z"].size
    return (r64, R.e_ref(r32["z"], r64["z"]),
            R.near_threshold(wlan_ref.MCS[r64["mcs"]][0], r64["z"]))


def _check_info(info, r64, label):
    assert (info.found, info.mcs, info.psdu_size, info.n_symbols,
            info.n_copied) == (r64["found"], r64["mcs"], r64["psdu_size"],
                               r64["n_symbols"], r64["n_copied"]), label
    if np.isnan(r64["snr_db"]):
        assert np.isnan(info.snr_db), label
    else:
        print(label, "snr_db", info.snr_db, "f64", r64["snr_db"])
        assert abs(info.snr_db - r64["snr_db"]) < R.SNR_TOL_DB, label


def _check_frame(got, ref, label):
    """got: (info, idx, z) of WlanEqualizer.equalize(symbols=True); ref:
    _reference(...). Returns the worst error in units of E_ref*max(1,|z|)."""
    info, idx, z = got
    r64, e_ref, near = ref
    _check_info(info, r64, label)
    n = 48 * r64["n_copied"]
    assert idx.size == n and z.size == n, label
    if n == 0:
        return 0.0
    scale = np.maximum(1.0, np.abs(r64["z"]))
    err = np.abs(z.astype(np.complex128) - r64["z"])
    ratio = float((err / (e_ref * scale)).max())
    print(label, "E_ref %.3g" % e_ref, "worst error / (E_ref*max(1,|z|)) "
          "%.3f" % ratio, "exempt %.4f" % near.mean())
    assert R.K_DEVICE * e_ref * scale.max() < R.DELTA, label
    assert near.mean() <= 0.01, label
    assert np.array_equal(idx[~near], r64["idx"][~near]), label
    assert (err <= R.K_DEVICE * e_ref * scale).all(), (label, ratio)
    return ratio


def _batch(cases):
    """(spec, frames) of whole cases laid end to end."""
    frames, off = [], 0
    for c in cases:
        frames.append((off, c["spec"].size // 64))
        off += c["spec"].size
    return np.concatenate([c["spec"] for c in cases]), frames


def _case_ref(c):
    return c["r64"], c["e_ref"], c["near"]


# ---- 1. parity -------------------------------------------------------------------

def test_parity_every_mcs(gpu):
    cases = R.parity_cases()
    spec, frames = _batch(cases)
    got = gpu.WlanEqualizer().equalize(spec, frames, symbols=True)
    assert len(got) == 8
    worst = max(_check_frame(g, _case_ref(c), "mcs %d" % c["mcs"])
                for g, c in zip(got, cases))
    print("worst ratio over the batch %.3f (K = %d)" % (worst, R.K_DEVICE))


# ---- 2. polarity wrap, striding ------------------------------------------------------

def test_polarity_wrap(gpu):
    c = R.case(0, 400, 12)
    assert c["r64"]["n_symbols"] == 135
    got, = gpu.WlanEqualizer().equalize(c["spec"], [(0, 138)], symbols=True)
    _check_frame(got, _case_ref(c), "wrap")
    # the symbols behind index 127 on their own
    assert np.array_equal(got[1][48 * 126:][~c["near"][48 * 126:]],
                          c["r64"]["idx"][48 * 126:][~c["near"][48 * 126:]])


def test_frames_strided_over_waves(gpu, grid_cap):
    cases = R.parity_cases() + [R.case(0, 400, 12)]
    spec, frames = _batch(cases)
    e = gpu.WlanEqualizer()
    got = e.equalize(spec, frames, symbols=True)
    assert len(got) == 9
    for i, (g, c) in enumerate(zip(got, cases)):
        _check_frame(g, _case_ref(c), "frame %d" % i)


# ---- 3. write discipline -------------------------------------------------------------

def _quiet(carriers, seed):
    """40 dB, two taps: no symbol near a threshold (asserted by the caller)."""
    return R.channel(carriers, np.random.default_rng(seed), 40.0, n_taps=2)


def _discipline_frames():
    """[(label, spec, n_avail)]"""
    rng = np.random.default_rng(77)
    whole, _ = R.frame_carriers(4, R.psdu_bytes(4, 60, 3))      # 6 symbols
    assert len(whole) == 9
    spec = _quiet(whole, 1)
    out = [("n_avail 0", spec[:0], 0), ("n_avail 2", spec[:128], 2),
           ("n_avail 3", spec[:192], 3), ("truncated", spec[:7 * 64], 7),
           ("whole", spec, 9)]
    bad = wlan_ref.signal_bits(2, 50)
    bad[17] ^= 1
    out.append(("parity", _quiet(R.custom_frame(bad, 2, 3, rng)[0], 2), 6))
    unk = wlan_ref.signal_bits(2, 50)
    unk[3] = 0                       # rate 10 -> 2: none the reference knows
    unk[17] = unk[:17].sum() & 1
    out.append(("rate", _quiet(R.custom_frame(unk, 2, 3, rng)[0], 3), 6))
    out.append(("zeros", np.zeros(6 * 64, np.complex64), 6))
    big = wlan_ref.signal_bits(3, 4095)
    out.append(("psdu 4095", _quiet(R.custom_frame(big, 2, 3, rng)[0], 4), 6))
    return out


def test_write_discipline(gpu):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("torch.cuda not available on GPU box")
    items = _discipline_frames()
    refs = [_reference(s) if n else (R.equalize(s), 0.0, np.zeros(0, bool))
            for _, s, n in items]
    by = {label: r for (label, _, _), r in zip(items, refs)}
    assert not by["parity"][0]["found"] and not by["rate"][0]["found"]
    assert not by["zeros"][0]["found"]
    assert (by["zeros"][0]["sig_idx"] == 0).all()
    assert by["truncated"][0]["n_copied"] == 4 < by["truncated"][0]["n_symbols"]
    assert (by["psdu 4095"][0]["psdu_size"], by["psdu 4095"][0]["n_symbols"],
            by["psdu 4095"][0]["n_copied"]) == (4095, 456, 3)
    assert by["n_avail 3"][0]["found"] and by["n_avail 3"][0]["n_copied"] == 0
    for _, _, near in refs:
        assert not near.any()        # so every index byte is compared
    gap = 5
    descs, so, oo = [], 0, gap
    for _, s, n in items:
        descs.append((so, n, oo, oo))
        so += s.size
        oo += 48 * max(n - 3, 0) + gap
    spec = np.concatenate([s for _, s, _ in items] + [np.zeros(64, np.complex64)])
    want_idx = np.full(oo, CANARY, np.uint8)
    touched = np.zeros(oo, bool)
    for (_, _, o, _), (r64, _, _) in zip(descs, refs):
        n = 48 * r64["n_copied"]
        want_idx[o:o + n] = r64["idx"]
        touched[o:o + n] = True
    n_info = len(items) + 2
    t_spec = torch.from_numpy(spec).cuda()
    t_idx = torch.full((oo,), CANARY, dtype=torch.uint8, device="cuda")
    t_eq = torch.full((oo,), complex(SENTINEL), dtype=torch.complex64,
                      device="cuda")
    t_info = torch.full((n_info * 24,), CANARY, dtype=torch.uint8,
                        device="cuda")
    e = gpu.WlanEqualizer()
    e.equalize_dev(t_spec.data_ptr(), descs, t_idx.data_ptr(),
                   t_info.data_ptr(), d_eq=t_eq.data_ptr())
    torch.cuda.synchronize()
    idx, eq = t_idx.cpu().numpy(), t_eq.cpu().numpy()
    info = t_info.cpu().numpy().view(gpu.WLAN_EQ_INFO_DTYPE)
    assert np.array_equal(idx, want_idx)              # values and guards
    assert (eq[~touched] == SENTINEL).all()
    assert (eq[touched] != SENTINEL).all()
    assert (t_info.cpu().numpy()[24 * len(items):] == CANARY).all()
    for i, ((label, _, n), (_, _, o, _), ref) in \
            enumerate(zip(items, descs, refs)):
        r64 = ref[0]
        m = 48 * r64["n_copied"]
        _check_frame((gpu._wlan_eq_info(info[i]), idx[o:o + m], eq[o:o + m]),
                     ref, label)
        if not r64["found"]:
            assert bytes(info[i].tobytes()[:20]) == bytes(20), label
    assert info[0]["snr_db"] == 0.0                   # n_avail 0
    assert info[1]["snr_db"] > 30 and info[1]["found"] == 0   # n_avail 2
    # without d_eq nothing but indices and info is written
    t_idx.fill_(CANARY)
    e.equalize_dev(t_spec.data_ptr(), descs, t_idx.data_ptr(),
                   t_info.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(t_idx.cpu().numpy(), want_idx)


# ---- 4. host path = device path; workspace regrowth ----------------------------------

def test_host_and_device_paths_agree(gpu):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("torch.cuda not available on GPU box")
    cases = R.parity_cases()
    e = gpu.WlanEqualizer()
    spec2, frames2 = _batch(cases[5:7])
    first = e.equalize(spec2, frames2, symbols=True)
    spec, frames = _batch(cases[5:7] + cases[:5] + cases[7:])
    second = e.equalize(spec, frames, symbols=True)    # grows the workspace
    fresh = gpu.WlanEqualizer().equalize(spec, frames, symbols=True)
    again = e.equalize(spec2, frames2, symbols=True)   # and shrinks the batch
    for a, b in list(zip(first, second)) + list(zip(second, fresh)) + \
            list(zip(first, again)):
        assert a[0] == b[0]
        assert a[1].tobytes() == b[1].tobytes()
        assert a[2].tobytes() == b[2].tobytes()
    # the device path, on a stream of its own
    descs, off = [], 0
    for so, na in frames:
        descs.append((so, na, off, off))
        off += 48 * (na - 3)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_spec = torch.from_numpy(spec).cuda()
        t_idx = torch.zeros(off, dtype=torch.uint8, device="cuda")
        t_eq = torch.zeros(off, dtype=torch.complex64, device="cuda")
        t_info = torch.zeros(24 * len(descs), dtype=torch.uint8,
                             device="cuda")
        e.equalize_dev(t_spec.data_ptr(), descs, t_idx.data_ptr(),
                       t_info.data_ptr(), d_eq=t_eq.data_ptr(),
                       stream=stream.cuda_stream)
    stream.synchronize()
    idx, eq = t_idx.cpu().numpy(), t_eq.cpu().numpy()
    info = t_info.cpu().numpy().view(gpu.WLAN_EQ_INFO_DTYPE)
    for i, ((_, _, o, _), h) in enumerate(zip(descs, second)):
        n = 48 * h[0].n_copied
        assert info[i].tobytes() == np.array(
            [tuple(h[0])], gpu.WLAN_EQ_INFO_DTYPE).tobytes()
        assert idx[o:o + n].tobytes() == h[1].tobytes()
        assert eq[o:o + n].tobytes() == h[2].tobytes()


# ---- 5. spectra to bytes ---------------------------------------------------------------

def test_spectra_to_bytes(gpu):
    cases = R.parity_cases()
    spec, spans = _batch(cases)
    cut = cases[4]["spec"][:64 * 6]                    # 3 of 6 data symbols
    bad = wlan_ref.signal_bits(2, 50)
    bad[17] ^= 1
    junk = _quiet(R.custom_frame(bad, 2, 3, np.random.default_rng(5))[0], 6)
    spans += [(spec.size, 6), (spec.size + cut.size, 6)]
    spec = np.concatenate([spec, cut, junk])
    got = gpu.wlan_receive(spec, spans)
    assert len(got) == 10
    for (info, psdu, crc_ok), c in zip(got, cases):
        # the reference alone recovers it (also in test_wlan_eq_cpu.py)
        out, _, ref_ok, _ = wlan_ref.decode(c["mcs"], c["psdu"],
                                            c["r64"]["idx"])
        assert ref_ok and out[2:].tobytes() == c["data"]
        assert (info.found, info.mcs, info.psdu_size) == \
            (True, c["mcs"], c["psdu"])
        assert psdu is not None and psdu.tobytes() == c["data"], c["mcs"]
        assert crc_ok, c["mcs"]
    assert got[8][0].found and got[8][0].n_copied == 3 < got[8][0].n_symbols
    assert got[8][1:] == (None, False)
    assert not got[9][0].found and got[9][1:] == (None, False)


# ---- 6. samples to bytes ---------------------------------------------------------------

def test_samples_to_bytes(gpu):
    """Metric chain, WlanRx, Fft(64), wlan_frame_spans, wlan_receive, composed
    as tests/test_wlan_rx_gpu.py composes the front end."""
    iq, data = R.sample_stream()
    sig = np.array(iq)
    n = sig.size
    delayed = np.concatenate([np.zeros(16, np.complex64), sig[:-16]])
    mc = gpu.cmul_conj_host(sig, delayed)
    abs48 = gpu.wlan_moving_sum_host(mc, 48)[:n]
    mag, _, _, _ = gpu.Mag2().filter(sig, n)
    power = gpu.wlan_moving_sum_host(mag.astype(np.float32), 64)[:n]
    cor = gpu.divide_mag_host(abs48, power)
    rx = gpu.WlanRx()
    fs, tags = rx.sync_short(delayed, abs48, cor)
    sy, frames = rx.sync_long(fs, tags)
    assert len(tags) == 2 and len(frames) == 2, (tags, frames)
    spans = gpu.wlan_frame_spans(tags, frames, fs.size)
    assert sum(64 * na for _, na in spans) == sy.size
    fft = gpu.Fft(64)
    outs, off = [], 0
    while off < sy.size:
        y, c, p, _ = fft.filter(sy[off:], sy.size - off)
        assert p > 0
        outs.append(y)
        off += c
    spec = np.concatenate(outs)
    got = gpu.wlan_receive(spec, spans)
    assert len(got) == 2
    for (info, psdu, crc_ok), d, (mcs, size) in \
            zip(got, data, R.SAMPLE_FRAMES):
        print("mcs", info.mcs, "psdu", info.psdu_size, "snr_db", info.snr_db)
        assert (info.found, info.mcs, info.psdu_size) == (True, mcs, size)
        assert info.n_copied == info.n_symbols
        assert psdu is not None and psdu.tobytes() == d and crc_ok
