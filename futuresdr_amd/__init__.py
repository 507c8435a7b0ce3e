"""futuresdr_amd — MI355X-native FutureSDR streaming-DSP hot path.

Python plumbing over the product C-ABI (include/futuresdr_hip.h,
implemented in csrc/futuresdr_hip.hip). The compute path is the HIP
extension; there is NO CPU fallback here — if the shared library or a HIP
device is missing, calls raise. The CPU restatement used for parity lives
in oracle/ (test infrastructure) and is never imported by this package.
"""
import collections
import ctypes
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libfutursdr_hip.so")

CF32 = np.dtype(np.complex64)

INSUFFICIENT_INPUT = 0
INSUFFICIENT_OUTPUT = 1
BOTH_SUFFICIENT = 2

OK = 0
ERR_NO_GPU = 1
ERR_HIP = 2
ERR_INVALID = 3
ERR_UNSUPPORTED = 4


class FsdrError(RuntimeError):
    pass


class _Result(ctypes.Structure):
    _fields_ = [
        ("consumed", ctypes.c_size_t),
        ("produced", ctypes.c_size_t),
        ("status", ctypes.c_int),
    ]


def build():
    """Compile the gfx950 HIP extension in-tree (hipcc, ~5 s)."""
    subprocess.run(["make", "-s", "-C", _DIR], check=True)


_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(
            f"futuresdr_amd HIP extension missing: {_SO} not built. "
            "Run futuresdr_amd.build() (or make -C futuresdr_amd). "
            "There is no CPU fallback — this is the GPU product path.")
    lib = ctypes.CDLL(_SO)
    sz = ctypes.c_size_t
    vp = ctypes.c_void_p
    f32p = ctypes.POINTER(ctypes.c_float)
    rp = ctypes.POINTER(_Result)

    lib.fsdr_last_error.restype = ctypes.c_char_p
    lib.fsdr_version.restype = ctypes.c_char_p
    lib.fsdr_device_count.restype = ctypes.c_int
    lib.fsdr_set_device.argtypes = [ctypes.c_int]
    lib.fsdr_fir_cf32_create.restype = vp
    lib.fsdr_fir_cf32_create.argtypes = [f32p, sz]
    lib.fsdr_fir_f32_create.restype = vp
    lib.fsdr_fir_f32_create.argtypes = [f32p, sz]
    lib.fsdr_fir_ccf32_create.restype = vp
    lib.fsdr_fir_ccf32_create.argtypes = [vp, sz]
    lib.fsdr_rotator_dev.restype = ctypes.c_int
    lib.fsdr_rotator_dev.argtypes = [vp, vp, sz, ctypes.c_float,
                                     ctypes.c_float, ctypes.c_float, vp,
                                     ctypes.POINTER(ctypes.c_float),
                                     ctypes.POINTER(ctypes.c_float)]
    lib.fsdr_decim_fir_cf32_create.restype = vp
    lib.fsdr_decim_fir_cf32_create.argtypes = [sz, f32p, sz]
    lib.fsdr_resamp_cf32_create.restype = vp
    lib.fsdr_resamp_cf32_create.argtypes = [sz, sz, f32p, sz]
    for fn in (lib.fsdr_resamp_f32_create, lib.fsdr_fm_demod_resamp_create):
        fn.restype = vp
        fn.argtypes = [sz, sz, f32p, sz]
    lib.fsdr_quad_demod_create.restype = vp
    lib.fsdr_quad_demod_create.argtypes = []
    lib.fsdr_fm_demod_resamp_fused.restype = ctypes.c_int
    lib.fsdr_fm_demod_resamp_fused.argtypes = [vp]
    szp = ctypes.POINTER(sz)
    lib.fsdr_iir_plan_create.restype = ctypes.c_int
    lib.fsdr_iir_plan_create.argtypes = [f32p, sz, ctypes.POINTER(vp)]
    lib.fsdr_iir_plan_destroy.restype = None
    lib.fsdr_iir_plan_destroy.argtypes = [vp]
    lib.fsdr_iir_plan_info.restype = ctypes.c_int
    lib.fsdr_iir_plan_info.argtypes = [vp, szp, szp, szp, szp]
    lib.fsdr_iir_plan_tables.restype = ctypes.c_int
    lib.fsdr_iir_plan_tables.argtypes = [vp, vp, vp, vp]
    lib.fsdr_iir_count.restype = None
    lib.fsdr_iir_count.argtypes = [sz, sz, sz, sz, sz, szp, szp, szp,
                                   ctypes.POINTER(ctypes.c_int)]
    lib.fsdr_iir_f32_create.restype = vp
    lib.fsdr_iir_f32_create.argtypes = [f32p, sz, f32p, sz]
    lib.fsdr_iir_plan_of.restype = vp
    lib.fsdr_iir_plan_of.argtypes = [vp]
    lib.fsdr_fg_add_vector_source_f32.restype = ctypes.c_int
    lib.fsdr_fg_add_vector_source_f32.argtypes = [vp, f32p, sz]
    lib.fsdr_lora_demod_create.restype = vp
    lib.fsdr_lora_demod_create.argtypes = [ctypes.c_uint, ctypes.c_int]
    lib.fsdr_lora_demod_set_frame.restype = ctypes.c_int
    lib.fsdr_lora_demod_set_frame.argtypes = [vp, ctypes.c_longlong,
                                              ctypes.c_double, ctypes.c_int]
    lib.fsdr_lora_downchirp.restype = ctypes.c_int
    lib.fsdr_lora_downchirp.argtypes = [ctypes.c_uint, ctypes.c_longlong,
                                        ctypes.c_double, vp]
    lib.fsdr_lora_log_i0.restype = ctypes.c_double
    lib.fsdr_lora_log_i0.argtypes = [ctypes.c_double]
    lib.fsdr_lora_demod_count.restype = ctypes.c_int
    lib.fsdr_lora_demod_count.argtypes = [ctypes.c_uint, sz, sz, szp, szp,
                                          ctypes.POINTER(ctypes.c_int)]
    lib.fsdr_wlan_decoder_create.restype = vp
    lib.fsdr_wlan_decoder_create.argtypes = []
    lib.fsdr_wlan_decoder_destroy.restype = None
    lib.fsdr_wlan_decoder_destroy.argtypes = [vp]
    lib.fsdr_wlan_decode_dev.restype = ctypes.c_int
    lib.fsdr_wlan_decode_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp]
    lib.fsdr_wlan_decode_host.restype = ctypes.c_int
    lib.fsdr_wlan_decode_host.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    lib.fsdr_wlan_frame_param.restype = ctypes.c_int
    lib.fsdr_wlan_frame_param.argtypes = [ctypes.c_uint, sz, szp, szp, szp]
    lib.fsdr_wlan_deinterleave_map.restype = ctypes.c_int
    lib.fsdr_wlan_deinterleave_map.argtypes = [ctypes.c_uint, vp]
    lib.fsdr_wlan_depuncture_map.restype = ctypes.c_int
    lib.fsdr_wlan_depuncture_map.argtypes = [ctypes.c_uint, sz, sz, sz, vp]
    lib.fsdr_wlan_signal_field.restype = ctypes.c_int
    lib.fsdr_wlan_signal_field.argtypes = [vp, ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_uint),
                                           szp]
    lib.fsdr_wlan_equalizer_create.restype = vp
    lib.fsdr_wlan_equalizer_create.argtypes = []
    lib.fsdr_wlan_equalizer_destroy.restype = None
    lib.fsdr_wlan_equalizer_destroy.argtypes = [vp]
    lib.fsdr_wlan_equalize_dev.restype = ctypes.c_int
    lib.fsdr_wlan_equalize_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp]
    lib.fsdr_wlan_equalize_host.restype = ctypes.c_int
    lib.fsdr_wlan_equalize_host.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    lib.fsdr_wlan_demap.restype = ctypes.c_int
    lib.fsdr_wlan_demap.argtypes = [ctypes.c_uint, vp, sz, vp]
    lib.fsdr_wlan_pilot_polarity.restype = ctypes.c_int
    lib.fsdr_wlan_pilot_polarity.argtypes = [sz, sz, vp]
    lib.fsdr_wlan_carrier_map.restype = ctypes.c_int
    lib.fsdr_wlan_carrier_map.argtypes = [vp]
    lib.fsdr_firdes_kaiser_multirate_f32.restype = sz
    lib.fsdr_firdes_kaiser_multirate_f32.argtypes = [sz, sz, sz,
                                                     ctypes.c_double, f32p,
                                                     sz]
    lib.fsdr_fft_cf32_create.restype = vp
    lib.fsdr_fft_cf32_create.argtypes = [sz, ctypes.c_int, ctypes.c_int, f32p]
    lib.fsdr_mag2_create.restype = vp
    lib.fsdr_moving_avg_create.restype = vp
    lib.fsdr_pfb_channelizer_create.restype = vp
    lib.fsdr_pfb_channelizer_create.argtypes = [sz, f32p, sz, ctypes.c_float]
    lib.fsdr_pfb_channelizer_window_map.restype = None
    lib.fsdr_pfb_channelizer_window_map.argtypes = [sz, sz, vp]
    lib.fsdr_pfb_channelizer_stream_dev.restype = ctypes.c_int
    lib.fsdr_pfb_channelizer_stream_dev.argtypes = [vp, vp, sz, vp, sz,
                                                    vp, ctypes.POINTER(sz),
                                                    ctypes.POINTER(sz)]
    lib.fsdr_pfb_channelizer_run_dev.restype = ctypes.c_int
    lib.fsdr_pfb_channelizer_run_dev.argtypes = [vp, vp, sz, vp, sz, vp,
                                                 ctypes.POINTER(sz)]
    lib.fsdr_pfb_synthesizer_create.restype = vp
    lib.fsdr_pfb_synthesizer_create.argtypes = [sz, f32p, sz]
    lib.fsdr_pfb_synthesizer_count.restype = None
    lib.fsdr_pfb_synthesizer_count.argtypes = [sz, sz, sz, sz, sz,
                                               ctypes.POINTER(sz),
                                               ctypes.POINTER(sz)]
    lib.fsdr_pfb_synthesizer_run_length.restype = sz
    lib.fsdr_pfb_synthesizer_run_length.argtypes = [sz, sz]
    for fn in (lib.fsdr_pfb_synthesizer_run_dev,
               lib.fsdr_pfb_synthesizer_stream_dev):
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, sz, sz, vp, sz, vp, ctypes.POINTER(sz),
                       ctypes.POINTER(sz)]
    u64 = ctypes.c_uint64
    u64p = ctypes.POINTER(u64)
    lib.fsdr_pfb_arb_schedule_create.restype = ctypes.c_int
    lib.fsdr_pfb_arb_schedule_create.argtypes = [ctypes.c_float, sz,
                                                 ctypes.POINTER(vp)]
    lib.fsdr_pfb_arb_schedule_destroy.restype = None
    lib.fsdr_pfb_arb_schedule_destroy.argtypes = [vp]
    lib.fsdr_pfb_arb_schedule_info.restype = ctypes.c_int
    lib.fsdr_pfb_arb_schedule_info.argtypes = [vp, u64p, u64p, u64p,
                                               ctypes.POINTER(sz),
                                               ctypes.POINTER(sz)]
    lib.fsdr_pfb_arb_schedule_count.restype = u64
    lib.fsdr_pfb_arb_schedule_count.argtypes = [vp, u64, u64]
    lib.fsdr_pfb_arb_schedule_records.restype = sz
    lib.fsdr_pfb_arb_schedule_records.argtypes = [vp, u64, sz, vp, vp, vp,
                                                  vp, sz]
    lib.fsdr_pfb_arb_schedule_work.restype = None
    lib.fsdr_pfb_arb_schedule_work.argtypes = [vp, sz, u64, sz, sz,
                                               ctypes.POINTER(sz),
                                               ctypes.POINTER(sz)]
    lib.fsdr_pfb_arb_startup_map.restype = None
    lib.fsdr_pfb_arb_startup_map.argtypes = [sz, vp]
    lib.fsdr_pfb_arb_resampler_create.restype = vp
    lib.fsdr_pfb_arb_resampler_create.argtypes = [ctypes.c_float, f32p, sz,
                                                  sz, sz]
    lib.fsdr_pfb_arb_resampler_schedule.restype = vp
    lib.fsdr_pfb_arb_resampler_schedule.argtypes = [vp]
    for fn in (lib.fsdr_pfb_arb_resampler_run_dev,
               lib.fsdr_pfb_arb_resampler_stream_dev):
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, sz, sz, vp, sz, sz, vp, ctypes.POINTER(sz),
                       ctypes.POINTER(sz)]
    lib.fsdr_xlating_fir_cf32_create.restype = vp
    lib.fsdr_xlating_fir_cf32_create.argtypes = [f32p, sz, sz,
                                                 ctypes.c_float,
                                                 ctypes.c_float]
    lib.fsdr_moving_avg_create.argtypes = [sz, ctypes.c_float, sz]
    lib.fsdr_filter_length.restype = sz
    lib.fsdr_filter_length.argtypes = [vp]
    ip = ctypes.POINTER(ctypes.c_int)
    lib.fsdr_filter_variant.restype = ctypes.c_int
    lib.fsdr_filter_variant.argtypes = [vp, ip, ip, ip]
    lib.fsdr_chain_variant.restype = ctypes.c_int
    lib.fsdr_chain_variant.argtypes = [vp, ip]
    lib.fsdr_filter_host.restype = ctypes.c_int
    lib.fsdr_filter_host.argtypes = [vp, vp, sz, vp, sz, rp]
    lib.fsdr_filter_dev.restype = ctypes.c_int
    lib.fsdr_filter_dev.argtypes = [vp, vp, sz, vp, sz, vp, rp]
    lib.fsdr_fft_bulk_dev.restype = ctypes.c_int
    lib.fsdr_fft_bulk_dev.argtypes = [vp, vp, vp, vp, sz, vp]
    lib.fsdr_filter_destroy.argtypes = [vp]
    lib.fsdr_cmul_conj_dev.restype = ctypes.c_int
    lib.fsdr_cmul_conj_dev.argtypes = [vp, sz, vp, sz, vp, sz, vp,
                                       ctypes.POINTER(sz)]
    lib.fsdr_divide_mag_dev.restype = ctypes.c_int
    lib.fsdr_divide_mag_dev.argtypes = [vp, sz, vp, sz, vp, sz, vp,
                                        ctypes.POINTER(sz)]
    lib.fsdr_wlan_rx_create.restype = vp
    lib.fsdr_wlan_rx_create.argtypes = []
    lib.fsdr_wlan_rx_destroy.argtypes = [vp]
    lib.fsdr_wlan_sync_short_run.restype = sz
    lib.fsdr_wlan_sync_short_run.argtypes = [vp, vp, vp, vp, sz, vp, sz,
                                             vp, vp, sz,
                                             ctypes.POINTER(sz),
                                             ctypes.POINTER(sz)]
    lib.fsdr_wlan_sync_long_run.restype = sz
    lib.fsdr_wlan_sync_long_run.argtypes = [vp, vp, sz, vp, vp, sz, vp,
                                            sz, vp, vp, sz,
                                            ctypes.POINTER(sz)]
    lib.fsdr_wlan_moving_sum_dev.restype = ctypes.c_int
    lib.fsdr_wlan_moving_sum_dev.argtypes = [vp, sz, vp, sz, sz,
                                             ctypes.c_int, vp,
                                             ctypes.POINTER(sz)]
    lib.fsdr_cmul_dev.restype = ctypes.c_int
    lib.fsdr_cmul_dev.argtypes = [vp, sz, vp, sz, vp, sz, vp,
                                  ctypes.POINTER(sz)]
    lib.fsdr_cmul_host.restype = ctypes.c_int
    lib.fsdr_cmul_host.argtypes = [vp, sz, vp, sz, vp, sz,
                                   ctypes.POINTER(sz)]
    lib.fsdr_dev_alloc.restype = ctypes.c_int
    lib.fsdr_dev_alloc.argtypes = [ctypes.POINTER(vp), sz]
    lib.fsdr_dev_free.argtypes = [vp]
    lib.fsdr_memcpy_h2d.restype = ctypes.c_int
    lib.fsdr_memcpy_h2d.argtypes = [vp, vp, sz]
    lib.fsdr_memcpy_d2h.restype = ctypes.c_int
    lib.fsdr_memcpy_d2h.argtypes = [vp, vp, sz]
    lib.fsdr_fill_uniform_cf32.restype = ctypes.c_int
    lib.fsdr_fill_uniform_cf32.argtypes = [vp, sz, ctypes.c_uint64,
                                           ctypes.c_uint64, vp]
    lib.fsdr_kaiser_beta.restype = ctypes.c_double
    lib.fsdr_kaiser_beta.argtypes = [ctypes.c_double]
    lib.fsdr_kaiser_window.restype = None
    lib.fsdr_kaiser_window.argtypes = [sz, ctypes.c_double,
                                       ctypes.POINTER(ctypes.c_double)]
    lib.fsdr_firdes_kaiser_lowpass_f32.restype = sz
    lib.fsdr_firdes_kaiser_lowpass_f32.argtypes = [
        ctypes.c_double, ctypes.c_double, ctypes.c_double, f32p, sz]
    lib.fsdr_firdes_lowpass_kaiser_n_f32.restype = ctypes.c_int
    lib.fsdr_firdes_lowpass_kaiser_n_f32.argtypes = [
        sz, ctypes.c_double, ctypes.c_double, f32p]
    lib.fsdr_chain_create.restype = vp
    lib.fsdr_chain_create.argtypes = [f32p, sz, f32p, sz, sz, sz]
    lib.fsdr_chain_run_dev.restype = ctypes.c_int
    lib.fsdr_chain_run_dev.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp,
                                       ctypes.POINTER(sz),
                                       ctypes.POINTER(sz)]
    lib.fsdr_chain_destroy.argtypes = [vp]
    lib.fsdr_synchronize.restype = ctypes.c_int
    lib.fsdr_fg_create.restype = vp
    lib.fsdr_fg_add_null_source_cf32.restype = ctypes.c_int
    lib.fsdr_fg_add_null_source_cf32.argtypes = [vp]
    lib.fsdr_fg_add_vector_source_cf32.restype = ctypes.c_int
    lib.fsdr_fg_add_vector_source_cf32.argtypes = [vp, vp, sz]
    lib.fsdr_fg_add_head.restype = ctypes.c_int
    lib.fsdr_fg_add_head.argtypes = [vp, ctypes.c_uint64]
    lib.fsdr_fg_add_filter.restype = ctypes.c_int
    lib.fsdr_fg_add_filter.argtypes = [vp, vp]
    lib.fsdr_fg_add_null_sink.restype = ctypes.c_int
    lib.fsdr_fg_add_null_sink.argtypes = [vp]
    lib.fsdr_fg_add_vector_sink.restype = ctypes.c_int
    lib.fsdr_fg_add_vector_sink.argtypes = [vp]
    lib.fsdr_fg_stream.restype = ctypes.c_int
    lib.fsdr_fg_stream.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.fsdr_fg_run.restype = ctypes.c_int
    lib.fsdr_fg_run.argtypes = [vp]
    lib.fsdr_fg_n_received.restype = ctypes.c_uint64
    lib.fsdr_fg_n_received.argtypes = [vp, ctypes.c_int]
    lib.fsdr_fg_vector_sink_get.restype = sz
    lib.fsdr_fg_vector_sink_get.argtypes = [vp, ctypes.c_int, vp, sz]
    lib.fsdr_fg_destroy.argtypes = [vp]
    lib.fsdr_filter_item_sizes.restype = sz
    lib.fsdr_filter_item_sizes.argtypes = [vp, ctypes.POINTER(sz)]
    lib.fsdr_ring_create.restype = vp
    lib.fsdr_ring_create.argtypes = [sz, sz, sz, sz]
    lib.fsdr_ring_writer_acquire.restype = ctypes.c_int
    lib.fsdr_ring_writer_acquire.argtypes = [vp, ctypes.POINTER(vp),
                                             ctypes.POINTER(sz)]
    lib.fsdr_ring_writer_commit.restype = ctypes.c_int
    lib.fsdr_ring_writer_commit.argtypes = [vp, sz]
    lib.fsdr_ring_reader_acquire.restype = ctypes.c_int
    lib.fsdr_ring_reader_acquire.argtypes = [vp, ctypes.POINTER(vp),
                                             ctypes.POINTER(sz)]
    lib.fsdr_ring_reader_release.restype = ctypes.c_int
    lib.fsdr_ring_reader_release.argtypes = [vp]
    lib.fsdr_ring_reader_release_consumed.restype = ctypes.c_int
    lib.fsdr_ring_reader_release_consumed.argtypes = [vp, sz, vp]
    lib.fsdr_ring_destroy.argtypes = [vp]
    lib.fsdr_ring_d2h_create.restype = vp
    lib.fsdr_ring_d2h_create.argtypes = [sz, sz, sz]
    lib.fsdr_ring_d2h_writer_acquire.restype = ctypes.c_int
    lib.fsdr_ring_d2h_writer_acquire.argtypes = [vp, ctypes.POINTER(vp),
                                                 ctypes.POINTER(sz), vp]
    lib.fsdr_ring_d2h_writer_commit.restype = ctypes.c_int
    lib.fsdr_ring_d2h_writer_commit.argtypes = [vp, sz, vp]
    lib.fsdr_ring_d2h_reader_acquire.restype = ctypes.c_int
    lib.fsdr_ring_d2h_reader_acquire.argtypes = [vp, ctypes.POINTER(vp),
                                                 ctypes.POINTER(sz)]
    lib.fsdr_ring_d2h_reader_release.restype = ctypes.c_int
    lib.fsdr_ring_d2h_reader_release.argtypes = [vp]
    lib.fsdr_ring_d2h_destroy.argtypes = [vp]
    _lib = lib
    return lib


def lib():
    return _load()


def exported_symbols():
    """Every symbol include/futuresdr_hip.h declares (for the CPU test)."""
    hdr = os.path.join(_DIR, "..", "include", "futuresdr_hip.h")
    import re
    syms = []
    with open(hdr) as f:
        for m in re.finditer(r"\b(fsdr_\w+)\s*\(", f.read()):
            syms.append(m.group(1))
    return sorted(set(syms))


def _check(rc):
    if rc != OK:
        raise FsdrError(f"fsdr error {rc}: "
                        f"{_load().fsdr_last_error().decode()}")


def _f32(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _c(a):
    return ctypes.c_void_p(a.ctypes.data)


def version():
    return _load().fsdr_version().decode()


def device_count():
    return _load().fsdr_device_count()


def set_device(i):
    _check(_load().fsdr_set_device(i))


def synchronize():
    _check(_load().fsdr_synchronize())


class Filter:
    """GPU filter handle mirroring futuredsp::Filter (lib.rs:48-68)."""

    ITEM_IN = CF32
    ITEM_OUT = CF32

    def __init__(self, handle):
        if not handle:
            raise FsdrError("filter create failed: "
                            f"{_load().fsdr_last_error().decode()}")
        self._h = handle

    @property
    def length(self):
        return _load().fsdr_filter_length(self._h)

    def variant(self):
        """(kk_mfma, kk_mfma32, tp_tpl): the kernel instantiation this
        handle's launches select, 0 where a family does not apply.
        Host-only."""
        kk, kk32, tp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(_load().fsdr_filter_variant(self._h, ctypes.byref(kk),
                                           ctypes.byref(kk32),
                                           ctypes.byref(tp)))
        return kk.value, kk32.value, tp.value

    def __del__(self):
        if getattr(self, "_h", None):
            _load().fsdr_filter_destroy(self._h)
            self._h = None

    def filter(self, inp, n_out):
        """Host-span path: numpy in -> (out, consumed, produced, status)."""
        lib = _load()
        inp = np.ascontiguousarray(inp, self.ITEM_IN)
        out = np.zeros(n_out, self.ITEM_OUT)
        r = _Result()
        _check(lib.fsdr_filter_host(
            self._h, ctypes.c_void_p(inp.ctypes.data), inp.size,
            ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(r)))
        return out[: r.produced], r.consumed, r.produced, r.status

    def filter_dev(self, d_in, n_in, d_out, n_out, stream=None):
        """Device-pointer path (ints = device addresses). Async."""
        lib = _load()
        r = _Result()
        _check(lib.fsdr_filter_dev(self._h, ctypes.c_void_p(d_in), n_in,
                                   ctypes.c_void_p(d_out), n_out,
                                   ctypes.c_void_p(stream or 0),
                                   ctypes.byref(r)))
        return r.consumed, r.produced, r.status


class Fir(Filter):
    """Fir block core — src/blocks/fir.rs + futuredsp fir.rs (cf32 x f32)."""

    def __init__(self, taps):
        self._taps_keep, p = _f32(taps)
        super().__init__(_load().fsdr_fir_cf32_create(p,
                                                      self._taps_keep.size))


class FirCC(Filter):
    """Complex-taps FIR — fir.rs:257-277 (WLAN correlator core)."""

    def __init__(self, taps):
        self._taps_keep = np.ascontiguousarray(taps, CF32)
        super().__init__(_load().fsdr_fir_ccf32_create(
            ctypes.c_void_p(self._taps_keep.ctypes.data),
            self._taps_keep.size))


def rotator_host(inp, phase_incr_angle, phase0=1.0 + 0.0j):
    """Rotator over a host span (stages via dev helpers)."""
    lib = _load()
    inp = np.ascontiguousarray(inp, CF32)
    n = inp.size
    d_in = ctypes.c_void_p()
    d_out = ctypes.c_void_p()
    _check(lib.fsdr_dev_alloc(ctypes.byref(d_in), max(n, 1) * 8))
    _check(lib.fsdr_dev_alloc(ctypes.byref(d_out), max(n, 1) * 8))
    try:
        _check(lib.fsdr_memcpy_h2d(d_in, ctypes.c_void_p(inp.ctypes.data),
                                   n * 8))
        fr = ctypes.c_float()
        fi = ctypes.c_float()
        _check(lib.fsdr_rotator_dev(d_in, d_out, n, phase_incr_angle,
                                    phase0.real, phase0.imag, None,
                                    ctypes.byref(fr), ctypes.byref(fi)))
        _check(lib.fsdr_synchronize())
        out = np.zeros(n, CF32)
        _check(lib.fsdr_memcpy_d2h(ctypes.c_void_p(out.ctypes.data), d_out,
                                   n * 8))
        return out, complex(fr.value, fi.value)
    finally:
        lib.fsdr_dev_free(d_in)
        lib.fsdr_dev_free(d_out)


class FirF32(Filter):
    ITEM_IN = np.dtype(np.float32)
    ITEM_OUT = np.dtype(np.float32)

    def __init__(self, taps):
        self._taps_keep, p = _f32(taps)
        super().__init__(_load().fsdr_fir_f32_create(p, self._taps_keep.size))


class DecimFir(Filter):
    def __init__(self, decimation, taps):
        self._taps_keep, p = _f32(taps)
        super().__init__(_load().fsdr_decim_fir_cf32_create(
            decimation, p, self._taps_keep.size))


class Resampler(Filter):
    def __init__(self, interp, decim, taps):
        self._taps_keep, p = _f32(taps)
        super().__init__(_load().fsdr_resamp_cf32_create(
            interp, decim, p, self._taps_keep.size))


class ResamplerF32(Filter):
    """PolyphaseResamplingFir<f32,f32,f32> —
    polyphase_resampling_fir.rs:126-141."""
    ITEM_IN = np.dtype(np.float32)
    ITEM_OUT = np.dtype(np.float32)

    def __init__(self, interp, decim, taps):
        self._taps_keep, p = _f32(taps)
        super().__init__(_load().fsdr_resamp_f32_create(
            interp, decim, p, self._taps_keep.size))


class QuadDemod(Filter):
    """d[i] = arg(x[i] * conj(x[i-1])), x[-1] carried across calls —
    the demod Apply of examples/fm-receiver/src/main.rs:99-104."""
    ITEM_OUT = np.dtype(np.float32)

    def __init__(self):
        super().__init__(_load().fsdr_quad_demod_create())


class FmDemodResampler(Filter):
    """QuadDemod then ResamplerF32 as one block (Complex32 in, f32 out);
    the demodulated stream stays on chip when `fused`."""
    ITEM_OUT = np.dtype(np.float32)

    def __init__(self, interp, decim, taps):
        self._taps_keep, p = _f32(taps)
        super().__init__(_load().fsdr_fm_demod_resamp_create(
            interp, decim, p, self._taps_keep.size))

    @property
    def fused(self):
        """True where calls run the fused kernel, False where they
        demodulate into scratch and run the f32 resampler kernels (span
        over the LDS budget, or FSDR_FM_FUSED=0). Host-only."""
        return bool(_load().fsdr_fm_demod_resamp_fused(self._h))


def iir_count(n_a, n_b, filled, n_in, n_out):
    """(filled_after, consumed, produced, status) of one IirFilter call
    whose memory holds `filled` samples (iir.rs:90-177). Needs no GPU."""
    fa, c, p = (ctypes.c_size_t() for _ in range(3))
    st = ctypes.c_int()
    _load().fsdr_iir_count(n_a, n_b, filled, n_in, n_out, ctypes.byref(fa),
                           ctypes.byref(c), ctypes.byref(p), ctypes.byref(st))
    return fa.value, c.value, p.value, st.value


class IirPlan:
    """The constant tables of the blocked IIR recurrence for feedback taps
    `a_taps`: host-only, needs no GPU. Raises FsdrError (with .code) where
    the taps are out of range or a table entry overflows f32."""

    def __init__(self, a_taps, _borrowed=None):
        lib = _load()
        self._own = _borrowed is None
        self._destroy = lib.fsdr_iir_plan_destroy
        if self._own:
            a, p = _f32(a_taps)
            self.n_a = a.size
            h = ctypes.c_void_p()
            rc = lib.fsdr_iir_plan_create(p, a.size, ctypes.byref(h))
            if rc != OK:
                err = FsdrError(f"fsdr error {rc}: "
                                f"{lib.fsdr_last_error().decode()}")
                err.code = rc
                raise err
            self._h = h
        else:
            self.n_a = np.asarray(a_taps).size
            self._h = ctypes.c_void_p(_borrowed)

    def __del__(self):
        # may run at interpreter exit, after the module globals are gone
        if getattr(self, "_own", False) and getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def info(self):
        """(chunk_len L, chunks_per_tile, tile, scan_pass_tiles)."""
        v = [ctypes.c_size_t() for _ in range(4)]
        _check(_load().fsdr_iir_plan_info(self._h,
                                          *(ctypes.byref(x) for x in v)))
        return tuple(x.value for x in v)

    def tables(self):
        """(H [L, n_a], chunk_pow [levels, n_a, n_a], tile_pow likewise) in
        float64 as the plan computed them; the kernels read each entry
        rounded to float32 once."""
        L, chunks, _, passes = self.info()
        n = self.n_a
        lc, lt = chunks.bit_length() - 1, passes.bit_length() - 1
        H = np.zeros((L, n), np.float64)
        pc = np.zeros((lc, n, n), np.float64)
        pt = np.zeros((lt, n, n), np.float64)
        _check(_load().fsdr_iir_plan_tables(self._h, _c(H), _c(pc), _c(pt)))
        return H, pc, pt


class Iir(Filter):
    """IirFilter<f32,f32,_> — futuredsp iir.rs:56-178: stateful, the
    memory carried on the device across calls."""
    ITEM_IN = np.dtype(np.float32)
    ITEM_OUT = np.dtype(np.float32)

    def __init__(self, a_taps, b_taps):
        self._a_keep, pa = _f32(a_taps)
        self._b_keep, pb = _f32(b_taps)
        super().__init__(_load().fsdr_iir_f32_create(
            pa, self._a_keep.size, pb, self._b_keep.size))

    @property
    def plan(self):
        """The handle's own plan (borrowed; keeps the handle alive)."""
        p = IirPlan(self._a_keep,
                    _borrowed=_load().fsdr_iir_plan_of(self._h))
        p._keep = self
        return p


LORA_RAW = 0
LORA_HARD = 1
LORA_SOFT = 2


def lora_downchirp(sf, cfo_int=0, cfo_frac=0.0):
    """The HARD/SOFT dechirp table of a LoraFftDemod: conj(build_upchirp(0,
    sf, 1, false)) (utils.rs:884-914, f32 phase) rotated by the cfo in f64.
    Needs no GPU."""
    if not 5 <= sf <= 12:
        raise FsdrError("lora: sf must be in [5,12]")
    out = np.zeros(1 << sf, CF32)
    _check(_load().fsdr_lora_downchirp(sf, cfo_int, cfo_frac, _c(out)))
    return out


def lora_log_i0(x):
    """ln I0(x) as the SOFT kernel evaluates it. Needs no GPU."""
    return _load().fsdr_lora_log_i0(float(x))


def lora_demod_count(sf, n_in, n_out):
    """(consumed, produced, status) of one LoraFftDemod call. Needs no
    GPU."""
    c, p = ctypes.c_size_t(), ctypes.c_size_t()
    st = ctypes.c_int()
    _check(_load().fsdr_lora_demod_count(sf, n_in, n_out, ctypes.byref(c),
                                         ctypes.byref(p), ctypes.byref(st)))
    return c.value, p.value, st.value


class LoraFftDemod(Filter):
    """The arithmetic of the reference's FftDemod (examples/lora
    fft_demod.rs) and of FrameSync's get_symbol_val (utils.rs:1059-1078):
    dechirp, FFT, |X|^2 and the bin reduction in one kernel. `mode` is
    LORA_RAW (uint16 argmax, 0xFFFF for zero energy), LORA_HARD (uint16
    symbol) or LORA_SOFT (float64[12] LLRs per symbol, MSB first)."""

    def __init__(self, sf, mode):
        self.sf, self.mode = sf, mode
        self.ITEM_OUT = np.dtype(np.float64 if mode == LORA_SOFT
                                 else np.uint16)
        super().__init__(_load().fsdr_lora_demod_create(sf, mode))

    def set_frame(self, cfo_int=0, cfo_frac=0.0, reduced_rate=False):
        """The frame_info state of fft_demod.rs:355-399; reduced_rate as
        :72-75 computes it."""
        _check(_load().fsdr_lora_demod_set_frame(self._h, cfo_int, cfo_frac,
                                                 int(bool(reduced_rate))))

    def filter(self, inp, n_out):
        """numpy in -> (y, consumed, produced, status); y is uint16[produced]
        or float64[produced, 12]."""
        lib = _load()
        inp = np.ascontiguousarray(inp, CF32)
        shape = (n_out, 12) if self.mode == LORA_SOFT else (n_out,)
        out = np.zeros(shape, self.ITEM_OUT)
        r = _Result()
        _check(lib.fsdr_filter_host(self._h, _c(inp), inp.size, _c(out),
                                    n_out, ctypes.byref(r)))
        return out[: r.produced], r.consumed, r.produced, r.status


class Fft(Filter):
    def __init__(self, length, inverse=False, fft_shift=False,
                 normalize=None):
        np_ = None
        if normalize is not None:
            np_ = ctypes.pointer(ctypes.c_float(normalize))
        super().__init__(_load().fsdr_fft_cf32_create(
            length, int(inverse), int(fft_shift), np_))

    def bulk_dev(self, d_in, d_out, frames, d_mag=0, stream=None):
        """One launch over `frames` device-resident frames (the batch
        path; fsdr_filter_dev keeps the reference's 32-frame quantum)."""
        _check(_load().fsdr_fft_bulk_dev(
            self._h, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out),
            ctypes.c_void_p(d_mag), frames, ctypes.c_void_p(stream or 0)))


class Mag2(Filter):
    ITEM_OUT = np.dtype(np.float32)

    def __init__(self):
        super().__init__(_load().fsdr_mag2_create())


class XlatingFir(Filter):
    """XlatingFir block — xlating_fir.rs (rotate + filter + decimate)."""

    def __init__(self, taps, decimation, offset, sample_rate):
        self._taps_keep, p = _f32(taps)
        super().__init__(_load().fsdr_xlating_fir_cf32_create(
            p, self._taps_keep.size, decimation, offset, sample_rate))


class PfbChannelizer(Filter):
    """PFB channelizer — pfb/channelizer.rs (any oversample N/i;
    decimation D = N/oversample). Stateful streaming via stream()."""

    def __init__(self, num_channels, taps, oversample_rate=1.0):
        self._taps_keep, p = _f32(taps)
        self.n = num_channels
        self.decim = int(num_channels / oversample_rate)
        super().__init__(_load().fsdr_pfb_channelizer_create(
            num_channels, p, self._taps_keep.size, oversample_rate))

    def _call(self, fn, x, cap, with_consumed):
        lib = _load()
        d_in = ctypes.c_void_p()
        d_out = ctypes.c_void_p()
        _check(lib.fsdr_dev_alloc(ctypes.byref(d_in), x.size * 8 + 8))
        _check(lib.fsdr_dev_alloc(ctypes.byref(d_out), self.n * cap * 8 + 8))
        try:
            if x.size:
                _check(lib.fsdr_memcpy_h2d(
                    d_in, ctypes.c_void_p(x.ctypes.data), x.size * 8))
            prod = ctypes.c_size_t()
            cons = ctypes.c_size_t()
            tail = ((ctypes.byref(prod), ctypes.byref(cons))
                    if with_consumed else (ctypes.byref(prod),))
            _check(fn(self._h, d_in, x.size, d_out, cap, None, *tail))
            _check(lib.fsdr_synchronize())
            out = np.zeros(self.n * cap, CF32)
            if out.size:
                _check(lib.fsdr_memcpy_d2h(ctypes.c_void_p(out.ctypes.data),
                                           d_out, self.n * cap * 8))
            return (out.reshape(self.n, cap)[:, :prod.value], cons.value)
        finally:
            lib.fsdr_dev_free(d_in)
            lib.fsdr_dev_free(d_out)

    def stream(self, chunk, out_cap=None):
        """Feed one host chunk through the stateful streaming path;
        returns ([num_channels, produced] array, consumed). out_cap is the
        room per channel (default: every available step). Unconsumed
        samples must be re-presented by the caller (slab semantics)."""
        chunk = np.ascontiguousarray(chunk, CF32)
        if out_cap is None:
            out_cap = max(1, (chunk.size + self.n * self._tpf())
                          // self.decim)
        return self._call(_load().fsdr_pfb_channelizer_stream_dev, chunk,
                          out_cap, True)

    def _tpf(self):
        return -(-self._taps_keep.size // self.n)

    def run(self, inp, out_cap=None):
        """Bulk one-shot from zero state over a host span; returns an
        array of shape [num_channels, produced], at most out_cap steps
        (default: every available step)."""
        inp = np.ascontiguousarray(inp, CF32)
        if out_cap is None:
            out_cap = max(1, (inp.size - self.n * self._tpf()) // self.decim)
        return self._call(_load().fsdr_pfb_channelizer_run_dev, inp,
                          out_cap, False)[0]


def pfb_channelizer_window_map(taps_per_filter, q):
    """src[w]: which of its window's pushes (0 = first fill push) slice
    position w (0 = oldest) of a channelizer window holds after
    taps_per_filter fill pushes and q more, -1 for a hole — the map the
    start-up kernel reads through. Needs no GPU."""
    src = np.zeros(taps_per_filter, np.int64)
    _load().fsdr_pfb_channelizer_window_map(taps_per_filter, q, _c(src))
    return src


def pfb_synthesizer_count(num_channels, taps_per_filter, pushes,
                          n_in_per_chan, out_cap):
    """(consumed_per_chan, produced) of one synthesizer call — the host
    planning of PfbSynthesizer.run/stream; needs no GPU."""
    cons = ctypes.c_size_t()
    prod = ctypes.c_size_t()
    _load().fsdr_pfb_synthesizer_count(
        num_channels, taps_per_filter, pushes, n_in_per_chan, out_cap,
        ctypes.byref(cons), ctypes.byref(prod))
    return cons.value, prod.value


def pfb_synthesizer_run_length(num_channels, taps_per_filter):
    """Steps one block of the fused synthesizer kernel owns (0: staged
    path only). Needs no GPU."""
    return _load().fsdr_pfb_synthesizer_run_length(num_channels,
                                                   taps_per_filter)


class PfbSynthesizer(Filter):
    """PFB synthesizer — pfb/synthesizer.rs. chans is [num_channels, T]
    (one row per channel); run() is one-shot from zero state, stream()
    carries the windows across calls."""

    def __init__(self, num_channels, taps):
        self._taps_keep, p = _f32(taps)
        self.n = num_channels
        super().__init__(_load().fsdr_pfb_synthesizer_create(
            num_channels, p, self._taps_keep.size))

    def _call(self, fn, chans, out_cap):
        lib = _load()
        chans = np.ascontiguousarray(chans, CF32).reshape(self.n, -1)
        t = chans.shape[1]
        if out_cap is None:
            out_cap = (t + 1) * self.n  # every step finds > N free slots
        d_in = ctypes.c_void_p()
        d_out = ctypes.c_void_p()
        _check(lib.fsdr_dev_alloc(ctypes.byref(d_in), chans.size * 8 + 8))
        _check(lib.fsdr_dev_alloc(ctypes.byref(d_out), out_cap * 8 + 8))
        try:
            if chans.size:
                _check(lib.fsdr_memcpy_h2d(d_in, _c(chans), chans.size * 8))
            cons = ctypes.c_size_t()
            prod = ctypes.c_size_t()
            _check(fn(self._h, d_in, t, t, d_out, out_cap, None,
                      ctypes.byref(cons), ctypes.byref(prod)))
            _check(lib.fsdr_synchronize())
            out = np.zeros(prod.value, CF32)
            if prod.value:
                _check(lib.fsdr_memcpy_d2h(_c(out), d_out, prod.value * 8))
            return out, cons.value
        finally:
            lib.fsdr_dev_free(d_in)
            lib.fsdr_dev_free(d_out)

    def run(self, chans, out_cap=None):
        """Bulk one-shot over host channel rows; returns (out,
        consumed_per_chan)."""
        return self._call(_load().fsdr_pfb_synthesizer_run_dev, chans,
                          out_cap)

    def stream(self, chans, out_cap=None):
        """One stateful call; returns (out, consumed_per_chan). Steps not
        consumed must be re-presented by the caller."""
        return self._call(_load().fsdr_pfb_synthesizer_stream_dev, chans,
                          out_cap)


def pfb_arb_startup_map(taps_per_filter):
    """src[s]: the fill push that slot s of the just-filled window holds,
    -1 for a hole (WindowBuffer::new(len, false)). Needs no GPU."""
    src = np.zeros(taps_per_filter, np.int64)
    _load().fsdr_pfb_arb_startup_map(taps_per_filter, _c(src))
    return src


class PfbArbSchedule:
    """The PfbArbResampler timing schedule for (rate, num_filters): which
    input yields which outputs, with which filter index and mu. Host-only,
    needs no GPU. Positions count the pushes after the window fill."""

    def __init__(self, rate, num_filters, _borrowed=None):
        lib = _load()
        self._own = _borrowed is None
        self._destroy = lib.fsdr_pfb_arb_schedule_destroy
        if self._own:
            h = ctypes.c_void_p()
            rc = lib.fsdr_pfb_arb_schedule_create(rate, num_filters,
                                                  ctypes.byref(h))
            if rc != OK:
                err = FsdrError(f"fsdr error {rc}: "
                                f"{lib.fsdr_last_error().decode()}")
                err.code = rc
                raise err
            self._h = h
        else:
            self._h = ctypes.c_void_p(_borrowed)
        rho, lam, opc = (ctypes.c_uint64() for _ in range(3))
        q, seg = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib.fsdr_pfb_arb_schedule_info(
            self._h, ctypes.byref(rho), ctypes.byref(lam), ctypes.byref(opc),
            ctypes.byref(q), ctypes.byref(seg)))
        self.preperiod, self.period = rho.value, lam.value
        self.outputs_per_period = opc.value
        self.checkpoint_spacing = q.value
        self.segment_inputs = seg.value

    def __del__(self):
        # may run at interpreter exit, after the module globals are gone
        if getattr(self, "_own", False) and getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def count(self, pushes_after_fill, n_inputs):
        return _load().fsdr_pfb_arb_schedule_count(
            self._h, pushes_after_fill, n_inputs)

    def records(self, first_input, n_inputs):
        """(in_index u64, base_index u32, boundary u8, mu f32), one entry
        per output of inputs [first_input, first_input + n_inputs)."""
        lib = _load()
        n = lib.fsdr_pfb_arb_schedule_records(
            self._h, first_input, n_inputs, None, None, None, None, 0)
        idx = np.zeros(n, np.uint64)
        base = np.zeros(n, np.uint32)
        bnd = np.zeros(n, np.uint8)
        mu = np.zeros(n, np.float32)
        lib.fsdr_pfb_arb_schedule_records(
            self._h, first_input, n_inputs, _c(idx), _c(base), _c(bnd),
            _c(mu), n)
        return idx, base, bnd, mu

    def work(self, taps_per_filter, pushes, n_in, out_cap):
        """(consumed, produced) of one resampler call by a stream that has
        consumed `pushes` inputs in all."""
        cons, prod = ctypes.c_size_t(), ctypes.c_size_t()
        _load().fsdr_pfb_arb_schedule_work(
            self._h, taps_per_filter, pushes, n_in, out_cap,
            ctypes.byref(cons), ctypes.byref(prod))
        return cons.value, prod.value


class PfbArbResampler(Filter):
    """PFB arbitrary-rate resampler — pfb/arb_resampler.rs, for
    num_channels channels in lockstep. chans is [num_channels, T] (or 1-D
    for one channel); run() is one-shot from zero state, stream() carries
    the window and the position across calls. Both return
    ([num_channels, produced] array, consumed_per_chan)."""

    def __init__(self, rate, taps, num_filters, num_channels=1):
        self._taps_keep, p = _f32(taps)
        self.rate = float(np.float32(rate))
        self.n = num_channels
        super().__init__(_load().fsdr_pfb_arb_resampler_create(
            rate, p, self._taps_keep.size, num_filters, num_channels))

    @property
    def schedule(self):
        """The handle's own schedule (borrowed; keeps the handle alive)."""
        s = PfbArbSchedule(
            None, None,
            _borrowed=_load().fsdr_pfb_arb_resampler_schedule(self._h))
        s._keep = self
        return s

    def out_cap_for(self, n_in):
        """An out_cap_per_chan with which a call takes all n_in inputs."""
        return int(np.ceil(n_in * self.rate * (1 + 1e-6))) + \
            int(np.ceil(self.rate)) + 2

    def _call(self, fn, chans, out_cap):
        lib = _load()
        chans = np.ascontiguousarray(chans, CF32).reshape(self.n, -1)
        t = chans.shape[1]
        if out_cap is None:
            out_cap = self.out_cap_for(t)
        d_in = ctypes.c_void_p()
        d_out = ctypes.c_void_p()
        _check(lib.fsdr_dev_alloc(ctypes.byref(d_in), chans.size * 8 + 8))
        _check(lib.fsdr_dev_alloc(ctypes.byref(d_out),
                                  self.n * out_cap * 8 + 8))
        try:
            if chans.size:
                _check(lib.fsdr_memcpy_h2d(d_in, _c(chans), chans.size * 8))
            cons = ctypes.c_size_t()
            prod = ctypes.c_size_t()
            _check(fn(self._h, d_in, t, t, d_out, out_cap, out_cap, None,
                      ctypes.byref(cons), ctypes.byref(prod)))
            _check(lib.fsdr_synchronize())
            out = np.zeros((self.n, out_cap), CF32)
            if prod.value:
                _check(lib.fsdr_memcpy_d2h(_c(out), d_out, out.size * 8))
            return out[:, :prod.value].copy(), cons.value
        finally:
            lib.fsdr_dev_free(d_in)
            lib.fsdr_dev_free(d_out)

    def run(self, chans, out_cap=None):
        return self._call(_load().fsdr_pfb_arb_resampler_run_dev, chans,
                          out_cap)

    def stream(self, chans, out_cap=None):
        """One stateful call. Inputs not consumed must be re-presented by
        the caller."""
        return self._call(_load().fsdr_pfb_arb_resampler_stream_dev, chans,
                          out_cap)


class MovingAvg(Filter):
    """MovingAvg block — moving_avg.rs:79-118 (stateful per-bin EMA)."""

    ITEM_IN = np.dtype(np.float32)
    ITEM_OUT = np.dtype(np.float32)

    def __init__(self, width, decay_factor, history):
        super().__init__(_load().fsdr_moving_avg_create(
            width, decay_factor, history))


class Chain:
    """Fused Fir -> DecimFir -> Fft pipeline (the bench hot path)."""

    def __init__(self, taps1, taps2, decim, fft_len):
        lib = _load()
        self._t1, p1 = _f32(taps1)
        self._t2, p2 = _f32(taps2)
        self.decim, self.fft_len = decim, fft_len
        self._h = lib.fsdr_chain_create(p1, self._t1.size, p2, self._t2.size,
                                        decim, fft_len)
        if not self._h:
            raise FsdrError("chain create failed: "
                            f"{lib.fsdr_last_error().decode()}")

    def __del__(self):
        if getattr(self, "_h", None):
            _load().fsdr_chain_destroy(self._h)
            self._h = None

    def variant(self):
        """MFMA K of the fused filter (0: no fused filter). Host-only."""
        kk = ctypes.c_int()
        _check(_load().fsdr_chain_variant(self._h, ctypes.byref(kk)))
        return kk.value

    def run_dev(self, d_in, n_in, d_out=0, out_cap=0, d_mag=0, mag_cap=0,
                stream=None):
        lib = _load()
        cons = ctypes.c_size_t()
        prod = ctypes.c_size_t()
        _check(lib.fsdr_chain_run_dev(
            self._h, ctypes.c_void_p(d_in), n_in, ctypes.c_void_p(d_out),
            out_cap, ctypes.c_void_p(d_mag), mag_cap,
            ctypes.c_void_p(stream or 0), ctypes.byref(cons),
            ctypes.byref(prod)))
        return cons.value, prod.value


class Flowgraph:
    """Native-driver flowgraph: mirrors Flowgraph::add + connect! + run
    (flowgraph.rs, runtime.rs) for 1-in/1-out chains on the GPU."""

    def __init__(self):
        self._h = _load().fsdr_fg_create()
        if not self._h:
            raise FsdrError("flowgraph create failed (no HIP device?)")
        self._keep = []  # keep filter objects alive

    def __del__(self):
        if getattr(self, "_h", None):
            _load().fsdr_fg_destroy(self._h)
            self._h = None

    def null_source(self):
        return _load().fsdr_fg_add_null_source_cf32(self._h)

    def vector_source(self, data):
        data = np.ascontiguousarray(data, CF32)
        self._keep.append(data)
        return _load().fsdr_fg_add_vector_source_cf32(
            self._h, ctypes.c_void_p(data.ctypes.data), data.size)

    def vector_source_f32(self, data):
        data, p = _f32(data)
        self._keep.append(data)
        return _load().fsdr_fg_add_vector_source_f32(self._h, p, data.size)

    def head(self, n):
        return _load().fsdr_fg_add_head(self._h, n)

    def filter(self, f):
        self._keep.append(f)
        return _load().fsdr_fg_add_filter(self._h, f._h)

    def null_sink(self):
        return _load().fsdr_fg_add_null_sink(self._h)

    def vector_sink(self):
        return _load().fsdr_fg_add_vector_sink(self._h)

    def stream(self, src, dst):
        _check(_load().fsdr_fg_stream(self._h, src, dst))

    def connect(self, *blocks):
        for a, b in zip(blocks, blocks[1:]):
            self.stream(a, b)

    def run(self):
        _check(_load().fsdr_fg_run(self._h))

    def n_received(self, block):
        return _load().fsdr_fg_n_received(self._h, block)

    def sink_data(self, block, dtype=CF32):
        lib = _load()
        nbytes = lib.fsdr_fg_vector_sink_get(self._h, block, None, 0)
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype)
        lib.fsdr_fg_vector_sink_get(self._h, block,
                                    ctypes.c_void_p(out.ctypes.data), nbytes)
        return out


def kaiser_lowpass(cutoff, transition_bw, max_ripple):
    """firdes::kaiser::lowpass<f32> — product host-side designer."""
    lib = _load()
    n = lib.fsdr_firdes_kaiser_lowpass_f32(cutoff, transition_bw,
                                           max_ripple, None, 0)
    out = np.zeros(n, np.float32)
    lib.fsdr_firdes_kaiser_lowpass_f32(
        cutoff, transition_bw, max_ripple,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
    return out


def kaiser_multirate(interp, decim, half_len=12, max_ripple=1e-4):
    """firdes::kaiser::multirate<f32> (basic.rs:412-442), the taps
    FirBuilder::resampling(interp, decim) designs."""
    lib = _load()
    n = lib.fsdr_firdes_kaiser_multirate_f32(interp, decim, half_len,
                                             max_ripple, None, 0)
    if n == 0:
        raise FsdrError(lib.fsdr_last_error().decode())
    out = np.zeros(n, np.float32)
    lib.fsdr_firdes_kaiser_multirate_f32(
        interp, decim, half_len, max_ripple,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
    return out


def lowpass_kaiser_n(n_taps, beta, cutoff):
    """firdes::lowpass over a kaiser(n_taps, beta) window (basic.rs:25-42)."""
    lib = _load()
    out = np.zeros(n_taps, np.float32)
    _check(lib.fsdr_firdes_lowpass_kaiser_n_f32(
        n_taps, beta, cutoff,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


def kaiser_beta(max_ripple):
    return _load().fsdr_kaiser_beta(max_ripple)


def _dev_roundtrip(fn, arrays_in, out_dtype, out_items, *extra):
    """Helper: upload arrays, call fn(d_ptrs..., d_out, ...), download."""
    lib = _load()
    ptrs = []
    try:
        for a in arrays_in:
            p = ctypes.c_void_p()
            _check(lib.fsdr_dev_alloc(ctypes.byref(p), max(1, a.nbytes)))
            _check(lib.fsdr_memcpy_h2d(p, ctypes.c_void_p(a.ctypes.data),
                                       a.nbytes))
            ptrs.append(p)
        out = np.zeros(out_items, out_dtype)
        d_out = ctypes.c_void_p()
        _check(lib.fsdr_dev_alloc(ctypes.byref(d_out), max(1, out.nbytes)))
        ptrs.append(d_out)
        produced = fn(ptrs[:-1], d_out, *extra)
        _check(lib.fsdr_synchronize())
        _check(lib.fsdr_memcpy_d2h(ctypes.c_void_p(out.ctypes.data), d_out,
                                   out.nbytes))
        return out, produced
    finally:
        for p in ptrs:
            lib.fsdr_dev_free(p)


def divide_mag_host(a, b):
    lib = _load()
    a = np.ascontiguousarray(a, CF32)
    b = np.ascontiguousarray(b, np.float32)
    n = min(a.size, b.size)

    def call(d_ins, d_out):
        m = ctypes.c_size_t()
        _check(lib.fsdr_divide_mag_dev(d_ins[0], a.size, d_ins[1], b.size,
                                       d_out, n, None, ctypes.byref(m)))
        return m.value

    out, m = _dev_roundtrip(call, [a, b], np.float32, n)
    return out[:m]


def cmul_conj_host(a, b):
    lib = _load()
    a = np.ascontiguousarray(a, CF32)
    b = np.ascontiguousarray(b, CF32)
    n = min(a.size, b.size)

    def call(d_ins, d_out):
        m = ctypes.c_size_t()
        _check(lib.fsdr_cmul_conj_dev(d_ins[0], a.size, d_ins[1], b.size,
                                      d_out, n, None, ctypes.byref(m)))
        return m.value

    out, m = _dev_roundtrip(call, [a, b], CF32, n)
    return out[:m]


def wlan_moving_sum_host(inp, length):
    lib = _load()
    is_c = np.iscomplexobj(inp)
    inp = np.ascontiguousarray(inp, CF32 if is_c else np.float32)
    n_out = inp.size + length - 1  # pad + sums (fresh state)

    def call(d_ins, d_out):
        p = ctypes.c_size_t()
        _check(lib.fsdr_wlan_moving_sum_dev(d_ins[0], inp.size, d_out,
                                            n_out, length, int(is_c), None,
                                            ctypes.byref(p)))
        return p.value

    out, p = _dev_roundtrip(call, [inp], inp.dtype, n_out)
    return out[:p]


class WlanRx:
    """WLAN rx front end host state machines (config 5): SyncShort
    (sync_short.rs:92-150) + SyncLong (sync_long.rs:96-185, GPU 64-tap
    correlator). Stateful like the reference blocks."""

    def __init__(self):
        self._h = _load().fsdr_wlan_rx_create()
        if not self._h:
            raise FsdrError("wlan rx create failed: "
                            + _load().fsdr_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            _load().fsdr_wlan_rx_destroy(self._h)
            self._h = None

    def sync_short(self, sig, abs48, cor, max_tags=64):
        """Returns (frame_samples, tags) where tags is a list of
        (output_index, coarse_freq_offset)."""
        lib = _load()
        sig = np.ascontiguousarray(sig, CF32)
        abs48 = np.ascontiguousarray(abs48, CF32)
        cor = np.ascontiguousarray(cor, np.float32)
        n = min(sig.size, abs48.size, cor.size)
        out = np.zeros(n, CF32)
        tag_idx = np.zeros(max_tags, np.uintp)
        tag_freq = np.zeros(max_tags, np.float32)
        n_tags = ctypes.c_size_t()
        consumed = ctypes.c_size_t()
        prod = lib.fsdr_wlan_sync_short_run(
            self._h, _c(sig), _c(abs48), _c(cor), n, _c(out), out.size,
            _c(tag_idx), _c(tag_freq), max_tags, ctypes.byref(n_tags),
            ctypes.byref(consumed))
        tags = [(int(tag_idx[i]), float(tag_freq[i]))
                for i in range(n_tags.value)]
        return out[:prod], tags

    def sync_long(self, frame_samples, tags, max_frames=16):
        """Returns (symbol_stream, frames) where frames is a list of
        (correlator_offset, fine_freq_offset)."""
        lib = _load()
        x = np.ascontiguousarray(frame_samples, CF32)
        tag_idx = np.array([t[0] for t in tags], np.uintp)
        tag_freq = np.array([t[1] for t in tags], np.float32)
        out = np.zeros(x.size + 128 * max(1, len(tags)), CF32)
        f_off = np.zeros(max_frames, np.uintp)
        f_freq = np.zeros(max_frames, np.float32)
        nf = ctypes.c_size_t()
        prod = lib.fsdr_wlan_sync_long_run(
            self._h, _c(x), x.size, _c(tag_idx), _c(tag_freq),
            len(tags), _c(out), out.size, _c(f_off), _c(f_freq),
            max_frames, ctypes.byref(nf))
        frames = [(int(f_off[i]), float(f_freq[i]))
                  for i in range(nf.value)]
        return out[:prod], frames


class _WlanFrame(ctypes.Structure):
    _fields_ = [
        ("mcs", ctypes.c_uint32),
        ("psdu_size", ctypes.c_uint32),
        ("sym_off", ctypes.c_size_t),
        ("out_off", ctypes.c_size_t),
        ("dec_off", ctypes.c_size_t),
    ]


def wlan_frame_param(mcs, psdu_size):
    """(n_symbols, n_data_bits, n_pad) of FrameParam::new (examples/wlan
    src/lib.rs:324-343); mcs 0..7 = Bpsk_1_2 .. Qam64_3_4. Needs no
    device."""
    if mcs < 0 or psdu_size < 0:
        raise FsdrError("wlan: mcs and psdu_size must not be negative")
    ns, nd, npad = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    _check(_load().fsdr_wlan_frame_param(mcs, psdu_size, ctypes.byref(ns),
                                         ctypes.byref(nd),
                                         ctypes.byref(npad)))
    return ns.value, nd.value, npad.value


def wlan_deinterleave_map(mcs):
    """m (n_cbps entries) with deinterleaved[m[k]] = rx_bits[k] inside one
    symbol (decoder.rs:50-64), read off the kernel's index map. Needs no
    device."""
    if mcs < 0:
        raise FsdrError("wlan: mcs must be in [0,7]")
    out = np.zeros(288, np.uint16)
    _check(_load().fsdr_wlan_deinterleave_map(mcs, _c(out)))
    return out[:(48, 48, 96, 96, 192, 192, 288, 288)[mcs]].astype(np.int64)


def wlan_depuncture_map(mcs, n_symbols, count, first=0):
    """The kernel's source of depunctured values first .. first+count-1 of
    a frame: 8*byte + bit into its index bytes, -1 for an erasure, -2 past
    the frame (reads 0). Needs no device."""
    if mcs < 0 or n_symbols < 0 or count < 0 or first < 0:
        raise FsdrError("wlan: negative argument")
    out = np.zeros(count, np.int32)
    _check(_load().fsdr_wlan_depuncture_map(mcs, n_symbols, first, count,
                                            _c(out)))
    return out


def wlan_signal_field(bits24):
    """(mcs, psdu_size) of the 24 decoded SIGNAL bits (one per element,
    e.g. np.unpackbits of the first three raw decoded bytes), or None as
    the reference's decode_signal_field (frame_equalizer.rs:142-174).
    Needs no device."""
    bits = np.ascontiguousarray(bits24, np.uint8)
    if bits.size != 24:
        raise FsdrError("wlan: the SIGNAL field has 24 bits")
    found, mcs, psdu = ctypes.c_int(), ctypes.c_uint(), ctypes.c_size_t()
    _check(_load().fsdr_wlan_signal_field(_c(bits), ctypes.byref(found),
                                          ctypes.byref(mcs),
                                          ctypes.byref(psdu)))
    return (mcs.value, psdu.value) if found.value else None


class WlanDecoder:
    """The bit work of the reference's WLAN Decoder block (examples/wlan
    src/decoder.rs, viterbi_decoder.rs) for a batch of frames, one frame per
    wavefront: index bytes -> deinterleave -> depuncture -> Viterbi ->
    descramble -> CRC-32. Positions past a frame's own bits read as 0 (see
    include/futuresdr_hip.h)."""

    def __init__(self):
        self._h = _load().fsdr_wlan_decoder_create()
        if not self._h:
            raise FsdrError("wlan decoder create failed: "
                            + _load().fsdr_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            _load().fsdr_wlan_decoder_destroy(self._h)
            self._h = None

    @staticmethod
    def _descs(frames):
        arr = (_WlanFrame * max(1, len(frames)))()
        for d, f in zip(arr, frames):
            if min(f) < 0:
                raise FsdrError("wlan: negative frame field")
            if f[0] > 0xFFFFFFFF or f[1] > 0xFFFFFFFF:
                raise FsdrError("wlan: mcs must be in [0,7], psdu_size at "
                                "most 1528")
            d.mcs, d.psdu_size, d.sym_off, d.out_off, d.dec_off = f
        return arr

    def decode_dev(self, d_syms, frames, d_out_bytes, d_crc_ok,
                   d_dec_bytes=None, stream=None):
        """Device-pointer path (ints = device addresses), asynchronous on
        `stream`. frames: (mcs, psdu_size, sym_off, out_off, dec_off)."""
        frames = list(frames)
        _check(_load().fsdr_wlan_decode_dev(
            self._h, ctypes.c_void_p(d_syms), self._descs(frames),
            len(frames), ctypes.c_void_p(d_out_bytes),
            ctypes.c_void_p(d_dec_bytes or 0), ctypes.c_void_p(d_crc_ok),
            ctypes.c_void_p(stream or 0)))

    def decode(self, frames, raw=False):
        """frames: a sequence of (mcs, psdu_size, uint8 constellation
        indices, 48 per symbol). Returns per frame (out_bytes, crc_ok), with
        raw=True (out_bytes, crc_ok, dec_bytes): out_bytes is the psdu_size+2
        descrambled bytes (two SERVICE bytes, then the PSDU), dec_bytes the
        ceil(n_data_bits/8) Viterbi bytes before descrambling."""
        frames = [(int(m), int(p), np.ascontiguousarray(s, np.uint8))
                  for m, p, s in frames]
        descs, so, oo, do = [], 0, 0, 0
        for m, p, s in frames:
            if m < 0 or m > 7 or p < 0 or p > 1528:
                raise FsdrError("wlan: mcs must be in [0,7], psdu_size at "
                                "most 1528")
            ns, nd, _ = wlan_frame_param(m, p)
            if s.size != 48 * ns:
                raise FsdrError(f"wlan: frame needs {48 * ns} indices, "
                                f"got {s.size}")
            descs.append((m, p, so, oo, do))
            so, oo, do = so + s.size, oo + p + 2, do + (nd + 7) // 8
        if not frames:
            return []
        syms = np.concatenate([s.reshape(-1) for _, _, s in frames])
        out = np.zeros(oo, np.uint8)
        dec = np.zeros(do, np.uint8) if raw else None
        crc = np.zeros(len(frames), np.uint8)
        _check(_load().fsdr_wlan_decode_host(
            self._h, _c(syms), self._descs(descs), len(descs), _c(out),
            _c(dec) if raw else None, _c(crc)))
        res = []
        for i, (m, p, so, oo, do) in enumerate(descs):
            r = (out[oo:oo + p + 2].copy(), bool(crc[i]))
            if raw:
                nd = wlan_frame_param(m, p)[1]
                r += (dec[do:do + (nd + 7) // 8].copy(),)
            res.append(r)
        return res


class _WlanEqFrame(ctypes.Structure):
    _fields_ = [
        ("sym_off", ctypes.c_size_t),
        ("n_avail", ctypes.c_uint32),
        ("idx_off", ctypes.c_size_t),
        ("eq_off", ctypes.c_size_t),
    ]


class _WlanEqInfo(ctypes.Structure):
    _fields_ = [
        ("found", ctypes.c_uint32),
        ("mcs", ctypes.c_uint32),
        ("psdu_size", ctypes.c_uint32),
        ("n_symbols", ctypes.c_uint32),
        ("n_copied", ctypes.c_uint32),
        ("snr_db", ctypes.c_float),
    ]


WLAN_EQ_INFO_DTYPE = np.dtype([("found", np.uint32), ("mcs", np.uint32),
                               ("psdu_size", np.uint32),
                               ("n_symbols", np.uint32),
                               ("n_copied", np.uint32),
                               ("snr_db", np.float32)])

WlanEqInfo = collections.namedtuple(
    "WlanEqInfo", "found mcs psdu_size n_symbols n_copied snr_db")


def _wlan_eq_info(rec):
    return WlanEqInfo(bool(rec["found"]), int(rec["mcs"]),
                      int(rec["psdu_size"]), int(rec["n_symbols"]),
                      int(rec["n_copied"]), float(rec["snr_db"]))


def wlan_demap(mcs, z):
    """Constellation indices of the values z by the reference's
    Modulation::demap (lib.rs:177-218), the function the equalizer kernel
    uses. Needs no device."""
    if mcs < 0:
        raise FsdrError("wlan: mcs must be in [0,7]")
    z = np.ascontiguousarray(z, CF32).reshape(-1)
    out = np.zeros(z.size, np.uint8)
    _check(_load().fsdr_wlan_demap(mcs, _c(z), z.size, _c(out)))
    return out


def wlan_pilot_polarity(count, first=0):
    """POLARITY[(first + i) % 127] for i < count as +1 / -1 (lib.rs:365),
    generated from the scrambler as the kernel does. Needs no device."""
    if count < 0 or first < 0:
        raise FsdrError("wlan: negative argument")
    out = np.zeros(count, np.int8)
    _check(_load().fsdr_wlan_pilot_polarity(first, count, _c(out)))
    return out


def wlan_carrier_map():
    """Output position of each of the 64 carriers in a symbol's 48 values,
    -1 for pilots, DC and guards (frame_equalizer.rs:55-57). Needs no
    device."""
    out = np.zeros(64, np.int8)
    _check(_load().fsdr_wlan_carrier_map(_c(out)))
    return out


class WlanEqualizer:
    """The reference's WLAN FrameEqualizer (examples/wlan src/
    frame_equalizer.rs) for a batch of frames: channel estimate, pilot
    phase, SIGNAL field, equalize and demap (see include/futuresdr_hip.h).
    Input is the plain 64-point FFT of WlanRx.sync_long's stream."""

    def __init__(self):
        self._h = _load().fsdr_wlan_equalizer_create()
        if not self._h:
            raise FsdrError("wlan equalizer create failed: "
                            + _load().fsdr_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            _load().fsdr_wlan_equalizer_destroy(self._h)
            self._h = None

    @staticmethod
    def _descs(frames):
        arr = (_WlanEqFrame * max(1, len(frames)))()
        for d, f in zip(arr, frames):
            if min(f) < 0 or f[1] > 0xFFFFFFFF:
                raise FsdrError("wlan: frame field out of range")
            d.sym_off, d.n_avail, d.idx_off, d.eq_off = f
        return arr

    def equalize_dev(self, d_spec, frames, d_idx, d_info, d_eq=None,
                     stream=None):
        """Device-pointer path (ints = device addresses), asynchronous on
        `stream`. frames: (sym_off, n_avail, idx_off, eq_off)."""
        frames = list(frames)
        _check(_load().fsdr_wlan_equalize_dev(
            self._h, ctypes.c_void_p(d_spec), self._descs(frames),
            len(frames), ctypes.c_void_p(d_idx), ctypes.c_void_p(d_eq or 0),
            ctypes.c_void_p(d_info), ctypes.c_void_p(stream or 0)))

    def equalize(self, spec, frames, symbols=False):
        """spec: the cf32 FFT stream; frames: (sym_off, n_avail) pairs in
        items of it. Returns per frame (info, indices), with symbols=True
        (info, indices, eq_symbols): info is a WlanEqInfo, indices the
        48*n_copied constellation indices, eq_symbols as many equalized
        values."""
        spec = np.ascontiguousarray(spec, CF32).reshape(-1)
        descs, off = [], 0
        for so, na in frames:
            so, na = int(so), int(na)
            if so < 0 or na < 0 or so + 64 * na > spec.size:
                raise FsdrError("wlan: frame outside the spectrum stream")
            descs.append((so, na, off, off))
            off += 48 * max(na - 3, 0)
        if not descs:
            return []
        idx = np.zeros(max(off, 1), np.uint8)
        eqs = np.zeros(max(off, 1), CF32) if symbols else None
        info = np.zeros(len(descs), WLAN_EQ_INFO_DTYPE)
        _check(_load().fsdr_wlan_equalize_host(
            self._h, _c(spec), self._descs(descs), len(descs), _c(idx),
            _c(eqs) if symbols else None, _c(info)))
        res = []
        for rec, (_, _, o, _) in zip(info, descs):
            n = 48 * int(rec["n_copied"])
            r = (_wlan_eq_info(rec), idx[o:o + n].copy())
            if symbols:
                r += (eqs[o:o + n].copy(),)
            res.append(r)
        return res


def wlan_frame_spans(tags, frames, n_samples):
    """(sym_off, n_avail) in the FFT stream of every frame that one
    WlanRx.sync_long(frame_samples, tags) call produced: tags as passed to
    it, frames as it returned them, n_samples = frame_samples.size. The
    rule is the state machine's: a tag with fewer than 448 samples to the
    next tag (or to the end) yields no frame; a frame yields 128 items plus
    64 per whole 80 samples behind them. One-shot only: it does not
    describe a stream fed to sync_long in several calls."""
    spans, off, j = [], 0, 0
    for t, (start, _) in enumerate(tags):
        end = tags[t + 1][0] if t + 1 < len(tags) else n_samples
        if end - start < 320 + 128 or j >= len(frames):
            continue
        n_sym = (end - (start + frames[j][0] + 128)) // 80
        spans.append((off, 2 + n_sym))
        off += 128 + 64 * n_sym
        j += 1
    return spans


def wlan_receive(spec, spans):
    """Spectra to bytes: equalize the frames `spans` ((sym_off, n_avail)
    pairs) of the FFT stream `spec`, then decode on the device every frame
    that is found, complete (n_copied == n_symbols) and within the
    decoder's limits (psdu <= 1528, <= 511 symbols), reading the index
    buffer where the equalizer wrote it. Returns per frame (info,
    psdu_bytes or None, crc_ok)."""
    lib = _load()
    spec = np.ascontiguousarray(spec, CF32).reshape(-1)
    descs, off = [], 0
    for so, na in spans:
        so, na = int(so), int(na)
        if so < 0 or na < 0 or so + 64 * na > spec.size:
            raise FsdrError("wlan: frame outside the spectrum stream")
        descs.append((so, na, off, 0))
        off += 48 * max(na - 3, 0)
    if not descs:
        return []
    info = np.zeros(len(descs), WLAN_EQ_INFO_DTYPE)
    ptrs = []

    def alloc(nbytes):
        p = ctypes.c_void_p()
        _check(lib.fsdr_dev_alloc(ctypes.byref(p), max(1, nbytes)))
        ptrs.append(p)
        return p

    try:
        d_spec, d_idx = alloc(spec.nbytes), alloc(off)
        d_info = alloc(info.nbytes)
        _check(lib.fsdr_memcpy_h2d(d_spec, _c(spec), spec.nbytes))
        eq = WlanEqualizer()  # alive until its work has finished
        eq.equalize_dev(d_spec.value, descs, d_idx.value, d_info.value)
        _check(lib.fsdr_synchronize())
        _check(lib.fsdr_memcpy_d2h(_c(info), d_info, info.nbytes))
        dec, which, oo = [], [], 0
        for i, (rec, d) in enumerate(zip(info, descs)):
            if rec["found"] and rec["n_copied"] == rec["n_symbols"] and \
                    rec["psdu_size"] <= 1528 and rec["n_symbols"] <= 511:
                dec.append((int(rec["mcs"]), int(rec["psdu_size"]), d[2],
                            oo, 0))
                which.append(i)
                oo += int(rec["psdu_size"]) + 2
        out = np.zeros(max(oo, 1), np.uint8)
        crc = np.zeros(max(len(dec), 1), np.uint8)
        if dec:
            d_out, d_crc = alloc(out.nbytes), alloc(crc.nbytes)
            decoder = WlanDecoder()
            decoder.decode_dev(d_idx.value, dec, d_out.value, d_crc.value)
            _check(lib.fsdr_synchronize())
            _check(lib.fsdr_memcpy_d2h(_c(out), d_out, out.nbytes))
            _check(lib.fsdr_memcpy_d2h(_c(crc), d_crc, crc.nbytes))
    finally:
        for p in ptrs:
            lib.fsdr_dev_free(p)
    res = [(_wlan_eq_info(rec), None, False) for rec in info]
    for k, (i, (_, psdu, _, o, _)) in enumerate(zip(which, dec)):
        res[i] = (res[i][0], out[o + 2:o + 2 + psdu].copy(), bool(crc[k]))
    return res


def cmul_host(a, b):
    lib = _load()
    a = np.ascontiguousarray(a, CF32)
    b = np.ascontiguousarray(b, CF32)
    m = min(a.size, b.size)
    out = np.zeros(m, CF32)
    mm = ctypes.c_size_t()
    _check(lib.fsdr_cmul_host(ctypes.c_void_p(a.ctypes.data), a.size,
                              ctypes.c_void_p(b.ctypes.data), b.size,
                              ctypes.c_void_p(out.ctypes.data), out.size,
                              ctypes.byref(mm)))
    return out[: mm.value]


def fill_uniform_dev(d_ptr, n, seed=0, offset=0, stream=None):
    _check(_load().fsdr_fill_uniform_cf32(ctypes.c_void_p(d_ptr), n, seed,
                                          offset,
                                          ctypes.c_void_p(stream or 0)))
