/* futuresdr_hip.h — C-ABI of the MI355X-native FutureSDR streaming-DSP hot
 * path. This is the drop-in boundary: plain pointers and
 * sizes, no framework types. A FutureSDR maintainer binds these symbols from
 * Rust with a plain `extern "C"` block.
 *
 * Contract mirrored, per entry point:
 *  - fsdr_filter_host/_dev mirror `futuredsp::Filter::filter(&self, &[I],
 *    &mut [O]) -> (usize, usize, ComputationStatus)` —
 *    /root/reference/crates/futuredsp/src/lib.rs:48-68. Same
 *    consumed/produced/status math as the cores they replace:
 *      fir:    crates/futuredsp/src/fir.rs:52-91
 *      decim:  crates/futuredsp/src/decimating_fir.rs:53-95
 *      resamp: crates/futuredsp/src/polyphase_resampling_fir.rs:70-124
 *      fft:    src/blocks/fft.rs:160-221 (m = min(in,out) rounded to len,
 *              capped at 32*len; consumed == produced == m)
 *      mag2:   src/blocks/apply.rs:100-131 (m = min(in,out))
 *      cmul:   src/blocks/combine.rs:92-135 (m = min(in0,in1,out))
 *  - fsdr_ring_* mirror the Slab stream-buffer circulation
 *    (src/runtime/buffer/slab.rs:110-152,369-399) and the accelerator
 *    buffer pattern (src/runtime/buffer/vulkan/{h2d,d2h}.rs,
 *    src/runtime/buffer/wgpu): N pinned-host buffers cycling empty<->full
 *    with a reserved-items history prefix.
 *  - fsdr_chain_* is the fused pipeline runner (the `fsdr_chain_run` of
 *    SURVEY.md §8b).
 *
 * Failure convention: int status + thread-local error string
 * (fsdr_last_error). The Rust Filter trait has no error path (lib.rs:60-64);
 * the ABI's failures are device/allocation errors only. All compute entry
 * points fail with FSDR_ERR_NO_GPU when no HIP device is present — there is
 * NO CPU fallback in the product (the CPU restatement lives in oracle/,
 * which is test infrastructure).
 *
 * Threading: a handle may be used from one thread at a time (same as the
 * reference, where one block owns its kernel). Distinct handles are
 * independent. `stream` parameters take a hipStream_t (or NULL for the
 * default stream) so callers (e.g. torch) can pass their own streams.
 */
#ifndef FUTURESDR_HIP_H
#define FUTURESDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Complex32 — layout-identical to num_complex::Complex<f32> (re, im). */
typedef struct { float re, im; } fsdr_cf32;

/* ComputationStatus — crates/futuredsp/src/lib.rs:31-45 */
typedef enum {
    FSDR_INSUFFICIENT_INPUT  = 0,
    FSDR_INSUFFICIENT_OUTPUT = 1,
    FSDR_BOTH_SUFFICIENT     = 2,
} fsdr_status;

typedef struct {
    size_t      consumed;
    size_t      produced;
    fsdr_status status;
} fsdr_filter_result;

/* Error codes (returned by every int-returning entry point). */
enum {
    FSDR_OK              = 0,
    FSDR_ERR_NO_GPU      = 1,
    FSDR_ERR_HIP         = 2,
    FSDR_ERR_INVALID     = 3,
    FSDR_ERR_UNSUPPORTED = 4,
};

/* ---- device management ---------------------------------------------- */
int         fsdr_device_count(void);
int         fsdr_set_device(int device);
int         fsdr_synchronize(void);
const char* fsdr_last_error(void);
const char* fsdr_version(void);

/* ---- Filter level ---------------------------------------------------- *
 * Opaque stateless-filter handle (GPU-backed). Replaces the futuredsp
 * cores behind the same span semantics. item types are fixed per
 * constructor; *_host paths stage through persistent device buffers
 * (PCIe-inclusive), *_dev paths take caller device pointers. */
typedef struct fsdr_filter fsdr_filter;

/* FirFilter<Complex32,Complex32,f32> — fir.rs:228-255 (f32 taps). */
fsdr_filter* fsdr_fir_cf32_create(const float* taps, size_t n_taps);
/* FirFilter<f32,f32,f32> — fir.rs:206-215. */
fsdr_filter* fsdr_fir_f32_create(const float* taps, size_t n_taps);
/* FirFilter<Complex32,Complex32,Complex32> — fir.rs:257-277 (complex
 * taps; the WLAN SyncLong correlator core, sync_long.rs:18-50). */
fsdr_filter* fsdr_fir_ccf32_create(const fsdr_cf32* taps, size_t n_taps);
/* DecimatingFirFilter<Complex32,Complex32,f32> — decimating_fir.rs. */
fsdr_filter* fsdr_decim_fir_cf32_create(size_t decimation,
                                        const float* taps, size_t n_taps);
/* PolyphaseResamplingFir<Complex32,Complex32,f32> — n_taps must be a
 * multiple of interp (polyphase_resampling_fir.rs:54-56 assert). */
fsdr_filter* fsdr_resamp_cf32_create(size_t interp, size_t decim,
                                     const float* taps, size_t n_taps);
/* PolyphaseResamplingFir<f32,f32,f32> — polyphase_resampling_fir.rs:
 * 126-141: the index math (:108-118) and consumed/produced/status
 * (:90-106) of the Complex32 handle on 4-byte items in and out; same
 * n_taps % interp assert. The audio resampler of the FM receiver
 * (examples/fm-receiver/src/main.rs:121-123). Spans that fit run an
 * LDS-tiled kernel, longer ones a one-output-per-lane kernel
 * (FSDR_RESAMP_TILED=0 forces the latter). */
fsdr_filter* fsdr_resamp_f32_create(size_t interp, size_t decim,
                                    const float* taps, size_t n_taps);
/* Quadrature demodulator — the stateful Apply<Complex32 -> f32> of
 * examples/fm-receiver/src/main.rs:99-104: d[i] = arg(x[i]*conj(x[i-1])),
 * x[-1] the carried `last`, (0,0) on a fresh handle. Counts follow
 * src/blocks/apply.rs:100-131 (m = min(in,out), consumed == produced == m,
 * BOTH_SUFFICIENT); length() is 1. `last` lives in device memory and is
 * updated from d_in[m-1] on the caller's stream after the kernel, with no
 * host sync (no update when m == 0). The product is formed as num_complex
 * does, each operation rounded on its own, so the first sample of a stream
 * (last = 0+0i, conj = (+0,-0)) has the reference's signed-zero result:
 * +0, -0, +0 or pi by the sign quadrant of x[0]. */
fsdr_filter* fsdr_quad_demod_create(void);
/* Fused FM back end, Complex32 in, f32 out: fsdr_quad_demod followed by
 * fsdr_resamp_f32 on the demodulated stream (main.rs:99-104,121-129,
 * `demod > resamp2`). consumed/produced/status are the resampler's
 * (polyphase_resampling_fir.rs:90-106) with consumed counting Complex32
 * inputs; `last` becomes x[consumed-1] and stays when consumed == 0. The
 * caller re-presents unconsumed inputs, and since d[i] depends on x[i]
 * and x[i-1] alone the output stream is that of the two-block flowgraph
 * under any chunking, bit for bit. One kernel demodulates a tile's input
 * span into LDS (atan2f once per input sample) and runs the polyphase dot
 * products from there; where the span exceeds the LDS budget, or with
 * FSDR_FM_FUSED=0, the handle demodulates into scratch and launches the
 * f32 resampler kernels. _fused: which of the two a handle takes now
 * (1 fused; diagnostics/tests; host-only). */
fsdr_filter* fsdr_fm_demod_resamp_create(size_t interp, size_t decim,
                                         const float* taps, size_t n_taps);
int fsdr_fm_demod_resamp_fused(const fsdr_filter* f);
/* IirFilter<f32,f32,_> — crates/futuredsp/src/iir.rs:56-178, the crate's
 * one StatefulFilter: y[k] = sum_j b[j]*in[k+n_b-1-j] + sum_j a[j]*y[k-1-j]
 * with `memory` (memory[j] = y[-1-j]) carried in device memory. One call
 * is taps_accessor_work (:79-178) literally:
 *  - n_in == 0 returns (0, 0).
 *  - While memory holds fewer than n_a samples it is filled from
 *    in[memory.len()] of this call's input (:102-118); a call whose input
 *    ends inside the fill, or is no longer than the pushes it made,
 *    returns (0, 0) and keeps the pushes (:105-129). The fill consumes
 *    nothing: the first n_a inputs of a stream are both the initial
 *    "previous outputs" and ordinary inputs. The handle mirrors this with
 *    a host-side fill count and device-to-device copies.
 *  - n = n_in >= n_b ? min(n_in - (n_b-1), n_out) : 0 outputs, consumed ==
 *    produced == n; BOTH_SUFFICIENT if n == n_in == n_out, else
 *    INSUFFICIENT_OUTPUT if n < n_in (for n_b > 1 every input-limited call;
 *    the reference's quirk, kept), else INSUFFICIENT_INPUT. A (0, 0) return
 *    of the first two cases is BOTH_SUFFICIENT for n_out == 0 and
 *    INSUFFICIENT_INPUT otherwise.
 *  - memory becomes y[n-1-j] for j < n and the old memory[j-n] beyond: a
 *    call with n < n_a shifts it. length() is n_b.
 * fsdr_iir_count is that accounting alone for a memory of `filled`
 * samples, host-only.
 * Limits: n_b in [1,64] (n_b == 0 is the reference's assert), n_a in
 * [0,8] (n_a == 0 is a FIR with these counts); outside, NULL plus an error
 * string. An in-place call (d_out == d_in) returns FSDR_ERR_INVALID.
 * The recurrence is run blocked ("IIR"): a lane walks a chunk
 * of outputs from zero state, chunk end states are combined over a tile,
 * and tile end states over the call, by doubling scans with constant
 * powers of the companion matrix A of `a` (first row a, ones below the
 * diagonal). Results differ from the serial loop by rounding only, inside
 * the bound tests/iir_ref.py states. All work is enqueued on `stream`
 * without a host sync; no block waits for another.
 * The plan holds those constants, computed in double from `a` alone and
 * rounded to f32 once; host-only, needs no GPU.
 *  _create: FSDR_ERR_INVALID for n_a > 8; FSDR_ERR_UNSUPPORTED where a
 *    table entry is not finite in f32, which covers a pole outside the
 *    unit circle. A deliberate deviation: the reference runs such a filter
 *    until it overflows. Poles on the unit circle are supported.
 *  _info: outputs per chunk L, chunks per tile, outputs per tile, and the
 *    tile states one pass of the tile scan covers (a longer call chains
 *    passes). NULL out-pointers are skipped.
 *  _tables: H[i*n_a+q] = (A^(i+1))[0][q] for i < L; chunk_pow[d] =
 *    A^(L*2^d) for d < log2(chunks per tile); tile_pow[d] = A^(tile*2^d)
 *    for d < log2(tile states per pass); matrices row-major n_a x n_a.
 *    The entries are the doubles the plan computed; the kernels read each
 *    one rounded to f32, i.e. (float)entry. NULL out-pointers are skipped.
 * fsdr_filter_variant reports zeros for this handle. */
typedef struct fsdr_iir_plan fsdr_iir_plan;
int fsdr_iir_plan_create(const float* a, size_t n_a, fsdr_iir_plan** out);
void fsdr_iir_plan_destroy(fsdr_iir_plan* p);
int fsdr_iir_plan_info(const fsdr_iir_plan* p, size_t* chunk_len,
                       size_t* chunks_per_tile, size_t* tile,
                       size_t* scan_pass_tiles);
int fsdr_iir_plan_tables(const fsdr_iir_plan* p, double* H,
                         double* chunk_pow, double* tile_pow);
void fsdr_iir_count(size_t n_a, size_t n_b, size_t filled, size_t n_in,
                    size_t n_out, size_t* filled_after, size_t* consumed,
                    size_t* produced, int* status);
fsdr_filter* fsdr_iir_f32_create(const float* a, size_t n_a, const float* b,
                                 size_t n_b);
const fsdr_iir_plan* fsdr_iir_plan_of(const fsdr_filter* f);
/* LoRa FFT demodulator — the arithmetic of examples/lora FftDemod
 * (src/fft_demod.rs) and of FrameSync's get_symbol_val (src/utils.rs:
 * 1059-1078) in one kernel: a symbol of N = 2^sf Complex32 samples times
 * the handle's downchirp table, N-point forward unnormalized FFT, |X|^2 =
 * re*re + im*im in f32, and a reduction over the bins fixed per handle:
 *  FSDR_LORA_RAW   u16 out: argmax under max_by(total_cmp), the LAST of
 *    equal maxima (utils.rs:1101-1109), or 0xFFFF (the reference's None)
 *    where the f64 sum of the bins is exactly 0.
 *  FSDR_LORA_HARD  u16 out: ((argmax - 1) mod N) / (reduced_rate ? 4 : 1)
 *    (fft_demod.rs:115-120, 238-248); no zero-energy case.
 *  FSDR_LORA_SOFT  double[12] out: compute_llrs' max-log branch
 *    (fft_demod.rs:126-208; max_log_approx is hard-wired true at :278) in
 *    f64 on the f32 magnitudes: bins with (|i - argmax| mod (N-1)) < 2 are
 *    signal, ps = signal/N, pn = noise/(N-3), a_n = sqrt(ps)/pn *
 *    sqrt(N*mag_n), ll_n = ln I0(a_n), or N*mag_n for every bin where any
 *    a_n >= 709; for bit i < sf, with s = gray(((n-1) mod N) /
 *    (reduced_rate ? 4 : 1)), out[sf-1-i] = max over bins with bit i of s
 *    set minus max over the others, both maxima starting at 0; out[sf..11]
 *    = 0. NaN/Inf input and all-zero input (pn = 0) are unspecified.
 * _create: sf in [5,12] and one of the modes, else NULL plus an error
 *   string. The handle is an fsdr_filter: fsdr_filter_host/_dev, _destroy
 *   and fsdr_fg_add_filter take it; length() is N (set_min_items,
 *   fft_demod.rs:269), items are 8 bytes in and 2 or 96 bytes out, and one
 *   call returns produced = min(n_in / N, n_out), consumed = produced * N
 *   with the decimating-FIR status rule for D = N and one tap. A trailing
 *   partial symbol is never read and nothing is written past `produced`.
 *   The kernel is stateless across symbols.
 * _set_frame: the per-frame state the reference takes from the frame_info
 *   tag (fft_demod.rs:355-399); the caller computes reduced_rate as :72-75
 *   does. Rebuilds the table on the host in f64 and uploads it with a
 *   blocking copy: call it between frames, not while a call that uses the
 *   old table is in flight on a non-blocking stream. A fresh handle has
 *   cfo 0 and reduced_rate 0. RAW ignores reduced_rate; its table is the
 *   downchirp of build_ref_chirps (utils.rs:1053-1057) under the same
 *   rotation. Tag parsing, the 4+cr symbol blocking and the frame-sync
 *   state machine stay with the caller.
 * fsdr_lora_downchirp (host-only): the HARD/SOFT table, N entries —
 *   build_upchirp(0, sf, 1, false) (utils.rs:884-914) in f32 arithmetic in
 *   the reference's operation order, conjugated in f64 (the constructor
 *   path fft_demod.rs:280-283; set_sf at :54-57 omits the conjugate and is
 *   out of scope, the handle's sf being fixed), rotated by
 *   e^{-2 pi i (cfo_int + cfo_frac)/N * j} in f64, rounded to f32.
 * fsdr_lora_log_i0 (host-only): the ln I0 evaluator the SOFT kernel runs.
 * fsdr_lora_demod_count (host-only): the counts of one call alone.
 * _downchirp and _count return FSDR_ERR_INVALID for sf outside [5,12]. */
enum { FSDR_LORA_RAW = 0, FSDR_LORA_HARD = 1, FSDR_LORA_SOFT = 2 };
fsdr_filter* fsdr_lora_demod_create(unsigned sf, int mode);
int fsdr_lora_demod_set_frame(fsdr_filter* f, long long cfo_int,
                              double cfo_frac, int reduced_rate);
int fsdr_lora_downchirp(unsigned sf, long long cfo_int, double cfo_frac,
                        fsdr_cf32* out);
double fsdr_lora_log_i0(double x);
int fsdr_lora_demod_count(unsigned sf, size_t n_in, size_t n_out,
                          size_t* consumed, size_t* produced, int* status);
/* Fft block — pow2 lengths in [4,4096] run the radix-4 Stockham kernel;
 * ANY other length in [2,2048] runs via Bluestein (two pow2 M>=2len-1
 * passes; the reference block is generic over rustfft plan lengths,
 * fft.rs:98-103). inverse/fft_shift flags and optional normalize factor
 * as src/blocks/fft.rs:92-121. */
fsdr_filter* fsdr_fft_cf32_create(size_t len, int inverse, int fft_shift,
                                  const float* normalize);
/* Apply |x|^2 (Complex32 -> f32) — the spectrum mag^2 map. */
fsdr_filter* fsdr_mag2_create(void);
/* XlatingFir (src/blocks/xlating_fir.rs): rotate-by-offset + filter +
 * decimate, fused: DecimatingFir with complex band-pass taps
 * (bpf[i] = e^{i*TAU*offset/fs*i}*taps[i]) and the output Rotator
 * (phase_incr = -TAU*offset*decimation/fs); rotator phase is carried
 * state. decimation must be >= 2 (xlating_fir.rs:44). */
fsdr_filter* fsdr_xlating_fir_cf32_create(const float* taps, size_t n_taps,
                                          size_t decimation, float offset,
                                          float sample_rate);
/* MovingAvg block (src/blocks/moving_avg.rs:79-118): stateful per-bin
 * EMA over width-sized f32 frames, emitting every `history` frames. */
fsdr_filter* fsdr_moving_avg_create(size_t width, float decay_factor,
                                    size_t history);
/* Host-side planning the MovingAvg call does, exposed for tests (no GPU
 * required). _count: frames consumed / spectra produced / new emission
 * phase of one work() call from phase *i_state (< history). _plan: the
 * single-emission fast path's chunking of `frames` frames (frames per
 * chunk, chunk count) and the first chunk inside the EMA's frame horizon
 * (returned; 0 when skip == 0 or nothing can be skipped). */
void fsdr_moving_avg_count(size_t in_frames, size_t out_frames,
                           size_t history, size_t* i_state,
                           size_t* consumed, size_t* produced);
int fsdr_moving_avg_plan(size_t frames, float decay_factor, int skip,
                         int* chunk_frames, int* n_chunks);

/* Filter::length() — lib.rs:65-67. */
size_t fsdr_filter_length(const fsdr_filter* f);

/* Which kernel instantiation the handle's launches select: the MFMA K,
 * the 32x32-MFMA K and the scalar template tap count fixed at create (0 =
 * that family does not apply; all three 0 = the untemplated kernel). A
 * resampler reports its 1:4 decimating sub-filter, or zeros without one.
 * NULL out-pointers are skipped (diagnostics/tests; host-only). */
int fsdr_filter_variant(const fsdr_filter* f, int* kk_mfma, int* kk_mfma32,
                        int* tp_tpl);

/* filter() over host spans. Stages H2D/D2H internally. */
int fsdr_filter_host(fsdr_filter* f, const void* in, size_t n_in,
                     void* out, size_t n_out, fsdr_filter_result* r);
/* filter() over device pointers, async on `stream` (no sync performed;
 * the result math is computed on the host and returns immediately). */
int fsdr_filter_dev(fsdr_filter* f, const void* d_in, size_t n_in,
                    void* d_out, size_t n_out, void* stream,
                    fsdr_filter_result* r);
/* Bulk batch FFT over `frames` fft_len-sized device-resident frames in
 * one launch (the 32-frame cap in fsdr_filter_dev mirrors the reference
 * work() quantum, fft.rs:56 — this is the GPU-native batch path the
 * chain uses). d_mag: optional fused |X|^2 output (nullable). */
int fsdr_fft_bulk_dev(fsdr_filter* f, const void* d_in, void* d_out,
                      void* d_mag, size_t frames, void* stream);
void fsdr_filter_destroy(fsdr_filter* f);

/* Combine (2-input zip-map), complex-multiply variant. m = produced. */
int fsdr_cmul_dev(const void* d_a, size_t n_a, const void* d_b, size_t n_b,
                  void* d_out, size_t n_out, void* stream, size_t* m);
int fsdr_cmul_host(const void* a, size_t n_a, const void* b, size_t n_b,
                   void* out, size_t n_out, size_t* m);

/* Rotator (futuredsp rotator.rs:23-49): out[i] = in[i] * phase0 *
 * e^{i*angle*(i+1)}, closed-form phase (the reference iterates — see the
 * parity note in tests/test_gpu_parity.py). Returns the final phase. */
int fsdr_rotator_dev(const void* d_in, void* d_out, size_t n,
                     float phase_incr_angle, float phase0_re,
                     float phase0_im, void* stream, float* final_re,
                     float* final_im);

/* PfbChannelizer (src/blocks/pfb/channelizer.rs, liquid-dsp scheme):
 * splits a Complex32 stream into num_channels frequency channels.
 * Supports any oversample_rate = N/i (decimation D = N/oversample,
 * channelizer.rs:100-105); num_channels must be a power of two in
 * [4,4096] (FFT kernel). Output is channel-major:
 * out[c*out_cap_per_chan + k]. The first N*tpf samples (tpf =
 * ceil(n_taps/N)) only fill the windows; every D samples after them give
 * one output step, min(out_cap_per_chan, remaining/D) steps per call, and
 * nothing is written past them. run_dev = bulk from zero state;
 * stream_dev carries the round-robin window state across calls and
 * consumes in D quanta after the N*tpf prefill (pair with the ring's
 * release_consumed carry for exact arbitrary-chunk streaming). Where the
 * reference needs one work() call to finish the fill and a second to
 * produce, one call here does both.
 * Start-up steps. The reference's windows are WindowBuffer::new(tpf,
 * false): fill push k of a window lands at slot 2k mod tpf
 * (window_buffer.rs:23-32), so a just-filled window is a shuffle of its
 * fill pushes (even tpf: half the slots still zero, half the pushes
 * lost; odd tpf: a permutation) until tpf further pushes have rewritten
 * every slot. Output step k is the textbook polyphase sum only once
 * (k+1)*D >= tpf*N; the tpf*N/D - 1 steps in front of it are computed
 * from the shuffled windows, as the reference computes them (none when
 * tpf = 1). stream_dev keeps every consumed sample until the stream has
 * 2*N*tpf pushes for this. _window_map: src[w] = which of its window's
 * pushes (0 = first fill push) slice position w, 0 = oldest, holds after
 * tpf fill pushes and q more, -1 for a hole; host-only. */
fsdr_filter* fsdr_pfb_channelizer_create(size_t num_channels,
                                         const float* taps, size_t n_taps,
                                         float oversample_rate);
void fsdr_pfb_channelizer_window_map(size_t taps_per_filter, size_t q,
                                     long long* src);
int fsdr_pfb_channelizer_run_dev(fsdr_filter* f, const void* d_in,
                                 size_t n_in, void* d_out,
                                 size_t out_cap_per_chan, void* stream,
                                 size_t* produced_per_chan);
int fsdr_pfb_channelizer_stream_dev(fsdr_filter* f, const void* d_chunk,
                                    size_t n, void* d_out,
                                    size_t out_cap_per_chan, void* stream,
                                    size_t* produced_per_chan,
                                    size_t* consumed);

/* PfbSynthesizer (src/blocks/pfb/synthesizer.rs:59-143): recombines
 * num_channels Complex32 channel streams into one stream at N times the
 * channel rate — per step an unnormalized inverse DFT across the
 * channels, then each output phase c through its polyphase filter
 * part[c][j] = taps[c + j*N] (tpf = ceil(n_taps/N) taps). num_channels
 * must be a power of two in [4,4096] (FFT kernel) and n_taps >=
 * num_channels (the reference's pad count underflows otherwise); a
 * violation returns NULL with an error string.
 * Input is channel-major, in[c*in_stride + t], n_in_per_chan <= in_stride
 * steps per channel — the layout fsdr_pfb_channelizer_* writes with
 * out_cap_per_chan as the stride. Output is the interleaved stream: the
 * first tpf-1 steps of a stream only fill the windows, every later step
 * emits N samples. consumed/produced follow the reference work() loop
 * (a step past the filling one runs only while MORE than N output slots
 * are free); _count is that arithmetic alone, host-only, for a handle
 * that has consumed `pushes` steps so far. One deviation: where the
 * reference would index out of range (the filling step with fewer than N
 * free slots), the call stops in front of that step and returns FSDR_OK.
 * run_dev = bulk from zero state, leaves the streaming state alone;
 * stream_dev carries the window contents and the push count across
 * calls, and the caller re-presents unconsumed steps. All work is
 * enqueued on `stream` without a host sync. _run_length: steps one block
 * of the fused kernel owns for (num_channels, taps_per_filter), 0 where
 * only the staged path applies (diagnostics/tests; host-only). */
fsdr_filter* fsdr_pfb_synthesizer_create(size_t num_channels,
                                         const float* taps, size_t n_taps);
void fsdr_pfb_synthesizer_count(size_t num_channels, size_t taps_per_filter,
                                size_t pushes, size_t n_in_per_chan,
                                size_t out_cap, size_t* consumed_per_chan,
                                size_t* produced);
size_t fsdr_pfb_synthesizer_run_length(size_t num_channels,
                                       size_t taps_per_filter);
int fsdr_pfb_synthesizer_run_dev(fsdr_filter* f, const void* d_in,
                                 size_t in_stride, size_t n_in_per_chan,
                                 void* d_out, size_t out_cap, void* stream,
                                 size_t* consumed_per_chan, size_t* produced);
int fsdr_pfb_synthesizer_stream_dev(fsdr_filter* f, const void* d_in,
                                    size_t in_stride, size_t n_in_per_chan,
                                    void* d_out, size_t out_cap,
                                    void* stream, size_t* consumed_per_chan,
                                    size_t* produced);

/* PfbArbResampler (src/blocks/pfb/arb_resampler.rs): resamples Complex32
 * by an arbitrary f32 rate. Per output it interpolates linearly between
 * two adjacent polyphase filters, (1-mu)*F[a](w) + mu*F[b](w'), with
 * part[f][j] = taps[f + j*num_filters] (tpf = ceil(n_taps/num_filters)).
 *
 * Schedule. Which input yields which outputs, and each output's filter
 * index and mu, come from the block's f32 timing recurrence
 * (arb_resampler.rs:132-140,183-186), which never sees the samples. It is
 * eventually periodic; the schedule object walks preperiod + period
 * inputs once at create, with the reference's own f32 operations, and
 * keeps a checkpoint (state + cumulative output count) every
 * checkpoint_spacing inputs, so any stream position is reached in O(1)
 * plus at most checkpoint_spacing steps. Host-only, needs no GPU.
 * Input positions count the pushes AFTER the window fill (the first tpf
 * inputs of a stream only fill the window, :202-215).
 *  _create: FSDR_ERR_INVALID for rate <= 0 (or NaN) or num_filters == 0;
 *    FSDR_ERR_UNSUPPORTED where the walk passes 2^25 inputs, one input
 *    yields more than 2048 outputs, num_filters > 2^20, or
 *    num_filters/rate >= 2^30.
 *  _info: preperiod and period in inputs, outputs per period, checkpoint
 *    spacing, and segment_inputs, the inputs one block of the kernel owns
 *    per pass. NULL out-pointers are skipped.
 *  _count: outputs of n_inputs inputs starting at pushes_after_fill.
 *  _records: per output of inputs [first_input, first_input + n_inputs):
 *    the input index, base_index, the Boundary flag (the output spans two
 *    inputs: filter num_filters-1 on the previous window, filter 0 on
 *    this one) and mu. Fills up to cap entries of each non-NULL array;
 *    returns the number of outputs.
 *  _work: consumed/produced of one resampler call (below) by a stream
 *    that has consumed `pushes` inputs in all, for taps_per_filter.
 *  fsdr_pfb_arb_startup_map: WindowBuffer::new(len, false) puts fill push
 *    k at slot 2k mod len; src[s] is the push that slot s of the filled
 *    window holds, -1 for a hole (stays zero). */
typedef struct fsdr_pfb_arb_schedule fsdr_pfb_arb_schedule;
int fsdr_pfb_arb_schedule_create(float rate, size_t num_filters,
                                 fsdr_pfb_arb_schedule** out);
void fsdr_pfb_arb_schedule_destroy(fsdr_pfb_arb_schedule* s);
int fsdr_pfb_arb_schedule_info(const fsdr_pfb_arb_schedule* s,
                               uint64_t* preperiod, uint64_t* period,
                               uint64_t* outputs_per_period,
                               size_t* checkpoint_spacing,
                               size_t* segment_inputs);
uint64_t fsdr_pfb_arb_schedule_count(const fsdr_pfb_arb_schedule* s,
                                     uint64_t pushes_after_fill,
                                     uint64_t n_inputs);
size_t fsdr_pfb_arb_schedule_records(const fsdr_pfb_arb_schedule* s,
                                     uint64_t first_input, size_t n_inputs,
                                     uint64_t* in_index,
                                     uint32_t* base_index,
                                     uint8_t* boundary, float* mu,
                                     size_t cap);
void fsdr_pfb_arb_schedule_work(const fsdr_pfb_arb_schedule* s,
                                size_t taps_per_filter, uint64_t pushes,
                                size_t n_in, size_t out_cap,
                                size_t* consumed, size_t* produced);
void fsdr_pfb_arb_startup_map(size_t taps_per_filter, long long* src);

/* The resampler itself, for num_channels >= 1 channels in lockstep (same
 * rate, taps and stream position, so one schedule serves them all).
 * _create mirrors the constructor asserts (:92-103: rate > 0, n_taps >=
 * num_filters, num_filters != 0) as NULL plus an error string, and fails
 * the same way where the schedule is unsupported or the kernel's LDS tile
 * cannot hold segment + taps_per_filter samples (taps_per_filter beyond
 * 255 at the least). Input is channel-major,
 * in[c*in_stride + t] — the layout fsdr_pfb_channelizer_* writes — and
 * output is out[c*out_stride + k].
 * One call is the reference's fill work() followed by one processing
 * work() on what remains: the first tpf inputs of a stream fill the
 * window and produce nothing; then n = min(n_in, (size_t)((float)out_cap
 * / rate)) inputs are processed (:218, f32 division). One deviation: the
 * call never writes past out_cap_per_chan — if those n inputs would yield
 * more, the largest prefix that fits is processed instead. Unconsumed
 * inputs stay with the caller. run_dev = bulk from zero state, leaves the
 * stream state alone; stream_dev carries the window and the position.
 * All work is enqueued on `stream` without a host sync. A one-channel
 * handle also runs through fsdr_filter_dev (stream semantics, status
 * BOTH_SUFFICIENT) and fsdr_fg_add_filter; with more channels
 * fsdr_filter_dev returns FSDR_ERR_INVALID. */
fsdr_filter* fsdr_pfb_arb_resampler_create(float rate, const float* taps,
                                           size_t n_taps,
                                           size_t num_filters,
                                           size_t num_channels);
const fsdr_pfb_arb_schedule* fsdr_pfb_arb_resampler_schedule(
    const fsdr_filter* f);
int fsdr_pfb_arb_resampler_run_dev(fsdr_filter* f, const void* d_in,
                                   size_t in_stride, size_t n_in_per_chan,
                                   void* d_out, size_t out_stride,
                                   size_t out_cap_per_chan, void* stream,
                                   size_t* consumed_per_chan,
                                   size_t* produced_per_chan);
int fsdr_pfb_arb_resampler_stream_dev(fsdr_filter* f, const void* d_in,
                                      size_t in_stride,
                                      size_t n_in_per_chan, void* d_out,
                                      size_t out_stride,
                                      size_t out_cap_per_chan, void* stream,
                                      size_t* consumed_per_chan,
                                      size_t* produced_per_chan);

/* WLAN sync-short autocorrelation helpers (examples/wlan/src/bin/
 * rx.rs:73-96): a*conj(b) Combine and the sliding-SUM MovingAverage
 * (moving_average.rs:65-105; one-shot: len-1 zero items then sums). */
int fsdr_cmul_conj_dev(const void* d_a, size_t n_a, const void* d_b,
                       size_t n_b, void* d_out, size_t n_out, void* stream,
                       size_t* m);
/* divide_mag Combine (rx.rs:97): out = |a| / b. */
int fsdr_divide_mag_dev(const void* d_a, size_t n_a, const void* d_b,
                        size_t n_b, void* d_out, size_t n_out, void* stream,
                        size_t* m);
int fsdr_wlan_moving_sum_dev(const void* d_in, size_t n_in, void* d_out,
                             size_t n_out, size_t len, int is_complex,
                             void* stream, size_t* produced);

/* WLAN rx front end (config 5): the host-side SyncShort state machine
 * (examples/wlan/src/sync_short.rs:92-150; THRESHOLD 0.56, MIN_GAP 480,
 * MAX_SAMPLES 540*80) and SyncLong (sync_long.rs:96-185; SEARCH_WINDOW
 * 320, 64-tap LONG correlator run on the GPU, top-2 peak sync, CP
 * strip). sync_short consumes aligned spans of (delayed signal, 48-avg
 * autocorrelation, correlation metric) and emits frame samples +
 * "wifi_start" tags; sync_long consumes that tagged stream and emits
 * 128 preamble samples + 64-sample OFDM symbols per frame, ready for
 * the 64-pt Fft block (rx.rs:84-103). */
typedef struct fsdr_wlan_rx fsdr_wlan_rx;
fsdr_wlan_rx* fsdr_wlan_rx_create(void);
void fsdr_wlan_rx_destroy(fsdr_wlan_rx* rx);
size_t fsdr_wlan_sync_short_run(fsdr_wlan_rx* rx, const fsdr_cf32* sig,
                                const fsdr_cf32* abs48, const float* cor,
                                size_t n, fsdr_cf32* out, size_t out_cap,
                                size_t* tag_idx, float* tag_freq,
                                size_t tag_cap, size_t* n_tags,
                                size_t* consumed_out);
size_t fsdr_wlan_sync_long_run(fsdr_wlan_rx* rx, const fsdr_cf32* in,
                               size_t n, const size_t* tag_idx,
                               const float* tag_freq, size_t num_tags,
                               fsdr_cf32* out, size_t out_cap,
                               size_t* frame_off, float* frame_freq,
                               size_t frame_cap, size_t* num_frames);

/* WLAN frame decoder — the bit work of examples/wlan Decoder (src/
 * decoder.rs:47-115) and ViterbiDecoder (src/viterbi_decoder.rs) for a batch
 * of frames in one kernel, one frame per wavefront: constellation indices
 * -> bits (bit k < n_bpsc of index i is rx bit i*n_bpsc + k, higher bits
 * of the byte ignored) -> per-symbol deinterleave -> depuncture (erasures
 * where the pattern is 0) -> hard-decision K=7 Viterbi (polynomials 0x6d,
 * 0x4f; byte paths shifted as 16-bit pairs; strict m0 > m1; get_output
 * after 6 trellis steps and then every 8, with a ring of n_traceback = 5, 10
 * or 9 entries for rates 1/2, 3/4, 2/3; best state = first maximum; the
 * first n_traceback bytes dropped) -> descramble (x^7+x^4+1, state from
 * decoded bits 0..6, out_bytes[0] = state, bits 7.. packed LSB first) ->
 * crc_ok = (CRC-32 of out_bytes[2 .. psdu+2] == 558161692). All integer;
 * results are bit-equal to the reference's arithmetic.
 * mcs 0..7 = Bpsk_1_2, Bpsk_3_4, Qpsk_1_2, Qpsk_3_4, Qam16_1_2, Qam16_3_4,
 * Qam64_2_3, Qam64_3_4 (lib.rs:223-282).
 * Tail rule: the decoder reads 16*(n_traceback + ceil(n_data_bits/8)) - 4
 * depunctured values, 76..164 more than the frame has. The reference reads
 * whatever earlier frames left in its array (never cleared), and past its
 * end for the largest frames. Here every such position reads as bit value
 * 0 (not an erasure): each frame decodes as a freshly constructed
 * reference Decoder would, for any frame size. With a 3/4 or 2/3 rate the
 * last PSDU byte can still come out wrong for some scrambler seeds (the
 * scrambled pad bits and this tail are no codeword, and the traceback is
 * short); the reference does the same, or worse, on its stale tail.
 * The SIGNAL field (frame_equalizer.rs:121-175) is this decode at
 * (mcs 0, psdu 0) on the 48 BPSK indices, first 24 decoded bits, followed
 * by fsdr_wlan_signal_field.
 * _create/_destroy: the handle owns its device buffers (descriptor upload,
 *   the staging of _host). Creating needs no device. One handle serves one
 *   stream at a time.
 * _decode_dev: `frames` is a host array, free for reuse on return. Frame i
 *   reads 48*n_symbols index bytes at d_syms + sym_off, writes psdu_size+2
 *   descrambled bytes at d_out_bytes + out_off, if d_dec_bytes is not NULL
 *   the ceil(n_data_bits/8) raw Viterbi bytes (before descrambling, MSB =
 *   earlier bit) at d_dec_bytes + dec_off, and d_crc_ok[i] = 0 or 1.
 *   Nothing else is written; output ranges must not overlap (not
 *   checked). Asynchronous on `stream`. FSDR_ERR_INVALID plus an error
 *   string, and no launch, for mcs > 7, psdu_size > 1528 or more than 511
 *   symbols (decoder.rs:157, lib.rs:43-45) in any frame, or a NULL
 *   pointer; n_frames == 0 is a successful no-op. Validation precedes the
 *   device check.
 * _decode_host: the same over host spans, synchronous; only the frames'
 *   own ranges of out_bytes and dec_bytes are written.
 * Host-only: _frame_param is FrameParam::new (lib.rs:324-343, psdu_size
 *   <= 4095). _deinterleave_map: out[k] = second[first[k]] of decoder.rs:
 *   50-64, n_cbps entries, read off the kernel's index map.
 *   _depuncture_map: for depunctured positions first .. first+count-1 of
 *   a frame of n_symbols, the kernel's source of each value: 8*byte + bit
 *   into the frame's index bytes, -1 for an erasure, -2 past the frame
 *   (reads 0). _signal_field: *found = 0 where the reference returns None
 *   (parity over bits 0..16 against bit 17, unknown rate in bits 0..3),
 *   else 1 with mcs and the length from bits 5..16; bits24 holds one bit
 *   per byte, nonzero = 1. */
typedef struct fsdr_wlan_decoder fsdr_wlan_decoder;
typedef struct {
    uint32_t mcs;
    uint32_t psdu_size;
    size_t   sym_off, out_off, dec_off; /* bytes; dec_off unused if NULL */
} fsdr_wlan_frame;
fsdr_wlan_decoder* fsdr_wlan_decoder_create(void);
void fsdr_wlan_decoder_destroy(fsdr_wlan_decoder* dec);
int fsdr_wlan_decode_dev(fsdr_wlan_decoder* dec, const void* d_syms,
                         const fsdr_wlan_frame* frames, size_t n_frames,
                         void* d_out_bytes, void* d_dec_bytes,
                         void* d_crc_ok, void* stream);
int fsdr_wlan_decode_host(fsdr_wlan_decoder* dec, const uint8_t* syms,
                          const fsdr_wlan_frame* frames, size_t n_frames,
                          uint8_t* out_bytes, uint8_t* dec_bytes,
                          uint8_t* crc_ok);
int fsdr_wlan_frame_param(unsigned mcs, size_t psdu_size, size_t* n_symbols,
                          size_t* n_data_bits, size_t* n_pad);
int fsdr_wlan_deinterleave_map(unsigned mcs, uint16_t* out);
int fsdr_wlan_depuncture_map(unsigned mcs, size_t n_symbols, size_t first,
                             size_t count, int32_t* out);
int fsdr_wlan_signal_field(const uint8_t* bits24, int* found, unsigned* mcs,
                           size_t* psdu_size);

/* WLAN frame equalizer — examples/wlan FrameEqualizer (src/
 * frame_equalizer.rs) for a batch of frames, lane = carrier. The reference
 * is a stream state machine driven by "wifi_start" tags; here the caller
 * says where each frame's symbols start and how many there are, and the
 * frames of a batch are independent.
 * Input: the plain forward 64-point FFT (no shift, no scaling) of
 * fsdr_wlan_sync_long_run's stream; per frame two long-training symbols,
 * the SIGNAL symbol, then data symbols. Carrier m is FFT bin (m + 32) % 64
 * (:234-237).
 * Every symbol (:239-271) is multiplied by (cos(-beta), sin(-beta)), beta =
 * arg of its pilot sum over carriers 11, 25, 39, 53: s11 - s25 + s39 + s53
 * for the training symbols, p*s11 + p*s39 + p*s25 - p*s53 otherwise, with
 * p = POLARITY[0] for SIGNAL and POLARITY[(j + 1) % 127] for data symbol j
 * (lib.rs:365, the x^7+x^4+1 scrambler seeded with ones, as +1 / -1).
 * Channel (:27-46): h = first training symbol; the second, s, gives on
 * carriers 6..58 except 32 noise += |h-s|^2, signal += |h+s|^2 and
 * h = (h+s) / (2*LONG[m]) (lib.rs:495); snr_db = 10*log10(signal/noise/2).
 * Equalize (:48-62): the 48 data carriers (6..58 without 11, 25, 32, 39,
 * 53) in ascending order, z = s/h by num-complex's division, index =
 * Modulation::demap(z) (lib.rs:177-218, strict comparisons, f32 thresholds;
 * NaN gives 0).
 * SIGNAL (:294-331, :121-175): equalized as BPSK, decoded as a frame of
 * (mcs 0, psdu 0) by the decoder above, first 24 decoded bits parsed by the
 * rule of fsdr_wlan_signal_field. No parse: found = 0 and nothing else of
 * the frame is written. A parse gives mcs, psdu_size (any length up to
 * 4095) and n_symbols (FrameParam::new); n_copied = min(n_symbols,
 * n_avail - 3) data symbols are equalized with that modulation.
 * Sums over carriers are formed in a different order than the reference's
 * loop, and atan2f/sincosf are the device's: results agree with the
 * reference's f32 arithmetic to rounding, not bit for bit.
 * _create/_destroy: the handle owns its workspace (h, snr, the SIGNAL
 *   indices and decode), a private decoder and the staging of _host.
 *   Creating needs no device. One handle serves one stream at a time.
 * _equalize_dev: `frames` is a host array, free for reuse on return. Frame
 *   i reads 64*n_avail cf32 at d_spec + sym_off and writes 48*n_copied
 *   index bytes at d_idx + idx_off, if d_eq is not NULL as many equalized
 *   cf32 values (the reference's `symbols` message) at d_eq + eq_off, and
 *   d_info[i] (always: all zeros except snr_db when not found; snr_db = 0
 *   when n_avail < 2). Nothing else is written; output ranges must not
 *   overlap (not checked). Three launches on `stream`, no host
 *   synchronisation. FSDR_ERR_INVALID plus an error string, and no launch,
 *   for a NULL pointer other than d_eq; n_frames == 0 is a successful
 *   no-op. Validation precedes the device check.
 * _equalize_host: the same over host spans, synchronous.
 * Host-only: _demap is the kernel's demap for mcs 0..7 on n values.
 *   _pilot_polarity: POLARITY[(first + i) % 127], i < count, as +1 / -1.
 *   _carrier_map: output position of carrier m, -1 for pilot, DC, guard. */
typedef struct fsdr_wlan_equalizer fsdr_wlan_equalizer;
typedef struct {
    size_t   sym_off; /* cf32 items into d_spec */
    uint32_t n_avail; /* 64-item symbols from sym_off, training and SIGNAL
                         included */
    size_t   idx_off; /* bytes into d_idx; room for 48*(n_avail-3), 0 if
                         n_avail < 3 */
    size_t   eq_off;  /* cf32 items into d_eq; unused if d_eq is NULL */
} fsdr_wlan_eq_frame;
typedef struct {
    uint32_t found, mcs, psdu_size, n_symbols, n_copied;
    float    snr_db;
} fsdr_wlan_eq_info;
fsdr_wlan_equalizer* fsdr_wlan_equalizer_create(void);
void fsdr_wlan_equalizer_destroy(fsdr_wlan_equalizer* eq);
int fsdr_wlan_equalize_dev(fsdr_wlan_equalizer* eq, const void* d_spec,
                           const fsdr_wlan_eq_frame* frames, size_t n_frames,
                           void* d_idx, void* d_eq, void* d_info,
                           void* stream);
int fsdr_wlan_equalize_host(fsdr_wlan_equalizer* eq, const fsdr_cf32* spec,
                            const fsdr_wlan_eq_frame* frames, size_t n_frames,
                            uint8_t* idx, fsdr_cf32* eq_syms,
                            fsdr_wlan_eq_info* info);
int fsdr_wlan_demap(unsigned mcs, const fsdr_cf32* z, size_t n, uint8_t* out);
int fsdr_wlan_pilot_polarity(size_t first, size_t count, int8_t* out);
int fsdr_wlan_carrier_map(int8_t out[64]);

/* MFMA-loop microbenchmark (diagnostics; tools/mfma_ubench.py): times
 * the chain kernel's inner MFMA loop on LDS staged once. */
int fsdr_mfma_ubench(int grid, int iters, double* tflops, void* stream);
/* Incremental chain ubench: real tile loop with components gated by
 * mode bits (1 staging loads, 2 LDS writes+barriers, 4 deposit+FFT);
 * reports executed-MFMA TF/s for pipe-utilization comparison. */
int fsdr_chain_ubench(int mode, double* tflops, void* stream);

/* ---- device memory helpers (for harnesses driving the _dev paths) ---- */
int fsdr_dev_alloc(void** d_ptr, size_t bytes);
int fsdr_dev_free(void* d_ptr);
int fsdr_memcpy_h2d(void* d_dst, const void* src, size_t bytes);
int fsdr_memcpy_d2h(void* dst, const void* d_src, size_t bytes);
/* Fill a device buffer with n Complex32 samples, re/im iid uniform[-1,1)
 * from a counter-based generator seeded by `seed` (deterministic,
 * device-generated — the NullSource/bench synthetic source). */
int fsdr_fill_uniform_cf32(void* d_ptr, size_t n, uint64_t seed,
                           uint64_t offset, void* stream);

/* ---- firdes (host-side tap designers; no GPU required) ---------------- *
 * Mirror crates/futuredsp/src/firdes/basic.rs + windows.rs:144 +
 * math/special_funs.rs:22-45 — the tap-generation row of SURVEY.md §8a. */
double fsdr_kaiser_beta(double max_ripple); /* basic.rs:444-452 */
void   fsdr_kaiser_window(size_t len, double beta, double* out);
/* firdes::kaiser::lowpass<f32> (basic.rs:310-321). Returns tap count;
 * fills out up to cap (query with out=NULL, cap=0). */
size_t fsdr_firdes_kaiser_lowpass_f32(double cutoff, double transition_bw,
                                      double max_ripple, float* out,
                                      size_t cap);
/* firdes::kaiser::multirate<f32> (basic.rs:412-442), the Nyquist filter
 * FirBuilder::resampling designs: 2*half_polyphase_len taps per polyphase
 * arm, one tap (1.0) for interp == decim == 1. Same query convention.
 * Returns 0 plus an error string where the reference asserts (a zero
 * interp, decim or half_polyphase_len, :418-423). */
size_t fsdr_firdes_kaiser_multirate_f32(size_t interp, size_t decim,
                                        size_t half_polyphase_len,
                                        double max_ripple, float* out,
                                        size_t cap);
/* firdes::lowpass<f32> over a kaiser window of explicit length
 * (basic.rs:25-42 with windows::kaiser) — fixed-length designer used by
 * the bench (127 taps). */
int fsdr_firdes_lowpass_kaiser_n_f32(size_t n_taps, double beta,
                                     double cutoff, float* out);

/* ---- Chain level ------------------------------------------------------ *
 * Fused hot path: Fir(taps1) -> DecimatingFir(decim, taps2) -> Fft(len).
 * Mirrors BASELINE configs[2]/[3]; per-stage math identical to the three
 * filters composed (intermediates stay resident in HBM). */
typedef struct fsdr_chain fsdr_chain;
fsdr_chain* fsdr_chain_create(const float* taps1, size_t n_taps1,
                              const float* taps2, size_t n_taps2,
                              size_t decim, size_t fft_len);
/* Run over device input; writes `frames*fft_len` Complex32 spectra to
 * d_out (may be NULL with out_cap 0 -> spectra discarded into an internal
 * buffer, NullSink-style). If d_mag is non-NULL also writes f32 |X|^2 of
 * each bin (the config-4 spectrum join payload). Async on stream. */
int fsdr_chain_run_dev(fsdr_chain* c, const void* d_in, size_t n_in,
                       void* d_out, size_t out_cap,
                       void* d_mag, size_t mag_cap,
                       void* stream, size_t* consumed, size_t* produced);
/* MFMA K of the fused (combined-taps) filter the chain kernels are
 * instantiated for, 0 when the chain has no fused filter
 * (diagnostics/tests; host-only). */
int fsdr_chain_variant(const fsdr_chain* c, int* fused_kk_mfma);
void fsdr_chain_destroy(fsdr_chain* c);

/* ---- Ring (Slab-style stream buffer) ---------------------------------- *
 * N pinned-host buffers + N device mirrors circulating between an empty
 * queue (writer side) and a full queue (reader side), carrying the
 * reader's UNCONSUMED tail in front of the next buffer exactly like
 * slab.rs:369-399 (device-side D2D on the ring's copy stream), so
 * arbitrary chunk sizes stream exactly. reserved_items = carry capacity
 * (>= the consumer's worst-case leftover; for a FIR chain:
 * taps-1 + decim*fft_len + decim). Writer: acquire -> fill host slice ->
 * commit(n) (enqueues async H2D on the copy stream). Reader: acquire
 * (waits for the copies; yields the device pointer at the carry start
 * and items = carry + payload) -> ... launch kernels consuming
 * `consumed` items ... -> release_consumed(consumed, compute_stream).
 * release() = consumed everything. Single-producer single-consumer. */
typedef struct fsdr_ring fsdr_ring;
fsdr_ring* fsdr_ring_create(size_t n_buffers, size_t items_per_buffer,
                            size_t item_bytes, size_t reserved_items);
int  fsdr_ring_writer_acquire(fsdr_ring* r, void** host_ptr, size_t* items);
int  fsdr_ring_writer_commit(fsdr_ring* r, size_t items);
int  fsdr_ring_reader_acquire(fsdr_ring* r, void** dev_ptr, size_t* items);
int  fsdr_ring_reader_release_consumed(fsdr_ring* r, size_t consumed,
                                       void* stream);
int  fsdr_ring_reader_release(fsdr_ring* r);
void fsdr_ring_destroy(fsdr_ring* r);

/* D2H return ring (vulkan d2h.rs Writer::submit / host Reader + the
 * circuit's empty recirculation): device producer fills ring buffers on
 * its stream, async D2H on the ring's copy stream hands pinned host
 * spans to the consumer. Writer acquire takes the producer's stream so
 * buffer reuse is ordered after the previous D2H without host syncs. */
typedef struct fsdr_ring_d2h fsdr_ring_d2h;
fsdr_ring_d2h* fsdr_ring_d2h_create(size_t n_buffers,
                                    size_t items_per_buffer,
                                    size_t item_bytes);
int  fsdr_ring_d2h_writer_acquire(fsdr_ring_d2h* r, void** dev_ptr,
                                  size_t* items, void* stream);
int  fsdr_ring_d2h_writer_commit(fsdr_ring_d2h* r, size_t items,
                                 void* stream);
int  fsdr_ring_d2h_reader_acquire(fsdr_ring_d2h* r, void** host_ptr,
                                  size_t* items);
int  fsdr_ring_d2h_reader_release(fsdr_ring_d2h* r);
void fsdr_ring_d2h_destroy(fsdr_ring_d2h* r);

/* ---- Flowgraph driver (native C++ harness) ---------------------------- *
 * Minimal mirror of Flowgraph::add / Flowgraph::stream / Runtime::run for
 * 1-in/1-out chains (src/runtime/flowgraph.rs:227-241,364-423,
 * runtime.rs:169-215, wrapped_kernel.rs:106-229) with
 * NullSource/VectorSource/Head/NullSink/VectorSink endpoints and
 * GPU-filter blocks. Stream data stays resident in HBM between blocks.
 * add_* return a block id (>= 0); connect defaults to the single
 * output->input ports, like connect!'s defaults
 * (crates/macros/src/lib.rs:56-60). */
typedef struct fsdr_fg fsdr_fg;
fsdr_fg* fsdr_fg_create(void);
int  fsdr_fg_add_null_source_cf32(fsdr_fg* fg);
int  fsdr_fg_add_vector_source_cf32(fsdr_fg* fg, const fsdr_cf32* data,
                                    size_t n);
int  fsdr_fg_add_vector_source_f32(fsdr_fg* fg, const float* data,
                                   size_t n);
int  fsdr_fg_add_head(fsdr_fg* fg, unsigned long long n);
int  fsdr_fg_add_filter(fsdr_fg* fg, fsdr_filter* f);
int  fsdr_fg_add_null_sink(fsdr_fg* fg);
int  fsdr_fg_add_vector_sink(fsdr_fg* fg);
int  fsdr_fg_stream(fsdr_fg* fg, int src_block, int dst_block);
int  fsdr_fg_run(fsdr_fg* fg);
unsigned long long fsdr_fg_n_received(fsdr_fg* fg, int block);
size_t fsdr_fg_vector_sink_get(fsdr_fg* fg, int block, void* out,
                               size_t cap_bytes);
void fsdr_fg_destroy(fsdr_fg* fg);
size_t fsdr_filter_item_sizes(const fsdr_filter* f, size_t* out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FUTURESDR_HIP_H */
