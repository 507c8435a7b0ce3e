/* futuresdr_hip.hip — MI355X-native (gfx950/CDNA4) implementation of the
 * FutureSDR streaming-DSP hot path, behind the C-ABI in
 * include/futuresdr_hip.h.
 *
 * Written for CDNA4 from scratch: 64-wide wavefronts, LDS-staged FIR tiles
 * with register sliding windows, SoA re/im LDS planes with a 2-dwords-per-16
 * pad (breaks the stride-16B bank pattern of the pair reads), radix-4
 * Stockham FFT in LDS, the PFB channelizer, the PFB synthesizer (one
 * fused gather + in-LDS IFFT + commutator kernel) and the PFB
 * arbitrary-rate resampler (f32 timing schedule as a checkpoint table,
 * re-walked per lane), and the FM receiver back end (quadrature demod
 * fused into the f32 polyphase resampler's staging pass), and the IIR
 * filter as a blocked recurrence (chunks from zero state, end states
 * combined by doubling scans with constant matrix powers), and the LoRa
 * FFT demodulator (dechirp while staging, in-LDS FFT, argmax or max-log
 * LLRs reduced per symbol), and the WLAN frame decoder (deinterleave,
 * depuncture, K=7 Viterbi, descramble and CRC-32 with one frame per
 * wavefront and one trellis state per lane). No CUDA shims, no hipify
 * output.
 *
 * Numerical semantics follow the reference cores (cited per function); the
 * status/consumed/produced math is bit-exact, the float results are
 * tolerance-compared (the reference itself permits reassociation on
 * nightly — crates/futuredsp/src/fir.rs:93-200 — and uses 5*eps for GPU
 * parity, examples/vulkan/src/main.rs:103).
 */
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <type_traits>
#include <vector>
#include <algorithm>
#include <cmath>

#include "../../include/futuresdr_hip.h"
#include "dev_buf.h" /* after hip_runtime.h: it names HIP, includes none */

/* ================= error plumbing ==================================== */

static thread_local char g_err[512];
static thread_local const char* g_err_ptr = "";

static void set_err(const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    g_err_ptr = g_err;
}

extern "C" const char* fsdr_last_error(void) { return g_err_ptr; }
extern "C" const char* fsdr_version(void) { return "futuresdr-hip 0.1 gfx950"; }

#define HIP_TRY(call)                                                        \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            snprintf(g_err, sizeof(g_err), "%s failed: %s (%s:%d)", #call,   \
                     hipGetErrorString(e_), __FILE__, __LINE__);             \
            g_err_ptr = g_err;                                               \
            return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice)   \
                       ? FSDR_ERR_NO_GPU                                     \
                       : FSDR_ERR_HIP;                                       \
        }                                                                    \
    } while (0)

static bool have_gpu() {
    static int cached = -1;
    if (cached < 0) {
        int n = 0;
        cached = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
    }
    return cached == 1;
}

#define REQUIRE_GPU()                                                        \
    do {                                                                     \
        if (!have_gpu()) {                                                   \
            set_err("no HIP device present — the futuresdr_hip product "     \
                    "path has no CPU fallback (oracle/ is test infra)");     \
            return FSDR_ERR_NO_GPU;                                          \
        }                                                                    \
    } while (0)

extern "C" int fsdr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int fsdr_set_device(int device) {
    REQUIRE_GPU();
    HIP_TRY(hipSetDevice(device));
    return FSDR_OK;
}
extern "C" int fsdr_synchronize(void) {
    REQUIRE_GPU();
    HIP_TRY(hipDeviceSynchronize());
    return FSDR_OK;
}

/* ================= shared device helpers ============================== */

/* LDS SoA plane padding: +2 dwords per 16 — breaks the 16 B lane-stride
 * bank pattern of the f32-pair (ds_read_b64) window loads while keeping
 * even-indexed pairs contiguous and 8 B-aligned (DESIGN.md kernel notes). */
__device__ __host__ __forceinline__ unsigned lds_pad(unsigned e) {
    return e + ((e >> 4) << 1);
}

/* floats per SoA plane for a tile of `elems` elements, rounded to a
 * 16 B multiple so the second plane stays aligned for pair reads. */
__device__ __host__ __forceinline__ unsigned plane_floats(unsigned elems) {
    return (lds_pad(elems - 1) + 4u) & ~3u;
}

/* LDS index swizzle for the ping/pong buffers: float2 element i sits at
 * bank (2i) mod 64, so accesses whose lane stride is a multiple of 32
 * elements (the strided Stockham stages) are up-to-8-way conflicted;
 * XORing bits 5..7 of the element index into bits 2..4 makes them
 * conflict-free while keeping contiguous stages conflict-free. */
__device__ __forceinline__ unsigned fft_swz(unsigned i) {
    /* full 5-bit XOR: two elements collide on a bank only when their
     * indices differ by a multiple of 1024 — conflict-free for every
     * Stockham stage stride at n <= 1024 (and 2-way max at 2048/4096).
     * FFT accesses are single float2 elements, so remapping any bit of
     * the element index is layout-legal. */
    return i ^ ((i >> 5) & 31u);
}

__device__ __forceinline__ float2 f2_add(float2 a, float2 b) {
    return make_float2(a.x + b.x, a.y + b.y);
}
__device__ __forceinline__ float2 f2_sub(float2 a, float2 b) {
    return make_float2(a.x - b.x, a.y - b.y);
}
__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

/* ================= FIR (decimation 1), Complex32 x f32 taps =========== *
 * Restates fir_kernel_core + the Complex<f32>/f32 MAC
 * (crates/futuredsp/src/fir.rs:76-88, 242-249): y[k] = sum_t x[k+t] *
 * h[T-1-t], accumulating re/im separately in fp32.
 *
 * Tiling: 256 lanes/block, R=4 consecutive outputs per lane, input tile in
 * SoA LDS planes (pad-2-per-16 keeps the 16 B lane-stride pair reads
 * conflict-free). Inner loop: 2 taps per step, 16 FMAs per step; the
 * window pair AND the (LDS-staged, reversed) tap pair for step s+1 are
 * prefetched during step s so no FMA waits on a just-issued LDS read
 * (the v1 kernel was SQ_WAIT_INST-bound at 28% of fp32 peak for exactly
 * that reason — profiles/rocprof_r01*). Requires n_taps_padded % 8 == 1
 * (host pads taps with leading zeros; padded taps multiply staged zeros
 * only). */

#define FIR_BLOCK 256
#define FIR_R 4
#define FIR_TILE_OUT (FIR_BLOCK * FIR_R) /* 1024 outputs per tile */

__global__ __launch_bounds__(FIR_BLOCK) void k_fir_cf32(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ taps, int n_taps_padded, long long n_out,
    long long n_in_valid) {
    const int tp = n_taps_padded;                     /* tp % 8 == 1 */
    const unsigned elems = FIR_TILE_OUT + tp - 1 + 6; /* + prefetch slack */
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_re = (float*)smem;
    float* s_im = s_re + plane_floats(elems);
    float* s_rt = s_im + plane_floats(elems); /* reversed taps, tp+1 slots */

    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x;
         tile * (long long)FIR_TILE_OUT < n_out; tile += gridDim.x) {
        const long long out_base = tile * FIR_TILE_OUT;
        for (unsigned i = tid; i < elems; i += FIR_BLOCK) {
            long long g = out_base + i;
            float2 v = (g < n_in_valid) ? in[g] : make_float2(0.f, 0.f);
            s_re[lds_pad(i)] = v.x;
            s_im[lds_pad(i)] = v.y;
        }
        for (int i = tid; i <= tp; i += FIR_BLOCK)
            s_rt[i] = (i < tp) ? taps[tp - 1 - i] : 0.f;
        __syncthreads();

        const unsigned eb = (unsigned)tid * FIR_R; /* tile-relative base */
        float ar[FIR_R] = {0.f, 0.f, 0.f, 0.f};
        float ai[FIR_R] = {0.f, 0.f, 0.f, 0.f};
        /* 4-pair rotating window: slot q holds pair q mod 4 (elements
         * 2q, 2q+1 relative to eb), flat layout w[2*slot + parity]. */
        float wre[8], wim[8];
#pragma unroll
        for (int p = 0; p < 3; p++) {
            float2 pr = *(const float2*)&s_re[lds_pad(eb + 2 * p)];
            float2 pi = *(const float2*)&s_im[lds_pad(eb + 2 * p)];
            wre[2 * p] = pr.x; wre[2 * p + 1] = pr.y;
            wim[2 * p] = pi.x; wim[2 * p + 1] = pi.y;
        }
        float2 ht0 = *(const float2*)&s_rt[0];
        const int pair_steps = (tp - 1) / 2; /* multiple of 4 */
        int s = 0;
        /* flat window index of tile-relative element e = 2s + d at phase
         * U = s%4: 2*((U + d/2) % 4) + d%2, d in [0,5] */
#define FIR_W(U, d) (2 * (((U) + (d) / 2) % 4) + (d) % 2)
#define FIR_STEP(U)                                                          \
    do {                                                                     \
        float2 nr = *(const float2*)&s_re[lds_pad(eb + 2 * s + 6)];          \
        float2 ni = *(const float2*)&s_im[lds_pad(eb + 2 * s + 6)];          \
        float2 ht1 = *(const float2*)&s_rt[2 * s + 2];                       \
        _Pragma("unroll") for (int j = 0; j < FIR_R; j++) {                  \
            ar[j] = fmaf(wre[FIR_W(U, j)], ht0.x, ar[j]);                    \
            ai[j] = fmaf(wim[FIR_W(U, j)], ht0.x, ai[j]);                    \
            ar[j] = fmaf(wre[FIR_W(U, j + 1)], ht0.y, ar[j]);                \
            ai[j] = fmaf(wim[FIR_W(U, j + 1)], ht0.y, ai[j]);                \
        }                                                                    \
        wre[2 * (((U) + 3) % 4)] = nr.x;                                     \
        wre[2 * (((U) + 3) % 4) + 1] = nr.y;                                 \
        wim[2 * (((U) + 3) % 4)] = ni.x;                                     \
        wim[2 * (((U) + 3) % 4) + 1] = ni.y;                                 \
        ht0 = ht1;                                                           \
        s++;                                                                 \
    } while (0)
        for (; s < pair_steps;) {
            FIR_STEP(0);
            FIR_STEP(1);
            FIR_STEP(2);
            FIR_STEP(3);
        }
#undef FIR_STEP
        /* final (unpaired) tap t = tp-1: element e = tp-1+j is in pair
         * ps + j/2 -> slot j/2 (ps % 4 == 0), parity j%2 */
        {
            const float h0 = s_rt[tp - 1];
#pragma unroll
            for (int j = 0; j < FIR_R; j++) {
                ar[j] = fmaf(wre[2 * (j / 2) + (j % 2)], h0, ar[j]);
                ai[j] = fmaf(wim[2 * (j / 2) + (j % 2)], h0, ai[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < FIR_R; j++) {
            long long o = out_base + eb + j;
            if (o < n_out) out[o] = make_float2(ar[j], ai[j]);
        }
        __syncthreads();
    }
}

/* ---- Fully-unrolled compile-time-tap-count FIR variant --------------- *
 * Same math as k_fir_cf32; TP is the padded tap count (TP % 4 == 1) and
 * the device tap array is REVERSED (rt[i] = h[n_taps-1-i], zero-filled to
 * TP). Linear SoA LDS planes (no pad): the window is read as float4
 * groups at 16 B lane stride (the conflict-free ds_read_b128 pattern) and
 * addresses are affine (fold to ds_read immediate offsets). Reversed taps
 * are staged in LDS too (keeping SMEM out of the loop: s_load shares
 * lgkmcnt with ds_read and forces lgkmcnt(0) drains). Accumulators are
 * float2 OUTPUT pairs so every v_pk_fma reads two adjacent float4
 * components — no register-pairing movs (the v3 variant spent ~40% of
 * VALU on such movs). */
template <int TP>
__global__ __launch_bounds__(FIR_BLOCK) void k_fir_cf32_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtaps, long long n_out, long long n_in_valid) {
    static_assert(TP % 4 == 1, "TP must be 1 mod 4");
    const unsigned elems = FIR_TILE_OUT + TP + 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_re = (float*)smem;
    float* s_im = s_re + ((elems + 7u) & ~7u);
    float* s_rt = s_im + ((elems + 7u) & ~7u); /* TP+3 floats */

    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x;
         tile * (long long)FIR_TILE_OUT < n_out; tile += gridDim.x) {
        const long long out_base = tile * FIR_TILE_OUT;
        for (unsigned i = tid; i < elems; i += FIR_BLOCK) {
            long long g = out_base + i;
            float2 v = (g < n_in_valid) ? in[g] : make_float2(0.f, 0.f);
            s_re[i] = v.x;
            s_im[i] = v.y;
        }
        for (int i = tid; i < TP + 3; i += FIR_BLOCK)
            s_rt[i] = (i < TP) ? rtaps[i] : 0.f;
        __syncthreads();

        const unsigned eb = (unsigned)tid * FIR_R;
        float2 a01r = make_float2(0.f, 0.f), a23r = a01r;
        float2 a01i = a01r, a23i = a01r;
        float4 r0 = *(const float4*)&s_re[eb];
        float4 r1 = *(const float4*)&s_re[eb + 4];
        float4 i0 = *(const float4*)&s_im[eb];
        float4 i1 = *(const float4*)&s_im[eb + 4];
        float4 hc = *(const float4*)&s_rt[0];
        constexpr int NG = (TP - 1) / 4; /* 4 taps per group */
        /* software pipeline: every load issued one group ahead of its use,
         * so in steady state no FMA waits on a just-issued ds_read */
#pragma unroll 8
        for (int m = 0; m < NG; m++) {
            const float4 rn = *(const float4*)&s_re[eb + 4 * m + 8];
            const float4 in_ = *(const float4*)&s_im[eb + 4 * m + 8];
            const float4 h4 = *(const float4*)&s_rt[4 * m + 4];
            const float wr[8] = {r0.x, r0.y, r0.z, r0.w,
                                 r1.x, r1.y, r1.z, r1.w};
            const float wi[8] = {i0.x, i0.y, i0.z, i0.w,
                                 i1.x, i1.y, i1.z, i1.w};
            const float ht[4] = {hc.x, hc.y, hc.z, hc.w};
#pragma unroll
            for (int tl = 0; tl < 4; tl++) {
                const float h = ht[tl];
                a01r.x = fmaf(wr[tl], h, a01r.x);
                a01r.y = fmaf(wr[tl + 1], h, a01r.y);
                a23r.x = fmaf(wr[tl + 2], h, a23r.x);
                a23r.y = fmaf(wr[tl + 3], h, a23r.y);
                a01i.x = fmaf(wi[tl], h, a01i.x);
                a01i.y = fmaf(wi[tl + 1], h, a01i.y);
                a23i.x = fmaf(wi[tl + 2], h, a23i.x);
                a23i.y = fmaf(wi[tl + 3], h, a23i.y);
            }
            r0 = r1; r1 = rn;
            i0 = i1; i1 = in_;
            hc = h4;
        }
        { /* final tap TP-1: r0 = elements TP-1..TP+2, hc = rt[TP-1..] */
            const float h = hc.x;
            a01r.x = fmaf(r0.x, h, a01r.x);
            a01r.y = fmaf(r0.y, h, a01r.y);
            a23r.x = fmaf(r0.z, h, a23r.x);
            a23r.y = fmaf(r0.w, h, a23r.y);
            a01i.x = fmaf(i0.x, h, a01i.x);
            a01i.y = fmaf(i0.y, h, a01i.y);
            a23i.x = fmaf(i0.z, h, a23i.x);
            a23i.y = fmaf(i0.w, h, a23i.y);
        }
        const float ar[4] = {a01r.x, a01r.y, a23r.x, a23r.y};
        const float ai[4] = {a01i.x, a01i.y, a23i.x, a23i.y};
#pragma unroll
        for (int j = 0; j < FIR_R; j++) {
            long long o = out_base + eb + j;
            if (o < n_out) out[o] = make_float2(ar[j], ai[j]);
        }
        __syncthreads();
    }
}

/* instantiation dispatch for the templated FIR (host side below) */
typedef void (*fir_tpl_fn)(const float2*, float2*, const float*, long long,
                           long long);
template <int TP>
static fir_tpl_fn fir_tpl_ptr() { return k_fir_cf32_tpl<TP>; }

/* ================= Decimating FIR (D=4 fast path), cf32 x f32 ========= *
 * Restates decimating_fir.rs:80-95 for Complex<f32>/f32: y[k] =
 * sum_t x[D-1 + k*D + t] * h[T-1-t].
 *
 * 256 lanes, R2=4 consecutive decimated outputs per lane; 8-pair rotating
 * window with one-step-ahead prefetch of both the window pair and the
 * LDS-staged reversed tap pair (same latency-hiding structure as
 * k_fir_cf32). Taps processed as tap 0 (prologue) + pairs (1,2),(3,4),...
 * Requires n_taps_padded % 16 == 1. */

#define DFIR_BLOCK 256
#define DFIR_R 4
#define DFIR_TILE_OUT (DFIR_BLOCK * DFIR_R) /* 1024 decimated outputs */

__global__ __launch_bounds__(DFIR_BLOCK) void k_fir_decim4_cf32(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ taps, int n_taps_padded, long long n_out,
    long long n_in_valid) {
    constexpr int D = 4;
    const int tp = n_taps_padded; /* tp % 16 == 1 */
    const unsigned elems = DFIR_TILE_OUT * D + tp - 1 + 20;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_re = (float*)smem;
    float* s_im = s_re + plane_floats(elems);
    float* s_rt = s_im + plane_floats(elems); /* reversed taps MINUS tap0 */

    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x;
         tile * (long long)DFIR_TILE_OUT < n_out; tile += gridDim.x) {
        const long long out_base = tile * DFIR_TILE_OUT;
        const long long in_base = out_base * D;
        for (unsigned i = tid; i < elems; i += DFIR_BLOCK) {
            long long g = in_base + i;
            float2 v = (g < n_in_valid) ? in[g] : make_float2(0.f, 0.f);
            s_re[lds_pad(i)] = v.x;
            s_im[lds_pad(i)] = v.y;
        }
        /* s_rt[i] = coefficient of tap t=i+1, i.e. taps[tp-2-i] */
        for (int i = tid; i <= tp; i += DFIR_BLOCK)
            s_rt[i] = (i < tp - 1) ? taps[tp - 2 - i] : 0.f;
        __syncthreads();

        /* lane-relative input element for (output j, tap t):
         * e = D-1 + 4j + t, with lane base eb = tid*R2*D */
        const unsigned eb = (unsigned)tid * DFIR_R * D;
        float ar[DFIR_R] = {0.f, 0.f, 0.f, 0.f};
        float ai[DFIR_R] = {0.f, 0.f, 0.f, 0.f};
        /* tap 0 prologue: e = 3 + 4j (odd -> single b32 reads) */
        {
            const float h = taps[tp - 1];
#pragma unroll
            for (int j = 0; j < DFIR_R; j++) {
                ar[j] = fmaf(s_re[lds_pad(eb + 3 + 4 * j)], h, ar[j]);
                ai[j] = fmaf(s_im[lds_pad(eb + 3 + 4 * j)], h, ai[j]);
            }
        }
        /* step s covers taps (1+2s, 2+2s); output j reads BOTH elements of
         * pair s+2+2j; window = 8 rotating pair slots (p % 8), prefetch
         * pair s+9 during step s. */
        float wre[16], wim[16];
#pragma unroll
        for (int p = 2; p <= 8; p++) {
            float2 pr = *(const float2*)&s_re[lds_pad(eb + 2 * p)];
            float2 pi = *(const float2*)&s_im[lds_pad(eb + 2 * p)];
            wre[(p % 8) * 2] = pr.x; wre[(p % 8) * 2 + 1] = pr.y;
            wim[(p % 8) * 2] = pi.x; wim[(p % 8) * 2 + 1] = pi.y;
        }
        float2 ht0 = *(const float2*)&s_rt[0];
        const int pair_steps = (tp - 1) / 2; /* multiple of 8 */
        int s = 0;
#define DFIR_STEP(U)                                                         \
    do {                                                                     \
        float2 nr = *(const float2*)&s_re[lds_pad(eb + 2 * (s + 9))];        \
        float2 ni = *(const float2*)&s_im[lds_pad(eb + 2 * (s + 9))];        \
        float2 ht1 = *(const float2*)&s_rt[2 * s + 2];                       \
        _Pragma("unroll") for (int j = 0; j < DFIR_R; j++) {                 \
            const int sl = (((U) + 2 + 2 * j) % 8) * 2;                      \
            ar[j] = fmaf(wre[sl], ht0.x, ar[j]);                             \
            ai[j] = fmaf(wim[sl], ht0.x, ai[j]);                             \
            ar[j] = fmaf(wre[sl + 1], ht0.y, ar[j]);                         \
            ai[j] = fmaf(wim[sl + 1], ht0.y, ai[j]);                         \
        }                                                                    \
        wre[(((U) + 1) % 8) * 2] = nr.x;                                     \
        wre[(((U) + 1) % 8) * 2 + 1] = nr.y;                                 \
        wim[(((U) + 1) % 8) * 2] = ni.x;                                     \
        wim[(((U) + 1) % 8) * 2 + 1] = ni.y;                                 \
        ht0 = ht1;                                                           \
        s++;                                                                 \
    } while (0)
        for (; s < pair_steps;) {
            DFIR_STEP(0); DFIR_STEP(1); DFIR_STEP(2); DFIR_STEP(3);
            DFIR_STEP(4); DFIR_STEP(5); DFIR_STEP(6); DFIR_STEP(7);
        }
#undef DFIR_STEP
#pragma unroll
        for (int j = 0; j < DFIR_R; j++) {
            long long o = out_base + (unsigned)tid * DFIR_R + j;
            if (o < n_out) out[o] = make_float2(ar[j], ai[j]);
        }
        __syncthreads();
    }
}

/* ---- MFMA FIR variant (f32-input matrix cores) ----------------------- *
 * Same math as k_fir_cf32_tpl, reformulated as an implicit GEMM for the
 * exact-f32 matrix cores (v_mfma_f32_16x16x4_f32 — same 157.3 TF peak as
 * the f32 VALU but ~30x fewer instructions, so the VALU overhead and
 * issue stalls of the FMA kernel disappear):
 *   C[i][j] = sum_k X[i][k] * H[k][j],  X[i][k] = x[base + 16 i + k],
 *   H[k][j] = rt[k - j]  (0 <= k-j < T else 0),  K = KK >= T+15, KK%4==0
 * => C[i][j] = y[base + 16 i + j]; one 16x16 C tile (re + im, two
 * accumulator chains = full MFMA issue rate) per wave per 256 outputs.
 * The H fragments depend only on the taps: computed once per block into
 * KK/4 VGPRs. A fragments are single ds_read_b32 per MFMA from linear
 * SoA planes with an XOR bank swizzle (rows stride 16 dwords; lanes r,
 * r+2m collide mod 32, so XOR bits 5..7 of the dword index into bits
 * 2..4 — conflict-free, verified in the bank math of DESIGN.md). */
typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned mfma_swz(unsigned idx) {
    return idx ^ (((idx >> 5) & 7u) << 2);
}

#define MFIR_BLOCK 256
#define MFIR_TILE 1024 /* 4 waves x 256 outputs */

template <int KK>
__global__ __launch_bounds__(MFIR_BLOCK) void k_fir_mfma_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtaps /* reversed, zero-filled to KK */,
    long long n_out, long long n_in_valid) {
    static_assert(KK % 4 == 0, "KK must be a multiple of 4");
    const unsigned elems = MFIR_TILE + KK + 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_re = (float*)smem;
    float* s_im = s_re + ((elems + 31u) & ~31u);
    float* s_rtx = s_im + ((elems + 31u) & ~31u); /* 15 zeros + rt[KK] + 1 */

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r16 = lane & 15;   /* A row / C col */
    const int k4 = lane >> 4;    /* k sub-slice 0..3 */

    /* B fragments: lane holds H[k0 + k4][j = r16] = rtx[k0+k4-r16],
     * identical for every tile -> compute once (s_rtx has a 15-zero
     * prologue so the index is never negative). */
    for (int i = tid; i < KK + 16; i += MFIR_BLOCK)
        s_rtx[i] = (i >= 15 && i < 15 + KK) ? rtaps[i - 15] : 0.f;
    __syncthreads();
    float bfrag[KK / 4];
#pragma unroll
    for (int s = 0; s < KK / 4; s++)
        bfrag[s] = s_rtx[15 + 4 * s + k4 - r16];
    __syncthreads();

    /* global staging is software-pipelined across the tile loop: tile
     * t+1's loads are issued right after the staging barrier of tile t,
     * so their HBM latency hides under t's 72 MFMAs. */
    constexpr int NL = (MFIR_TILE + KK + 8 + 2 * MFIR_BLOCK - 1) /
                       (2 * MFIR_BLOCK); /* float4 (2 complex) per slot */
    float4 stg[NL];
    auto load_tile = [&](long long tl) {
        const long long ob = tl * MFIR_TILE;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            unsigned i = 2 * (tid + j * MFIR_BLOCK);
            long long g = ob + i;
            float2 v0 = (i < elems && g < n_in_valid)
                            ? in[g] : make_float2(0.f, 0.f);
            float2 v1 = (i + 1 < elems && g + 1 < n_in_valid)
                            ? in[g + 1] : make_float2(0.f, 0.f);
            stg[j] = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    };
    load_tile(blockIdx.x);
    for (long long tile = blockIdx.x;
         tile * (long long)MFIR_TILE < n_out; tile += gridDim.x) {
        const long long out_base = tile * MFIR_TILE;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            unsigned i = 2 * (tid + j * MFIR_BLOCK);
            if (i < elems) {
                unsigned d = mfma_swz(i);
                *(float2*)&s_re[d] = make_float2(stg[j].x, stg[j].z);
                *(float2*)&s_im[d] = make_float2(stg[j].y, stg[j].w);
            }
        }
        __syncthreads();
        if ((tile + gridDim.x) * (long long)MFIR_TILE < n_out)
            load_tile(tile + gridDim.x);

        const unsigned ab = (unsigned)wave * 256 + 16u * r16 + k4;
        /* one accumulator pair, re/im alternating: same-C spacing = 2
         * MFMA issues = 64 cyc/SIMD >= the 40-cyc dependent latency
         * (extra pairs measured slower — register pressure only) */
        v4f cre = {0.f, 0.f, 0.f, 0.f};
        v4f cim = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KK / 4; s++) {
            float a_re = s_re[mfma_swz(ab + 4 * s)];
            float a_im = s_im[mfma_swz(ab + 4 * s)];
            cre = __builtin_amdgcn_mfma_f32_16x16x4f32(a_re, bfrag[s], cre,
                                                       0, 0, 0);
            cim = __builtin_amdgcn_mfma_f32_16x16x4f32(a_im, bfrag[s], cim,
                                                       0, 0, 0);
        }
        /* C layout: col = lane&15, row = (lane>>4)*4 + q (cdna4 16x16) */
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int row = k4 * 4 + q;
            long long o = out_base + (long long)wave * 256 + 16 * row + r16;
            if (o < n_out) out[o] = make_float2(cre[q], cim[q]);
        }
        __syncthreads();
    }
}

/* ---- MFMA FIR, 32x32x2 variant --------------------------------------- *
 * Same implicit GEMM as k_fir_mfma_tpl but on v_mfma_f32_32x32x2_f32:
 * one 32x32 C tile pair (re+im) = 1024 outputs per WAVE, single-wave
 * blocks — 4x less staging and barrier overhead per output than the
 * 16x16 shape (at the cost of K = T+31 shift inflation). B fragments are
 * re-read from LDS per tile (80 broadcast reads) to keep registers for
 * occupancy. A-plane XOR swizzle: idx ^ (((idx>>5)&15)<<1) makes the
 * 32-dword row stride conflict-free up to a residual 2-way (rows r,
 * r+16) while preserving even-pair adjacency for the staging writes. */
__device__ __forceinline__ unsigned mfma32_swz(unsigned idx) {
    return idx ^ (((idx >> 5) & 15u) << 1);
}

#define MFIR32_BLOCK 64
#define MFIR32_TILE 1024 /* one wave, one 32x32 C pair */

typedef float v16f __attribute__((ext_vector_type(16)));

template <int KK2>
__global__ __launch_bounds__(MFIR32_BLOCK) void k_fir_mfma32_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtaps /* reversed, zero-filled to KK2 */,
    long long n_out, long long n_in_valid) {
    static_assert(KK2 % 2 == 0, "KK2 must be even");
    const unsigned elems = MFIR32_TILE + KK2 + 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_re = (float*)smem;
    float* s_im = s_re + ((elems + 31u) & ~31u);
    float* s_rtx = s_im + ((elems + 31u) & ~31u); /* 31 zeros + rt + 1 */

    const int tid = threadIdx.x;
    const int r32 = tid & 31; /* A row / C col */
    const int k2 = tid >> 5;  /* k sub-slice 0..1 */

    for (int i = tid; i < KK2 + 32; i += MFIR32_BLOCK)
        s_rtx[i] = (i >= 31 && i < 31 + KK2) ? rtaps[i - 31] : 0.f;
    __syncthreads();

    constexpr int NL =
        (MFIR32_TILE + KK2 + 8 + 2 * MFIR32_BLOCK - 1) / (2 * MFIR32_BLOCK);
    float4 stg[NL];
    auto load_tile = [&](long long tl) {
        const long long ob = tl * MFIR32_TILE;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            unsigned i = 2 * (tid + j * MFIR32_BLOCK);
            long long g = ob + i;
            float2 v0 = (i < elems && g < n_in_valid)
                            ? in[g] : make_float2(0.f, 0.f);
            float2 v1 = (i + 1 < elems && g + 1 < n_in_valid)
                            ? in[g + 1] : make_float2(0.f, 0.f);
            stg[j] = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    };
    load_tile(blockIdx.x);
    for (long long tile = blockIdx.x;
         tile * (long long)MFIR32_TILE < n_out; tile += gridDim.x) {
        const long long out_base = tile * MFIR32_TILE;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            unsigned i = 2 * (tid + j * MFIR32_BLOCK);
            if (i < elems) {
                unsigned d = mfma32_swz(i);
                *(float2*)&s_re[d] = make_float2(stg[j].x, stg[j].z);
                *(float2*)&s_im[d] = make_float2(stg[j].y, stg[j].w);
            }
        }
        __syncthreads();
        if ((tile + gridDim.x) * (long long)MFIR32_TILE < n_out)
            load_tile(tile + gridDim.x);

        const unsigned ab = 32u * r32 + k2;
        v16f cre = {};
        v16f cim = {};
#pragma unroll
        for (int s = 0; s < KK2 / 2; s++) {
            float b = s_rtx[31 + 2 * s + k2 - r32];
            float a_re = s_re[mfma32_swz(ab + 2 * s)];
            float a_im = s_im[mfma32_swz(ab + 2 * s)];
            cre = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re, b, cre, 0, 0, 0);
            cim = __builtin_amdgcn_mfma_f32_32x32x2f32(a_im, b, cim, 0, 0, 0);
        }
        /* C layout (cdna4 32x32): col = lane&31,
         * row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) */
#pragma unroll
        for (int q = 0; q < 16; q++) {
            int row = (q & 3) + 8 * (q >> 2) + 4 * k2;
            long long o = out_base + 32 * row + r32;
            if (o < n_out) out[o] = make_float2(cre[q], cim[q]);
        }
        __syncthreads();
    }
}

/* ---- MFMA phase-split decimating FIR (D=4) --------------------------- *
 * decimating_fir.rs:80-95 semantics via the phase decomposition
 * (t = 4u+v => y[k] = sum_v sum_u P_v[k+u]*rtv[v][u], P_v[i] = x[3+v+4i])
 * with each phase dot-product run as the same implicit GEMM as
 * k_fir_mfma_tpl: C accumulates over all 4 phases. KKD >= ceil(T/4)+15,
 * KKD%4==0. Staging is software-pipelined across the tile loop.
 *
 * The family is built from the chain_* pieces below, each written once:
 *   k_decim4_mfma_tpl       halves staging + store-C-rows epilogue
 *   k_decim4_fft_mfma_tpl   halves staging + FFT epilogue (+ stagger)
 *   k_decim4_fft_mfma2_tpl  the same at 512 threads / 2048 outputs, with
 *                           a two-frame fft1024_block epilogue
 *   k_decim4_fft_mfma_ap_tpl  all-phase staging + FFT epilogue
 *   k_decim4_fft_mfma_ws_tpl  all-phase staging, FFT pipelined into the
 *                             next tile's MFMA phases
 *   k_mfma_ubench_tpl, k_chain_ubench_tpl  diagnostics */
#define MDFIR_BLOCK 256
#define MDFIR_TILE 1024 /* decimated outputs per block */

/* forward declarations (defined with the FFT kernel below): in-block
 * forward Stockham FFT over swizzled LDS ping/pong buffers. fft_pow2_fwd
 * runs any pow2 n (radix-4 + radix-2 tail) with tpf threads striding the
 * butterflies and returns the buffer holding the result; ALL threads of
 * the block must call it with the same n (block-wide barriers inside). */
__device__ float2* fft_pow2_fwd(float2* a, float2* b,
                                const float2* __restrict__ twid, int n,
                                int tf, int tpf);
__device__ void fft1024_block(float2* ping, float2* pong,
                              const float2* __restrict__ twid, int tf);
/* fft1024_block result lands in `pong` (5 swaps); read pong[fft_swz(i)] */

/* LDS twiddle table of the ws kernel: stage s (0..4) holds 256 >> 2s
 * entries starting at ws_tw_off(s) = 0, 256, 320, 336, 340. */
#define WS_TW_ENTRIES 341
__host__ __device__ constexpr unsigned ws_tw_off(int s) {
    return (1024u - (1024u >> (2 * s))) / 3u;
}

/* Geometry of the family's LDS layouts, shared by the kernels (which
 * carve their pointers from the *_rtx/ws_fbuf offsets) and the launchers
 * (which request the *_bytes): the two cannot disagree.
 *
 * Each phase plane is split into 4 sub-planes by element%4 so a lane's
 * MFMA K-walk (idx = ab+4s) becomes stride-1: one ds_read_b128 feeds 4
 * K-steps (the b32-per-MFMA A-reads were the round-1 issue-stall,
 * SQ_WAIT_INST_ANY 46% — profiles/pmc_r02).
 *
 * halves: two phases resident at a time ([re_v0, re_v1, im_v0, im_v1]) —
 *   halves LDS vs all-phase planes, doubling resident blocks/CU;
 *   accumulators carry across the two halves, and each half's global
 *   loads are issued under the other half's MFMAs. The 512-thread kernel
 *   is this layout at <KKD, 512, 2048>.
 * ap: all 4 phases resident ([8][SPm]: re v0..3, im v0..3).
 * ws: ap + a 1024-entry in-place FFT strip + the WS_TW_ENTRIES twiddles. */
template <int KKD_, int BLOCK_ = MDFIR_BLOCK, int TILE_ = MDFIR_TILE>
struct ChainGeom {
    static_assert(KKD_ % 4 == 0, "KKD must be a multiple of 4");
    static constexpr int KKD = KKD_, BLOCK = BLOCK_, TILE = TILE_;
    static constexpr unsigned elemsP = TILE + KKD + 8; /* per phase plane */
    static constexpr unsigned SPm = (elemsP + 31u) & ~31u;
    static constexpr unsigned SUB = SPm / 4;
    static constexpr unsigned span = 3 + 4 * elemsP; /* input elems/tile */
    static constexpr int NL2 = (2 * elemsP + 3 + BLOCK - 1) / BLOCK;
    static constexpr unsigned GROUPS = elemsP + 1; /* aligned 4-groups */
    static constexpr int NG = (GROUPS + BLOCK - 1) / BLOCK;
    static constexpr int RTW = KKD + 16; /* s_rtx row: 15 zeros + KKD + 1 */
    /* float offsets into the dynamic LDS segment */
    static constexpr unsigned halves_rtx = 4 * SPm;
    static constexpr unsigned ap_rtx = 8 * SPm;
    static constexpr unsigned ws_fbuf = ap_rtx + 4 * RTW;
    static constexpr size_t halves_bytes =
        (halves_rtx + 4 * RTW) * sizeof(float);
    static constexpr size_t ap_bytes = (ap_rtx + 4 * RTW) * sizeof(float);
    static constexpr size_t ws_bytes =
        ws_fbuf * sizeof(float) + (1024 + WS_TW_ENTRIES) * sizeof(float2);
};

/* A thread's place in the 16x16x4 MFMA tiling. Its K-walk in a sub-plane:
 * sub = k4 (asub), dword offset abase + s = wave*64 + 4*r16 + s —
 * stride-1 in s, 16 B aligned at s%4==0. */
struct chain_lane {
    int tid, wave, r16, k4;
    unsigned abase, asub;
};
template <class G>
__device__ __forceinline__ chain_lane chain_lane_of(int tid) {
    const int lane = tid & 63;
    const int r16 = lane & 15, k4 = lane >> 4;
    const int wave = tid >> 6;
    return {tid, wave, r16, k4, (unsigned)wave * 64 + 4u * r16,
            (unsigned)k4 * G::SUB};
}

/* s_rtx[4][KKD+16]: phase v's taps rtv[v][0..KKD) behind a 15-zero
 * prologue (the B fragment of output row r reads at 15 + k - r). */
template <class G>
__device__ __forceinline__ void chain_load_taps(
    float* s_rtx, const float* __restrict__ rtv, int tid) {
    for (int i = tid; i < 4 * G::RTW; i += G::BLOCK) {
        int v = i / G::RTW, t = i % G::RTW;
        s_rtx[i] =
            (t >= 15 && t < 15 + G::KKD) ? rtv[v * G::KKD + (t - 15)] : 0.f;
    }
}

/* The K-walk of one phase v over its re/im planes: b128 groups [g0,g1)
 * and, if `tail`, the non-multiple-of-4 K remainder. g0/g1 let the ws
 * kernel split a phase across two FFT-stage windows. PRIO brackets the
 * run with s_setprio to boost MFMA waves over the FFT/staging phases of
 * co-resident blocks (T5); the bare-loop ubench runs without it.
 *
 * b128 A-reads: one ds_read_b128 pair feeds 8 MFMAs (4 K-steps x
 * re/im), cutting the per-MFMA issue overhead (round-1 b32 reads:
 * SQ_WAIT_INST_ANY-heavy, profiles/pmc_sq_r02.txt). One accumulator
 * pair, re/im alternating: same-C spacing = 2 MFMA issues = 64
 * cyc/SIMD >= the 40-cyc dependent latency, so extra accumulator
 * pairs only cost registers (measured: dual pairs were ~3% slower,
 * forcing 8 waves/SIMD via VGPR caps 2x slower from spills). */
template <class G, bool PRIO = true>
__device__ __forceinline__ void chain_mfma_phase(
    const float* re_plane, const float* im_plane, const float* s_rtx, int v,
    const chain_lane& ln, v4f& cre, v4f& cim, int g0 = 0,
    int g1 = (G::KKD / 4) / 4, bool tail = true) {
    constexpr int KKD = G::KKD;
    const float* pre = re_plane + ln.asub;
    const float* pim = im_plane + ln.asub;
    const unsigned abase = ln.abase;
    float bfrag[KKD / 4];
#pragma unroll
    for (int s = 0; s < KKD / 4; s++)
        bfrag[s] = s_rtx[v * G::RTW + 15 + 4 * s + ln.k4 - ln.r16];
    if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < (KKD / 4) / 4; t++) {
        if (t < g0 || t >= g1) continue;
        float4 ar = *(const float4*)&pre[abase + 4 * t];
        float4 ai = *(const float4*)&pim[abase + 4 * t];
        cre = __builtin_amdgcn_mfma_f32_16x16x4f32(ar.x, bfrag[4 * t],
                                                   cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_16x16x4f32(ai.x, bfrag[4 * t],
                                                   cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ar.y, bfrag[4 * t + 1], cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ai.y, bfrag[4 * t + 1], cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ar.z, bfrag[4 * t + 2], cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ai.z, bfrag[4 * t + 2], cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ar.w, bfrag[4 * t + 3], cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ai.w, bfrag[4 * t + 3], cim, 0, 0, 0);
    }
    if (tail) {
#pragma unroll
        for (int s = (KKD / 4) & ~3; s < KKD / 4; s++) {
            float a_re = pre[abase + s];
            float a_im = pim[abase + s];
            cre = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a_re, bfrag[s], cre, 0, 0, 0);
            cim = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a_im, bfrag[s], cim, 0, 0, 0);
        }
    }
    if (PRIO) __builtin_amdgcn_s_setprio(0);
}

/* -- halves staging: phases {2h, 2h+1} of a tile at a time -------------- */

/* elements of phases {2h, 2h+1}: rel = 3 + 4i + 2h + vloc; samples at or
 * past n_in_valid read as zero */
template <class G>
__device__ __forceinline__ void chain_load_half(
    const float2* __restrict__ in, long long tl, int h,
    long long n_in_valid, int tid, float2 (&stg)[G::NL2]) {
    const long long ib = tl * G::TILE * 4;
#pragma unroll
    for (int j = 0; j < G::NL2; j++) {
        unsigned idx = (unsigned)(tid + j * G::BLOCK);
        unsigned rel = 3 + 4 * (idx >> 1) + 2 * h + (idx & 1u);
        long long g = ib + rel;
        stg[j] = (rel < G::span && g < n_in_valid) ? in[g]
                                                   : make_float2(0.f, 0.f);
    }
}

template <class G>
__device__ __forceinline__ void chain_write_half(
    float* planes, int tid, const float2 (&stg)[G::NL2]) {
#pragma unroll
    for (int j = 0; j < G::NL2; j++) {
        unsigned idx = (unsigned)(tid + j * G::BLOCK);
        unsigned i = idx >> 1, vloc = idx & 1u;
        if (i < G::elemsP) {
            unsigned d = (i & 3u) * G::SUB + (i >> 2);
            planes[vloc * G::SPm + d] = stg[j].x;
            planes[(2 + vloc) * G::SPm + d] = stg[j].y;
        }
    }
}

/* the two resident phases of half h */
template <class G, bool PRIO = true>
__device__ __forceinline__ void chain_mfma_half(
    const float* planes, const float* s_rtx, int h, const chain_lane& ln,
    v4f& cre, v4f& cim, bool tail = true) {
#pragma unroll
    for (int vloc = 0; vloc < 2; vloc++)
        chain_mfma_phase<G, PRIO>(planes + (unsigned)vloc * G::SPm,
                                  planes + (unsigned)(2 + vloc) * G::SPm,
                                  s_rtx, 2 * h + vloc, ln, cre, cim, 0,
                                  (G::KKD / 4) / 4, tail);
}

/* -- all-phase staging (ap, ws) ----------------------------------------- *
 * Staging by ALIGNED 4-sample groups: group q = x[4q..4q+3] = two 16B
 * float4 loads (x is 32B-aligned at 4q when the base pointer is
 * 16B-aligned — host guards). Sample x[4q+w] belongs to phase v=(w+1)&3
 * at position q (w==3) or q-1 (w<3), since P_v[i] = x[3+v+4i]. Halves
 * the VMEM instruction count vs float2 loads — the incremental ubench
 * showed the staging loads cost ~25 points of MFMA-pipe utilization
 * (issue/latency interference). */

/* Staging loader of the ap and ws chain kernels: tile tl's aligned
 * 4-sample groups q = tid + j*BLOCK (group q = x[4q..4q+3] past the
 * tile base = two 16B loads) into stqa[j]/stqb[j]; samples at or past
 * n_in_valid read as zero.
 *
 * Interior tiles — every sample the tile stages lies below n_in_valid, a
 * block-uniform test — take a straight-line path: all 2*NG loads issue
 * back to back and the consumer waits with counted vmcnt as it uses each
 * group. The last j keeps its q < GROUPS lane predicate (exec mask only,
 * no else-arm), so nothing past the staged range is fetched. With the
 * per-lane guard on every group instead, its else-arm's narrow loads share
 * destination registers with the wide ones and the compiler drains
 * vmcnt(0) before each group: NG dependent HBM round trips per tile
 * (profiles/chain_staging_loads.txt). Only boundary tiles pay that now. */
template <class G>
__device__ __forceinline__ void chain_stage_load(
    const float2* __restrict__ in, long long tl, long long n_in_valid,
    int tid, float4 (&stqa)[G::NG], float4 (&stqb)[G::NG]) {
    constexpr unsigned GROUPS = G::GROUPS;
    constexpr int NG = G::NG;
    const long long qb = tl * G::TILE;
    if ((qb + GROUPS) * 4 <= n_in_valid) {
        const float4* p = (const float4*)(in + (qb + tid) * 4);
#pragma unroll
        for (int j = 0; j < NG; j++) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)(j + 1) * G::BLOCK <= GROUPS ||
                (unsigned)(tid + j * G::BLOCK) < GROUPS) {
                a = p[2 * j * G::BLOCK];
                b = p[2 * j * G::BLOCK + 1];
            }
            stqa[j] = a;
            stqb[j] = b;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NG; j++) {
        unsigned q = (unsigned)(tid + j * G::BLOCK);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < GROUPS) {
            long long xq = (qb + q) * 4;
            if (xq + 3 < n_in_valid) {
                a = *(const float4*)&in[xq];
                b = *(const float4*)&in[xq + 2];
            } else {
                float2 e0 = (xq < n_in_valid) ? in[xq]
                                              : make_float2(0.f, 0.f);
                float2 e1 = (xq + 1 < n_in_valid)
                                ? in[xq + 1] : make_float2(0.f, 0.f);
                float2 e2 = (xq + 2 < n_in_valid)
                                ? in[xq + 2] : make_float2(0.f, 0.f);
                float2 e3 = (xq + 3 < n_in_valid)
                                ? in[xq + 3] : make_float2(0.f, 0.f);
                a = make_float4(e0.x, e0.y, e1.x, e1.y);
                b = make_float4(e2.x, e2.y, e3.x, e3.y);
            }
        }
        stqa[j] = a;
        stqb[j] = b;
    }
}

/* The staged groups into the 8 phase planes. PIN (ws) uses the group on
 * every path, not only under the lane predicates below: the compiler then
 * waits for it here, with a counted vmcnt, and knows at the next
 * chain_stage_load that no staging load is pending. With the waits only
 * inside the predicated blocks it assumed they might have been skipped
 * and drained vmcnt(0), the output stores included, before reusing these
 * registers for the next tile's loads.
 *
 * planes and tid come by reference, as the kernels' capturing lambdas
 * hand them on: taken by value the compiler shares the per-group plane
 * offsets differently and the ws kernel's instruction stream moves
 * (tools/isa_diff.py against the build before). */
template <class G, bool PIN>
__device__ __forceinline__ void chain_write_all(
    float* const& planes, const int& tid, const float4 (&stqa)[G::NG],
    const float4 (&stqb)[G::NG]) {
    constexpr unsigned SPm = G::SPm, SUB = G::SUB;
#pragma unroll
    for (int j = 0; j < G::NG; j++) {
        unsigned q = (unsigned)(tid + j * G::BLOCK);
        float4 a = stqa[j], b = stqb[j];
        if (PIN)
            asm volatile("" ::"v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w),
                         "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w));
        if (q >= G::GROUPS) continue;
        if (q >= 1) { /* w=0,1,2 -> phases 1,2,3 at position q-1 */
            unsigned d1 = ((q - 1) & 3u) * SUB + ((q - 1) >> 2);
            planes[1u * SPm + d1] = a.x;
            planes[5u * SPm + d1] = a.y;
            planes[2u * SPm + d1] = a.z;
            planes[6u * SPm + d1] = a.w;
            planes[3u * SPm + d1] = b.x;
            planes[7u * SPm + d1] = b.y;
        }
        if (q < G::elemsP) { /* w=3 -> phase 0 at position q */
            unsigned d0 = (q & 3u) * SUB + (q >> 2);
            planes[0u * SPm + d0] = b.z;
            planes[4u * SPm + d0] = b.w;
        }
    }
}

/* -- epilogues ----------------------------------------------------------- */

/* store the tile's C rows: the filter-level output y2 */
__device__ __forceinline__ void chain_store_rows(
    float2* __restrict__ out, long long out_base, long long n_out,
    const chain_lane& ln, const v4f& cre, const v4f& cim) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        int row = ln.k4 * 4 + q;
        long long o = out_base + (long long)ln.wave * 256 + 16 * row + ln.r16;
        if (o < n_out) out[o] = make_float2(cre[q], cim[q]);
    }
}

/* The FFT epilogue of the halves and ap kernels (deposit C swizzled,
 * fft_pow2_fwd, guarded spectrum and |X|^2 stores) stays written out in
 * both: behind one helper, in every parameter shape tried, the ap tile
 * loop keeps its instructions but shifts its register allocation, and
 * that loop is held to the stream that was measured (tools/isa_diff.py,
 * profiles/chain_refactor.txt). */

/* -- kernels -------------------------------------------------------------- */

template <int KKD>
__global__ __launch_bounds__(MDFIR_BLOCK) void k_decim4_mfma_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtv /* [4][KKD], rtv[v][u] = rt[4u+v] */,
    long long n_out, long long n_in_valid) {
    using G = ChainGeom<KKD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* planes = (float*)smem;           /* [4][SPm] */
    float* s_rtx = planes + G::halves_rtx;  /* [4][KKD+16] */
    const chain_lane ln = chain_lane_of<G>(threadIdx.x);
    const int tid = ln.tid;

    chain_load_taps<G>(s_rtx, rtv, tid);
    __syncthreads();

    float2 stgA[G::NL2], stgB[G::NL2];
    auto load_half = [&](long long tl, int h, float2 (&stg)[G::NL2]) {
        chain_load_half<G>(in, tl, h, n_in_valid, tid, stg);
    };
    auto write_half = [&](const float2 (&stg)[G::NL2]) {
        chain_write_half<G>(planes, tid, stg);
    };
    auto mfma_half = [&](int h, v4f& cre, v4f& cim) {
        chain_mfma_half<G>(planes, s_rtx, h, ln, cre, cim);
    };

    load_half(blockIdx.x, 0, stgA);
    for (long long tile = blockIdx.x;
         tile * (long long)G::TILE < n_out; tile += gridDim.x) {
        v4f cre = {0.f, 0.f, 0.f, 0.f};
        v4f cim = {0.f, 0.f, 0.f, 0.f};
        write_half(stgA);
        __syncthreads();
        load_half(tile, 1, stgB);     /* in flight under half-0 MFMAs */
        mfma_half(0, cre, cim);
        __syncthreads();
        write_half(stgB);
        __syncthreads();
        if ((tile + gridDim.x) * (long long)G::TILE < n_out)
            load_half(tile + gridDim.x, 0, stgA); /* under half-1 MFMAs */
        mfma_half(1, cre, cim);
        chain_store_rows(out, tile * G::TILE, n_out, ln, cre, cim);
        __syncthreads();
    }
}

template <int KKD, int MINWG = 1>
__global__ __launch_bounds__(MDFIR_BLOCK, MINWG) void k_decim4_fft_mfma_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtv /* [4][KKD], rtv[v][u] = rt[4u+v] */,
    long long n_out, long long n_in_valid,
    const float2* __restrict__ twid /* fft_len-entry forward table */,
    float* __restrict__ mag_out /* nullable |X|^2 */,
    int fft_len /* pow2 64..1024; tile = 1024/fft_len frames */,
    int stagger /* s_sleep(7) loops per co-residency slot: desyncs the
                   per-tile phases of co-resident blocks so one block's
                   staging/FFT interval overlaps the others' MFMA runs
                   (the bare MFMA loop reaches 97% of peak —
                   tools/mfma_ubench.py — so pipe idle = phase lock) */) {
    using G = ChainGeom<KKD>;
    if (stagger > 0) {
        int loops = (int)(blockIdx.x & 7u) * stagger;
        for (int i = 0; i < loops; i++) __builtin_amdgcn_s_sleep(7);
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* planes = (float*)smem;           /* [4][SPm] */
    float* s_rtx = planes + G::halves_rtx;  /* [4][KKD+16] */
    const chain_lane ln = chain_lane_of<G>(threadIdx.x);
    const int tid = ln.tid;

    chain_load_taps<G>(s_rtx, rtv, tid);
    __syncthreads();

    float2 stgA[G::NL2], stgB[G::NL2];
    auto load_half = [&](long long tl, int h, float2 (&stg)[G::NL2]) {
        chain_load_half<G>(in, tl, h, n_in_valid, tid, stg);
    };
    auto write_half = [&](const float2 (&stg)[G::NL2]) {
        chain_write_half<G>(planes, tid, stg);
    };
    auto mfma_half = [&](int h, v4f& cre, v4f& cim) {
        chain_mfma_half<G>(planes, s_rtx, h, ln, cre, cim);
    };

    load_half(blockIdx.x, 0, stgA);
    for (long long tile = blockIdx.x;
         tile * (long long)G::TILE < n_out; tile += gridDim.x) {
        v4f cre = {0.f, 0.f, 0.f, 0.f};
        v4f cim = {0.f, 0.f, 0.f, 0.f};
        write_half(stgA);
        __syncthreads();
        load_half(tile, 1, stgB);     /* in flight under half-0 MFMAs */
        mfma_half(0, cre, cim);
        __syncthreads();
        write_half(stgB);
        __syncthreads();
        if ((tile + gridDim.x) * (long long)G::TILE < n_out)
            load_half(tile + gridDim.x, 0, stgA); /* under half-1 MFMAs */
        mfma_half(1, cre, cim);
        __syncthreads(); /* phase planes are dead; reuse them as FFT LDS */
        static_assert(G::TILE == 1024, "tile == 1024 decimated outputs");
        static_assert(2 * 1024 * 2 <= 4 * G::SPm,
                      "ping + pong (2 x 1024 float2) fit in 4 phase planes");
        const long long out_base = tile * G::TILE;
        float2* ping = (float2*)planes;       /* 1024 float2 = 8 KB */
        float2* pong = ping + 1024;
        const unsigned Lm = (unsigned)fft_len - 1u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int row = ln.k4 * 4 + q;
            unsigned pos = ln.wave * 256 + 16 * row + ln.r16; /* y2 idx */
            ping[(pos & ~Lm) | fft_swz(pos & Lm)] =
                make_float2(cre[q], cim[q]);
        }
        __syncthreads();
        { /* one FFT per frame; frames share the block in lockstep */
            const int F = 1024 / fft_len;
            const int tpf = MDFIR_BLOCK / F;
            const int fl = tid / tpf, tfr = tid - fl * tpf;
            float2* res = fft_pow2_fwd(ping + (size_t)fl * fft_len,
                                       pong + (size_t)fl * fft_len, twid,
                                       fft_len, tfr, tpf) -
                          (size_t)fl * fft_len; /* uniform base */
            for (int i = tid; i < 1024; i += MDFIR_BLOCK) {
                long long o = out_base + i;
                if (o < n_out) {
                    float2 v =
                        res[((unsigned)i & ~Lm) | fft_swz((unsigned)i & Lm)];
                    if (out) out[o] = v; /* null = NullSink'd spectra */
                    if (mag_out) mag_out[o] = v.x * v.x + v.y * v.y;
                }
            }
        }
        __syncthreads();
    }
}

/* All-phase staging variant (FSDR_CHAIN_ALLPHASE=1): all 4 phase planes
 * resident at once (8 planes, ~36 KB LDS -> 4 blocks/CU instead of 6),
 * ONE staging write + barrier per tile and a contiguous 160-MFMA run —
 * trades occupancy for fewer barrier convoys. Experiment for the
 * phase-structure bound documented in profiles/pmc_sq_r02.txt. */
template <int KKD>
__global__ __launch_bounds__(MDFIR_BLOCK) void k_decim4_fft_mfma_ap_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtv /* [4][KKD], rtv[v][u] = rt[4u+v] */,
    long long n_out, long long n_in_valid,
    const float2* __restrict__ twid /* fft_len-entry forward table */,
    float* __restrict__ mag_out /* nullable |X|^2 */,
    int fft_len) {
    using G = ChainGeom<KKD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* planes = (float*)smem;        /* [8][SPm]: re v0..3, im v0..3 */
    float* s_rtx = planes + G::ap_rtx;   /* [4][KKD+16] */
    const chain_lane ln = chain_lane_of<G>(threadIdx.x);
    const int tid = ln.tid;

    chain_load_taps<G>(s_rtx, rtv, tid);
    __syncthreads();

    float4 stqa[G::NG], stqb[G::NG];
    auto load_all = [&](long long tl) {
        chain_stage_load<G>(in, tl, n_in_valid, tid, stqa, stqb);
    };
    auto write_all = [&]() {
        chain_write_all<G, false>(planes, tid, stqa, stqb);
    };

    load_all(blockIdx.x);
    for (long long tile = blockIdx.x;
         tile * (long long)G::TILE < n_out; tile += gridDim.x) {
        v4f cre = {0.f, 0.f, 0.f, 0.f};
        v4f cim = {0.f, 0.f, 0.f, 0.f};
        write_all();
        __syncthreads();
        if ((tile + gridDim.x) * (long long)G::TILE < n_out)
            load_all(tile + gridDim.x); /* under this tile's MFMAs */
#pragma unroll
        for (int v = 0; v < 4; v++)
            chain_mfma_phase<G>(planes + (unsigned)v * G::SPm,
                                planes + (4u + v) * G::SPm, s_rtx, v, ln,
                                cre, cim);
        __syncthreads(); /* planes dead; reuse as FFT LDS */
        static_assert(2 * 1024 * 2 <= 8 * G::SPm,
                      "ping + pong (2 x 1024 float2) fit in the planes");
        const long long out_base = tile * G::TILE;
        float2* ping = (float2*)planes;
        float2* pong = ping + 1024;
        const unsigned Lm = (unsigned)fft_len - 1u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int row = ln.k4 * 4 + q;
            unsigned pos = ln.wave * 256 + 16 * row + ln.r16;
            ping[(pos & ~Lm) | fft_swz(pos & Lm)] =
                make_float2(cre[q], cim[q]);
        }
        __syncthreads();
        {
            const int F = 1024 / fft_len;
            const int tpf = MDFIR_BLOCK / F;
            const int fl = tid / tpf, tfr = tid - fl * tpf;
            float2* res = fft_pow2_fwd(ping + (size_t)fl * fft_len,
                                       pong + (size_t)fl * fft_len, twid,
                                       fft_len, tfr, tpf) -
                          (size_t)fl * fft_len;
            for (int i = tid; i < 1024; i += MDFIR_BLOCK) {
                long long o = out_base + i;
                if (o < n_out) {
                    float2 v =
                        res[((unsigned)i & ~Lm) | fft_swz((unsigned)i & Lm)];
                    if (out) out[o] = v;
                    if (mag_out) mag_out[o] = v.x * v.x + v.y * v.y;
                }
            }
        }
        __syncthreads();
    }
}

/* Software-pipelined variant (FSDR_CHAIN_WS=1, fft_len==1024 only):
 * tile t's FFT stages are interleaved between tile t+1's MFMA vloc
 * groups, so the FFT's VALU/LDS work issues inside the MFMA pipe's
 * 32-cyc/SIMD instruction shadow instead of serializing after it (the
 * incremental ubench priced the serial FFT at ~1800 CU-cyc/tile). The
 * FFT runs IN-PLACE (DIF radix-4, digit-reversed output read) in a
 * dedicated 8 KB LDS strip so staging planes stay resident; with the
 * 2.7 KB twiddle table ~48.3 KB LDS at K=80 (51.4 KB at K=144) ->
 * 3 blocks/CU (vs the ap kernel's 4). After the staging loads an
 * iteration issues no further VMEM instruction: twiddles come from LDS
 * and the outputs are stored ahead of the next iteration's loads. */
__device__ __forceinline__ unsigned rev4_10(unsigned i) {
    /* reverse 5 base-4 digits of a 10-bit index */
    unsigned r = 0;
#pragma unroll
    for (int d = 0; d < 5; d++) {
        r = (r << 2) | (i & 3u);
        i >>= 2;
    }
    return r;
}

template <int KKD>
__global__ __launch_bounds__(MDFIR_BLOCK, 3) void k_decim4_fft_mfma_ws_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtv, long long n_out, long long n_in_valid,
    const float2* __restrict__ twid /* 1024-entry forward table */,
    float* __restrict__ mag_out) {
    using G = ChainGeom<KKD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* planes = (float*)smem;              /* [8][SPm] */
    float* s_rtx = planes + G::ap_rtx;         /* [4][KKD+16] */
    float2* fbuf = (float2*)(planes + G::ws_fbuf); /* 1024 f2, in-place */
    float2* s_tw = fbuf + 1024;                /* [WS_TW_ENTRIES] */
    const chain_lane ln = chain_lane_of<G>(threadIdx.x);
    const int tid = ln.tid;

    chain_load_taps<G>(s_rtx, rtv, tid);
    /* The FFT stages' twiddles, once per block: stage s reads
     * twid[q << 2s], q < 256 >> 2s, kept as one compact run per stage
     * (256+64+16+4+1 entries, stage s at ws_tw_off(s)) so a stage's reads
     * are contiguous in LDS. A global load inside an FFT window would
     * return in order behind the next tile's staging loads and drain them
     * ahead of the window's barrier. */
    for (int i = tid; i < WS_TW_ENTRIES; i += MDFIR_BLOCK) {
        int s = (i >= 256) + (i >= 320) + (i >= 336) + (i >= 340);
        s_tw[i] = twid[(size_t)(i - ws_tw_off(s)) << (2 * s)];
    }
    __syncthreads();

    float4 stqa[G::NG], stqb[G::NG];
    auto load_all = [&](long long tl) {
        chain_stage_load<G>(in, tl, n_in_valid, tid, stqa, stqb);
    };
    auto write_all = [&]() {
        chain_write_all<G, true>(planes, tid, stqa, stqb);
    };
    /* one phase's K-walk, or its b128 groups [g0,g1) */
    auto mfma_phase = [&](int v, v4f& cre, v4f& cim, int g0, int g1,
                          bool tail) {
        chain_mfma_phase<G>(planes + (unsigned)v * G::SPm,
                            planes + (4u + v) * G::SPm, s_rtx, v, ln, cre,
                            cim, g0, g1, tail);
    };
    /* one in-place DIF radix-4 stage: 256 butterflies, 1 per thread.
     * Stage s: sub-length L = 1024>>(2s), quarter m = L/4; y_r stored
     * back at q + r*m with twiddles W_L^{rq} (derived from one load). */
    auto fft_stage = [&](int s) {
        const unsigned L = 1024u >> (2 * s);
        const unsigned m = L >> 2;
        unsigned bf = (unsigned)tid;
        unsigned blk = bf / m, q = bf - blk * m;
        unsigned base = blk * L + q;
        float2 x0 = fbuf[fft_swz(base)];
        float2 x1 = fbuf[fft_swz(base + m)];
        float2 x2 = fbuf[fft_swz(base + 2 * m)];
        float2 x3 = fbuf[fft_swz(base + 3 * m)];
        float2 t0 = f2_add(x0, x2), t1 = f2_sub(x0, x2);
        float2 t2 = f2_add(x1, x3), t3 = f2_sub(x1, x3);
        float2 t3r = make_float2(t3.y, -t3.x); /* -i * t3 (forward) */
        float2 w1 = s_tw[ws_tw_off(s) + q]; /* = twid[q << 2s] */
        float2 w2 = cmulf(w1, w1);
        float2 w3 = cmulf(w2, w1);
        fbuf[fft_swz(base)] = f2_add(t0, t2);
        fbuf[fft_swz(base + m)] = cmulf(f2_add(t1, t3r), w1);
        fbuf[fft_swz(base + 2 * m)] = cmulf(f2_sub(t0, t2), w2);
        fbuf[fft_swz(base + 3 * m)] = cmulf(f2_sub(t1, t3r), w3);
    };

    v4f cre = {0.f, 0.f, 0.f, 0.f};
    v4f cim = {0.f, 0.f, 0.f, 0.f};
    bool have_prev = false;
    long long prev_base = 0;
    /* A tile's spectrum leaves the FFT strip at the end of the iteration
     * that finishes its FFT, but is stored only in the next iteration,
     * between the staging write and the staging loads. VMEM retires in
     * order and vmcnt counts loads and stores alike: stored where they
     * are read, the stores would be younger than the staging loads in
     * flight, and chain_write_all's wait for the last group (vmcnt(0),
     * the number of stores not being static) would drain them at the loop
     * top, a store round trip per tile. Stored here they are older than
     * those loads; chain_write_all's unconditional waits (PIN) let the
     * compiler issue chain_stage_load behind them without a vmcnt wait,
     * so the next wait they meet is the next loop top's
     * (tests/test_chain_isa_cpu.py holds both).
     * Measured: -92 us of ~3640 on the bench's chain kernel; the wait
     * ahead of the staging loads alone, while it was there, cost nothing
     * measurable (profiles/chain_staging_loads.txt). */
    float2 held[4] = {};
    bool have_held = false;
    long long held_base = 0;
    auto store_held = [&]() {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            long long o = held_base + tid + k * MDFIR_BLOCK;
            if (o < n_out) {
                float2 v = held[k];
                if (out) out[o] = v;
                if (mag_out) mag_out[o] = v.x * v.x + v.y * v.y;
            }
        }
    };
    load_all(blockIdx.x);
    for (long long tile = blockIdx.x;
         tile * (long long)MDFIR_TILE < n_out; tile += gridDim.x) {
        write_all();
        if (have_prev) { /* deposit C(prev) into the FFT strip */
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int row = ln.k4 * 4 + q;
                unsigned pos = ln.wave * 256 + 16 * row + ln.r16;
                fbuf[fft_swz(pos)] = make_float2(cre[q], cim[q]);
            }
        }
        if (have_held) store_held(); /* ahead of the staging loads */
        __syncthreads();
        if ((tile + gridDim.x) * (long long)MDFIR_TILE < n_out)
            load_all(tile + gridDim.x);
        cre = (v4f){0.f, 0.f, 0.f, 0.f};
        cim = (v4f){0.f, 0.f, 0.f, 0.f};
        constexpr int NB = (KKD / 4) / 4; /* b128 groups per phase */
        constexpr int GH = NB / 2;
        mfma_phase(0, cre, cim, 0, NB, true);
        if (have_prev) fft_stage(0);
        __syncthreads();
        mfma_phase(1, cre, cim, 0, NB, true);
        if (have_prev) fft_stage(1);
        __syncthreads();
        mfma_phase(2, cre, cim, 0, NB, true);
        if (have_prev) fft_stage(2);
        __syncthreads();
        mfma_phase(3, cre, cim, 0, GH, false);
        if (have_prev) fft_stage(3);
        __syncthreads();
        mfma_phase(3, cre, cim, GH, NB, true);
        if (have_prev) fft_stage(4);
        __syncthreads();
        if (have_prev) { /* spectrum of prev: out of the strip, held */
#pragma unroll
            for (int k = 0; k < 4; k++)
                held[k] = fbuf[fft_swz(
                    rev4_10((unsigned)(tid + k * MDFIR_BLOCK)))];
            held_base = prev_base;
            have_held = true;
        }
        prev_base = tile * MDFIR_TILE;
        have_prev = true;
        __syncthreads();
    }
    if (have_held) store_held();
    /* epilogue: FFT + output of the final tile */
    if (have_prev) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int row = ln.k4 * 4 + q;
            unsigned pos = ln.wave * 256 + 16 * row + ln.r16;
            fbuf[fft_swz(pos)] = make_float2(cre[q], cim[q]);
        }
        __syncthreads();
        for (int s = 0; s < 5; s++) {
            fft_stage(s);
            __syncthreads();
        }
        for (int i = tid; i < 1024; i += MDFIR_BLOCK) {
            long long o = prev_base + i;
            if (o < n_out) {
                float2 v = fbuf[fft_swz(rev4_10((unsigned)i))];
                if (out) out[o] = v;
                if (mag_out) mag_out[o] = v.x * v.x + v.y * v.y;
            }
        }
    }
}

/* 512-thread experiment (FSDR_CHAIN_BLOCK512): the halves tile loop at
 * twice the block and tile, two 1024-pt FFT frames per tile. */
template <int KKD>
__global__ __launch_bounds__(512) void k_decim4_fft_mfma2_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtv /* [4][KKD], rtv[v][u] = rt[4u+v] */,
    long long n_out, long long n_in_valid,
    const float2* __restrict__ twid /* 1024-entry forward table */,
    float* __restrict__ mag_out /* nullable |X|^2 */) {
    using G = ChainGeom<KKD, 512, 2048>;
    static_assert(G::TILE == 2 * 1024 && G::BLOCK == 2 * 256,
                  "two 1024-pt FFT frames per tile, 256 threads each");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* planes = (float*)smem;           /* [4][SPm] */
    float* s_rtx = planes + G::halves_rtx;  /* [4][KKD+16] */
    const chain_lane ln = chain_lane_of<G>(threadIdx.x);
    const int tid = ln.tid;

    chain_load_taps<G>(s_rtx, rtv, tid);
    __syncthreads();

    float2 stgA[G::NL2], stgB[G::NL2];
    auto load_half = [&](long long tl, int h, float2 (&stg)[G::NL2]) {
        chain_load_half<G>(in, tl, h, n_in_valid, tid, stg);
    };
    auto write_half = [&](const float2 (&stg)[G::NL2]) {
        chain_write_half<G>(planes, tid, stg);
    };
    auto mfma_half = [&](int h, v4f& cre, v4f& cim) {
        chain_mfma_half<G>(planes, s_rtx, h, ln, cre, cim);
    };

    load_half(blockIdx.x, 0, stgA);
    for (long long tile = blockIdx.x;
         tile * (long long)G::TILE < n_out; tile += gridDim.x) {
        const long long out_base = tile * G::TILE;
        v4f cre = {0.f, 0.f, 0.f, 0.f};
        v4f cim = {0.f, 0.f, 0.f, 0.f};
        write_half(stgA);
        __syncthreads();
        load_half(tile, 1, stgB);     /* in flight under half-0 MFMAs */
        mfma_half(0, cre, cim);
        __syncthreads();
        write_half(stgB);
        __syncthreads();
        if ((tile + gridDim.x) * (long long)G::TILE < n_out)
            load_half(tile + gridDim.x, 0, stgA); /* under half-1 MFMAs */
        mfma_half(1, cre, cim);
        __syncthreads(); /* phase planes are dead; reuse them as FFT LDS:
                            frame f ping = fbase + f*2048, pong = +1024 */
        static_assert(2 * 2048 * 2 <= 4 * G::SPm,
                      "2 frames x (ping + pong) fit in 4 phase planes");
        float2* fbase = (float2*)planes; /* 4096 float2 = 32 KB */
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int row = ln.k4 * 4 + q;
            int pos = ln.wave * 256 + 16 * row + ln.r16; /* y2 index in tile */
            int fr = pos >> 10, idx = pos & 1023;
            fbase[fr * 2048 + fft_swz((unsigned)idx)] =
                make_float2(cre[q], cim[q]);
        }
        __syncthreads();
        {
            int fl = tid >> 8, tf = tid & 255;
            fft1024_block(fbase + fl * 2048, fbase + fl * 2048 + 1024,
                          twid, tf);
        }
        for (int i = tid; i < G::TILE; i += G::BLOCK) {
            long long o = out_base + i;
            if (o < n_out) {
                int fr = i >> 10, idx = i & 1023;
                float2 v = fbase[fr * 2048 + 1024 + fft_swz((unsigned)idx)];
                if (out) out[o] = v; /* null = NullSink'd spectra */
                if (mag_out) mag_out[o] = v.x * v.x + v.y * v.y;
            }
        }
        __syncthreads();
    }
}

/* MFMA-loop microbenchmark (tools/mfma_ubench.py): the decim kernel's
 * inner loop on LDS staged ONCE — no per-tile staging, no FFT, no
 * barriers in the hot loop, no setprio, b128 groups only (no K tail).
 * Measures the intrinsic ceiling of the b128-fed 16x16x4-f32 loop at
 * this occupancy. */
template <int KKD>
__global__ __launch_bounds__(MDFIR_BLOCK) void k_mfma_ubench_tpl(
    const float* __restrict__ rtv, float2* __restrict__ out, int iters) {
    using G = ChainGeom<KKD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* planes = (float*)smem;
    float* s_rtx = planes + G::halves_rtx;
    const chain_lane ln = chain_lane_of<G>(threadIdx.x);
    const int tid = ln.tid;
    chain_load_taps<G>(s_rtx, rtv, tid);
    for (int i = tid; i < (int)(4 * G::SPm); i += MDFIR_BLOCK)
        planes[i] = (float)(i & 255) * 0.001f;
    __syncthreads();
    v4f cre = {0.f, 0.f, 0.f, 0.f};
    v4f cim = {0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int vloc = 0; vloc < 2; vloc++)
            chain_mfma_phase<G, false>(
                planes + (unsigned)vloc * G::SPm,
                planes + (unsigned)(2 + vloc) * G::SPm, s_rtx,
                2 * ((it ^ vloc) & 1) + vloc, ln, cre, cim, 0,
                (KKD / 4) / 4, false);
    }
    long long o = (long long)blockIdx.x * MDFIR_BLOCK + tid;
    out[o] = make_float2(cre[0] + cre[1] + cre[2] + cre[3],
                         cim[0] + cim[1] + cim[2] + cim[3]);
}

/* Incremental chain ubench: the halves tile loop with components gated by
 * MODE to isolate the integration cost (tools/mfma_ubench.py):
 *   bit0 (1): global staging loads of the real input
 *   bit1 (2): LDS write_half phases + their barriers
 *   bit2 (4): deposit + in-block FFT + output writes
 * MODE 7 == the production kernel shape (the same chain_* calls; the K
 * tail is left out in every mode); MODE 0 ~= the bare loop. */
template <int KKD, int MODE>
__global__ __launch_bounds__(MDFIR_BLOCK) void k_chain_ubench_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtv, long long n_out, long long n_in_valid,
    const float2* __restrict__ twid) {
    using G = ChainGeom<KKD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* planes = (float*)smem;
    float* s_rtx = planes + G::halves_rtx;
    const chain_lane ln = chain_lane_of<G>(threadIdx.x);
    const int tid = ln.tid;
    chain_load_taps<G>(s_rtx, rtv, tid);
    for (int i = tid; i < (int)(4 * G::SPm); i += MDFIR_BLOCK)
        planes[i] = (float)(i & 255) * 0.001f;
    __syncthreads();
    constexpr int NL2 = G::NL2;
    float2 stgA[NL2], stgB[NL2];
    auto load_half = [&](long long tl, int h, float2 (&stg)[NL2]) {
        if (MODE & 1) {
            chain_load_half<G>(in, tl, h, n_in_valid, tid, stg);
        } else {
#pragma unroll
            for (int j = 0; j < NL2; j++)
                stg[j] = make_float2((float)(tid + j + h) * 1e-3f,
                                     (float)(tl & 63) * 1e-3f);
        }
    };
    auto write_half = [&](const float2 (&stg)[NL2]) {
        if (MODE & 2) {
            chain_write_half<G>(planes, tid, stg);
        } else { /* keep stg live without LDS traffic */
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < NL2; j++) acc += stg[j].x;
            if (acc == 1e30f) planes[tid] = acc; /* never taken */
        }
    };
    auto mfma_half = [&](int h, v4f& cre, v4f& cim) {
        chain_mfma_half<G>(planes, s_rtx, h, ln, cre, cim, false);
    };
    load_half(blockIdx.x, 0, stgA);
    for (long long tile = blockIdx.x;
         tile * (long long)MDFIR_TILE < n_out; tile += gridDim.x) {
        const long long out_base = tile * MDFIR_TILE;
        v4f cre = {0.f, 0.f, 0.f, 0.f};
        v4f cim = {0.f, 0.f, 0.f, 0.f};
        write_half(stgA);
        if (MODE & 2) __syncthreads();
        load_half(tile, 1, stgB);
        mfma_half(0, cre, cim);
        if (MODE & 2) __syncthreads();
        write_half(stgB);
        if (MODE & 2) __syncthreads();
        if ((tile + gridDim.x) * (long long)MDFIR_TILE < n_out)
            load_half(tile + gridDim.x, 0, stgA);
        mfma_half(1, cre, cim);
        if (MODE & 4) {
            __syncthreads();
            float2* ping = (float2*)planes;
            float2* pong = ping + 1024;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int row = ln.k4 * 4 + q;
                unsigned pos = ln.wave * 256 + 16 * row + ln.r16;
                ping[fft_swz(pos)] = make_float2(cre[q], cim[q]);
            }
            __syncthreads();
            fft1024_block(ping, pong, twid, tid);
            for (int i = tid; i < 1024; i += MDFIR_BLOCK) {
                long long o = out_base + i;
                if (o < n_out) out[o] = pong[fft_swz((unsigned)i)];
            }
            __syncthreads();
        } else {
            chain_store_rows(out, out_base, n_out, ln, cre, cim);
            if (MODE & 2) __syncthreads();
        }
    }
}

/* ---- template-size tables and their dispatch -------------------------- *
 * Each templated kernel family is instantiated for one table of sizes,
 * stated once here. The create functions pick the smallest entry that
 * fits (tpl_at_least, 0 if none does); the launchers map the stored
 * runtime value back onto the compile-time constant: tpl_dispatch calls
 * f(std::integral_constant<int, K>) for the matching K, or returns false. */
template <int... Ks>
struct tpl_table {};
using fir_tpl_tps = tpl_table<17, 33, 65, 129, 257, 513>;   /* TP >= T */
using fir_mfma_ks = tpl_table<32, 64, 96, 144, 272, 528>;   /* K >= T+15 */
using fir_mfma32_ks = tpl_table<48, 96, 160, 288, 544>;     /* K >= T+31 */
using decim4_tpl_tpds = tpl_table<8, 16, 32, 64, 128>;      /* 4*TPD >= T */
/* D=4 MFMA family: per-phase K = ceil(T/4)+15 rounded to 4 */
using decim4_mfma_ks = tpl_table<20, 32, 48, 80, 144>;

template <int... Ks>
static int tpl_at_least(tpl_table<Ks...>, size_t need) {
    for (int k : {Ks...})
        if ((size_t)k >= need) return k;
    return 0;
}
template <int... Ks, class F>
static bool tpl_dispatch(tpl_table<Ks...>, int k, F&& f) {
    return ((k == Ks && (f(std::integral_constant<int, Ks>{}), true)) || ...);
}

extern "C" int fsdr_chain_ubench(int mode, double* tflops, void* stream) {
    REQUIRE_GPU();
    using G = ChainGeom<80>;
    const int KKD = G::KKD;
    const long long n_out = 1 << 24; /* decimated outputs (2^26 inputs) */
    const long long n_in = 4 * n_out + 1024;
    dev_buf b_taps, b_in, b_out, b_tw; /* freed on every return */
    HIP_TRY(b_taps.ensure(4 * KKD * sizeof(float)));
    HIP_TRY(hipMemset(b_taps.ptr, 1, b_taps.bytes));
    HIP_TRY(b_in.ensure(n_in * sizeof(float2)));
    HIP_TRY(hipMemset(b_in.ptr, 2, b_in.bytes));
    HIP_TRY(b_out.ensure(n_out * sizeof(float2)));
    std::vector<float2> tw(1024);
    for (int k = 0; k < 1024; k++) {
        double a = -2.0 * M_PI * k / 1024.0;
        tw[k] = make_float2((float)cos(a), (float)sin(a));
    }
    HIP_TRY(b_tw.upload(tw.data(), tw.size()));
    float* d_taps = b_taps.as<float>();
    float2 *d_in = b_in.as<float2>(), *d_out = b_out.as<float2>(),
           *d_tw = b_tw.as<float2>();
    hipStream_t st = (hipStream_t)stream;
    int grid = 8192;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    for (int rep = 0; rep < 2; rep++) {
        if (rep == 1) HIP_TRY(hipEventRecord(e0, st));
        if (!tpl_dispatch(tpl_table<0, 1, 2, 3, 4, 6, 7>{}, mode, [&](auto m) {
                hipLaunchKernelGGL(
                    HIP_KERNEL_NAME(
                        (k_chain_ubench_tpl<G::KKD, decltype(m)::value>)),
                    dim3(grid), dim3(G::BLOCK), G::halves_bytes, st, d_in,
                    d_out, d_taps, n_out, n_in, d_tw);
            })) {
            set_err("mode must be in {0,1,2,3,4,6,7}");
            return FSDR_ERR_INVALID;
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    double fl = (double)n_out * 4 * KKD * 4.0; /* 4 phases x KKD x 4 */
    *tflops = fl / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return FSDR_OK;
}

extern "C" int fsdr_mfma_ubench(int grid, int iters, double* tflops,
                                void* stream) {
    REQUIRE_GPU();
    using G = ChainGeom<80>;
    const int KKD = G::KKD;
    const size_t lds = G::halves_bytes;
    dev_buf b_taps, b_out; /* freed on every return */
    HIP_TRY(b_taps.ensure(4 * KKD * sizeof(float)));
    HIP_TRY(hipMemset(b_taps.ptr, 1, b_taps.bytes));
    HIP_TRY(b_out.ensure((size_t)grid * MDFIR_BLOCK * sizeof(float2)));
    float* d_taps = b_taps.as<float>();
    float2* d_out = b_out.as<float2>();
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mfma_ubench_tpl<KKD>), dim3(grid),
                       dim3(MDFIR_BLOCK), lds, st, d_taps, d_out, iters);
    HIP_TRY(hipEventRecord(e0, st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mfma_ubench_tpl<KKD>), dim3(grid),
                       dim3(MDFIR_BLOCK), lds, st, d_taps, d_out, iters);
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    /* flops: grid blocks x 4 waves x iters x 2 vloc x KKD/4 steps x 2
     * (re+im) MFMAs x 2048 flops */
    double fl = (double)grid * 4 * iters * 2 * (KKD / 4) * 2 * 2048.0;
    *tflops = fl / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return FSDR_OK;
}

/* ---- Phase-split decimating FIR, D=4, compile-time taps -------------- *
 * Same math as decimating_fir.rs:80-95 (D=4): y[k] = sum_t x[3+4k+t] *
 * h[T-1-t]. Decompose t = 4u+v: y[k] = sum_v sum_u P_v[k+u] * rt[4u+v]
 * with P_v[i] = x[3+v+4i] and rt[t] = h[T-1-t] — four stride-1 sub-FIRs
 * over de-interleaved phase planes, staged at write time (free). Each
 * sub-FIR then uses the exact k_fir_cf32_tpl structure: conflict-free
 * 16 B lane-stride ds_read_b128 groups, affine offsets, pipelined loads.
 * TPD = per-phase padded tap count (multiple of 4, 4*TPD >= T). Plane
 * stride is 8 mod 32 dwords so the de-interleaving writes are
 * bank-conflict-free. */
#define DFIRT_BLOCK 256
#define DFIRT_R 4
#define DFIRT_TILE (DFIRT_BLOCK * DFIRT_R) /* 1024 decimated outputs */

__device__ __host__ __forceinline__ unsigned dfirt_sp(int tpd) {
    return ((((unsigned)(DFIRT_TILE + tpd + 12)) + 31u) & ~31u) + 8u;
}

template <int TPD>
__global__ __launch_bounds__(DFIRT_BLOCK) void k_fir_decim4_tpl(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ rtv /* [4][TPD+4], rtv[v][u]=rt[4u+v] */,
    long long n_out, long long n_in_valid) {
    static_assert(TPD % 4 == 0, "TPD must be a multiple of 4");
    const unsigned SP = dfirt_sp(TPD);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    /* two phases resident at a time: [re_v0, re_v1, im_v0, im_v1] — halves
     * the LDS footprint (8 -> 4 planes), doubling blocks/CU vs the
     * all-phases layout (the all-phase version was LDS-capacity-bound at
     * 4 blocks/CU). Accumulators carry across the two halves. */
    float* planes = (float*)smem;   /* [4][SP] */
    float* s_rt = planes + 4u * SP; /* [4][TPD+4] */

    const int tid = threadIdx.x;
    const unsigned span = 3 + 4 * (DFIRT_TILE + TPD + 8); /* input elems */
    for (long long tile = blockIdx.x;
         tile * (long long)DFIRT_TILE < n_out; tile += gridDim.x) {
        const long long out_base = tile * DFIRT_TILE;
        const long long in_base = out_base * 4;
        const unsigned eb = (unsigned)tid * DFIRT_R;
        float2 a01r = make_float2(0.f, 0.f), a23r = a01r;
        float2 a01i = a01r, a23i = a01r;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            /* stage phases v = 2*half, 2*half+1: input elements with
             * (rel-3) % 4 in {2h, 2h+1}; each element = P_v[i] at
             * rel = 3 + 4i + v */
            for (unsigned idx = tid; 2 * idx + 3 < span;
                 idx += DFIRT_BLOCK) {
                unsigned i = idx >> 1, vloc = idx & 1u;
                unsigned rel = 3 + 4 * i + 2 * half + vloc;
                if (rel >= span) continue;
                long long g = in_base + rel;
                float2 x = (g < n_in_valid) ? in[g] : make_float2(0.f, 0.f);
                planes[vloc * SP + i] = x.x;
                planes[(2 + vloc) * SP + i] = x.y;
            }
            if (half == 0)
                for (int i = tid; i < 4 * (TPD + 4); i += DFIRT_BLOCK)
                    s_rt[i] = rtv[i];
            __syncthreads();
#pragma unroll
            for (int vloc = 0; vloc < 2; vloc++) {
                const float* pre = planes + (unsigned)vloc * SP;
                const float* pim = planes + (unsigned)(2 + vloc) * SP;
                const float* rt =
                    s_rt + (unsigned)(2 * half + vloc) * (TPD + 4);
                float4 r0 = *(const float4*)&pre[eb];
                float4 r1 = *(const float4*)&pre[eb + 4];
                float4 i0 = *(const float4*)&pim[eb];
                float4 i1 = *(const float4*)&pim[eb + 4];
                float4 hc = *(const float4*)&rt[0];
                constexpr int NG = TPD / 4;
#pragma unroll 4
                for (int m = 0; m < NG; m++) {
                    const float4 rn = *(const float4*)&pre[eb + 4 * m + 8];
                    const float4 in_ = *(const float4*)&pim[eb + 4 * m + 8];
                    const float4 h4 = *(const float4*)&rt[4 * m + 4];
                    const float wr[8] = {r0.x, r0.y, r0.z, r0.w,
                                         r1.x, r1.y, r1.z, r1.w};
                    const float wi[8] = {i0.x, i0.y, i0.z, i0.w,
                                         i1.x, i1.y, i1.z, i1.w};
                    const float ht[4] = {hc.x, hc.y, hc.z, hc.w};
#pragma unroll
                    for (int tl = 0; tl < 4; tl++) {
                        const float h = ht[tl];
                        a01r.x = fmaf(wr[tl], h, a01r.x);
                        a01r.y = fmaf(wr[tl + 1], h, a01r.y);
                        a23r.x = fmaf(wr[tl + 2], h, a23r.x);
                        a23r.y = fmaf(wr[tl + 3], h, a23r.y);
                        a01i.x = fmaf(wi[tl], h, a01i.x);
                        a01i.y = fmaf(wi[tl + 1], h, a01i.y);
                        a23i.x = fmaf(wi[tl + 2], h, a23i.x);
                        a23i.y = fmaf(wi[tl + 3], h, a23i.y);
                    }
                    r0 = r1; r1 = rn;
                    i0 = i1; i1 = in_;
                    hc = h4;
                }
            }
            __syncthreads(); /* before restaging / next tile */
        }
        const float ar[4] = {a01r.x, a01r.y, a23r.x, a23r.y};
        const float ai[4] = {a01i.x, a01i.y, a23i.x, a23i.y};
#pragma unroll
        for (int j = 0; j < DFIRT_R; j++) {
            long long o = out_base + eb + j;
            if (o < n_out) out[o] = make_float2(ar[j], ai[j]);
        }
    }
}

typedef void (*dfir_tpl_fn)(const float2*, float2*, const float*, long long,
                            long long);

/* Generic decimating FIR (any D) — correctness fallback: one output per
 * lane per iteration, direct reads through L1/L2 (no LDS staging). */
__global__ void k_fir_decim_generic_cf32(const float2* __restrict__ in,
                                         float2* __restrict__ out,
                                         const float* __restrict__ taps,
                                         int n_taps, long long decim,
                                         long long n_out,
                                         long long n_in_valid) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         k < n_out; k += stride) {
        float sre = 0.f, sim = 0.f;
        long long base = decim - 1 + k * decim;
        for (int t = 0; t < n_taps; t++) {
            float2 x = (base + t < n_in_valid) ? in[base + t]
                                               : make_float2(0.f, 0.f);
            float h = taps[n_taps - 1 - t];
            sre = fmaf(x.x, h, sre);
            sim = fmaf(x.y, h, sim);
        }
        out[k] = make_float2(sre, sim);
    }
}

/* ================= FIR cf32 x cf32 (complex taps) ===================== *
 * FirFilter<Complex32,Complex32,Complex32> — fir.rs:257-277 (stable path):
 * accum + sample*tap with the num_complex multiply. This is the WLAN
 * SyncLong correlator core (examples/wlan/src/sync_long.rs:18-50, 64
 * complex taps). Correctness-first kernel: LDS-staged tile, one output
 * per lane x4 lane-strided (stride-1 LDS reads), taps staged in LDS.
 * An MFMA/window-optimized variant is a later-round item.
 */
__global__ __launch_bounds__(256) void k_fir_ccf32(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float2* __restrict__ taps, int n_taps, long long n_out,
    long long n_in_valid) {
    const unsigned TILE = 1024;
    const unsigned elems = TILE + n_taps - 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* s_x = (float2*)smem;          /* elems */
    float2* s_h = s_x + elems;            /* reversed taps */
    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x; tile * (long long)TILE < n_out;
         tile += gridDim.x) {
        const long long out_base = tile * TILE;
        for (unsigned i = tid; i < elems; i += 256) {
            long long g = out_base + i;
            s_x[i] = (g < n_in_valid) ? in[g] : make_float2(0.f, 0.f);
        }
        for (int i = tid; i < n_taps; i += 256)
            s_h[i] = taps[n_taps - 1 - i]; /* reversed */
        __syncthreads();
        for (int j = 0; j < 4; j++) {
            unsigned k = tid + j * 256;
            float sre = 0.f, sim = 0.f;
            for (int t = 0; t < n_taps; t++) {
                float2 x = s_x[k + t];
                float2 h = s_h[t];
                sre = fmaf(x.x, h.x, sre);
                sre = fmaf(-x.y, h.y, sre);
                sim = fmaf(x.x, h.y, sim);
                sim = fmaf(x.y, h.x, sim);
            }
            long long o = out_base + k;
            if (o < n_out) out[o] = make_float2(sre, sim);
        }
        __syncthreads();
    }
}

/* Parallel MovingAvg fast path (used when at most one emission occurs,
 * at the end of the processed frames — e.g. the bench's spectrum sink
 * with history == frames): the EMA recurrence is chunked over frames and
 * the per-chunk EMAs composed exactly:
 *   ema(chunk_0..c) = (1-d)^len_c * ema(chunk_0..c-1) + partial_c.
 *
 * Only chunks [c0, n_chunks) are computed and summed: the host proves the
 * weight om^(frames - end_c) of every earlier chunk is exactly 0.0f (see
 * movavg_horizon), so they cannot change a bit of the result. Partial
 * rows below c0 are never written nor read. */
#define MOVAVG_BATCH 16 /* loads issued per thread before it waits */

/* One EMA step. The loops used to say `om*p + decay*t` and leave the
 * rounding to the compiler's contraction, which chose differently in
 * the two shapes (read off the gfx950 ISA of the previous build): the
 * float4 loop was v_pk_mul + v_pk_fma, i.e. fma(decay, t, round(om*p)),
 * the scalar loop v_pk_mul + v_add, i.e. round(om*p) + round(decay*t).
 * Those two forms are now spelled out with contraction off, so the
 * output stays bit-identical to that build and no longer depends on how
 * the loop is unrolled or which compiler builds it. */
__device__ __forceinline__ float movavg_step_v4(float p, float t, float om,
                                                float decay) {
#pragma clang fp contract(off)
    const float m = om * p;
    return isfinite(t) ? fmaf(decay, t, m) : m;
}

__device__ __forceinline__ float movavg_step_s(float p, float t, float om,
                                               float decay) {
#pragma clang fp contract(off)
    const float m = om * p;
    const float d = decay * t;
    return isfinite(t) ? m + d : m;
}

__global__ void k_moving_avg_chunks(const float* __restrict__ in,
                                    float* __restrict__ partial, int width,
                                    long long frames, int n_chunks,
                                    int chunk_frames, float decay, int c0) {
    /* The frame loop is a serial recurrence, but its loads do not depend
     * on it: with few live chunks the kernel is load-latency bound, so
     * loads go out MOVAVG_BATCH at a time ahead of the dependent
     * multiply-adds. The per-bin operation order is that of the plain
     * loop. */
    const float om = 1.0f - decay;
    /* width % 4 == 0 fast shape: one float4 of bins per thread */
    if ((width & 3) == 0) {
        int w4 = width >> 2;
        long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
        long long total = (long long)(n_chunks - c0) * w4;
        long long stride = (long long)gridDim.x * blockDim.x;
        for (; id < total; id += stride) {
            int lc = (int)(id / w4);
            int b4 = (int)(id - (long long)lc * w4);
            int c = c0 + lc;
            long long f0 = (long long)c * chunk_frames;
            long long f1 = f0 + chunk_frames;
            if (f1 > frames) f1 = frames;
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            long long f = f0;
            for (; f + MOVAVG_BATCH <= f1; f += MOVAVG_BATCH) {
                v4f t[MOVAVG_BATCH];
#pragma unroll
                for (int u = 0; u < MOVAVG_BATCH; u++)
                    t[u] = *(const v4f*)&in[(f + u) * width + 4 * b4];
                /* left alone, the compiler sinks each load to its use to
                 * save registers and 2-3 stay in flight (a sched_barrier
                 * here does not hold them either): passing the whole
                 * batch through an empty asm makes it issue every load
                 * first; it then waits once per batch, not per frame */
                static_assert(MOVAVG_BATCH == 16, "operand list below");
                asm volatile(""
                             : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]),
                               "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]),
                               "+v"(t[8]), "+v"(t[9]), "+v"(t[10]),
                               "+v"(t[11]), "+v"(t[12]), "+v"(t[13]),
                               "+v"(t[14]), "+v"(t[15]));
#pragma unroll
                for (int u = 0; u < MOVAVG_BATCH; u++) {
                    p.x = movavg_step_v4(p.x, t[u].x, om, decay);
                    p.y = movavg_step_v4(p.y, t[u].y, om, decay);
                    p.z = movavg_step_v4(p.z, t[u].z, om, decay);
                    p.w = movavg_step_v4(p.w, t[u].w, om, decay);
                }
            }
            for (; f < f1; f++) {
                float4 t = *(const float4*)&in[f * width + 4 * b4];
                p.x = movavg_step_v4(p.x, t.x, om, decay);
                p.y = movavg_step_v4(p.y, t.y, om, decay);
                p.z = movavg_step_v4(p.z, t.z, om, decay);
                p.w = movavg_step_v4(p.w, t.w, om, decay);
            }
            *(float4*)&partial[(long long)c * width + 4 * b4] = p;
        }
        return;
    }
    long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long total = (long long)(n_chunks - c0) * width;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (; id < total; id += stride) {
        int lc = (int)(id / width);
        int b = (int)(id - (long long)lc * width);
        int c = c0 + lc;
        long long f0 = (long long)c * chunk_frames;
        long long f1 = f0 + chunk_frames;
        if (f1 > frames) f1 = frames;
        float p = 0.f;
        long long f = f0;
        for (; f + MOVAVG_BATCH <= f1; f += MOVAVG_BATCH) {
            float t[MOVAVG_BATCH];
#pragma unroll
            for (int u = 0; u < MOVAVG_BATCH; u++)
                t[u] = in[(f + u) * width + b];
#pragma unroll
            for (int u = 0; u < MOVAVG_BATCH; u++)
                p = movavg_step_s(p, t[u], om, decay);
        }
        for (; f < f1; f++)
            p = movavg_step_s(p, in[f * width + b], om, decay);
        partial[(long long)c * width + b] = p;
    }
}

__global__ void k_moving_avg_combine(const float* __restrict__ partial,
                                     float* __restrict__ avg,
                                     float* __restrict__ out /* nullable */,
                                     int width, long long frames,
                                     int n_chunks, int chunk_frames,
                                     float decay, int c0) {
    /* fully parallel closed form: result[b] = om^frames * avg[b] +
     * sum_c om^(frames - end_c) * partial[c][b]; one block per bin,
     * chunks spread over lanes, LDS tree reduction. Chunks below c0
     * carry weight 0.0f and are left out; the lane a chunk lands on
     * does not depend on c0, so the live terms add in a fixed order. */
    __shared__ float red[256];
    const int b = blockIdx.x;
    if (b >= width) return;
    const float om = 1.0f - decay;
    float acc = 0.f;
    for (int c = threadIdx.x; c < n_chunks; c += blockDim.x) {
        if (c < c0) continue;
        long long end = (long long)(c + 1) * chunk_frames;
        if (end > frames) end = frames;
        acc += powf(om, (float)(frames - end)) *
               partial[(long long)c * width + b];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float a = powf(om, (float)frames) * avg[b] + red[0];
        avg[b] = a;
        if (out) out[b] = a;
    }
}

/* ================= XlatingFir ========================================= *
 * src/blocks/xlating_fir.rs: DecimatingFir with complex band-pass taps
 * (bpf[i] = e^{i*TAU*offset/fs * i} * taps[i], :79-88) fused with the
 * output Rotator (:91-94,116: phase_incr = -TAU*offset*D/fs applied
 * in-place to the produced samples). Correctness-first kernel (LDS tile,
 * lane-strided outputs); the rotator phase uses the closed form (the
 * reference iterates — tolerance note in tests). */
__global__ __launch_bounds__(256) void k_xlating_decim_ccf32(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float2* __restrict__ taps /* reversed bpf taps */, int n_taps,
    long long decim, long long n_out, long long n_in_valid, double theta,
    float p0r, float p0i) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* s_h = (float2*)smem;
    for (int i = threadIdx.x; i < n_taps; i += blockDim.x) s_h[i] = taps[i];
    __syncthreads();
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         k < n_out; k += stride) {
        float sre = 0.f, sim = 0.f;
        long long base = decim - 1 + k * decim;
        for (int t = 0; t < n_taps; t++) {
            float2 x = (base + t < n_in_valid) ? in[base + t]
                                               : make_float2(0.f, 0.f);
            float2 hh = s_h[t];
            sre = fmaf(x.x, hh.x, sre);
            sre = fmaf(-x.y, hh.y, sre);
            sim = fmaf(x.x, hh.y, sim);
            sim = fmaf(x.y, hh.x, sim);
        }
        /* f64 angle + mod-2pi reduction (see k_rotator) */
        double a = theta * (double)(k + 1);
        a -= 6.283185307179586 * floor(a * 0.15915494309189535);
        float s, cth;
        __sincosf((float)a, &s, &cth);
        float pr = cth * p0r - s * p0i;
        float pi = cth * p0i + s * p0r;
        out[k] = make_float2(sre * pr - sim * pi, sre * pi + sim * pr);
    }
}

/* LDS-tiled XlatingFir (same output math as k_xlating_decim_ccf32): a
 * tile of XT_TILE outputs stages its whole input span into padded SoA
 * planes once; complex bpf taps in LDS. Fallback to the naive kernel
 * when the span exceeds the LDS budget (host decides). */
#define XT_BLOCK 256
#define XT_R 2
#define XT_TILE (XT_BLOCK * XT_R)

__global__ __launch_bounds__(XT_BLOCK) void k_xlating_decim_tiled_ccf32(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float2* __restrict__ taps /* reversed bpf taps */, int n_taps,
    int decim, long long n_out, long long n_in_valid, double theta,
    float p0r, float p0i, int span) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_re = (float*)smem;
    float* s_im = s_re + plane_floats((unsigned)span);
    float* s_hr = s_im + plane_floats((unsigned)span);
    float* s_hi = s_hr + n_taps;
    for (int i = threadIdx.x; i < n_taps; i += XT_BLOCK) {
        s_hr[i] = taps[i].x;
        s_hi[i] = taps[i].y;
    }
    const long long tiles = (n_out + XT_TILE - 1) / XT_TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long out_base = tile * XT_TILE;
        const long long in_base = decim - 1 + out_base * decim;
        __syncthreads();
        for (int i = threadIdx.x; i < span; i += XT_BLOCK) {
            long long g = in_base + i;
            float2 v = (g < n_in_valid) ? in[g] : make_float2(0.f, 0.f);
            s_re[lds_pad((unsigned)i)] = v.x;
            s_im[lds_pad((unsigned)i)] = v.y;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < XT_R; r++) {
            long long k = out_base + threadIdx.x + r * XT_BLOCK;
            if (k >= n_out) break;
            unsigned rel = (unsigned)((k - out_base) * decim);
            float sre = 0.f, sim = 0.f;
#pragma unroll 4
            for (int t = 0; t < n_taps; t++) {
                unsigned a = lds_pad(rel + (unsigned)t);
                float xr = s_re[a], xi = s_im[a];
                float hr = s_hr[t], hi = s_hi[t];
                sre = fmaf(xr, hr, sre);
                sre = fmaf(-xi, hi, sre);
                sim = fmaf(xr, hi, sim);
                sim = fmaf(xi, hr, sim);
            }
            /* f64 angle + mod-2pi reduction (see k_rotator) */
            double a = theta * (double)(k + 1);
            a -= 6.283185307179586 * floor(a * 0.15915494309189535);
            float s, cth;
            __sincosf((float)a, &s, &cth);
            float pr = cth * p0r - s * p0i;
            float pi = cth * p0i + s * p0r;
            out[k] = make_float2(sre * pr - sim * pi, sre * pi + sim * pr);
        }
    }
}

/* ================= WLAN sync-short helpers ============================ *
 * examples/wlan/src/bin/rx.rs:73-96 autocorrelation chain pieces:
 * a*conj(b) Combine (:81) and the sliding-SUM MovingAverage
 * (moving_average.rs:65-105) with its len-1 zero prologue. */
__global__ void k_cmul_conj(const float2* __restrict__ a,
                            const float2* __restrict__ b,
                            float2* __restrict__ o, long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         i < n; i += stride) {
        float2 x = a[i], y = b[i];
        o[i] = make_float2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y);
    }
}

/* divide_mag Combine — rx.rs:97: out = |a| / b (cf32, f32) -> f32 */
__global__ void k_divide_mag(const float2* __restrict__ a,
                             const float* __restrict__ b,
                             float* __restrict__ o, long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         i < n; i += stride) {
        float2 x = a[i];
        o[i] = sqrtf(x.x * x.x + x.y * x.y) / b[i];
    }
}

/* one output per lane: out[i] = sum in[i..i+len) (per float lane);
 * the zero prologue is emitted by the host wrapper */
__global__ void k_moving_sum(const float* __restrict__ in,
                             float* __restrict__ out, int width, int len,
                             long long n_out_items) {
    long long stride = (long long)gridDim.x * blockDim.x;
    long long total = n_out_items * width;
    for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         id < total; id += stride) {
        long long i = id / width;
        int q = (int)(id - i * width);
        float sum = 0.f;
        for (int t = 0; t < len; t++) sum += in[(i + t) * width + q];
        out[id] = sum;
    }
}

/* ================= PFB channelizer ==================================== *
 * src/blocks/pfb/channelizer.rs (liquid-dsp scheme), bulk closed form
 * of the round-robin window state for ANY decimation D = N/oversample
 * (channelizer.rs:126-210). Derivation: push p of the input stream
 * lands in window w(p) = (N-1-p) mod N (decrement_base_index); after
 * P = prefill + (k+1)*D pushes (prefill = N*tpf), output step k reads
 * window b's newest-j element x[pmax(b) - j*N] with
 *   pmax(b) = P-1 - ((P-1 - (N-1-b)) mod N)
 * through filter i(b) = (b - base - 1) mod N, base = (N-1-P) mod N:
 *   fft_buf[k][b] = sum_j x[pmax(b) - j*N] * part[i(b)][j]
 * (part = partition_filter_taps, utilities.rs:5-25; the FirFilter's
 * reversed taps turn the oldest->newest window into newest-j order).
 * `p_before` = pushes before this launch's first step (global),
 * `bufbase` = global stream index of in[0] (streaming carries the last
 * N*tpf consumed samples in front). D == N collapses to the maximally
 * decimated form (base stays N-1, i == b). */
__global__ void k_pfb_dots(const float2* __restrict__ in,
                           float2* __restrict__ fb,
                           const float* __restrict__ part /* [N][tpf] */,
                           int N, int tpf, int D, long long steps,
                           long long p_before, long long bufbase) {
    long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long total = steps * N;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (; id < total; id += stride) {
        long long k = id / N;
        int b = (int)(id - k * N);
        long long P = p_before + (k + 1) * (long long)D;
        int base = (int)(((N - 1 - P) % N + N) % N);
        int i = ((b - base - 1) % N + N) % N;
        long long pmax =
            P - 1 - (((P - 1 - (N - 1 - b)) % N + N) % N);
        float sre = 0.f, sim = 0.f;
        for (int j = 0; j < tpf; j++) {
            float2 x = in[pmax - (long long)j * N - bufbase];
            float tap = part[i * tpf + j];
            sre = fmaf(x.x, tap, sre);
            sim = fmaf(x.y, tap, sim);
        }
        fb[k * N + b] = make_float2(sre, sim);
    }
}

/* Start-up steps. The reference's windows are WindowBuffer::new(tpf,
 * false) (channelizer.rs:117, window_buffer.rs:13-32): fill push k of a
 * window lands at slot 2k mod tpf, so the just-filled window is a shuffle
 * of its fill pushes (even tpf: half the slots stay zero and half the
 * pushes are overwritten; odd tpf: a permutation), and it is the clean
 * oldest->newest window of k_pfb_dots only once tpf ordinary pushes have
 * rewritten every slot. Window b takes stream pushes p = (N-1-b) + m*N,
 * m = 0, 1, ...; with L = tpf fill pushes and q < L pushes after them,
 * slice position w (0 = oldest) is slot x = (q+w) mod L, which holds push
 * ordinal m = L+x once rewritten (x < q), else the last fill push with
 * 2m = x (mod L), else nothing. Returns m, or -1 for a hole (reads as 0);
 * q >= L is the steady state m = q+w. */
__host__ __device__ static inline int pfb_chan_window_src(int L, int q,
                                                          int w) {
    if (q >= L) return q + w;
    const int x = (q + w) % L;
    if (x < q) return L + x;
    if (((x + L) & 1) == 0) return (x + L) / 2;
    if ((x & 1) == 0) return x / 2;
    return -1;
}

/* The steps whose push count P = p_before + (k+1)*D is still below
 * 2*N*tpf, rewritten after k_pfb_dots: its sum with every window read
 * through pfb_chan_window_src, in the same newest-first order (the
 * launch order does not matter to the result: this kernel reads `in`
 * only). q = (P+b)/N - tpf
 * pushes have followed window b's fill. A start-up step reaches back to
 * push 0, so `in` holds the whole stream so far (bufbase = 0 for the
 * bulk entry; the streaming entry keeps it that long). */
__global__ void k_pfb_dots_startup(const float2* __restrict__ in,
                                   float2* __restrict__ fb,
                                   const float* __restrict__ part, int N,
                                   int tpf, int D, long long steps,
                                   long long p_before, long long bufbase) {
    long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long total = steps * N;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (; id < total; id += stride) {
        long long k = id / N;
        int b = (int)(id - k * N);
        long long P = p_before + (k + 1) * (long long)D;
        int base = (int)(((N - 1 - P) % N + N) % N);
        int i = ((b - base - 1) % N + N) % N;
        int q = (int)((P + b) / N) - tpf;
        float sre = 0.f, sim = 0.f;
        for (int j = 0; j < tpf; j++) {
            int m = pfb_chan_window_src(tpf, q, tpf - 1 - j);
            if (m < 0) continue;
            float2 x = in[(N - 1 - b) + (long long)m * N - bufbase];
            float tap = part[i * tpf + j];
            sre = fmaf(x.x, tap, sre);
            sim = fmaf(x.y, tap, sim);
        }
        fb[k * N + b] = make_float2(sre, sim);
    }
}

__global__ void k_pfb_scatter(const float2* __restrict__ ifft,
                              float2* __restrict__ out, int N,
                              long long steps, long long cap) {
    long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long total = steps * N;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (; id < total; id += stride) {
        long long k = id / N;
        int cidx = (int)(id - k * N);
        out[cidx * cap + k] = ifft[k * N + cidx];
    }
}

/* ================= PFB synthesizer ==================================== *
 * src/blocks/pfb/synthesizer.rs:59-143. Per time step t one sample of
 * every channel goes through an unnormalized inverse DFT,
 *   v[t][c] = sum_m x_m[t] e^{+2 pi i m c / N},
 * and v[t][c] is pushed into channel c's tpf-deep window; once the
 * windows are full every step emits N outputs in channel order,
 *   out[(t-(tpf-1))*N + c] = sum_{j<tpf} part[c][j] * v[t-j][c]
 * (part = partition_filter_taps, utilities.rs:5-25; FirFilter applies the
 * reversed taps to the oldest->newest window, fir.rs:76-88).
 *
 * In the kernels below time is relative to the call: t in [0, S) are the
 * S steps consumed now, t in [-H, 0) the H <= tpf-1 carried frames
 * (IFFT'd, oldest first). Steps t >= t_first emit. The tap table is
 * transposed, partT[j*N + c], so lanes along c read it coalesced. */
#define SYN_BLOCK 256
#define SYN_TT 32 /* consecutive steps per lane in the staged commutator */

/* staged 1/3: transposing gather in[c*stride + t] -> g[t*N + c] through
 * a 32x32 LDS tile (reads coalesced along t, writes along c; the 33rd
 * column makes the transposed read conflict-free). */
__global__ __launch_bounds__(SYN_BLOCK) void k_pfb_synth_gather(
    const float2* __restrict__ in, float2* __restrict__ g, int N,
    long long stride, long long steps) {
    __shared__ float2 tile[32][33];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const long long tiles_c = (N + 31) / 32;
    const long long tiles = tiles_c * ((steps + 31) / 32);
    for (long long id = blockIdx.x; id < tiles; id += gridDim.x) {
        const long long tb = (id / tiles_c) * 32;
        const int cb = (int)(id % tiles_c) * 32;
        for (int r = ly; r < 32; r += 8) {
            const int c = cb + r;
            const long long t = tb + lx;
            if (c < N && t < steps) tile[r][lx] = in[c * stride + t];
        }
        __syncthreads();
        for (int r = ly; r < 32; r += 8) {
            const long long t = tb + r;
            const int c = cb + lx;
            if (c < N && t < steps) g[t * N + c] = tile[lx][r];
        }
        __syncthreads();
    }
}

/* staged 3/3: commutator FIR over the IFFT'd frames v[(H+t)*N + c]. A
 * lane owns one channel and SYN_TT consecutive steps, so the tpf frames
 * a step reads are the ones its neighbours just pulled through L2. */
__global__ void k_pfb_synth_comm(const float2* __restrict__ v,
                                 float2* __restrict__ out,
                                 const float* __restrict__ partT, int N,
                                 int tpf, long long H, long long t_first,
                                 long long steps_out) {
    const long long runs = (steps_out + SYN_TT - 1) / SYN_TT;
    const long long total = runs * N;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         id < total; id += stride) {
        const long long r = id / N;
        const int c = (int)(id - r * N);
        const long long k0 = r * SYN_TT;
        const long long k1 = k0 + SYN_TT < steps_out ? k0 + SYN_TT
                                                     : steps_out;
        for (long long k = k0; k < k1; k++) {
            const float2* vt = v + (H + t_first + k) * N + c;
            float sre = 0.f, sim = 0.f;
            for (int j = 0; j < tpf; j++) {
                float2 x = vt[-(long long)j * N];
                float tap = partT[j * N + c];
                sre = fmaf(x.x, tap, sre);
                sim = fmaf(x.y, tap, sim);
            }
            out[k * N + c] = make_float2(sre, sim);
        }
    }
}

/* Start-up rows. The reference's WindowBuffer::new(len, false)
 * (window_buffer.rs:13-32) does not fill in order: fill-phase push k
 * lands at position 2k mod tpf, so until the tpf ordinary pushes that
 * follow have rewritten every position, the window is a shuffle of the
 * early frames with some lost and some holes still zero. The first tpf
 * emitted steps e = 0..tpf-1 (global step tpf-1+e) therefore differ from
 * the steady-state formula, and this kernel rewrites them the way the
 * reference computes them. Window position w of step e is buffer slot
 * x = (e+w) mod tpf, which holds frame tpf+x once rewritten (x < e),
 * else the last fill push k < tpf with 2k = x (mod tpf), else zero.
 * ve = IFFT'd frames of global steps 0..2tpf-2. */
__global__ void k_pfb_synth_startup(const float2* __restrict__ ve,
                                    float2* __restrict__ out,
                                    const float* __restrict__ partT, int N,
                                    int tpf, int e0, int n_e) {
    const long long total = (long long)n_e * N;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         id < total; id += stride) {
        const int e = e0 + (int)(id / N), c = (int)(id % N);
        float sre = 0.f, sim = 0.f;
        for (int w = 0; w < tpf; w++) {
            const int x = (e + w) % tpf;
            int fr;
            if (x < e) fr = tpf + x;
            else if (((x + tpf) & 1) == 0) fr = (x + tpf) / 2;
            else if ((x & 1) == 0) fr = x / 2;
            else continue;
            float2 v = ve[(long long)fr * N + c];
            float tap = partT[(tpf - 1 - w) * N + c];
            sre = fmaf(v.x, tap, sre);
            sim = fmaf(v.y, tap, sim);
        }
        out[id] = make_float2(sre, sim);
    }
}

/* fused: gather + IFFT + commutator in one launch, v never leaves LDS.
 * A block owns R consecutive steps [t0, t0+R) and rebuilds the hp >=
 * tpf-1 frames in front of them (block 0 takes them from the carried
 * history instead). It works in passes of F >= 8 steps: every channel's
 * F consecutive samples are one >= 64 B global read, transposed into
 * `stage` as F frames (frame stride FS = N + 64/F float2, which spreads
 * the 64 lanes of the transposing write over all banks). Groups of G
 * frames then run the in-LDS FFT, G frames side by side with
 * blockDim/G threads each, between their stage frame and a slot of the ring of
 * M = G + tpf-1 frames; IFFT(x) = conj(FFT(conj x)), so samples are
 * conjugated on load and the ring holds conj(v). The commutator reads
 * the ring with lanes along c and stores whole output rows. Frames are
 * kept fft_swz-permuted throughout. */
template <int NL>
__global__ __launch_bounds__(1024) void k_pfb_synth_fused(
    const float2* __restrict__ in, long long stride, long long S,
    const float2* __restrict__ hist_old, long long H,
    float2* __restrict__ hist_new, long long hn_first, long long hn_keep,
    float2* __restrict__ out, long long t_first,
    const float* __restrict__ partT, const float2* __restrict__ twid,
    int N, int log2n, int tpf, int F, int G, int FS, int R, int hp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* stage = (float2*)smem;                /* [F][FS] */
    float2* ring = stage + (size_t)F * FS;        /* [M][FS] */
    const int M = G + tpf - 1;
    const int tid = threadIdx.x;
    const int nth = blockDim.x;    /* == F*N/NL */
    const int tpg = nth / G;       /* threads per frame in the FFT */
    const int fl = tid / tpg, tf = tid - fl * tpg;
    /* a pass's F*N samples, NL per thread, held in registers from their
     * global load until the stage is free: the next pass's loads are in
     * flight under this pass's FFTs and commutator */
    float2 pre[NL];
    auto load_pass = [&](long long tb) {
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int idx = tid + k * nth;
            const int c = idx / F, f = idx - c * F;
            const long long t = tb + f;
            pre[k] = t < S ? in[c * stride + t] : make_float2(0.f, 0.f);
        }
    };

    for (long long t0 = (long long)blockIdx.x * R; t0 < S;
         t0 += (long long)gridDim.x * R) {
        const long long tend = t0 + R < S ? t0 + R : S;
        const long long tb0 = t0 == 0 ? 0 : t0 - hp;
        load_pass(tb0);
        /* ring slot of step t is (t - t0 + hp) mod M */
        if (t0 == 0) {
            for (int idx = tid; idx < (tpf - 1) * N; idx += nth) {
                const int jf = idx >> log2n, c = idx & (N - 1);
                const long long t = -(long long)(tpf - 1) + jf;
                float2 x = make_float2(0.f, 0.f);
                if (t >= -H) {
                    x = hist_old[(H + t) * N + c];
                    x.y = -x.y;
                }
                const int slot = (int)((t + hp) % M);
                ring[(size_t)slot * FS + fft_swz(c)] = x;
            }
        }
        for (long long tb = tb0; tb < tend; tb += F) {
#pragma unroll
            for (int k = 0; k < NL; k++) {
                const int idx = tid + k * nth;
                const int c = idx / F, f = idx - c * F;
                stage[(size_t)f * FS + fft_swz(c)] =
                    make_float2(pre[k].x, -pre[k].y);
            }
            __syncthreads();
            if (tb + F < tend) load_pass(tb + F);
            for (int g0 = 0; g0 < F && tb + g0 < tend; g0 += G) {
                {
                    const long long q = tb + g0 + fl - t0 + hp;
                    float2* a = stage + (size_t)(g0 + fl) * FS;
                    float2* b = ring + (size_t)(q % M) * FS;
                    float2* res = fft_pow2_fwd(a, b, twid, N, tf, tpg);
                    if (res == a) { /* even stage count: move to the ring */
                        for (int i = tf; i < N; i += tpg) b[i] = a[i];
                        __syncthreads();
                    }
                }
                for (int idx = tid; idx < G * N; idx += nth) {
                    const int gf = idx >> log2n, c = idx & (N - 1);
                    const long long t = tb + g0 + gf;
                    if (t < t0 || t >= tend) continue;
                    const int s = (int)((t - t0 + hp) % M);
                    const unsigned cs = fft_swz(c);
                    if (hist_new && t >= hn_first) {
                        float2 x = ring[(size_t)s * FS + cs];
                        x.y = -x.y;
                        hist_new[(hn_keep + t - hn_first) * N + c] = x;
                    }
                    if (t < t_first) continue;
                    float sre = 0.f, sim = 0.f;
                    int sj = s;
                    for (int j = 0; j < tpf; j++) {
                        float2 x = ring[(size_t)sj * FS + cs];
                        float tap = partT[j * N + c];
                        sre = fmaf(x.x, tap, sre);
                        sim = fmaf(x.y, tap, sim);
                        if (--sj < 0) sj += M;
                    }
                    out[(t - t_first) * N + c] = make_float2(sre, -sim);
                }
                __syncthreads();
            }
        }
    }
}

/* ================= PFB arbitrary-rate resampler ======================= *
 * src/blocks/pfb/arb_resampler.rs. The block's timing state (tau,
 * base_index, mu, Interpolate/Boundary) is a serial f32 recurrence that
 * never sees the samples; it decides how many outputs each input yields
 * and which two filters and mu each output blends. arb_update/arb_step
 * restate it one reference op per op, round-to-nearest and uncontracted,
 * shared by the host walk (schedule create, counts) and the device walk,
 * so both see the same states bit for bit. The recurrence is eventually
 * periodic, so the host keeps one ArbCk every ARB_Q inputs
 * over preperiod + period inputs and any stream position folds onto that
 * table.
 *
 * k_pfb_arb: a block owns segments of R = W*RL inputs. Phase 1: lane l <
 * W seeks input s0 + l*RL (checkpoint + at most ARB_Q-1 silent steps),
 * then walks its RL inputs and writes one record per output to LDS at
 * the offset its cumulative output count gives, so the records are
 * compact along the output index. Phase 2: per channel, the block
 * stages the segment's samples (plus tpf of history) in LDS and lanes
 * along the output index compute and store; the walk is paid once for
 * all channels. The samples of channel c+1 are loaded into registers
 * while channel c computes (channel 0's during the walk). Staging takes
 * a block-uniform unguarded path for a segment whose window lies inside
 * this call's input, a clamped one (carried history in front, zeros
 * past the end) otherwise. */
#define ARB_Q 16    /* checkpoint spacing: a seek walks at most 15 inputs */
#define ARB_CAP 2048 /* output records per segment */
#define ARB_BLOCK 256
#define ARB_NV 9     /* staged float2 per lane: R + tpf + 1 <= 9*256 */

struct ArbSt { float tau, mu; unsigned base, bnd; };
struct ArbCk { float tau, mu; unsigned base, bnd; unsigned long long cum; };

/* One IEEE f32 operation each, never fused with a neighbour. The pragma
 * is what keeps them apart: the __fadd_rn/__fmul_rn intrinsics are plain
 * operators in the HIP headers, and under the default -ffp-contract=fast
 * the multiply in bf = tau*nf fuses with the subtraction in mu = bf -
 * base into one v_fma_f32, which changes mu. */
__host__ __device__ static inline float arb_fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__host__ __device__ static inline float arb_fsub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__host__ __device__ static inline float arb_fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

/* update_timing_state, arb_resampler.rs:132-140. `floor() as usize`
 * saturates: a negative bf (tau is slightly negative after a Boundary
 * when delay < 1/nf) and NaN give 0. */
__host__ __device__ static inline void arb_update(ArbSt& s, float delay,
                                                  float nff) {
    s.tau = arb_fadd(s.tau, delay);
    const float bf = arb_fmul(s.tau, nff);
    s.base = bf >= 2147483648.f ? 0x7fffffffu
             : (bf > 0.f ? (unsigned)floorf(bf) : 0u);
    s.mu = arb_fsub(bf, (float)s.base);
}

/* consume_single's control flow, :142-188: emit(base_index, boundary, mu)
 * per output, returns their number. max_out bounds the loop (a rate so
 * large that tau stops advancing would spin; create refuses those). */
template <class Emit>
__host__ __device__ static inline unsigned arb_step(ArbSt& s, unsigned nf,
                                                    float delay, float nff,
                                                    unsigned max_out,
                                                    Emit&& emit) {
    unsigned cnt = 0;
    while (s.base < nf && cnt <= max_out) {
        if (s.bnd) {
            emit(s.base, 1u, s.mu);
            cnt++;
            arb_update(s, delay, nff);
            s.bnd = 0;
        } else if (s.base == nf - 1) {
            s.bnd = 1;
            s.base = nf;
        } else {
            emit(s.base, 0u, s.mu);
            cnt++;
            arb_update(s, delay, nff);
        }
    }
    s.tau = arb_fsub(s.tau, 1.0f);
    s.base -= nf;
    return cnt;
}

struct ArbNoEmit {
    __host__ __device__ void operator()(unsigned, unsigned, float) const {}
};

/* where fill push k of a tpf-slot window lands, or -1 when a later fill
 * push overwrites it: WindowBuffer::new(len, false) writes push k at
 * (start_idx - num_samples_missing) mod len = 2k mod len
 * (window_buffer.rs:23-32). Odd tpf: 2 is invertible, every push keeps
 * its slot. Even tpf: only even slots are hit, twice; the second half of
 * the pushes wins. */
__host__ __device__ static inline long long arb_fill_slot(long long tpf,
                                                          long long k) {
    if ((tpf & 1) == 0 && k < tpf / 2) return -1;
    return (2 * k) % tpf;
}

struct ArbParams {
    const ArbCk* ck;
    unsigned long long rho, lam, opc, P0, cum0;
    float delay, nff;
    unsigned nf, maxo1;
    int tpf, C, RL, W;
};

/* fill pushes k0..k0+nfill-1 into the window slots they end up in */
__global__ void k_pfb_arb_fill(const float2* __restrict__ in,
                               long long in_stride,
                               float2* __restrict__ hist, int C, int tpf,
                               long long k0, long long nfill) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nfill * C) return;
    const long long c = i / nfill, j = i % nfill;
    const long long slot = arb_fill_slot(tpf, k0 + j);
    if (slot >= 0) hist[c * tpf + slot] = in[c * in_stride + j];
}

/* the window after n more inputs: the last tpf of (old window ++ inputs) */
__global__ void k_pfb_arb_hist(const float2* __restrict__ in,
                               long long in_stride, long long n,
                               const float2* __restrict__ hist_old,
                               float2* __restrict__ hist_new, int C,
                               int tpf) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)C * tpf) return;
    const long long c = i / tpf, j = i % tpf;
    const long long g = n - tpf + j;
    hist_new[i] = g < 0 ? hist_old[c * tpf + tpf + g] : in[c * in_stride + g];
}

template <bool TAPS_LDS>
__global__ __launch_bounds__(ARB_BLOCK) void k_pfb_arb(
    const float2* __restrict__ in, long long in_stride, long long n,
    const float2* __restrict__ hist, float2* __restrict__ out,
    long long out_stride, long long M, const float* __restrict__ rtaps,
    ArbParams p, long long nseg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int tpf = p.tpf, R = p.W * p.RL;
    unsigned* r_i = (unsigned*)smem;
    unsigned* r_b = r_i + ARB_CAP;
    float* r_mu = (float*)(r_b + ARB_CAP);
    unsigned long long* lanecum = (unsigned long long*)(r_mu + ARB_CAP);
    float2* xs = (float2*)(lanecum + ARB_BLOCK + 2);
    const float* tp = rtaps;
    if (TAPS_LDS) {
        float* tl = (float*)(xs + R + tpf + 1);
        for (int j = tid; j < (int)p.nf * tpf; j += ARB_BLOCK)
            tl[j] = rtaps[j];
        tp = tl; /* first read is behind the segment loop's barriers */
    }
    for (long long seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const long long s0 = seg * R;
        const int len = (int)(n - s0 < R ? n - s0 : R);
        const int nl = (len + p.RL - 1) / p.RL;
        /* segment samples: xs[j] is call-relative input s0 - tpf + j, j in
         * [0, R + tpf]; slot R + tpf is read but never selected. They are
         * loaded into registers a channel ahead by straight-line clamped
         * loads (no per-element branch, so one wait serves them all):
         * unguarded where the segment's window lies inside this call's
         * input, else carried history in front and zeros past the end. */
        const bool interior = s0 >= tpf && len == R;
        const int nv = (R + tpf) / ARB_BLOCK + 1; /* block-uniform */
        float2 v[ARB_NV];
#pragma unroll
        for (int q = 0; q < ARB_NV; q++) v[q] = make_float2(0.f, 0.f);
        auto stage = [&](int c) {
            const float2* xc = in + (long long)c * in_stride;
            if (interior) {
                const float2* src = xc + (s0 - tpf);
#pragma unroll
                for (int q = 0; q < ARB_NV; q++) {
                    if (q >= nv) break;
                    const int j = tid + q * ARB_BLOCK;
                    v[q] = src[j < R + tpf ? j : R + tpf - 1];
                }
            } else {
                const float2* hc = hist + (long long)c * tpf + tpf;
#pragma unroll
                for (int q = 0; q < ARB_NV; q++) {
                    if (q >= nv) break;
                    const long long g = s0 - tpf + tid + q * ARB_BLOCK;
                    const float2 x = g < 0 ? hc[g] : xc[g < n ? g : n - 1];
                    v[q] = g < n ? x : make_float2(0.f, 0.f);
                }
            }
        };
        stage(0); /* in flight during the walk */
        /* ---- phase 1: the schedule of this segment ---- */
        ArbSt st = {0.f, 0.f, 0u, 0u};
        unsigned long long mycum = 0;
        if (tid < nl) {
            const unsigned long long pos =
                p.P0 + (unsigned long long)s0 + (unsigned)(tid * p.RL);
            unsigned long long k = 0, fp = pos;
            if (pos >= p.rho) {
                k = (pos - p.rho) / p.lam;
                fp = p.rho + (pos - p.rho) % p.lam;
            }
            const ArbCk c = p.ck[fp / ARB_Q];
            st.tau = c.tau; st.mu = c.mu; st.base = c.base; st.bnd = c.bnd;
            mycum = c.cum + k * p.opc;
            const int pre = (int)(fp % ARB_Q);
            for (int i = 0; i < pre; i++)
                mycum += arb_step(st, p.nf, p.delay, p.nff, p.maxo1,
                                  ArbNoEmit());
            lanecum[tid] = mycum;
        }
        __syncthreads();
        const unsigned long long segcum = lanecum[0];
        if (tid < nl) {
            unsigned off = (unsigned)(mycum - segcum);
            const int first = tid * p.RL;
            const int cnt = len - first < p.RL ? len - first : p.RL;
            for (int i = 0; i < cnt; i++) {
                const unsigned idx = (unsigned)(first + i);
                arb_step(st, p.nf, p.delay, p.nff, p.maxo1,
                         [&](unsigned base, unsigned bnd, float mu) {
                             if (off < ARB_CAP) {
                                 r_i[off] = idx;
                                 r_b[off] = base | (bnd << 31);
                                 r_mu[off] = mu;
                             }
                             off++;
                         });
            }
            if (tid == nl - 1) lanecum[ARB_BLOCK] = off;
        }
        __syncthreads();
        const unsigned tot = (unsigned)lanecum[ARB_BLOCK];
        const int nout = (int)(tot < ARB_CAP ? tot : ARB_CAP);
        const long long obase = (long long)(segcum - p.cum0);
        /* ---- phase 2: the outputs, channel by channel ---- */
        for (int c = 0; c < p.C; c++) {
#pragma unroll
            for (int q = 0; q < ARB_NV; q++) {
                const int j = tid + q * ARB_BLOCK;
                if (j <= R + tpf) xs[j] = v[q];
            }
            __syncthreads();
            /* the next channel's samples fly while this one computes */
            if (c + 1 < p.C) stage(c + 1);
            float2* oc = out + (long long)c * out_stride;
            /* the records are re-read from LDS per channel: holding a
             * lane's eight in registers cost 214 VGPRs and two waves per
             * SIMD */
            for (int o = tid; o < nout; o += ARB_BLOCK) {
                const unsigned rbo = r_b[o];
                /* Interpolate: F[base] and F[base+1] on window i.
                 * Boundary: F[nf-1] on window i-1, F[0] on window i. */
                const unsigned bnd = rbo >> 31;
                const unsigned base = rbo & 0x7fffffffu;
                const float* ta = tp + (size_t)(bnd ? p.nf - 1 : base) * tpf;
                const float* tb = tp + (size_t)(bnd ? 0u : base + 1) * tpf;
                const float2* w = xs + r_i[o] + 1 - bnd;
                float2 y0 = make_float2(0.f, 0.f), y1 = y0;
                float2 xcur = w[0];
                for (int t = 0; t < tpf; t++) {
                    const float2 xnext = w[t + 1];
                    const float2 x1 = bnd ? xnext : xcur;
                    const float h0 = ta[t], h1 = tb[t];
                    y0.x = fmaf(xcur.x, h0, y0.x);
                    y0.y = fmaf(xcur.y, h0, y0.y);
                    y1.x = fmaf(x1.x, h1, y1.x);
                    y1.y = fmaf(x1.y, h1, y1.y);
                    xcur = xnext;
                }
                const float mu = r_mu[o], om = 1.0f - mu;
                const long long og = obase + o;
                if (og >= 0 && og < M)
                    oc[og] = make_float2(fmaf(om, y0.x, mu * y1.x),
                                         fmaf(om, y0.y, mu * y1.y));
            }
            __syncthreads();
        }
    }
}

/* ================= MovingAvg ========================================== *
 * src/blocks/moving_avg.rs:79-118: per-bin EMA over WIDTH-sized frames,
 * emit every `history` frames; avg state lives in HBM (stateful block).
 * One lane per bin, sequential over frames (frames are a recurrence). */
__global__ void k_moving_avg(const float* __restrict__ in,
                             float* __restrict__ out,
                             float* __restrict__ avg, int width,
                             long long frames, int i0, int history,
                             float decay) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= width) return;
    float a = avg[b];
    int i = i0;
    long long prod = 0;
    for (long long f = 0; f < frames; f++) {
        float t = in[f * width + b];
        if (isfinite(t))
            a = (1.0f - decay) * a + decay * t;
        else
            a *= 1.0f - decay;
        if (++i == history) {
            out[prod * width + b] = a;
            i = 0;
            prod++;
        }
    }
    avg[b] = a;
}

/* ================= Rotator ============================================ *
 * Rotator::rotate — crates/futuredsp/src/rotator.rs:23-49: out[i] =
 * in[i] * phase0 * e^{i*theta*(i+1)}. The reference iterates
 * phase *= phase_incr per sample (accumulating f32 rounding); this kernel
 * computes the phase in closed form per sample (sincosf), which tracks
 * the IDEAL rotation — parity vs the oracle is tolerance-bounded by the
 * oracle's own drift (documented in tests). */
__global__ void k_rotator(const float2* __restrict__ in,
                          float2* __restrict__ out, long long n,
                          double theta, float p0r, float p0i) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         i < n; i += stride) {
        /* angle product + mod-2pi reduction in f64: f32 theta*(i+1) loses
         * ~0.25 rad past i~3e6 and (float)(i+1) is inexact past 2^24 */
        double a = theta * (double)(i + 1);
        a -= 6.283185307179586 * floor(a * 0.15915494309189535);
        float s, c;
        __sincosf((float)a, &s, &c);
        float pr = c * p0r - s * p0i;
        float pi = c * p0i + s * p0r;
        float2 x = in[i];
        out[i] = make_float2(x.x * pr - x.y * pi, x.x * pi + x.y * pr);
    }
}

/* ================= FIR f32 x f32 (plumbing config) ==================== *
 * fir.rs:206-215 semantics; simple LDS-staged kernel (this path is the
 * reference's perf/fir plumbing shape, not the metric). */
__global__ __launch_bounds__(256) void k_fir_f32(
    const float* __restrict__ in, float* __restrict__ out,
    const float* __restrict__ taps, int n_taps, long long n_out,
    long long n_in_valid) {
    const unsigned TILE = 1024;
    const unsigned elems = TILE + n_taps - 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_x = (float*)smem;
    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x; tile * (long long)TILE < n_out;
         tile += gridDim.x) {
        const long long out_base = tile * TILE;
        for (unsigned i = tid; i < elems; i += 256) {
            long long g = out_base + i;
            s_x[i] = (g < n_in_valid) ? in[g] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < 4; j++) {
            unsigned k = tid + j * 256; /* lane-strided: stride-1 reads */
            float sum = 0.f;
            for (int t = 0; t < n_taps; t++)
                sum = fmaf(s_x[k + t], taps[n_taps - 1 - t], sum);
            long long o = out_base + k;
            if (o < n_out) out[o] = sum;
        }
        __syncthreads();
    }
}

/* ================= Polyphase resampler, cf32 x f32 ==================== *
 * polyphase_resampling_fir.rs:108-118: y[k] = sum_t i[k*M/L + t] *
 * taps[L*(Tpp-t-1) + (k*M)%L]. Correctness-first kernel: taps staged in
 * LDS (per-lane bank index), one output per lane, inputs via L1/L2. */
__global__ void k_resamp_cf32(const float2* __restrict__ in,
                              float2* __restrict__ out,
                              const float* __restrict__ taps, int n_taps,
                              int interp, int decim, long long n_out,
                              long long n_in_valid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_taps = (float*)smem;
    for (int i = threadIdx.x; i < n_taps; i += blockDim.x)
        s_taps[i] = taps[i];
    __syncthreads();
    const int tpp = n_taps / interp;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         k < n_out; k += stride) {
        int bank = (int)((k * decim) % interp);
        long long idx = k * decim / interp;
        float sre = 0.f, sim = 0.f;
        for (int t = 0; t < tpp; t++) {
            float2 x = (idx + t < n_in_valid) ? in[idx + t]
                                              : make_float2(0.f, 0.f);
            float h = s_taps[interp * (tpp - t - 1) + bank];
            sre = fmaf(x.x, h, sre);
            sim = fmaf(x.y, h, sim);
        }
        out[k] = make_float2(sre, sim);
    }
}

/* LDS-tiled resampler (polyphase_resampling_fir.rs:108-118 semantics,
 * identical output math to k_resamp_cf32): a tile of RS_TILE outputs
 * stages its whole input span into padded SoA LDS planes once, then
 * each lane runs its tpp-tap phase dot product from LDS — removes the
 * per-output global gather of the naive kernel. Fallback to
 * k_resamp_cf32 when the span exceeds the LDS budget (host decides). */
#define RS_BLOCK 256
#define RS_R 2
#define RS_TILE (RS_BLOCK * RS_R)

__global__ __launch_bounds__(RS_BLOCK) void k_resamp_tiled_cf32(
    const float2* __restrict__ in, float2* __restrict__ out,
    const float* __restrict__ taps, int n_taps, int interp, int decim,
    long long n_out, long long n_in_valid, int span) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_re = (float*)smem;
    float* s_im = s_re + plane_floats((unsigned)span);
    float* s_taps = s_im + plane_floats((unsigned)span);
    for (int i = threadIdx.x; i < n_taps; i += RS_BLOCK)
        s_taps[i] = taps[i];
    const int tpp = n_taps / interp;
    const long long tiles = (n_out + RS_TILE - 1) / RS_TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long out_base = tile * RS_TILE;
        const long long in_base = out_base * decim / interp;
        __syncthreads(); /* previous tile's reads done before restage */
        for (int i = threadIdx.x; i < span; i += RS_BLOCK) {
            long long g = in_base + i;
            float2 v = (g < n_in_valid) ? in[g] : make_float2(0.f, 0.f);
            s_re[lds_pad((unsigned)i)] = v.x;
            s_im[lds_pad((unsigned)i)] = v.y;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RS_R; r++) {
            long long k = out_base + threadIdx.x + r * RS_BLOCK;
            if (k >= n_out) break;
            int bank = (int)((k * decim) % interp);
            unsigned rel = (unsigned)(k * decim / interp - in_base);
            float sre = 0.f, sim = 0.f;
            const float* tb = s_taps + bank;
#pragma unroll 4
            for (int t = 0; t < tpp; t++) {
                unsigned a = lds_pad(rel + (unsigned)t);
                float h = tb[interp * (tpp - t - 1)];
                sre = fmaf(s_re[a], h, sre);
                sim = fmaf(s_im[a], h, sim);
            }
            out[k] = make_float2(sre, sim);
        }
    }
}

/* ================= Polyphase resampler, f32 x f32 ===================== *
 * PolyphaseResamplingFir<f32,f32,f32>, polyphase_resampling_fir.rs:126-141
 * — the index math of :108-118 on real items. Every f32 resampler kernel
 * below (naive, tiled, fused FM) forms an output the same way: from 0, t
 * ascending, one fmaf per tap. An output's bits therefore do not depend
 * on which kernel, tile or chunk computed it. */

/* Naive kernel (spans over the LDS budget): one output per lane, inputs
 * via L1/L2. No window passes the caller's n_in (resamp_status). */
__global__ void k_resamp_f32(const float* __restrict__ in,
                             float* __restrict__ out,
                             const float* __restrict__ taps, int n_taps,
                             int interp, int decim, long long n_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_taps = (float*)smem;
    for (int i = threadIdx.x; i < n_taps; i += blockDim.x)
        s_taps[i] = taps[i];
    __syncthreads();
    const int tpp = n_taps / interp;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         k < n_out; k += stride) {
        int bank = (int)((k * decim) % interp);
        const float* x = in + k * decim / interp;
        const float* tb = s_taps + bank;
        float sum = 0.f;
        for (int t = 0; t < tpp; t++)
            sum = fmaf(x[t], tb[interp * (tpp - t - 1)], sum);
        out[k] = sum;
    }
}

/* A tile's plane is padded (lds_pad) where decim is even: lane k reads
 * around k*decim/interp, and a power of two in that stride piles the
 * lanes onto a few banks. With an odd decim the plain layout is already
 * spread, and its addresses are base + t: no arithmetic per tap. */
template <bool PAD>
__device__ __forceinline__ unsigned rs_at(unsigned e) {
    return PAD ? lds_pad(e) : e;
}

/* The dot products of one staged tile: s_x holds the tile's input span,
 * element 0 = input in_base = out_base*decim / interp, and r0 is that
 * division's remainder. Output out_base + j then starts (r0 + j*decim) /
 * interp elements in, on bank (r0 + j*decim) % interp: 32-bit arithmetic
 * (the host keeps RS_TILE*decim + interp under 2^31). */
template <bool PAD>
__device__ __forceinline__ void resamp_tile_dots_f32(
    const float* s_x, const float* s_taps, float* __restrict__ out,
    long long out_base, long long n_out, unsigned r0, int interp, int decim,
    int tpp) {
#pragma unroll
    for (int r = 0; r < RS_R; r++) {
        const unsigned j = threadIdx.x + r * RS_BLOCK;
        if (out_base + j >= n_out) break;
        const unsigned num = r0 + j * (unsigned)decim;
        const unsigned rel = num / (unsigned)interp;
        const unsigned bank = num - rel * (unsigned)interp;
        const float* tb = s_taps + bank;
        float sum = 0.f;
#pragma unroll 4
        for (int t = 0; t < tpp; t++)
            sum = fmaf(s_x[rs_at<PAD>(rel + (unsigned)t)],
                       tb[interp * (tpp - t - 1)], sum);
        out[out_base + j] = sum;
    }
}

/* LDS-tiled kernel in the shape of k_resamp_tiled_cf32, one plane. */
template <bool PAD>
__global__ __launch_bounds__(RS_BLOCK) void k_resamp_tiled_f32(
    const float* __restrict__ in, float* __restrict__ out,
    const float* __restrict__ taps, int n_taps, int interp, int decim,
    long long n_out, long long n_in_valid, int span) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_x = (float*)smem;
    float* s_taps = s_x + plane_floats((unsigned)span);
    for (int i = threadIdx.x; i < n_taps; i += RS_BLOCK)
        s_taps[i] = taps[i];
    const int tpp = n_taps / interp;
    const long long tiles = (n_out + RS_TILE - 1) / RS_TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long out_base = tile * RS_TILE;
        const long long in_base = out_base * decim / interp;
        const unsigned r0 = (unsigned)(out_base * decim - in_base * interp);
        __syncthreads(); /* previous tile's reads done before restage */
        for (int i = threadIdx.x; i < span; i += RS_BLOCK) {
            long long g = in_base + i;
            s_x[rs_at<PAD>((unsigned)i)] = (g < n_in_valid) ? in[g] : 0.f;
        }
        __syncthreads();
        resamp_tile_dots_f32<PAD>(s_x, s_taps, out, out_base, n_out, r0,
                                  interp, decim, tpp);
    }
}

/* ================= Quadrature demodulator ============================= *
 * examples/fm-receiver/src/main.rs:99-104: d[i] = arg(x[i]*conj(x[i-1])).
 * The product as num_complex writes it (Mul for Complex: re = a.re*b.re -
 * a.im*b.im, im = a.re*b.im + a.im*b.re, with b = conj(p) = (p.re,
 * -p.im)), every operation rounded on its own: with p = 0+0i, b is
 * (+0, -0) and the signed zeros reach atan2f as they do in the reference. */
__device__ __forceinline__ float quad_demod1(float2 a, float2 p) {
    const float br = p.x, bi = -p.y;
    const float re = __fsub_rn(__fmul_rn(a.x, br), __fmul_rn(a.y, bi));
    const float im = __fadd_rn(__fmul_rn(a.x, bi), __fmul_rn(a.y, br));
    return atan2f(im, re);
}

/* d[g] for lane-consecutive g, in two steps so that a caller can have
 * several loads in flight. Load: x[g] in one coalesced access (0 past
 * n_valid), and on lane 0 of a wave x[g-1], or the carried `last` at the
 * stream start. Value: every other lane takes x[g-1] from the lane below.
 * All 64 lanes of a wave call _value together (the shuffle reads the
 * neighbour's register). */
struct quad_demod_pair {
    float2 v, p; /* x[g]; x[g-1], lane 0 only */
};

__device__ __forceinline__ quad_demod_pair quad_demod_load(
    const float2* __restrict__ in, const float2* __restrict__ last,
    long long g, long long n_valid) {
    quad_demod_pair q;
    q.v = q.p = make_float2(0.f, 0.f);
    if (g < n_valid) {
        q.v = in[g];
        if ((threadIdx.x & 63) == 0) q.p = g == 0 ? *last : in[g - 1];
    }
    return q;
}

__device__ __forceinline__ float quad_demod_value(quad_demod_pair q,
                                                  bool valid) {
    float2 p = make_float2(__shfl_up(q.v.x, 1), __shfl_up(q.v.y, 1));
    if ((threadIdx.x & 63) == 0) p = q.p;
    return valid ? quad_demod1(q.v, p) : 0.f;
}

__global__ __launch_bounds__(256) void k_quad_demod(
    const float2* __restrict__ in, float* __restrict__ out,
    const float2* __restrict__ last, long long n) {
    /* block-uniform trip count: quad_demod_value needs whole waves */
    for (long long base = blockIdx.x * 256ll; base < n;
         base += gridDim.x * 256ll) {
        const long long g = base + threadIdx.x;
        const float d =
            quad_demod_value(quad_demod_load(in, last, g, n), g < n);
        if (g < n) out[g] = d;
    }
}

/* Fused quadrature demod + f32 polyphase resampler: k_resamp_tiled_f32
 * whose staging pass demodulates. A tile loads its Complex32 span once,
 * writes each d[i] once into the LDS plane (atan2f per input sample, not
 * per tap) and runs the same dot products; the demodulated stream never
 * reaches HBM. */
#define FM_LD 4

template <bool PAD>
__global__ __launch_bounds__(RS_BLOCK) void k_fm_demod_resamp(
    const float2* __restrict__ in, float* __restrict__ out,
    const float* __restrict__ taps, const float2* __restrict__ last,
    int n_taps, int interp, int decim, long long n_out,
    long long n_in_valid, int span) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_d = (float*)smem;
    float* s_taps = s_d + plane_floats((unsigned)span);
    for (int i = threadIdx.x; i < n_taps; i += RS_BLOCK)
        s_taps[i] = taps[i];
    const int tpp = n_taps / interp;
    const long long tiles = (n_out + RS_TILE - 1) / RS_TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long out_base = tile * RS_TILE;
        const long long in_base = out_base * decim / interp;
        const unsigned r0 = (unsigned)(out_base * decim - in_base * interp);
        __syncthreads(); /* previous tile's reads done before restage */
        /* FM_LD loads of a lane issued together: one round trip to
         * memory per FM_LD*RS_BLOCK samples, not one per RS_BLOCK */
        for (int i0 = 0; i0 < span; i0 += FM_LD * RS_BLOCK) {
            quad_demod_pair q[FM_LD];
#pragma unroll
            for (int u = 0; u < FM_LD; u++) {
                const int i = i0 + u * RS_BLOCK + threadIdx.x;
                q[u] = quad_demod_load(in, last, in_base + i,
                                       i < span ? n_in_valid : 0);
            }
#pragma unroll
            for (int u = 0; u < FM_LD; u++) {
                const int i = i0 + u * RS_BLOCK + threadIdx.x;
                const float d = quad_demod_value(
                    q[u], i < span && in_base + i < n_in_valid);
                if (i < span) s_d[rs_at<PAD>((unsigned)i)] = d;
            }
        }
        __syncthreads();
        resamp_tile_dots_f32<PAD>(s_d, s_taps, out, out_base, n_out, r0,
                                  interp, decim, tpp);
    }
}

/* ================= FFT: radix-4 Stockham in LDS ======================= *
 * Unnormalized DFT, rustfft convention (forward e^{-2pi i kn/N}) — the
 * reference Fft block's math (src/blocks/fft.rs:190-194). Stockham
 * autosort, radix-4 stages (plus one radix-2 stage when log2 N is odd):
 * half the LDS round trips and barriers of radix-2. One or more frames
 * per 256-thread block, ping-pong LDS, twiddle table (float2,
 * W[k] = e^{-2pi i k/N}, k < N, f64-computed on host). Supports
 * fft_shift / normalize per fft.rs:179-210, and an optional fused |X|^2
 * output (the spectrum Apply stage, examples/spectrum cpu.rs:21-28).
 */
__device__ __forceinline__ float2 cmul_tw(float2 a, float2 w, int inverse) {
    if (inverse) w.y = -w.y;
    return cmulf(a, w);
}

/* In-block 1024-pt forward FFT (unnormalized), 256 threads, for the
 * chain's fused decim+FFT kernel. Same radix-4 DIF scheme and fft_swz
 * LDS swizzle as k_fft_stockham. */
__device__ float2* fft_pow2_fwd(float2* a, float2* b,
                                const float2* __restrict__ twid, int n,
                                int tf, int tpf) {
    int scur = 1;
    int ncur = n;
    while (ncur >= 4) {
        const int m4 = ncur >> 2;
        for (int bf = tf; bf < n / 4; bf += tpf) {
            const int p = bf / scur;
            const int q = bf - p * scur;
            const int tw = n / ncur;
            float2 x0 = a[fft_swz(q + scur * p)];
            float2 x1 = a[fft_swz(q + scur * (p + m4))];
            float2 x2 = a[fft_swz(q + scur * (p + 2 * m4))];
            float2 x3 = a[fft_swz(q + scur * (p + 3 * m4))];
            float2 e0 = f2_add(x0, x2), e1 = f2_sub(x0, x2);
            float2 o0 = f2_add(x1, x3), o1 = f2_sub(x1, x3);
            float2 o1r = make_float2(o1.y, -o1.x);
            /* one twiddle load; W^2p, W^3p derived by complex mults
             * (unit-vector products, ~2 ulp — the 3-load version was
             * VMEM-issue-bound inside the fused chain kernel) */
            float2 w1 = twid[(size_t)p * tw];
            float2 w2 = cmulf(w1, w1);
            float2 w3 = cmulf(w2, w1);
            b[fft_swz(q + scur * (4 * p + 0))] = f2_add(e0, o0);
            b[fft_swz(q + scur * (4 * p + 1))] = cmulf(f2_add(e1, o1r), w1);
            b[fft_swz(q + scur * (4 * p + 2))] = cmulf(f2_sub(e0, o0), w2);
            b[fft_swz(q + scur * (4 * p + 3))] = cmulf(f2_sub(e1, o1r), w3);
        }
        float2* t = a; a = b; b = t;
        scur <<= 2;
        ncur >>= 2;
        __syncthreads();
    }
    if (ncur == 2) { /* radix-2 tail for odd log2n */
        for (int bf = tf; bf < n / 2; bf += tpf) {
            const int p = bf / scur;
            const int q = bf - p * scur;
            float2 xa = a[fft_swz(q + scur * p)];
            float2 xb = a[fft_swz(q + scur * (p + 1))];
            b[fft_swz(q + scur * 2 * p)] = f2_add(xa, xb);
            b[fft_swz(q + scur * (2 * p + 1))] =
                cmulf(f2_sub(xa, xb), twid[(size_t)p * (n / 2)]);
        }
        float2* t = a; a = b; b = t;
        __syncthreads();
    }
    return a;
}

__device__ void fft1024_block(float2* ping, float2* pong,
                              const float2* __restrict__ twid,
                              int tf /* thread-in-frame, stride 256 */) {
    (void)fft_pow2_fwd(ping, pong, twid, 1024, tf, 256);
    /* 5 radix-4 stages = 5 ping/pong swaps: result in `pong`. */
}

/* ---- Bluestein (non-pow2 lengths) ------------------------------------ *
 * X[k] = w(k) * IFFT_M(FFT_M(x.w) * B)[k] / M, w the quadratic chirp
 * and B the precomputed transform of the wrapped conj chirp (tables in
 * fsdr_fft_cf32_create). The M-point passes reuse k_fft_stockham. */
__global__ void k_bluestein_pre(const float2* __restrict__ in,
                                float2* __restrict__ out /* frames*M */,
                                const float2* __restrict__ chirp, int n,
                                int M, long long frames, int shift_in) {
    long long total = frames * M;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         id < total; id += stride) {
        long long fr = id / M;
        int j = (int)(id - fr * M);
        float2 v = make_float2(0.f, 0.f);
        if (j < n) {
            int src = shift_in ? (j + n / 2) % n : j; /* fft.rs:179-185 */
            v = cmulf(in[fr * n + src], chirp[j]);
        }
        out[id] = v;
    }
}

__global__ void k_bluestein_mul(float2* __restrict__ x,
                                const float2* __restrict__ B, int M,
                                long long frames) {
    long long total = frames * M;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         id < total; id += stride)
        x[id] = cmulf(x[id], B[id % M]);
}

__global__ void k_bluestein_post(const float2* __restrict__ conv,
                                 float2* __restrict__ out,
                                 float* __restrict__ mag /* nullable */,
                                 const float2* __restrict__ chirp, int n,
                                 int M, long long frames, int shift_out,
                                 float scale) {
    long long total = frames * n;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         id < total; id += stride) {
        long long fr = id / n;
        int k = (int)(id - fr * n);
        int src = shift_out ? (k + n / 2) % n : k; /* fft.rs:196-204 */
        float2 v = cmulf(conv[fr * M + src], chirp[src]);
        v.x *= scale;
        v.y *= scale;
        out[id] = v;
        if (mag) mag[id] = v.x * v.x + v.y * v.y;
    }
}

__global__ __launch_bounds__(256) void k_fft_stockham(
    const float2* __restrict__ in, float2* __restrict__ out,
    float* __restrict__ mag_out /* nullable */,
    const float2* __restrict__ twid, int n, int log2n, int frames_per_block,
    int inverse, int fft_shift, float norm /* 0 = none */,
    long long n_frames) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* ping = (float2*)smem;                 /* [fpb][n] */
    float2* pong = ping + (size_t)frames_per_block * n;

    const int tpf = blockDim.x / frames_per_block;   /* threads per frame */
    const int fl = threadIdx.x / tpf;                /* frame within block */
    const int tf = threadIdx.x % tpf;                /* thread within frame */

    for (long long fb = (long long)blockIdx.x * frames_per_block;
         fb < n_frames; fb += (long long)gridDim.x * frames_per_block) {
        const long long frame = fb + fl;
        float2* a = ping + (size_t)fl * n;
        float2* b = pong + (size_t)fl * n;
        if (frame < n_frames) {
            const float2* src = in + frame * n;
            if (inverse && fft_shift) {       /* fft.rs:179-185: shift input */
                for (int i = tf; i < n; i += tpf)
                    a[fft_swz(i)] = src[(i + n / 2) % n];
            } else {
                for (int i = tf; i < n; i += tpf) a[fft_swz(i)] = src[i];
            }
        }
        __syncthreads();
        int scur = 1;
        int ncur = n;
        while (ncur >= 4) {
            const int m4 = ncur >> 2;
            if (frame < n_frames) {
                for (int bf = tf; bf < n / 4; bf += tpf) {
                    const int p = bf / scur;
                    const int q = bf - p * scur;
                    const int tw = n / ncur; /* twiddle stride */
                    float2 x0 = a[fft_swz(q + scur * p)];
                    float2 x1 = a[fft_swz(q + scur * (p + m4))];
                    float2 x2 = a[fft_swz(q + scur * (p + 2 * m4))];
                    float2 x3 = a[fft_swz(q + scur * (p + 3 * m4))];
                    /* DIF radix-4: butterflies first, output twiddles
                     * W^p, W^2p, W^3p on frequencies 1..3 (omega4 = -i
                     * forward, +i inverse). One twiddle load; the
                     * squares/cubes are derived (unit-vector products,
                     * ~2 ulp). */
                    float2 e0 = f2_add(x0, x2), e1 = f2_sub(x0, x2);
                    float2 o0 = f2_add(x1, x3), o1 = f2_sub(x1, x3);
                    float2 o1r = inverse ? make_float2(-o1.y, o1.x)
                                         : make_float2(o1.y, -o1.x);
                    float2 w1 = twid[(size_t)p * tw];
                    if (inverse) w1.y = -w1.y;
                    float2 w2 = cmulf(w1, w1);
                    float2 w3 = cmulf(w2, w1);
                    b[fft_swz(q + scur * (4 * p + 0))] = f2_add(e0, o0);
                    b[fft_swz(q + scur * (4 * p + 1))] =
                        cmulf(f2_add(e1, o1r), w1);
                    b[fft_swz(q + scur * (4 * p + 2))] =
                        cmulf(f2_sub(e0, o0), w2);
                    b[fft_swz(q + scur * (4 * p + 3))] =
                        cmulf(f2_sub(e1, o1r), w3);
                }
            }
            float2* t = a; a = b; b = t;
            scur <<= 2;
            ncur >>= 2;
            __syncthreads();
        }
        if (ncur == 2) { /* final radix-2 stage when log2n is odd */
            if (frame < n_frames) {
                for (int bf = tf; bf < n / 2; bf += tpf) {
                    const int p = bf / scur;
                    const int q = bf - p * scur;
                    float2 xa = a[fft_swz(q + scur * p)];
                    float2 xb = a[fft_swz(q + scur * (p + 1))];
                    b[fft_swz(q + scur * 2 * p)] = f2_add(xa, xb);
                    b[fft_swz(q + scur * (2 * p + 1))] =
                        cmul_tw(f2_sub(xa, xb), twid[(size_t)p * (n / 2)],
                                inverse);
                }
            }
            float2* t = a; a = b; b = t;
            __syncthreads();
        }
        if (frame < n_frames) {
            float2* dst = out + frame * n;
            const bool shift_out = (!inverse) && fft_shift; /* fft.rs:196-204 */
            for (int i = tf; i < n; i += tpf) {
                float2 v = a[fft_swz(shift_out ? (i + n / 2) % n : i)];
                if (norm != 0.f) { v.x *= norm; v.y *= norm; }
                dst[i] = v;
                if (mag_out) mag_out[frame * n + i] = v.x * v.x + v.y * v.y;
            }
        }
        __syncthreads();
    }
}

/* ================= element-wise ======================================= */

__global__ void k_mag2(const float2* __restrict__ in, float* __restrict__ out,
                       long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         i < n; i += stride) {
        float2 v = in[i];
        out[i] = v.x * v.x + v.y * v.y; /* norm_sqr — spectrum cpu.rs:21-28 */
    }
}

__global__ void k_cmul(const float2* __restrict__ a,
                       const float2* __restrict__ b, float2* __restrict__ o,
                       long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
         i < n; i += stride)
        o[i] = cmulf(a[i], b[i]);
}

/* Deterministic synthetic source: splitmix64 per element, re/im iid
 * uniform[-1,1) (the reference bench convention,
 * crates/futuredsp/benches/benchmarks.rs:23-30). */
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

/* lowbias32 (Wellons): full-avalanche 32-bit hash — two 32-bit mults
 * per 32 output bits vs splitmix64's two 64-bit mults per 64 (64-bit
 * integer mults are multi-op on CDNA4; the fill was ALU-capped below
 * write bandwidth). */
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

__global__ void k_fill_uniform_cf32(float2* __restrict__ out, long long n,
                                    uint64_t seed, uint64_t offset) {
    /* A pair of samples is one float4 store (the source write is inside
     * the bench's timed region — keep it at write bandwidth).
     * Counter-based: deterministic by (seed, element index). */
    const uint32_t sm =
        (uint32_t)seed * 0x9E3779B9u ^ (uint32_t)(seed >> 32);
    long long np = n >> 1;
    long long stride = (long long)gridDim.x * blockDim.x;
    auto pair_at = [&](long long p) {
        long long i = 2 * p;
        uint64_t c64 = 0x5D5D5D5Dull + offset + (uint64_t)i;
        uint32_t c = (uint32_t)c64 ^ (uint32_t)(c64 >> 32) * 0x85EBCA6Bu;
        uint32_t r0 = lowbias32(c * 4u + sm);
        uint32_t r1 = lowbias32(c * 4u + 1u + sm);
        uint32_t r2 = lowbias32(c * 4u + 2u + sm);
        uint32_t r3 = lowbias32(c * 4u + 3u + sm);
        const float s = 2.0f / 16777216.0f;
        return make_float4((r0 >> 8) * s - 1.0f, (r1 >> 8) * s - 1.0f,
                           (r2 >> 8) * s - 1.0f, (r3 >> 8) * s - 1.0f);
    };
    /* Two pairs, a grid stride apart, per iteration: both are hashed
     * before either is stored, so a thread has two stores in flight
     * instead of one behind ~60 dependent integer ops (measured: 1.63 ->
     * 1.56 ms per 8.6 GB fill, profiles/chain_ws_overlap.txt). */
    long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    for (; p + stride < np; p += 2 * stride) {
        float4 a = pair_at(p), b = pair_at(p + stride);
        *(float4*)&out[2 * p] = a;
        *(float4*)&out[2 * (p + stride)] = b;
    }
    if (p < np) *(float4*)&out[2 * p] = pair_at(p);
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        long long i = n - 1;
        uint64_t h =
            splitmix64(seed ^ (0x5D5D5D5Dull + offset + (uint64_t)i));
        out[i] = make_float2(((uint32_t)h >> 8) * (2.0f / 16777216.0f) -
                                 1.0f,
                             ((uint32_t)(h >> 32) >> 8) *
                                     (2.0f / 16777216.0f) -
                                 1.0f);
    }
}

/* ================= IIR filter (futuredsp iir.rs:79-178) ================
 * y[k] = sum_j b[j] x[k+nb-1-j] + sum_q a[q] y[k-1-q] as a blocked linear
 * recurrence. With the state vector s = (y[k-1], ...,
 * y[k-na]) one step is s' = A s + e0 * fir[k], A the companion matrix of
 * a, so a run of outputs from state s is its run from zero state plus the
 * homogeneous response of s. A lane walks one chunk of IIR_L outputs from
 * zero state; the chunk end states are combined across the 256 chunks of
 * a tile by a doubling scan with the constant matrices A^(L*2^d), and the
 * tile end states across the call likewise with A^(tile*2^d). No block
 * waits for another: tile states, their scan and the outputs are three
 * launches.
 *
 * Chunk c of a tile belongs to lane c/4 of wave c%4, so scan levels 0 and
 * 1 (chunk distance 1, 2) cross the waves through LDS and levels 2..7
 * (distance 4*2^k) are __shfl_up by 2^k inside a wave, where "chunk >=
 * distance" is exactly "lane >= 2^k". The staged tile is padded by one
 * float per 64 (IIR_POS), which makes the lanes' chunk walks (stride 64
 * floats) and the coalesced staging/store passes both conflict-free. */
#define IIR_BLOCK 256
#define IIR_L 16                    /* outputs per chunk */
#define IIR_C 256                   /* chunks per tile: one per lane */
#define IIR_TILE (IIR_L * IIR_C)    /* 4096 outputs */
#define IIR_LEVELS 8                /* log2(IIR_C) */
#define IIR_P 1024                  /* tile states per pass of the scan */
#define IIR_P_LEVELS 10             /* log2(IIR_P) */
#define IIR_NA_MAX 8
#define IIR_NB_MAX 64
#define IIR_POS(s) ((s) + ((s) >> 6))
#define IIR_XS_FLOATS (IIR_POS(IIR_TILE + IIR_NB_MAX - 1) + 1)

struct IirA { float a[IIR_NA_MAX]; };

/* thread -> chunk of the tile (or tile state of the pass), and back, in a
 * block of W waves: element c belongs to lane c/W of wave c%W */
template <int W = IIR_BLOCK / 64>
__device__ __forceinline__ int iir_chunk_of(int tid) {
    return (tid & 63) * W + (tid >> 6);
}
template <int W = IIR_BLOCK / 64>
__device__ __forceinline__ int iir_tid_of(int c) {
    return (c % W) * 64 + c / W;
}

/* p += M o, M row-major NA x NA (block-uniform, so scalar loads) */
template <int NA>
__device__ __forceinline__ void iir_matvec_add(float (&p)[NA],
                                               const float (&o)[NA],
                                               const float* __restrict__ M) {
#pragma unroll
    for (int q = 0; q < NA; q++) {
        float acc = p[q];
#pragma unroll
        for (int r = 0; r < NA; r++) acc = fmaf(M[q * NA + r], o[r], acc);
        p[q] = acc;
    }
}

/* Inclusive doubling scan over the NT states of a block of NT threads:
 * P_c = sum_{k<=c} B^(c-k) p_k with pw[d] = B^(2^d). The first log2(NT/64)
 * levels cross the waves through sc (NA*NT floats), the rest are shuffles. */
template <int NA, int NT = IIR_BLOCK>
__device__ __forceinline__ void iir_scan(float (&p)[NA],
                                         const float* __restrict__ pw,
                                         float* sc) {
    constexpr int W = NT / 64;
    constexpr int LW = W == 4 ? 2 : 4, LV = LW + 6;
    static_assert((1 << LW) == W, "4 or 16 waves");
    const int tid = threadIdx.x, c = iir_chunk_of<W>(tid), lane = tid & 63;
    float o[NA];
#pragma unroll
    for (int d = 0; d < LW; d++) {
#pragma unroll
        for (int r = 0; r < NA; r++) sc[r * NT + tid] = p[r];
        __syncthreads();
        const int src = iir_tid_of<W>(c >= (1 << d) ? c - (1 << d) : 0);
#pragma unroll
        for (int r = 0; r < NA; r++) o[r] = sc[r * NT + src];
        __syncthreads();
        if (c >= (1 << d)) iir_matvec_add<NA>(p, o, pw + d * NA * NA);
    }
#pragma unroll
    for (int d = LW; d < LV; d++) {
#pragma unroll
        for (int r = 0; r < NA; r++)
            o[r] = __shfl_up(p[r], 1 << (d - LW), 64);
        if (lane >= (1 << (d - LW)))
            iir_matvec_add<NA>(p, o, pw + d * NA * NA);
    }
}

/* Stage inputs [base, base + IIR_TILE + nb - 1) of `in` into xs. GUARD:
 * the boundary tile, zero past n_need; interior tiles issue their 16 (or
 * 4 wide, when `in` is 16-byte aligned) loads back to back. */
template <bool GUARD>
__device__ __forceinline__ void iir_stage(const float* __restrict__ in,
                                          long long base, long long n_need,
                                          int nb, float* xs) {
    const int tid = threadIdx.x;
    const float* src = in + base;
    float t = 0.f;
    const bool tail = tid < nb - 1;
    if (GUARD) {
        const long long left = n_need - base;
        float v[IIR_L];
#pragma unroll
        for (int u = 0; u < IIR_L; u++) {
            const int s = tid + IIR_BLOCK * u;
            v[u] = s < left ? src[s] : 0.f;
        }
        if (tail && IIR_TILE + tid < left) t = src[IIR_TILE + tid];
#pragma unroll
        for (int u = 0; u < IIR_L; u++)
            xs[IIR_POS(tid + IIR_BLOCK * u)] = v[u];
    } else if ((((uintptr_t)in) & 15) == 0) {
        /* IIR_TILE*4 bytes is a multiple of 16: aligned for every tile */
        float4 v[IIR_L / 4];
#pragma unroll
        for (int u = 0; u < IIR_L / 4; u++)
            v[u] = ((const float4*)src)[tid + IIR_BLOCK * u];
        if (tail) t = src[IIR_TILE + tid];
#pragma unroll
        for (int u = 0; u < IIR_L / 4; u++) {
            const int p = IIR_POS(4 * (tid + IIR_BLOCK * u));
            xs[p] = v[u].x; xs[p + 1] = v[u].y;
            xs[p + 2] = v[u].z; xs[p + 3] = v[u].w;
        }
    } else {
        float v[IIR_L];
#pragma unroll
        for (int u = 0; u < IIR_L; u++) v[u] = src[tid + IIR_BLOCK * u];
        if (tail) t = src[IIR_TILE + tid];
#pragma unroll
        for (int u = 0; u < IIR_L; u++)
            xs[IIR_POS(tid + IIR_BLOCK * u)] = v[u];
    }
    if (tail) xs[IIR_POS(IIR_TILE + tid)] = t;
}

/* The lane's chunk from zero state: z[i] = fir[c0+i] + sum_q a[q] z[i-1-q]
 * (z[<0] = 0). The FIR part slides a 16-float register window down the
 * staged tile, one LDS read per tap. */
template <int NA>
__device__ __forceinline__ void iir_chunk(const float* xs,
                                          const float* __restrict__ b,
                                          int nb, const IirA& a,
                                          float (&z)[IIR_L]) {
    const int c0 = iir_chunk_of(threadIdx.x) * IIR_L;
    float w[IIR_L];
#pragma unroll
    for (int i = 0; i < IIR_L; i++) {
        w[i] = xs[IIR_POS(c0 + nb - 1 + i)];
        z[i] = 0.f;
    }
    for (int j = 0;; j++) {
        const float bj = b[j];
#pragma unroll
        for (int i = 0; i < IIR_L; i++) z[i] = fmaf(bj, w[i], z[i]);
        if (j + 1 == nb) break;
#pragma unroll
        for (int i = IIR_L - 1; i > 0; i--) w[i] = w[i - 1];
        w[0] = xs[IIR_POS(c0 + nb - 2 - j)];
    }
#pragma unroll
    for (int i = 0; i < IIR_L; i++) {
        float acc = z[i];
#pragma unroll
        for (int q = 0; q < NA; q++)
            if (i - 1 - q >= 0) acc = fmaf(a.a[q], z[i - 1 - q], acc);
        z[i] = acc;
    }
}

/* Zero-state end state of every tile but the call's last (all of them
 * full, so there is no boundary here): T[tile*NA + q]. Writes nothing
 * else. */
template <int NA>
__global__ __launch_bounds__(IIR_BLOCK) void k_iir_tile_state(
    const float* __restrict__ in, float* __restrict__ T,
    const float* __restrict__ b, int nb, IirA a,
    const float* __restrict__ pc, long long n_tiles) {
    __shared__ float xs[IIR_XS_FLOATS];
    __shared__ float sc[NA * IIR_BLOCK];
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        iir_stage<false>(in, tile * IIR_TILE, 0, nb, xs);
        __syncthreads();
        float z[IIR_L];
        iir_chunk<NA>(xs, b, nb, a, z);
        float p[NA];
#pragma unroll
        for (int q = 0; q < NA; q++) p[q] = z[IIR_L - 1 - q];
        iir_scan<NA>(p, pc, sc);
        if (threadIdx.x == IIR_BLOCK - 1) {
#pragma unroll
            for (int q = 0; q < NA; q++) T[tile * NA + q] = p[q];
        }
        __syncthreads(); /* xs is restaged next */
    }
}

/* S[k] = state entering tile k: S[0] = mem, S[k+1] = A^tile S[k] + T[k].
 * One block of IIR_P threads; IIR_P tile states per pass of the doubling
 * scan, the last state of a pass seeding the next. */
template <int NA>
__global__ __launch_bounds__(IIR_P) void k_iir_tile_scan(
    const float* __restrict__ T, float* __restrict__ S,
    const float* __restrict__ mem, const float* __restrict__ pt,
    long long n_tiles) {
    __shared__ float sc[NA * IIR_P];
    const int tid = threadIdx.x, c = iir_chunk_of<IIR_P / 64>(tid);
    float carry[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) carry[q] = mem[q];
    if (tid < NA) S[tid] = mem[tid];
    for (long long base = 0; base < n_tiles - 1; base += IIR_P) {
        const long long k = base + c;
        float p[NA];
#pragma unroll
        for (int q = 0; q < NA; q++)
            p[q] = k < n_tiles - 1 ? T[k * NA + q] : 0.f;
        if (c == 0) iir_matvec_add<NA>(p, carry, pt);
        iir_scan<NA, IIR_P>(p, pt, sc);
        if (k < n_tiles - 1) {
#pragma unroll
            for (int q = 0; q < NA; q++) S[(k + 1) * NA + q] = p[q];
        }
        if (tid == IIR_P - 1) {
#pragma unroll
            for (int q = 0; q < NA; q++) sc[q] = p[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NA; q++) carry[q] = sc[q];
        __syncthreads();
    }
}

/* The outputs: the chunk pass again, the in-tile scan seeded with the
 * tile's incoming state S[tile], y = z + H s per chunk, coalesced store
 * through the staging buffer. The block of the last tile also writes the
 * memory the next call sees (iir.rs:154-160 after n steps): y[n-1-j], or
 * where that lies in front of this tile, the incoming state, which for
 * tile 0 is the old memory shifted (a call with n < na). */
template <int NA>
__global__ __launch_bounds__(IIR_BLOCK) void k_iir_apply(
    const float* __restrict__ in, float* __restrict__ out,
    const float* __restrict__ S, float* __restrict__ mem_new,
    const float* __restrict__ b, int nb, IirA a,
    const float* __restrict__ H, const float* __restrict__ pc, long long n,
    long long n_tiles) {
    __shared__ float xs[IIR_XS_FLOATS];
    __shared__ float sc[(NA ? NA : 1) * IIR_BLOCK];
    const int tid = threadIdx.x, c = iir_chunk_of(tid);
    const long long n_need = n + nb - 1;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long base = tile * IIR_TILE;
        if (base + IIR_TILE + nb - 1 > n_need)
            iir_stage<true>(in, base, n_need, nb, xs);
        else
            iir_stage<false>(in, base, n_need, nb, xs);
        __syncthreads();
        float z[IIR_L];
        iir_chunk<NA>(xs, b, nb, a, z);
        if constexpr (NA > 0) {
            float s_in[NA], p[NA], s[NA];
#pragma unroll
            for (int q = 0; q < NA; q++) {
                s_in[q] = S[tile * NA + q];
                p[q] = z[IIR_L - 1 - q];
            }
            if (c == 0) iir_matvec_add<NA>(p, s_in, pc);
            iir_scan<NA>(p, pc, sc);
#pragma unroll
            for (int q = 0; q < NA; q++) sc[q * IIR_BLOCK + tid] = p[q];
            __syncthreads();
            const int src = iir_tid_of(c > 0 ? c - 1 : 0);
#pragma unroll
            for (int q = 0; q < NA; q++)
                s[q] = c > 0 ? sc[q * IIR_BLOCK + src] : s_in[q];
#pragma unroll
            for (int i = 0; i < IIR_L; i++) {
                float corr = 0.f;
#pragma unroll
                for (int q = 0; q < NA; q++)
                    corr = fmaf(H[i * NA + q], s[q], corr);
                z[i] += corr;
            }
        } else {
            __syncthreads(); /* every lane is done reading xs */
        }
#pragma unroll
        for (int i = 0; i < IIR_L; i++) xs[IIR_POS(c * IIR_L + i)] = z[i];
        __syncthreads();
        const long long left = n - base;
#pragma unroll
        for (int u = 0; u < IIR_L; u++) {
            const int s = tid + IIR_BLOCK * u;
            if (s < left) out[base + s] = xs[IIR_POS(s)];
        }
        if (NA > 0 && tile == n_tiles - 1 && tid < NA) {
            const long long m = n - 1 - tid;
            mem_new[tid] = m >= base ? xs[IIR_POS((int)(m - base))]
                                     : S[tile * NA + (base - 1 - m)];
        }
        __syncthreads(); /* xs is restaged next */
    }
}

/* ================= LoRa FFT demodulator =================================
 * One symbol of N = 2^sf samples times the handle's downchirp, N-point
 * forward FFT, |X|^2 in f32, then one of three reductions over the bins
 * ("LoRa FFT demodulator"): RAW is get_symbol_val
 * (examples/lora/src/utils.rs:1059-1078), HARD is fft_demod.rs:115-120 +
 * 238-248, SOFT the max-log branch of compute_llrs (fft_demod.rs:126-208).
 * A block of 256 threads holds LORA spb = min(16, max(1, 1024/N)) symbols
 * in fft_swz ping/pong buffers, 256/spb threads each; the product is
 * formed while staging, the spectrum never leaves LDS, and a symbol leaves
 * as one u16 or twelve f64. Blocks walk the batches of spb symbols
 * persistently. */
#define LORA_BLOCK 256
#define LORA_RAW 0
#define LORA_HARD 1
#define LORA_SOFT 2
#define LORA_MAX_SF 12
#define LORA_RED_DOUBLES (4 * 2 * LORA_MAX_SF) /* 4 waves x 24 maxima */

/* ln I0(x), x >= 0, for the SOFT log-likelihoods. Below 20 the power series
 * sum_j (x^2/4)^j / (j!)^2 the reference sums (fft_demod.rs:9-23), all
 * terms positive, cut where a term falls under 1e-17 of the sum (at most
 * ~50 terms); from 20 on Hankel's expansion I0(x) = e^x / sqrt(2 pi x) *
 * sum_k ((2k-1)!!)^2 / (k! (8x)^k), whose smallest term is ~e^(-2x) <=
 * 4e-18 there, so ln I0 = x - ln(2 pi x)/2 + ln(sum) never forms e^709.
 * Both agree with the reference's series to a few ulp of the sum. */
#define LORA_I0_TERMS 96
struct LoraInvSquares { /* v[j] = 1/j^2: the series without a division */
    double v[LORA_I0_TERMS];
    constexpr LoraInvSquares() : v() {
        for (int j = 1; j < LORA_I0_TERMS; j++)
            v[j] = 1.0 / ((double)j * (double)j);
    }
};
static constexpr LoraInvSquares lora_inv_sq;

__host__ __device__ static inline double lora_log_i0(double x) {
    x = fabs(x);
    if (x < 20.0) {
        const double base = 0.25 * x * x;
        double add = 1.0, sum = 1.0;
        for (int j = 1; j < LORA_I0_TERMS; j++) {
            add *= base * lora_inv_sq.v[j];
            sum += add;
            if (add < 1e-17 * sum) break;
        }
        return log(sum);
    }
    const double r = 0.125 / x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; k++) {
        const double m = (double)(2 * k - 1);
        const double next = term * (m * m * r / (double)k);
        if (!(next < term)) break; /* the expansion has turned */
        term = next;
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return x - 0.5 * log(6.283185307179586476925 * x) + log(sum);
}

/* Reduce v over the tps threads of a symbol (tps a power of two, the
 * symbol's threads contiguous and aligned to it): xor butterflies inside a
 * wave, then one exchange through sc (4 entries, one per wave) when the
 * symbol spans several waves. Every thread of the symbol gets the result.
 * op must be commutative and associative. Called by the whole block. */
template <class T, class Op>
__device__ __forceinline__ T lora_sym_reduce(T v, Op op, int tps, T* sc) {
    const int w = tps < 64 ? tps : 64;
    for (int off = w >> 1; off; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    if (tps > 64) {
        const int wv = threadIdx.x >> 6, nw = tps >> 6;
        const int w0 = (threadIdx.x / tps) * nw;
        if ((threadIdx.x & 63) == 0) sc[wv] = v;
        __syncthreads();
        v = sc[w0];
        for (int k = 1; k < nw; k++) v = op(v, sc[w0 + k]);
        __syncthreads();
    }
    return v;
}

/* E = N * spb / 256 samples per thread, so a symbol's staging loads are
 * issued together. n_sym whole symbols; out is u16[n_sym] (RAW, HARD) or
 * f64[n_sym][12] (SOFT). Dynamic LDS: 2 * spb * N float2, then
 * LORA_RED_DOUBLES doubles. */
template <int MODE, int E>
__global__ __launch_bounds__(LORA_BLOCK) void k_lora_demod(
    const float2* __restrict__ in, void* __restrict__ out,
    const float2* __restrict__ chirp, const float2* __restrict__ twid,
    int sf, int spb, int reduced, long long n_sym) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = 1 << sf;
    float2* ping = (float2*)smem;
    float2* pong = ping + (size_t)spb * n;
    double* red = (double*)(pong + (size_t)spb * n);
    const int tps = LORA_BLOCK / spb;      /* threads per symbol */
    const int sl = threadIdx.x / tps;      /* symbol within the block */
    const int ts = threadIdx.x - sl * tps; /* thread within the symbol */
    const int div = reduced ? 4 : 1;
    const long long n_batches = (n_sym + spb - 1) / spb;
    for (long long bt = blockIdx.x; bt < n_batches; bt += gridDim.x) {
        const long long sym = bt * spb + sl;
        const bool live = sym < n_sym;
        float2* a = ping + (size_t)sl * n;
        float2* b = pong + (size_t)sl * n;
        {
            /* volk_32fc_x2_multiply_32fc(samples, downchirp); a symbol
             * past the end stages zeros and stores nothing */
            float2 x[E], c[E];
            const float2* src = in + (live ? sym : 0) * n;
#pragma unroll
            for (int u = 0; u < E; u++) {
                x[u] = live ? src[ts + u * tps] : make_float2(0.f, 0.f);
                c[u] = chirp[ts + u * tps];
            }
#pragma unroll
            for (int u = 0; u < E; u++)
                a[fft_swz((unsigned)(ts + u * tps))] = cmulf(x[u], c[u]);
        }
        __syncthreads();
        const float2* res = fft_pow2_fwd(a, b, twid, n, ts, tps);
        float* mag = (float*)(res == a ? b : a); /* the idle buffer */
        /* |X|^2 as volk_32fc_magnitude_squared_32f (no contraction), and
         * the argmax under max_by(total_cmp): the magnitudes are >= +0, so
         * their bit patterns order as unsigned and (bits << 32 | index)
         * has the largest magnitude, then the last index, as its maximum */
        unsigned long long key = 0;
#pragma unroll
        for (int u = 0; u < E; u++) {
            const int i = ts + u * tps;
            const float2 v = res[fft_swz((unsigned)i)];
            const float m =
                __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));
            const unsigned long long k =
                ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)i;
            key = k > key ? k : key;
            if (MODE == LORA_SOFT) mag[i] = m; /* read back by this thread */
        }
        key = lora_sym_reduce(
            key,
            [](unsigned long long p, unsigned long long q) {
                return p > q ? p : q;
            },
            tps, (unsigned long long*)red);
        const int idx = (int)(unsigned)key;
        const float top = __uint_as_float((unsigned)(key >> 32));
        if (MODE == LORA_RAW) {
            /* utils.rs:1071-1077: None where the f64 sum of the bins is 0,
             * which for magnitudes >= 0 is where the largest is 0 */
            if (live && ts == 0)
                ((unsigned short*)out)[sym] =
                    top == 0.f ? (unsigned short)0xFFFF : (unsigned short)idx;
        } else if (MODE == LORA_HARD) {
            if (live && ts == 0)
                ((unsigned short*)out)[sym] =
                    (unsigned short)(((idx - 1) & (n - 1)) / div);
        } else {
            auto add = [](double p, double q) { return p + q; };
            double sig = 0.0, noi = 0.0;
#pragma unroll
            for (int u = 0; u < E; u++) {
                const int i = ts + u * tps;
                const int d = i > idx ? i - idx : idx - i;
                const double m = (double)mag[i];
                if (d % (n - 1) < 2) sig += m; else noi += m;
            }
            sig = lora_sym_reduce(sig, add, tps, red);
            noi = lora_sym_reduce(noi, add, tps, red);
            const double ps = sig / (double)n, pn = noi / (double)(n - 3);
            const double K = sqrt(ps) / pn;
            /* the argument grows with the magnitude, so "any bin reaches
             * 709" is "the largest bin does" */
            const bool clip = !(K * sqrt((double)top * (double)n) < 709.0);
            /* ll_n grows with the magnitude in either branch, so the
             * maximum of ll over a set of bins is ll of the set's largest
             * magnitude: the 2 * sf maxima are taken over the f32
             * magnitudes and ln I0 runs 2 * sf times per symbol, not N.
             * -1 marks a set without bins (its maximum stays 0). */
            float mx1[LORA_MAX_SF], mx0[LORA_MAX_SF];
#pragma unroll
            for (int bit = 0; bit < LORA_MAX_SF; bit++)
                mx1[bit] = mx0[bit] = -1.f;
#pragma unroll
            for (int u = 0; u < E; u++) {
                const int i = ts + u * tps;
                const float m = mag[i];
                int s = ((i - 1) & (n - 1)) / div;
                s ^= s >> 1; /* Gray map, fft_demod.rs:192-194 */
#pragma unroll
                for (int bit = 0; bit < LORA_MAX_SF; bit++) {
                    const bool one = (s >> bit) & 1;
                    mx1[bit] = fmaxf(mx1[bit], one ? m : -1.f);
                    mx0[bit] = fmaxf(mx0[bit], one ? -1.f : m);
                }
            }
            /* the 24 maxima: butterflies, then one exchange for all */
            const int w = tps < 64 ? tps : 64;
#pragma unroll
            for (int bit = 0; bit < LORA_MAX_SF; bit++) {
                for (int off = w >> 1; off; off >>= 1) {
                    mx1[bit] = fmaxf(mx1[bit], __shfl_xor(mx1[bit], off, 64));
                    mx0[bit] = fmaxf(mx0[bit], __shfl_xor(mx0[bit], off, 64));
                }
            }
            if (tps > 64) {
                float* redf = (float*)red;
                const int wv = threadIdx.x >> 6, nw = tps >> 6;
                const int w0 = sl * nw;
                if ((threadIdx.x & 63) == 0) {
#pragma unroll
                    for (int bit = 0; bit < LORA_MAX_SF; bit++) {
                        redf[wv * 2 * LORA_MAX_SF + 2 * bit] = mx1[bit];
                        redf[wv * 2 * LORA_MAX_SF + 2 * bit + 1] = mx0[bit];
                    }
                }
                __syncthreads();
                for (int k = 0; k < nw; k++) {
                    const float* r = redf + (w0 + k) * 2 * LORA_MAX_SF;
#pragma unroll
                    for (int bit = 0; bit < LORA_MAX_SF; bit++) {
                        mx1[bit] = fmaxf(mx1[bit], r[2 * bit]);
                        mx0[bit] = fmaxf(mx0[bit], r[2 * bit + 1]);
                    }
                }
            }
            /* every lane now holds all 24; lane j < 24 of the symbol turns
             * number j (max_x1 of bit j/2 for even j, max_x0 for odd) into
             * its ll, and the even lane next to it writes the difference:
             * llrs[sf-1-bit] = max_x1 - max_x0, MSB first; the rest 0 */
            for (int base = 0; base < 2 * LORA_MAX_SF; base += tps) {
                const int j = base + ts;
                float m = -1.f;
#pragma unroll
                for (int bit = 0; bit < LORA_MAX_SF; bit++) {
                    m = j == 2 * bit ? mx1[bit] : m;
                    m = j == 2 * bit + 1 ? mx0[bit] : m;
                }
                double ll = 0.0;
                if (m >= 0.f) {
                    const double mn = (double)m * (double)n;
                    ll = clip ? mn : lora_log_i0(K * sqrt(mn));
                }
                const double d = ll - __shfl_xor(ll, 1, 64);
                const int bit = j >> 1;
                if (live && !(j & 1) && bit < LORA_MAX_SF)
                    ((double*)out)[sym * LORA_MAX_SF +
                                   (bit < sf ? sf - 1 - bit : bit)] =
                        bit < sf ? d : 0.0;
            }
        }
        __syncthreads(); /* the buffers are restaged next */
    }
}

/* ================= host-side status math ============================== */

static size_t sat_sub(size_t a, size_t b) { return a > b ? a - b : 0; }

/* fir.rs:69-74 */
static fsdr_filter_result fir_status(size_t n_in, size_t nt, size_t n_out) {
    size_t prod = sat_sub(n_in + 1, nt);
    fsdr_filter_result r;
    if (prod > n_out) {
        r.consumed = r.produced = n_out;
        r.status = FSDR_INSUFFICIENT_OUTPUT;
    } else if (prod == n_out) {
        r.consumed = r.produced = prod;
        r.status = FSDR_BOTH_SUFFICIENT;
    } else {
        r.consumed = r.produced = prod;
        r.status = FSDR_INSUFFICIENT_INPUT;
    }
    return r;
}

/* decimating_fir.rs:71-78,94 */
static fsdr_filter_result decim_status(size_t D, size_t n_in, size_t nt,
                                       size_t n_out) {
    size_t consumable = sat_sub(n_in + 1, nt) / D;
    fsdr_filter_result r;
    if (consumable > n_out) {
        r.produced = n_out;
        r.status = FSDR_INSUFFICIENT_OUTPUT;
    } else if (consumable == n_out) {
        r.produced = n_out;
        r.status = FSDR_BOTH_SUFFICIENT;
    } else {
        r.produced = consumable;
        r.status = FSDR_INSUFFICIENT_INPUT;
    }
    r.consumed = r.produced * D;
    return r;
}

/* polyphase_resampling_fir.rs:90-106 */
static fsdr_filter_result resamp_status(size_t L, size_t M, size_t nt_total,
                                        size_t n_in, size_t n_out) {
    size_t nt = nt_total / L;
    size_t prod = sat_sub(sat_sub(n_in + 1, nt) * L, 1) / M;
    prod = (prod / L) * L;
    fsdr_filter_result r;
    if (prod > n_out) {
        r.produced = (n_out / L) * L;
        r.status = FSDR_INSUFFICIENT_OUTPUT;
    } else if (prod == n_out) {
        r.produced = prod;
        r.status = FSDR_BOTH_SUFFICIENT;
    } else {
        r.produced = prod;
        r.status = FSDR_INSUFFICIENT_INPUT;
    }
    r.consumed = (r.produced / L) * M;
    return r;
}

/* ================= filter handles ===================================== */

enum FilterKind { K_FIR_CF32, K_FIR_F32, K_DECIM_CF32, K_RESAMP_CF32,
                  K_FFT_CF32, K_MAG2, K_FIR_CCF32, K_MOVAVG,
                  K_XLATING, K_PFB, K_PFB_SYNTH, K_PFB_ARB, K_RESAMP_F32,
                  K_QUAD_DEMOD, K_FM_DEMOD_RESAMP, K_IIR_F32, K_LORA_DEMOD };

/* "On unless the variable parses to 0", and "the variable's integer value,
 * or dflt when unset". Both read the environment on every call: the tests
 * flip these switches between calls inside one process. */
static bool env_on(const char* name) {
    const char* e = getenv(name);
    return !e || atoi(e) != 0;
}
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

/* Two copies of a carried state in one buffer, `n` items of T each. A
 * launch reads live() and writes next(); the caller flips once the launch
 * is enqueued. */
struct carried_state {
    dev_buf buf;
    size_t i = 0;
    template <class T>
    T* live(size_t n) const { return buf.as<T>() + i * n; }
    template <class T>
    T* next(size_t n) const { return buf.as<T>() + (i ^ 1) * n; }
    void flip() { i ^= 1; }
};

/* A handle owns all of its device memory as dev_buf members, and its
 * inner handles and host-side plans through ~fsdr_filter: destroying the
 * handle is the only place any of it is released, so a *_create that
 * fails part-way deletes the handle and returns null. Each block family
 * keeps its state in its own member struct; a handle uses its family's
 * and leaves the others empty. */
struct fsdr_filter {
    FilterKind kind;
    size_t item_in = 8, item_out = 8;
    size_t length = 0; /* what fsdr_filter_length reports (min_items) */
    /* staging buffers of the host-span path (fsdr_filter_host) */
    dev_buf stage_in, stage_out;

    /* Fir, FirCC, FirF32, DecimatingFir, XlatingFir and the polyphase
     * resamplers (FM back end included): the taps as the generic kernel
     * of the kind reads them, and for the cf32 FIR and the decimating FIR
     * the template variants picked at create, each with its own taps
     * layout (0 = that variant does not apply). */
    struct {
        size_t n_taps = 0;   /* true tap count */
        size_t decim = 1, interp = 1;
        int n_padded = 0;    /* device taps length (leading zeros) */
        dev_buf taps;
        int tp_tpl = 0;      /* template tap count */
        dev_buf rtaps;       /* reversed taps zero-filled to tp_tpl; for
                                decimation 4, four phase rows of them */
        int kk_mfma = 0;     /* MFMA variant K (>= n_taps+15, %4==0) */
        dev_buf mtaps;       /* reversed taps zero-filled to kk_mfma */
        int kk_mfma32 = 0;   /* 32x32 variant K (>= n_taps+31, even) */
        dev_buf mtaps32;
        /* 1:4 cf32 resampler: the decimating FIR whose MFMA kernel it
         * launches */
        fsdr_filter* decim4 = nullptr;
    } fir;

    /* XlatingFir: fir.taps holds the band-pass taps (float2, reversed) */
    struct {
        float theta = 0.f;                /* rotator increment */
        float rot_re = 1.f, rot_im = 0.f; /* rotator phase, carried */
    } xlat;

    /* Fft. Bluestein (non-pow2 len): m = next pow2 >= 2*len-1; chirp
     * w(k) = e^{sigma*pi*i*k^2/len}; B = DFT_m of the wrapped conj chirp.
     * fft.rs is generic over rustfft plan lengths; this closes the
     * pow2-only gap via two pow2 m-point passes per batch, in `work`. */
    struct {
        size_t len = 0;
        int inverse = 0, shift = 0;
        float norm = 0.f;
        dev_buf twid;        /* len (Bluestein: m) twiddles */
        size_t m = 0;        /* 0 = plain pow2 Stockham */
        dev_buf chirp, B, work;
    } fft;

    /* MovingAvg */
    struct {
        size_t width = 0, history = 0;
        size_t i = 0;        /* frames since the last emission */
        float decay = 0.f;
        dev_buf avg;         /* the EMA state, width floats */
        /* chunk partials of the fast path. Not a staging buffer: on the
         * host path stage_in holds the input that the partials kernel is
         * still reading. */
        dev_buf partials;
    } movavg;

    /* What the three PFB blocks share: the channel count, taps per
     * polyphase filter, and (channelizer, synthesizer) the inner IFFT. */
    struct {
        size_t channels = 0, tpf = 0;
        fsdr_filter* ifft = nullptr;
    } pfb;

    /* PFB channelizer. Streaming state: the last channels*tpf consumed
     * samples (every consumed sample while pushes < 2*channels*tpf, for
     * the start-up steps) and the total pushes (channelizer.rs
     * round-robin state). */
    struct {
        size_t decim = 1;    /* channels / oversample_rate */
        dev_buf taps;        /* part[i][c] = taps[i + c*channels] */
        size_t pushes = 0;
        dev_buf hist;
        dev_buf work;        /* [hist, chunk] of one stream call */
        dev_buf dots, spectra; /* IFFT input and output, steps*channels */
    } chan;

    /* PFB synthesizer. The stream carries the last tpf-1 IFFT'd frames
     * and the IFFT'd frames of steps 0..2tpf-2 for the start-up rows; the
     * one-shot entry point keeps its start-up frames apart so it leaves a
     * stream on the same handle alone. */
    struct {
        dev_buf taps;        /* partT[j*channels + c]: partition, transposed */
        size_t steps = 0;    /* consumed by the stream so far */
        carried_state hist;  /* (tpf-1)*channels float2 per copy */
        dev_buf early, early_oneshot;
        dev_buf gathered, frames; /* staged path: IFFT input, [hist, IFFT'd] */
    } synth;

    /* PFB arb resampler: the owned schedule and its checkpoints on the
     * device; the stream carries each channel's window of tpf samples. */
    struct {
        fsdr_pfb_arb_schedule* sched = nullptr;
        dev_buf taps;        /* rpart[f][t] = part[f][tpf-1-t] */
        dev_buf ck;
        size_t consumed = 0; /* inputs so far, the tpf fill pushes included */
        carried_state window; /* channels*tpf float2 per copy */
        dev_buf window_oneshot;
    } arb;

    /* QuadDemod / FM demod+resampler: the carried Complex32 `last`
     * (main.rs:99-104), zero on a fresh handle. */
    struct {
        dev_buf last;
        dev_buf staged;      /* unfused FM path: the demodulated span */
    } demod;

    /* IIR: the owned plan (a and the tables) with the tables on the
     * device (H, chunk powers, tile powers). mem[j] = y[-1-j]. */
    struct {
        fsdr_iir_plan* plan = nullptr;
        size_t n_b = 0;
        dev_buf b, tables;
        size_t filled = 0;   /* memory.len(): the fill count */
        carried_state mem;   /* IIR_NA_MAX floats per copy */
        dev_buf tile_states; /* tile states, then the states entering each */
    } iir;

    /* LoRa FFT demodulator: N = 2^sf. */
    struct {
        unsigned sf = 0;
        int mode = 0, reduced = 0; /* LORA_RAW/HARD/SOFT; reduced rate */
        dev_buf chirp;       /* downchirp of the current frame, N entries */
        dev_buf twid;        /* N-point twiddles */
    } lora;

    ~fsdr_filter(); /* below, once the plan types are complete */
};

/* Allocate exactly n items and copy them up; on failure set `err` and
 * leave the buffer empty. */
template <class T>
static bool upload(dev_buf& b, const T* host, size_t n, const char* err) {
    if (b.upload(host, n) == hipSuccess) return true;
    set_err(err);
    return false;
}
template <class T>
static bool upload(dev_buf& b, const std::vector<T>& v, const char* err) {
    return upload(b, v.data(), v.size(), err);
}

/* n zeroed bytes */
static bool alloc_zeroed(dev_buf& b, size_t n, const char* err) {
    if (b.ensure(n) == hipSuccess && b.zero() == hipSuccess) return true;
    set_err(err);
    return false;
}

/* pad taps to tp ≡ 1 (mod m) with leading zeros (zero taps
 * multiply staged zeros beyond the true window; result unchanged). */
static int upload_taps_padded(fsdr_filter* f, const float* taps, size_t nt,
                              int mod) {
    size_t tp = nt;
    while (tp % mod != 1 % mod) tp++;
    std::vector<float> h(tp, 0.f);
    memcpy(h.data() + (tp - nt), taps, nt * sizeof(float));
    HIP_TRY(f->fir.taps.upload(h.data(), tp));
    f->fir.n_padded = (int)tp;
    return FSDR_OK;
}

/* taps reversed and zero-filled to `len` (>= nt) */
static bool upload_reversed(dev_buf& b, const float* taps, size_t nt,
                            size_t len, const char* err) {
    std::vector<float> rt(len, 0.f);
    for (size_t i = 0; i < nt; i++) rt[i] = taps[nt - 1 - i];
    return upload(b, rt, err);
}

/* decimation-4 phase split: row v of `stride` floats holds
 * h[nt-1-(4u+v)] at u < n_u, zeros elsewhere */
static bool upload_phase_split(dev_buf& b, const float* taps, size_t nt,
                               int n_u, int stride, const char* err) {
    std::vector<float> rows(4 * (size_t)stride, 0.f);
    for (int v = 0; v < 4; v++)
        for (int u = 0; u < n_u; u++) {
            size_t t = 4 * (size_t)u + v;
            if (t < nt) rows[v * stride + u] = taps[nt - 1 - t];
        }
    return upload(b, rows, err);
}

/* a *_create that fails after the handle exists; the error is set */
static fsdr_filter* create_failed(fsdr_filter* f) {
    delete f;
    return nullptr;
}

static fsdr_filter* create_common(FilterKind k) {
    if (!have_gpu()) {
        set_err("no HIP device present — cannot create GPU filter");
        return nullptr;
    }
    fsdr_filter* f = new fsdr_filter();
    f->kind = k;
    return f;
}

extern "C" fsdr_filter* fsdr_fir_cf32_create(const float* taps,
                                             size_t n_taps) {
    if (!taps || n_taps == 0) { set_err("null/empty taps"); return nullptr; }
    fsdr_filter* f = create_common(K_FIR_CF32);
    if (!f) return nullptr;
    f->length = f->fir.n_taps = n_taps;
    /* the template variants take reversed taps zero-filled to the
     * smallest instantiated size that fits */
    f->fir.tp_tpl = tpl_at_least(fir_tpl_tps{}, n_taps);
    f->fir.kk_mfma32 = tpl_at_least(fir_mfma32_ks{}, n_taps + 31);
    f->fir.kk_mfma = tpl_at_least(fir_mfma_ks{}, n_taps + 15);
    if (upload_taps_padded(f, taps, n_taps, 8) != FSDR_OK ||
        (f->fir.tp_tpl &&
         !upload_reversed(f->fir.rtaps, taps, n_taps, f->fir.tp_tpl,
                          "reversed taps upload failed")) ||
        (f->fir.kk_mfma32 &&
         !upload_reversed(f->fir.mtaps32, taps, n_taps, f->fir.kk_mfma32,
                          "mfma32 taps upload failed")) ||
        (f->fir.kk_mfma &&
         !upload_reversed(f->fir.mtaps, taps, n_taps, f->fir.kk_mfma,
                          "mfma taps upload failed")))
        return create_failed(f);
    return f;
}

extern "C" fsdr_filter* fsdr_fir_ccf32_create(const fsdr_cf32* taps,
                                              size_t n_taps) {
    if (!taps || n_taps == 0) { set_err("null/empty taps"); return nullptr; }
    fsdr_filter* f = create_common(K_FIR_CCF32);
    if (!f) return nullptr;
    f->length = f->fir.n_taps = n_taps;
    f->fir.n_padded = (int)n_taps;
    if (!upload(f->fir.taps, taps, n_taps, "taps upload failed"))
        return create_failed(f);
    return f;
}

extern "C" fsdr_filter* fsdr_fir_f32_create(const float* taps,
                                            size_t n_taps) {
    if (!taps || n_taps == 0) { set_err("null/empty taps"); return nullptr; }
    fsdr_filter* f = create_common(K_FIR_F32);
    if (!f) return nullptr;
    f->length = f->fir.n_taps = n_taps;
    f->fir.n_padded = (int)n_taps;
    f->item_in = f->item_out = 4;
    if (!upload(f->fir.taps, taps, n_taps, "taps upload failed"))
        return create_failed(f);
    return f;
}

extern "C" fsdr_filter* fsdr_decim_fir_cf32_create(size_t decimation,
                                                   const float* taps,
                                                   size_t n_taps) {
    if (!taps || n_taps == 0 || decimation == 0) {
        set_err("invalid decimating FIR parameters");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_DECIM_CF32);
    if (!f) return nullptr;
    f->length = f->fir.n_taps = n_taps;
    f->fir.decim = decimation;
    int mod = (decimation == 4) ? 16 : 1; /* fast path needs tp%16==1 */
    if (upload_taps_padded(f, taps, n_taps, mod) != FSDR_OK)
        return create_failed(f);
    if (decimation == 4 && n_taps <= 512) {
        /* MFMA variant: per-phase K = ceil(T/4)+15 rounded to 4; rows of
         * K. Phase-split template: rows of tpd+4 holding tpd taps. */
        size_t tpd_true = (n_taps + 3) / 4;
        const int kkd = f->fir.kk_mfma =
            tpl_at_least(decim4_mfma_ks{}, tpd_true + 15);
        const int tpd = f->fir.tp_tpl =
            tpl_at_least(decim4_tpl_tpds{}, tpd_true);
        if ((kkd && !upload_phase_split(f->fir.mtaps, taps, n_taps, kkd, kkd,
                                        "decim mfma taps upload failed")) ||
            !upload_phase_split(f->fir.rtaps, taps, n_taps, tpd, tpd + 4,
                                "rtv upload failed"))
            return create_failed(f);
    }
    return f;
}

/* The polyphase handles: argument check (decided before a GPU is needed),
 * then the taps upload. */
static fsdr_filter* resamp_create(FilterKind kind, size_t item_in,
                                  size_t item_out, size_t interp,
                                  size_t decim, const float* taps,
                                  size_t n_taps) {
    if (!taps || n_taps == 0 || interp == 0 || decim == 0 ||
        n_taps % interp != 0) {
        /* polyphase_resampling_fir.rs:54-56 assert */
        set_err("invalid resampler parameters (n_taps % interp must be 0)");
        return nullptr;
    }
    fsdr_filter* f = create_common(kind);
    if (!f) return nullptr;
    f->length = f->fir.n_taps = n_taps;
    f->fir.n_padded = (int)n_taps;
    f->fir.interp = interp;
    f->fir.decim = decim;
    f->item_in = item_in;
    f->item_out = item_out;
    if (!upload(f->fir.taps, taps, n_taps, "taps upload failed"))
        return create_failed(f);
    return f;
}

extern "C" fsdr_filter* fsdr_resamp_cf32_create(size_t interp, size_t decim,
                                                const float* taps,
                                                size_t n_taps) {
    fsdr_filter* f =
        resamp_create(K_RESAMP_CF32, 8, 8, interp, decim, taps, n_taps);
    /* interp==1, decim==4 (the config-3 "4:1" shape): y[k] =
     * sum_t x[4k+t]*h[T-1-t] is the decimating FIR evaluated with its
     * window origin shifted by D-1, so route it to the MFMA decim
     * kernel with the input pointer rebased (launch site). */
    if (f && interp == 1 && decim == 4 && n_taps <= 512)
        f->fir.decim4 = fsdr_decim_fir_cf32_create(4, taps, n_taps);
    return f;
}

extern "C" fsdr_filter* fsdr_resamp_f32_create(size_t interp, size_t decim,
                                               const float* taps,
                                               size_t n_taps) {
    return resamp_create(K_RESAMP_F32, 4, 4, interp, decim, taps, n_taps);
}

extern "C" fsdr_filter* fsdr_quad_demod_create(void) {
    fsdr_filter* f = create_common(K_QUAD_DEMOD);
    if (!f) return nullptr;
    f->item_out = 4;
    f->length = 1; /* an Apply block needs one item */
    if (!alloc_zeroed(f->demod.last, sizeof(float2),
                      "demodulator state alloc failed"))
        return create_failed(f);
    return f;
}

extern "C" fsdr_filter* fsdr_fm_demod_resamp_create(size_t interp,
                                                    size_t decim,
                                                    const float* taps,
                                                    size_t n_taps) {
    fsdr_filter* f =
        resamp_create(K_FM_DEMOD_RESAMP, 8, 4, interp, decim, taps, n_taps);
    if (f && !alloc_zeroed(f->demod.last, sizeof(float2),
                           "demodulator state alloc failed"))
        return create_failed(f);
    return f;
}


extern "C" fsdr_filter* fsdr_fft_cf32_create(size_t len, int inverse,
                                             int fft_shift,
                                             const float* normalize) {
    const bool pow2 = (len & (len - 1)) == 0;
    if (pow2 ? (len < 4 || len > 4096) : (len < 2 || len > 2048)) {
        set_err("fft len: pow2 in [4,4096], or any length in [2,2048] "
                "(Bluestein via 2*len-1-padded pow2 passes)");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_FFT_CF32);
    if (!f) return nullptr;
    f->fft.len = len;
    f->fft.inverse = inverse;
    f->fft.shift = fft_shift;
    f->fft.norm = normalize ? *normalize : 0.f;
    f->length = len; /* min_items = len (fft.rs:106-109) */
    size_t tlen = len;
    if (!pow2) {
        size_t M = 4;
        while (M < 2 * len - 1) M <<= 1;
        f->fft.m = M;
        tlen = M; /* twiddles for the M-point passes */
        /* chirp w(k) = e^{sigma*pi*i*k^2/len}, sigma = -1 fwd / +1 inv;
         * k^2 reduced mod 2*len in integers before the f64 angle */
        const double sg = inverse ? 1.0 : -1.0;
        std::vector<float2> w(len);
        std::vector<double> wr(len), wi(len);
        for (size_t k = 0; k < len; k++) {
            unsigned long long r = (k * k) % (2 * len);
            double a = sg * M_PI * (double)r / (double)len;
            wr[k] = cos(a);
            wi[k] = sin(a);
            w[k] = make_float2((float)wr[k], (float)wi[k]);
        }
        /* V_seq = wrapped conj(w); B = forward DFT_M(V_seq) in f64 */
        std::vector<double> vr(M, 0.0), vi(M, 0.0);
        for (size_t j = 0; j < len; j++) {
            vr[j] = wr[j];
            vi[j] = -wi[j];
            if (j) {
                vr[M - j] = wr[j];
                vi[M - j] = -wi[j];
            }
        }
        std::vector<double> cm(M), sm(M);
        for (size_t k = 0; k < M; k++) {
            double a = -2.0 * M_PI * (double)k / (double)M;
            cm[k] = cos(a);
            sm[k] = sin(a);
        }
        std::vector<float2> B(M);
        for (size_t k = 0; k < M; k++) {
            double sre = 0.0, sim = 0.0;
            for (size_t j2 = 0; j2 < M; j2++) {
                if (vr[j2] == 0.0 && vi[j2] == 0.0) continue;
                size_t idx = (k * j2) % M;
                double c = cm[idx], s = sm[idx];
                sre += vr[j2] * c - vi[j2] * s;
                sim += vr[j2] * s + vi[j2] * c;
            }
            B[k] = make_float2((float)sre, (float)sim);
        }
        if (!upload(f->fft.chirp, w, "bluestein table upload failed") ||
            !upload(f->fft.B, B, "bluestein table upload failed"))
            return create_failed(f);
    }
    /* twiddle table W[k] = e^{-2πik/tlen}, k < tlen, computed in f64
     * (radix-4 needs indices up to 3(tlen/4-1)) */
    std::vector<float2> tw(tlen);
    for (size_t k = 0; k < tlen; k++) {
        double a = -2.0 * M_PI * (double)k / (double)tlen;
        tw[k] = make_float2((float)cos(a), (float)sin(a));
    }
    if (!upload(f->fft.twid, tw, "twiddle upload failed"))
        return create_failed(f);
    return f;
}

extern "C" fsdr_filter* fsdr_mag2_create(void) {
    fsdr_filter* f = create_common(K_MAG2);
    if (!f) return nullptr;
    f->item_out = 4;
    f->length = 1;
    return f;
}

extern "C" fsdr_filter* fsdr_xlating_fir_cf32_create(const float* taps,
                                                     size_t n_taps,
                                                     size_t decimation,
                                                     float offset,
                                                     float sample_rate) {
    /* xlating_fir.rs:44 assert decimation >= 2 */
    if (!taps || n_taps == 0 || decimation < 2) {
        set_err("xlating fir: taps required, decimation must be >= 2");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_XLATING);
    if (!f) return nullptr;
    f->length = f->fir.n_taps = n_taps;
    f->fir.n_padded = (int)n_taps;
    f->fir.decim = decimation;
    /* bpf taps, f32 math identical to from_polar (:79-88), stored
     * REVERSED for the kernel */
    std::vector<float2> bpf(n_taps);
    for (size_t i = 0; i < n_taps; i++) {
        float ang = (float)i * 6.2831853071795864769f * offset / sample_rate;
        float2 rot = make_float2(cosf(ang), sinf(ang));
        size_t src_i = i;
        bpf[n_taps - 1 - src_i] =
            make_float2(rot.x * taps[src_i], rot.y * taps[src_i]);
    }
    if (!upload(f->fir.taps, bpf, "bpf taps upload failed"))
        return create_failed(f);
    /* rotator increment (:91-94) and unit start phase (rotator.rs:17-19) */
    f->xlat.theta = -6.2831853071795864769f * offset * (float)decimation /
                    sample_rate;
    f->xlat.rot_re = 1.0f;
    f->xlat.rot_im = 0.0f;
    return f;
}

extern "C" fsdr_filter* fsdr_pfb_channelizer_create(size_t num_channels,
                                                    const float* taps,
                                                    size_t n_taps,
                                                    float oversample_rate) {
    /* channelizer.rs:94-106 asserts */
    if (num_channels <= 2 || !taps || n_taps < num_channels) {
        set_err("pfb: num_channels > 2 and taps.len() >= num_channels");
        return nullptr;
    }
    /* channelizer.rs:100-104: oversample_rate must be N/i, i in [1,N] */
    if (!(oversample_rate > 0.f) ||
        fmodf((float)num_channels, oversample_rate) != 0.f) {
        set_err("pfb: oversample rate must be N/i for i in [1, N]");
        return nullptr;
    }
    if ((num_channels & (num_channels - 1)) != 0 || num_channels < 4 ||
        num_channels > 4096) {
        set_err("pfb: num_channels must be a power of two in [4,4096] "
                "(FFT kernel constraint)");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_PFB);
    if (!f) return nullptr;
    f->pfb.channels = num_channels;
    /* channelizer.rs:105: decimation_factor = N / oversample_rate */
    f->chan.decim = (size_t)((float)num_channels / oversample_rate);
    size_t tpf = (n_taps + num_channels - 1) / num_channels;
    f->pfb.tpf = tpf;
    f->length = n_taps;
    /* partition_filter_taps (utilities.rs:5-25): part[i][c] = taps[i+c*N],
     * zero-padded */
    std::vector<float> part(num_channels * tpf, 0.f);
    for (size_t i = 0; i < num_channels; i++) {
        size_t cnt = 0;
        for (size_t t = i; t < n_taps; t += num_channels)
            part[i * tpf + cnt++] = taps[t];
    }
    if (!upload(f->chan.taps, part, "pfb taps upload failed") ||
        !(f->pfb.ifft = fsdr_fft_cf32_create(num_channels, 1, 0, nullptr)))
        return create_failed(f);
    return f;
}

/* ---- PFB synthesizer: host-side planning ----------------------------- */

/* One work() call of synthesizer.rs:86-118 in closed form: `pushes`
 * steps consumed so far, n steps of input, out_cap output slots. The
 * first tpf-1 steps only fill the windows; the next (filling) step emits
 * whatever the room (the flag is updated after the step, :115-117);
 * every later step needs MORE than N free slots (:94). The reference
 * indexes out of range when the filling step has fewer than N slots;
 * here the call stops in front of that step instead. */
static void pfb_synth_count(size_t N, size_t tpf, size_t pushes, size_t n,
                            size_t out_cap, size_t* fill_out,
                            size_t* steps_out) {
    size_t fill = pushes < tpf - 1 ? std::min(tpf - 1 - pushes, n) : 0;
    size_t rem = n - fill, steps = 0;
    const size_t room = out_cap > N ? (out_cap - N + N - 1) / N : 0;
    if (rem == 0) {
        steps = 0;
    } else if (pushes + fill == tpf - 1) {
        if (out_cap >= N) {
            steps = 1;
            if (rem > 1 && out_cap > 2 * N)
                steps += std::min(rem - 1, room - 1);
        }
    } else {
        steps = std::min(rem, room);
    }
    *fill_out = fill;
    *steps_out = steps;
}

extern "C" void fsdr_pfb_synthesizer_count(size_t num_channels,
                                           size_t taps_per_filter,
                                           size_t pushes,
                                           size_t n_in_per_chan,
                                           size_t out_cap,
                                           size_t* consumed_per_chan,
                                           size_t* produced) {
    size_t fill = 0, steps = 0;
    if (num_channels && taps_per_filter)
        pfb_synth_count(num_channels, taps_per_filter, pushes,
                        n_in_per_chan, out_cap, &fill, &steps);
    if (consumed_per_chan) *consumed_per_chan = fill + steps;
    if (produced) *produced = steps * num_channels;
}

/* Shape of the fused kernel for (N, tpf): F steps per pass (>= 8 so a
 * channel's read is >= 64 B, more for small N to keep 256 threads in
 * butterflies), G frames per FFT group (F, halved until the LDS fits),
 * R = 32 F steps per block (halo recomputation <= (tpf-1+F)/R), hp the
 * halo rounded up to whole passes. Returns false where the fused path
 * stops: N > 1024, or stage + ring over the 160 KB LDS even at G = 1. */
struct SynthPlan { int F, G, FS, R, hp, threads, NL; size_t lds; };
static bool pfb_synth_plan(size_t N, size_t tpf, SynthPlan* pl) {
    if (N < 4 || N > 1024 || (N & (N - 1)) || tpf == 0) return false;
    size_t F = 2048 / N;
    F = F < 8 ? 8 : (F > 64 ? 64 : F);
    const size_t FS = N + 64 / F;
    const size_t R = 32 * F;
    const size_t hp = (tpf - 1 + F - 1) / F * F;
    if (hp > R) return false;
    size_t G = F;
    while (G > 1 && (F + G + tpf - 1) * FS * 8 > 160 * 1024) G >>= 1;
    const size_t lds = (F + G + tpf - 1) * FS * 8;
    if (lds > 160 * 1024) return false;
    pl->F = (int)F; pl->G = (int)G; pl->FS = (int)FS; pl->R = (int)R;
    pl->hp = (int)hp; pl->lds = lds;
    /* a quarter of a pass's samples, within [256, 1024]: the LDS a block
     * holds grows with F*N, so its thread count has to as well or the CU
     * runs out of waves to hide the loads behind */
    size_t th = F * N / 4;
    th = th < 256 ? 256 : (th > 1024 ? 1024 : th);
    pl->threads = (int)th;
    pl->NL = (int)(F * N / th);
    return true;
}

extern "C" size_t fsdr_pfb_synthesizer_run_length(size_t num_channels,
                                                  size_t taps_per_filter) {
    SynthPlan pl;
    return pfb_synth_plan(num_channels, taps_per_filter, &pl) ? pl.R : 0;
}

extern "C" fsdr_filter* fsdr_pfb_synthesizer_create(size_t num_channels,
                                                    const float* taps,
                                                    size_t n_taps) {
    if (!taps) { set_err("pfb synthesizer: null taps"); return nullptr; }
    if ((num_channels & (num_channels - 1)) != 0 || num_channels < 4 ||
        num_channels > 4096) {
        set_err("pfb synthesizer: num_channels must be a power of two in "
                "[4,4096] (FFT kernel constraint)");
        return nullptr;
    }
    /* utilities.rs:5-25: the zero-pad count underflows otherwise */
    if (n_taps < num_channels) {
        set_err("pfb synthesizer: taps.len() >= num_channels");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_PFB_SYNTH);
    if (!f) return nullptr;
    const size_t N = num_channels;
    const size_t tpf = (n_taps + N - 1) / N;
    f->pfb.channels = N;
    f->pfb.tpf = tpf;
    f->length = n_taps;
    /* partition_filter_taps, transposed: partT[j][c] = taps[c + j*N] */
    std::vector<float> part(N * tpf, 0.f);
    for (size_t t = 0; t < n_taps; t++) part[t] = taps[t];
    if (!upload(f->synth.taps, part, "pfb synthesizer taps upload failed") ||
        !(f->pfb.ifft = fsdr_fft_cf32_create(N, 1, 0, nullptr)))
        return create_failed(f);
    return f;
}

/* ---- PFB arb resampler: host-side schedule --------------------------- */

struct fsdr_pfb_arb_schedule {
    float rate = 0.f, delay = 0.f, nff = 0.f;
    unsigned nf = 0;
    unsigned maxo1 = 0; /* most outputs any one input yields */
    unsigned long long rho = 0, lam = 0, opc = 0;
    std::vector<ArbCk> ck; /* state + cumulative outputs every ARB_Q */
    int RL = 0, W = 0;     /* inputs per lane, lanes per segment */
};

#define ARB_WALK_CAP (1ull << 25)

static inline bool arb_same(const ArbSt& a, const ArbSt& b) {
    return memcmp(&a.tau, &b.tau, 4) == 0 && memcmp(&a.mu, &b.mu, 4) == 0 &&
           a.base == b.base && a.bnd == b.bnd;
}

extern "C" int fsdr_pfb_arb_schedule_create(float rate, size_t num_filters,
                                            fsdr_pfb_arb_schedule** out) {
    if (!out) { set_err("null argument"); return FSDR_ERR_INVALID; }
    *out = nullptr;
    if (!(rate > 0.f)) {
        set_err("PfbArbResampler: resampling rate must be greater than zero");
        return FSDR_ERR_INVALID;
    }
    if (num_filters == 0) {
        set_err("PfbArbResampler: number of filter banks must be greater "
                "than zero");
        return FSDR_ERR_INVALID;
    }
    if (num_filters > (1u << 20) ||
        !((double)num_filters / (double)rate < 1073741824.0)) {
        set_err("pfb arb schedule: num_filters must be at most 2^20 and "
                "num_filters/rate below 2^30");
        return FSDR_ERR_UNSUPPORTED;
    }
    const unsigned nf = (unsigned)num_filters;
    const float delay = 1.0f / rate, nff = (float)num_filters;
    unsigned maxo = 0;
    bool too_many = false;
    auto step = [&](ArbSt& s) {
        const unsigned c = arb_step(s, nf, delay, nff, ARB_CAP, ArbNoEmit());
        if (c > maxo) maxo = c;
        if (c > ARB_CAP) too_many = true;
        return c;
    };
    const char* e_out = "pfb arb schedule: one input yields more than 2048 "
                        "outputs";
    const char* e_long = "pfb arb schedule: preperiod + period exceed 2^25 "
                         "inputs";
    /* Brent: the period lam, then the preperiod rho */
    const ArbSt s0 = {0.f, 0.f, 0u, 0u};
    ArbSt tort = s0, hare = s0;
    step(hare);
    unsigned long long power = 1, lam = 1;
    while (!arb_same(tort, hare)) {
        if (too_many) { set_err(e_out); return FSDR_ERR_UNSUPPORTED; }
        if (power == lam) {
            if (power > ARB_WALK_CAP) {
                set_err(e_long);
                return FSDR_ERR_UNSUPPORTED;
            }
            tort = hare;
            power *= 2;
            lam = 0;
        }
        step(hare);
        lam++;
    }
    if (too_many) { set_err(e_out); return FSDR_ERR_UNSUPPORTED; }
    tort = hare = s0;
    for (unsigned long long i = 0; i < lam; i++) step(hare);
    unsigned long long rho = 0;
    while (!arb_same(tort, hare)) {
        step(tort);
        step(hare);
        if (++rho > ARB_WALK_CAP) {
            set_err(e_long);
            return FSDR_ERR_UNSUPPORTED;
        }
    }
    if (rho + lam > ARB_WALK_CAP) {
        set_err(e_long);
        return FSDR_ERR_UNSUPPORTED;
    }
    fsdr_pfb_arb_schedule* s = new fsdr_pfb_arb_schedule();
    s->rate = rate; s->delay = delay; s->nff = nff; s->nf = nf;
    s->rho = rho; s->lam = lam;
    s->ck.reserve((rho + lam + ARB_Q - 1) / ARB_Q);
    ArbSt st = s0;
    unsigned long long cum = 0, cum_rho = 0;
    for (unsigned long long i = 0; i < rho + lam; i++) {
        if (i % ARB_Q == 0)
            s->ck.push_back({st.tau, st.mu, st.base, st.bnd, cum});
        if (i == rho) cum_rho = cum;
        cum += step(st);
    }
    s->opc = cum - cum_rho;
    s->maxo1 = maxo < 1 ? 1 : maxo;
    /* segment shape: a lane walks RL inputs (8, fewer where one lane's
     * outputs alone would pass ARB_CAP), W lanes per segment so that its
     * outputs fit ARB_CAP whatever the position */
    s->RL = 8;
    if ((unsigned)s->RL * s->maxo1 > ARB_CAP) s->RL = ARB_CAP / s->maxo1;
    s->W = (int)std::min<unsigned>(ARB_BLOCK,
                                   ARB_CAP / ((unsigned)s->RL * s->maxo1));
    *out = s;
    return FSDR_OK;
}

extern "C" void fsdr_pfb_arb_schedule_destroy(fsdr_pfb_arb_schedule* s) {
    delete s;
}

extern "C" int fsdr_pfb_arb_schedule_info(const fsdr_pfb_arb_schedule* s,
                                          uint64_t* preperiod,
                                          uint64_t* period,
                                          uint64_t* outputs_per_period,
                                          size_t* checkpoint_spacing,
                                          size_t* segment_inputs) {
    if (!s) { set_err("null schedule"); return FSDR_ERR_INVALID; }
    if (preperiod) *preperiod = s->rho;
    if (period) *period = s->lam;
    if (outputs_per_period) *outputs_per_period = s->opc;
    if (checkpoint_spacing) *checkpoint_spacing = ARB_Q;
    if (segment_inputs) *segment_inputs = (size_t)s->W * s->RL;
    return FSDR_OK;
}

/* state in front of input `pos` (pushes after the fill) and the outputs
 * of the inputs before it: fold onto the table, then < ARB_Q steps */
static unsigned long long arb_seek(const fsdr_pfb_arb_schedule* s,
                                   unsigned long long pos, ArbSt* st) {
    unsigned long long k = 0, fp = pos;
    if (pos >= s->rho) {
        k = (pos - s->rho) / s->lam;
        fp = s->rho + (pos - s->rho) % s->lam;
    }
    const ArbCk& c = s->ck[fp / ARB_Q];
    st->tau = c.tau; st->mu = c.mu; st->base = c.base; st->bnd = c.bnd;
    unsigned long long cum = c.cum + k * s->opc;
    for (unsigned i = 0; i < fp % ARB_Q; i++)
        cum += arb_step(*st, s->nf, s->delay, s->nff, s->maxo1, ArbNoEmit());
    return cum;
}

extern "C" uint64_t fsdr_pfb_arb_schedule_count(
    const fsdr_pfb_arb_schedule* s, uint64_t pushes_after_fill,
    uint64_t n_inputs) {
    if (!s) return 0;
    ArbSt st;
    return arb_seek(s, pushes_after_fill + n_inputs, &st) -
           arb_seek(s, pushes_after_fill, &st);
}

extern "C" size_t fsdr_pfb_arb_schedule_records(
    const fsdr_pfb_arb_schedule* s, uint64_t first_input, size_t n_inputs,
    uint64_t* in_index, uint32_t* base_index, uint8_t* boundary, float* mu,
    size_t cap) {
    if (!s) return 0;
    ArbSt st;
    arb_seek(s, first_input, &st);
    size_t k = 0;
    for (size_t i = 0; i < n_inputs; i++)
        arb_step(st, s->nf, s->delay, s->nff, s->maxo1,
                 [&](unsigned base, unsigned bnd, float m) {
                     if (k < cap) {
                         if (in_index) in_index[k] = first_input + i;
                         if (base_index) base_index[k] = base;
                         if (boundary) boundary[k] = (uint8_t)bnd;
                         if (mu) mu[k] = m;
                     }
                     k++;
                 });
    return k;
}

/* One resampler call: the fill work() (:202-215), then one processing
 * work() on the rest with n = min(n_in, (usize)(out_cap as f32 / rate))
 * (:218; `as usize` truncates and saturates). Guard: where those n
 * inputs would yield more than out_cap, the largest prefix that fits. */
static void arb_work(const fsdr_pfb_arb_schedule* s, size_t tpf,
                     unsigned long long pushes, size_t n_in, size_t out_cap,
                     size_t* fill_out, size_t* n_out, size_t* prod_out) {
    size_t fill = 0;
    if (pushes < tpf) fill = std::min<unsigned long long>(tpf - pushes, n_in);
    size_t n = 0, prod = 0;
    const size_t rem = n_in - fill;
    if (pushes + fill >= tpf && rem > 0) {
        const float q = (float)out_cap / s->rate;
        size_t lim = 0;
        if (q >= 18446744073709551616.f) lim = SIZE_MAX;
        else if (q > 0.f) lim = (size_t)q;
        n = std::min(rem, lim);
        const unsigned long long P = pushes + fill - tpf;
        prod = fsdr_pfb_arb_schedule_count(s, P, n);
        if (prod > out_cap) {
            size_t lo = 0, hi = n; /* count(lo) fits, count(hi) does not */
            while (hi - lo > 1) {
                const size_t mid = lo + (hi - lo) / 2;
                if (fsdr_pfb_arb_schedule_count(s, P, mid) <= out_cap)
                    lo = mid;
                else
                    hi = mid;
            }
            n = lo;
            prod = fsdr_pfb_arb_schedule_count(s, P, n);
        }
    }
    *fill_out = fill; *n_out = n; *prod_out = prod;
}

extern "C" void fsdr_pfb_arb_schedule_work(const fsdr_pfb_arb_schedule* s,
                                           size_t taps_per_filter,
                                           uint64_t pushes, size_t n_in,
                                           size_t out_cap, size_t* consumed,
                                           size_t* produced) {
    size_t fill = 0, n = 0, prod = 0;
    if (s && taps_per_filter)
        arb_work(s, taps_per_filter, pushes, n_in, out_cap, &fill, &n, &prod);
    if (consumed) *consumed = fill + n;
    if (produced) *produced = prod;
}

extern "C" void fsdr_pfb_arb_startup_map(size_t taps_per_filter,
                                         long long* src) {
    if (!src) return;
    for (size_t s = 0; s < taps_per_filter; s++) src[s] = -1;
    for (size_t k = 0; k < taps_per_filter; k++) {
        const long long slot = arb_fill_slot((long long)taps_per_filter,
                                             (long long)k);
        if (slot >= 0) src[slot] = (long long)k;
    }
}

/* LDS of k_pfb_arb: records, lane offsets, the staged segment, and the
 * taps where they fit beside them */
static size_t pfb_arb_lds(const fsdr_pfb_arb_schedule* s, size_t tpf,
                          bool* taps_lds) {
    const size_t R = (size_t)s->W * s->RL;
    const size_t base = 3 * ARB_CAP * 4 + (ARB_BLOCK + 2) * 8 +
                        (R + tpf + 1) * 8;
    const size_t tb = (size_t)s->nf * tpf * 4;
    *taps_lds = tb <= 16 * 1024 && base + tb <= 64 * 1024;
    return base + (*taps_lds ? tb : 0);
}

extern "C" fsdr_filter* fsdr_pfb_arb_resampler_create(float rate,
                                                      const float* taps,
                                                      size_t n_taps,
                                                      size_t num_filters,
                                                      size_t num_channels) {
    /* arb_resampler.rs:92-103 */
    if (!(rate > 0.f)) {
        set_err("PfbArbResampler: resampling rate must be greater than zero");
        return nullptr;
    }
    if (!taps || n_taps < num_filters) {
        set_err("PfbArbResampler: prototype filter length must be at least "
                "num_filters");
        return nullptr;
    }
    if (num_filters == 0) {
        set_err("PfbArbResampler: number of filter banks must be greater "
                "than zero");
        return nullptr;
    }
    if (num_channels == 0 || num_channels > 65536) {
        set_err("pfb arb resampler: num_channels must be in [1,65536]");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_PFB_ARB);
    if (!f) return nullptr;
    if (fsdr_pfb_arb_schedule_create(rate, num_filters, &f->arb.sched) !=
        FSDR_OK)
        return create_failed(f);
    const fsdr_pfb_arb_schedule* s = f->arb.sched;
    const size_t nf = num_filters, tpf = (n_taps + nf - 1) / nf;
    bool taps_lds;
    if ((size_t)s->W * s->RL + tpf + 1 > ARB_NV * ARB_BLOCK ||
        pfb_arb_lds(s, tpf, &taps_lds) > 64 * 1024) {
        set_err("pfb arb resampler: taps per filter too long for the LDS "
                "tile");
        return create_failed(f);
    }
    f->pfb.channels = num_channels;
    f->pfb.tpf = tpf;
    f->length = n_taps;
    /* partition_filter_taps (utilities.rs:5-25), each part reversed */
    std::vector<float> rp(nf * tpf, 0.f);
    for (size_t t = 0; t < n_taps; t++)
        rp[(t % nf) * tpf + (tpf - 1 - t / nf)] = taps[t];
    const char* err = "pfb arb resampler upload failed";
    if (!upload(f->arb.taps, rp, err) || !upload(f->arb.ck, s->ck, err) ||
        !alloc_zeroed(f->arb.window.buf, 2 * num_channels * tpf * 8, err))
        return create_failed(f);
    return f;
}

extern "C" const fsdr_pfb_arb_schedule* fsdr_pfb_arb_resampler_schedule(
    const fsdr_filter* f) {
    return f && f->kind == K_PFB_ARB ? f->arb.sched : nullptr;
}

/* ---- IIR plan: the constant matrices of the blocked recurrence -------- */

struct fsdr_iir_plan {
    int na = 0;
    std::vector<float> a;
    /* H[i][q] = (A^(i+1))[0][q], i < IIR_L; pc[d] = A^(IIR_L*2^d) and
     * pt[d] = A^(IIR_TILE*2^d), d < IIR_P_LEVELS, row-major na x na; all
     * formed in double (Hd, pcd, ptd: what _tables copies out) and rounded
     * to f32 once (what the kernels read) */
    std::vector<double> Hd, pcd, ptd;
    std::vector<float> H, pc, pt;
};

extern "C" int fsdr_iir_plan_create(const float* a, size_t n_a,
                                    fsdr_iir_plan** out) {
    if (!out) { set_err("null argument"); return FSDR_ERR_INVALID; }
    *out = nullptr;
    if (n_a > IIR_NA_MAX || (n_a && !a)) {
        set_err("iir: n_a must be in [0,8]");
        return FSDR_ERR_INVALID;
    }
    const int na = (int)n_a;
    typedef std::vector<double> Mat;
    auto mul = [na](const Mat& x, const Mat& y) {
        Mat z((size_t)na * na, 0.0);
        for (int i = 0; i < na; i++)
            for (int k = 0; k < na; k++)
                for (int j = 0; j < na; j++)
                    z[i * na + j] += x[i * na + k] * y[k * na + j];
        return z;
    };
    fsdr_iir_plan* p = new fsdr_iir_plan();
    p->na = na;
    p->a.assign(a, a + n_a);
    bool finite = true;
    auto put = [&finite](std::vector<double>& dd, std::vector<float>& df,
                         const double* v, size_t n) {
        for (size_t i = 0; i < n; i++) {
            const float f = (float)v[i];
            if (!std::isfinite(f)) finite = false;
            dd.push_back(v[i]);
            df.push_back(f);
        }
    };
    Mat A((size_t)na * na, 0.0);
    for (int q = 0; q < na; q++) {
        A[q] = (double)a[q];
        if (q) A[q * na + q - 1] = 1.0;
    }
    Mat M = A;
    for (int i = 0; i < IIR_L; i++) { /* M = A^(i+1) */
        put(p->Hd, p->H, M.data(), na);
        if (i + 1 < IIR_L) M = mul(M, A);
    }
    for (int d = 0; d < IIR_LEVELS + IIR_P_LEVELS; d++) {
        /* M = A^(IIR_L*2^d); IIR_L * 2^IIR_LEVELS is the tile */
        const bool chunk = d < IIR_LEVELS;
        put(chunk ? p->pcd : p->ptd, chunk ? p->pc : p->pt, M.data(),
            (size_t)na * na);
        M = mul(M, M);
    }
    if (!finite) {
        delete p;
        set_err("iir: a table entry is not finite in f32 (a pole outside "
                "the unit circle)");
        return FSDR_ERR_UNSUPPORTED;
    }
    *out = p;
    return FSDR_OK;
}

extern "C" void fsdr_iir_plan_destroy(fsdr_iir_plan* p) { delete p; }

extern "C" int fsdr_iir_plan_info(const fsdr_iir_plan* p, size_t* chunk_len,
                                  size_t* chunks_per_tile, size_t* tile,
                                  size_t* scan_pass_tiles) {
    if (!p) { set_err("null plan"); return FSDR_ERR_INVALID; }
    if (chunk_len) *chunk_len = IIR_L;
    if (chunks_per_tile) *chunks_per_tile = IIR_C;
    if (tile) *tile = IIR_TILE;
    if (scan_pass_tiles) *scan_pass_tiles = IIR_P;
    return FSDR_OK;
}

extern "C" int fsdr_iir_plan_tables(const fsdr_iir_plan* p, double* H,
                                    double* chunk_pow, double* tile_pow) {
    if (!p) { set_err("null plan"); return FSDR_ERR_INVALID; }
    if (H) std::copy(p->Hd.begin(), p->Hd.end(), H);
    if (chunk_pow) std::copy(p->pcd.begin(), p->pcd.end(), chunk_pow);
    if (tile_pow) std::copy(p->ptd.begin(), p->ptd.end(), tile_pow);
    return FSDR_OK;
}

/* iir.rs:90-129,136,166-177: the fill, the counts and the status of one
 * call by a filter whose memory holds `filled` samples. */
extern "C" void fsdr_iir_count(size_t n_a, size_t n_b, size_t filled,
                               size_t n_in, size_t n_out,
                               size_t* filled_after, size_t* consumed,
                               size_t* produced, int* status) {
    const int idle = n_out == 0 ? FSDR_BOTH_SUFFICIENT
                                : FSDR_INSUFFICIENT_INPUT;
    size_t m = filled, pushes = 0, n = 0;
    int st = idle;
    bool run = n_in != 0;
    while (run && m < n_a) {
        if (n_in <= m) { run = false; break; }
        m++;
        pushes++;
    }
    if (run && pushes == n_in) run = false;
    if (run) {
        n = n_in >= n_b ? std::min(n_in - (n_b - 1), n_out) : 0;
        st = n == n_in && n == n_out ? FSDR_BOTH_SUFFICIENT
             : n < n_in              ? FSDR_INSUFFICIENT_OUTPUT
                                     : FSDR_INSUFFICIENT_INPUT;
    }
    if (filled_after) *filled_after = n_in ? m : filled;
    if (consumed) *consumed = n;
    if (produced) *produced = n;
    if (status) *status = st;
}

extern "C" fsdr_filter* fsdr_iir_f32_create(const float* a, size_t n_a,
                                            const float* b, size_t n_b) {
    if (!b || n_b == 0 || n_b > IIR_NB_MAX) {
        /* n_b == 0: iir.rs:132 assert */
        set_err("iir: n_b must be in [1,64]");
        return nullptr;
    }
    fsdr_iir_plan* plan = nullptr;
    if (fsdr_iir_plan_create(a, n_a, &plan) != FSDR_OK) return nullptr;
    fsdr_filter* f = create_common(K_IIR_F32);
    if (!f) { delete plan; return nullptr; }
    f->iir.plan = plan;
    f->length = f->iir.n_b = n_b;
    f->item_in = f->item_out = 4;
    std::vector<float> tb(plan->H);
    tb.insert(tb.end(), plan->pc.begin(), plan->pc.end());
    tb.insert(tb.end(), plan->pt.begin(), plan->pt.end());
    tb.push_back(0.f); /* no feedback: the tables are empty */
    const char* err = "iir upload failed";
    if (!upload(f->iir.b, b, n_b, err) || !upload(f->iir.tables, tb, err) ||
        !alloc_zeroed(f->iir.mem.buf, 2 * IIR_NA_MAX * sizeof(float), err))
        return create_failed(f);
    return f;
}

extern "C" const fsdr_iir_plan* fsdr_iir_plan_of(const fsdr_filter* f) {
    return f && f->kind == K_IIR_F32 ? f->iir.plan : nullptr;
}

/* ---- LoRa FFT demodulator: tables, counts, handle --------------------- */

/* conj(build_upchirp(0, sf, 1, preamble)) rotated by the frame's cfo and
 * rounded to f32. The chirp is utils.rs:884-914 in f32 and in its
 * operation order (the phase reaches ~1.3e4 rad at sf 12, so its f32
 * rounding is part of the definition): id = my_modulo(0 - 1, N) = N - 1
 * and n_fold = 1 for the demodulator's table (preamble false), id = 0 and
 * n_fold = N for build_ref_chirps' (preamble true). Conjugate
 * (fft_demod.rs:280-283) and rotation e^{-2 pi i (cfo_int + cfo_frac)/N * j}
 * (:384-398) are in f64. */
static void lora_downchirp_table(unsigned sf, bool preamble,
                                 long long cfo_int, double cfo_frac,
                                 fsdr_cf32* out) {
#pragma clang fp contract(off)
    const size_t n = (size_t)1 << sf;
    const size_t id = preamble ? 0 : n - 1;
    const size_t n_fold = n - id;
    const float nf = (float)n;
    const float pi = 3.14159265358979323846f;
    for (size_t j = 0; j < n; j++) {
        const float t = (float)j / 1.0f;
        const float off = j < n_fold ? 0.5f : 1.5f;
        const float ph =
            2.0f * pi * (t * t / (2.f * nf) + ((float)id / nf - off) * t);
        const double xr = (double)cosf(ph), xi = -(double)sinf(ph);
        const double th = -2.0 * M_PI * ((double)cfo_int + cfo_frac) /
                          (double)n * (double)j;
        const double pr = cos(th), pi_ = sin(th);
        out[j].re = (float)(xr * pr - xi * pi_);
        out[j].im = (float)(xr * pi_ + xi * pr);
    }
}

static bool lora_sf_ok(unsigned sf) { return sf >= 5 && sf <= LORA_MAX_SF; }

extern "C" int fsdr_lora_downchirp(unsigned sf, long long cfo_int,
                                   double cfo_frac, fsdr_cf32* out) {
    if (!lora_sf_ok(sf) || !out) {
        set_err("lora: sf must be in [5,12]");
        return FSDR_ERR_INVALID;
    }
    lora_downchirp_table(sf, false, cfo_int, cfo_frac, out);
    return FSDR_OK;
}

extern "C" double fsdr_lora_log_i0(double x) { return lora_log_i0(x); }

extern "C" int fsdr_lora_demod_count(unsigned sf, size_t n_in, size_t n_out,
                                     size_t* consumed, size_t* produced,
                                     int* status) {
    if (!lora_sf_ok(sf)) {
        set_err("lora: sf must be in [5,12]");
        return FSDR_ERR_INVALID;
    }
    const fsdr_filter_result r =
        decim_status((size_t)1 << sf, n_in, 1, n_out);
    if (consumed) *consumed = r.consumed;
    if (produced) *produced = r.produced;
    if (status) *status = (int)r.status;
    return FSDR_OK;
}

static int lora_upload_chirp(fsdr_filter* f, long long cfo_int,
                             double cfo_frac) {
    std::vector<fsdr_cf32> t((size_t)1 << f->lora.sf);
    lora_downchirp_table(f->lora.sf, f->lora.mode == LORA_RAW, cfo_int,
                         cfo_frac, t.data());
    HIP_TRY(hipMemcpy(f->lora.chirp.ptr, t.data(),
                      t.size() * sizeof(fsdr_cf32), hipMemcpyHostToDevice));
    return FSDR_OK;
}

extern "C" fsdr_filter* fsdr_lora_demod_create(unsigned sf, int mode) {
    if (!lora_sf_ok(sf)) {
        set_err("lora: sf must be in [5,12]");
        return nullptr;
    }
    if (mode != LORA_RAW && mode != LORA_HARD && mode != LORA_SOFT) {
        set_err("lora: mode must be FSDR_LORA_RAW, _HARD or _SOFT");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_LORA_DEMOD);
    if (!f) return nullptr;
    const size_t n = (size_t)1 << sf;
    f->lora.sf = sf;
    f->lora.mode = mode;
    f->length = n; /* set_min_items(N), fft_demod.rs:269 */
    f->item_out = mode == LORA_SOFT ? LORA_MAX_SF * sizeof(double) : 2;
    std::vector<float2> tw(n);
    for (size_t k = 0; k < n; k++) {
        const double a = -2.0 * M_PI * (double)k / (double)n;
        tw[k] = make_float2((float)cos(a), (float)sin(a));
    }
    const char* err = "lora table upload failed";
    if (!upload(f->lora.twid, tw, err) ||
        f->lora.chirp.ensure(n * sizeof(float2)) != hipSuccess ||
        lora_upload_chirp(f, 0, 0.0) != FSDR_OK) {
        set_err(err);
        return create_failed(f);
    }
    return f;
}

extern "C" int fsdr_lora_demod_set_frame(fsdr_filter* f, long long cfo_int,
                                         double cfo_frac, int reduced_rate) {
    REQUIRE_GPU();
    if (!f || f->kind != K_LORA_DEMOD) {
        set_err("not a lora demodulator");
        return FSDR_ERR_INVALID;
    }
    f->lora.reduced = reduced_rate != 0;
    return lora_upload_chirp(f, cfo_int, cfo_frac);
}

extern "C" fsdr_filter* fsdr_moving_avg_create(size_t width,
                                               float decay_factor,
                                               size_t history) {
    if (width == 0 || history == 0 || !(decay_factor >= 0.f) ||
        decay_factor > 1.f) {
        /* moving_avg.rs:59-62 assert */
        set_err("decay_factor must be in [0,1], width/history > 0");
        return nullptr;
    }
    fsdr_filter* f = create_common(K_MOVAVG);
    if (!f) return nullptr;
    f->movavg.width = width;
    f->movavg.history = history;
    f->movavg.decay = decay_factor;
    f->item_in = f->item_out = 4;
    f->length = width; /* min_items analogue */
    if (!alloc_zeroed(f->movavg.avg, width * sizeof(float),
                      "avg state alloc failed"))
        return create_failed(f);
    return f;
}

extern "C" size_t fsdr_filter_length(const fsdr_filter* f) {
    return f ? f->length : 0;
}

/* Which kernel instantiation the handle's launches select (the
 * precomputed template parameters; 0 = that family does not apply). A
 * resampler reports its 1:4 sub-filter, or zeros without one. */
extern "C" int fsdr_filter_variant(const fsdr_filter* f, int* kk_mfma,
                                   int* kk_mfma32, int* tp_tpl) {
    if (!f) { set_err("null filter"); return FSDR_ERR_INVALID; }
    if (f->kind == K_RESAMP_CF32 && f->fir.decim4) f = f->fir.decim4;
    if (kk_mfma) *kk_mfma = f->fir.kk_mfma;
    if (kk_mfma32) *kk_mfma32 = f->fir.kk_mfma32;
    if (tp_tpl) *tp_tpl = f->fir.tp_tpl;
    return FSDR_OK;
}

/* item sizes for the flowgraph driver (fsdr_fg.cpp) */
extern "C" size_t fsdr_filter_item_sizes(const fsdr_filter* f,
                                         size_t* out_bytes) {
    if (!f) { if (out_bytes) *out_bytes = 8; return 8; }
    if (out_bytes) *out_bytes = f->item_out;
    return f->item_in;
}

fsdr_filter::~fsdr_filter() {
    delete fir.decim4;
    delete pfb.ifft;
    delete arb.sched;
    delete iir.plan;
}

extern "C" void fsdr_filter_destroy(fsdr_filter* f) {
    if (f) delete f;
}

/* ---- kernel launch helpers ---- */

static int grid_for(long long work_items, int block) {
    long long g = (work_items + block - 1) / block;
    const long long cap = 256 * 32; /* 256 CUs, grid-stride beyond */
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

/* Block cap of a persistent-tile launch: `dflt` unless FSDR_FIR_GRID_CAP
 * parses to a value >= 1 (tests force several tiles per block with it; a
 * value below 1 is ignored, so it cannot launch an empty grid). */
static long long grid_cap(long long dflt) {
    if (const char* e = getenv("FSDR_FIR_GRID_CAP")) {
        long long v = atoll(e);
        if (v >= 1) return v;
    }
    return dflt;
}

/* Frame horizon of the MovingAvg EMA: the smallest H with |om|^H < 2^-160,
 * om = 1 - decay as the kernels form it (in float). A chunk that ends k
 * frames before the emission is weighted by powf(om, k) in
 * k_moving_avg_combine. 2^-160 is 2^10 times below half the smallest fp32
 * denormal (2^-150), so for every k >= H the exact power rounds to zero
 * with a margin no last-ulp error of powf (nor the float rounding of k
 * above 2^24) comes near: the device weight is exactly +-0.0f. The chunk
 * partials are finite (decay is held to [0,1] at create, so they are
 * convex combinations of finite inputs, non-finite ones being filtered),
 * so such a term is +-0 and adding it changes no
 * bit of the sum: skipping it is exact, not approximate. Returns 0 when
 * there is no horizon (|om| >= 1, or decay not a number). */
static long long movavg_horizon(float decay) {
    const double om = fabs((double)(1.0f - decay));
    if (om == 0.0) return 1;
    if (!(om < 1.0)) return 0;
    const double h = ceil(160.0 * M_LN2 / -log(om));
    if (!(h < 9.0e18)) return 0;
    return h < 1.0 ? 1 : (long long)h;
}

/* MovingAvg frame accounting, equal to running
 *   while (cons < in_frames && prod < out_frames) {
 *       if (++i == history) { i = 0; prod++; }
 *       cons++;
 *   }
 * from cons = prod = 0 and 0 <= *i < history: the first emission comes
 * after history - i frames, then one every history frames, and the loop
 * stops on the frame of the out_frames-th emission. */
static void movavg_count(size_t in_frames, size_t out_frames, size_t history,
                         size_t* cons, size_t* prod, size_t* i) {
    *cons = *prod = 0;
    if (out_frames == 0 || in_frames == 0) return;
    const size_t first = history - *i;
    size_t need = SIZE_MAX; /* frames up to the last emission, saturated */
    if (out_frames - 1 <= (SIZE_MAX - first) / history)
        need = first + (out_frames - 1) * history;
    const size_t c = in_frames < need ? in_frames : need;
    *cons = c;
    if (c < first) {
        *i += c;
    } else {
        *prod = 1 + (c - first) / history;
        *i = (c - first) % history;
    }
}

/* Chunking of the MovingAvg single-emission fast path over `frames` (> 0)
 * frames, and the first chunk that can still weigh in: chunk c ends at
 * min((c+1)*cf, frames) and counts iff frames - end_c < H, i.e.
 * (c+1)*cf > frames - H. The last chunk ends at frames, so the result is
 * at most nch-1. */
static int movavg_plan(size_t frames, float decay, bool skip, int* cf_out,
                       int* nch_out) {
    int cf = 64; /* measured best (16 and 256 both slower) */
    int nch = (int)((frames + cf - 1) / cf);
    if (nch > 1024) { nch = 1024; cf = (int)((frames + nch - 1) / nch); }
    *cf_out = cf;
    *nch_out = nch;
    int c0 = 0;
    const long long H = movavg_horizon(decay);
    if (skip && H > 0 && (long long)frames > H) {
        c0 = (int)(((long long)frames - H) / cf);
        if (c0 > nch - 1) c0 = nch - 1;
    }
    return c0;
}

extern "C" void fsdr_moving_avg_count(size_t in_frames, size_t out_frames,
                                      size_t history, size_t* i_state,
                                      size_t* consumed, size_t* produced) {
    movavg_count(in_frames, out_frames, history, consumed, produced,
                 i_state);
}

extern "C" int fsdr_moving_avg_plan(size_t frames, float decay_factor,
                                    int skip, int* chunk_frames,
                                    int* n_chunks) {
    return movavg_plan(frames, decay_factor, skip != 0, chunk_frames,
                       n_chunks);
}

static int launch_fir_cf32(fsdr_filter* f, const void* d_in, void* d_out,
                           size_t n_out, size_t n_in, hipStream_t st) {
    if (n_out == 0) return FSDR_OK;
    long long tiles = ((long long)n_out + FIR_TILE_OUT - 1) / FIR_TILE_OUT;
    /* one tile per block by default: independent blocks overlap their
     * staging latency with other blocks' compute (a per-block tile loop
     * stalls all 4 waves of the block at each staging barrier) */
    long long cap = grid_cap(256 * 16);
    int grid = (int)std::min<long long>(tiles, cap);
    if (f->fir.kk_mfma && env_int("FSDR_FIR_MFMA32", 0) != 0) {
        /* 32x32 variant reuses d_mtaps when kk32 <= allocated; host
         * uploads a separate array sized for K = T+31 */
        long long tiles32 =
            ((long long)n_out + MFIR32_TILE - 1) / MFIR32_TILE;
        long long cap32 = grid_cap(256 * 64);
        int grid32 = (int)std::min<long long>(tiles32, cap32);
        unsigned elems32 = MFIR32_TILE + f->fir.kk_mfma32 + 8;
        size_t lds32 = (2 * (size_t)((elems32 + 31u) & ~31u) +
                        f->fir.kk_mfma32 + 36) * sizeof(float);
        if (!tpl_dispatch(fir_mfma32_ks{}, f->fir.kk_mfma32, [&](auto K) {
                hipLaunchKernelGGL(
                    HIP_KERNEL_NAME(k_fir_mfma32_tpl<decltype(K)::value>),
                    dim3(grid32), dim3(MFIR32_BLOCK), lds32, st,
                    (const float2*)d_in, (float2*)d_out,
                    f->fir.mtaps32.as<float>(), (long long)n_out,
                    (long long)n_in);
            })) {
            set_err("bad mfma32 K");
            return FSDR_ERR_INVALID;
        }
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    if (f->fir.kk_mfma && env_on("FSDR_FIR_MFMA")) {
        unsigned elems = MFIR_TILE + f->fir.kk_mfma + 8;
        size_t lds = (2 * (size_t)((elems + 31u) & ~31u) + f->fir.kk_mfma + 20)
                     * sizeof(float);
        if (!tpl_dispatch(fir_mfma_ks{}, f->fir.kk_mfma, [&](auto K) {
                hipLaunchKernelGGL(
                    HIP_KERNEL_NAME(k_fir_mfma_tpl<decltype(K)::value>),
                    dim3(grid), dim3(MFIR_BLOCK), lds, st,
                    (const float2*)d_in, (float2*)d_out,
                    f->fir.mtaps.as<float>(), (long long)n_out,
                    (long long)n_in);
            })) {
            set_err("bad mfma K");
            return FSDR_ERR_INVALID;
        }
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    if (f->fir.tp_tpl) {
        unsigned elems = FIR_TILE_OUT + f->fir.tp_tpl + 8;
        size_t lds = (2 * (size_t)((elems + 7u) & ~7u) + f->fir.tp_tpl + 3) *
                     sizeof(float);
        if (!tpl_dispatch(fir_tpl_tps{}, f->fir.tp_tpl, [&](auto TP) {
                hipLaunchKernelGGL(
                    HIP_KERNEL_NAME(k_fir_cf32_tpl<decltype(TP)::value>),
                    dim3(grid), dim3(FIR_BLOCK), lds, st,
                    (const float2*)d_in, (float2*)d_out,
                    f->fir.rtaps.as<float>(), (long long)n_out,
                    (long long)n_in);
            })) {
            set_err("bad template tap count");
            return FSDR_ERR_INVALID;
        }
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    unsigned elems = FIR_TILE_OUT + f->fir.n_padded - 1 + 6;
    size_t lds = (2 * (size_t)plane_floats(elems) + f->fir.n_padded + 4) *
                 sizeof(float);
    hipLaunchKernelGGL(k_fir_cf32, dim3(grid), dim3(FIR_BLOCK), lds, st,
                       (const float2*)d_in, (float2*)d_out,
                       f->fir.taps.as<float>(), f->fir.n_padded,
                       (long long)n_out, (long long)n_in);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int run_fir_cf32(fsdr_filter* f, const void* d_in, size_t n_in,
                        void* d_out, size_t n_out, void* stream,
                        fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    *r = fir_status(n_in, f->fir.n_taps, n_out);
    return launch_fir_cf32(f, d_in, d_out, r->produced, n_in, st);
}

static int launch_decim_cf32(fsdr_filter* f, const void* d_in, void* d_out,
                             size_t n_out, size_t n_in, hipStream_t st) {
    if (n_out == 0) return FSDR_OK;
    if (f->fir.decim == 4 && f->fir.kk_mfma && env_on("FSDR_DECIM_MFMA")) {
        long long tiles = ((long long)n_out + MDFIR_TILE - 1) / MDFIR_TILE;
        long long cap = grid_cap(256 * 64);
        int grid = (int)std::min<long long>(tiles, cap);
        if (!tpl_dispatch(decim4_mfma_ks{}, f->fir.kk_mfma, [&](auto K) {
                using G = ChainGeom<decltype(K)::value>;
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_decim4_mfma_tpl<G::KKD>),
                                   dim3(grid), dim3(G::BLOCK),
                                   G::halves_bytes, st, (const float2*)d_in,
                                   (float2*)d_out, f->fir.mtaps.as<float>(),
                                   (long long)n_out, (long long)n_in);
            })) {
            set_err("bad decim mfma K");
            return FSDR_ERR_INVALID;
        }
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    if (f->fir.decim == 4 && f->fir.tp_tpl) {
        long long tiles = ((long long)n_out + DFIRT_TILE - 1) / DFIRT_TILE;
        long long cap = grid_cap(256 * 64);
        int grid = (int)std::min<long long>(tiles, cap);
        size_t lds = (4 * (size_t)dfirt_sp(f->fir.tp_tpl) +
                      4 * ((size_t)f->fir.tp_tpl + 4)) * sizeof(float);
        if (!tpl_dispatch(decim4_tpl_tpds{}, f->fir.tp_tpl, [&](auto TPD) {
                hipLaunchKernelGGL(
                    HIP_KERNEL_NAME(k_fir_decim4_tpl<decltype(TPD)::value>),
                    dim3(grid), dim3(DFIRT_BLOCK), lds, st,
                    (const float2*)d_in, (float2*)d_out,
                    f->fir.rtaps.as<float>(), (long long)n_out,
                    (long long)n_in);
            })) {
            set_err("bad decim template tap count");
            return FSDR_ERR_INVALID;
        }
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    if (f->fir.decim == 4) {
        unsigned elems = DFIR_TILE_OUT * 4 + f->fir.n_padded - 1 + 20;
        size_t lds = (2 * (size_t)plane_floats(elems) + f->fir.n_padded + 4)
                     * sizeof(float);
        long long tiles =
            ((long long)n_out + DFIR_TILE_OUT - 1) / DFIR_TILE_OUT;
        int grid = (int)std::min<long long>(tiles, grid_cap(256 * 8));
        hipLaunchKernelGGL(k_fir_decim4_cf32, dim3(grid), dim3(DFIR_BLOCK),
                           lds, st, (const float2*)d_in, (float2*)d_out,
                           f->fir.taps.as<float>(), f->fir.n_padded,
                           (long long)n_out, (long long)n_in);
    } else {
        hipLaunchKernelGGL(k_fir_decim_generic_cf32,
                           dim3(grid_for((long long)n_out, 256)), dim3(256),
                           0, st, (const float2*)d_in, (float2*)d_out,
                           f->fir.taps.as<float>(),
                           f->fir.n_padded, /* == n_taps for generic */
                           (long long)f->fir.decim, (long long)n_out,
                           (long long)n_in);
    }
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int run_decim_cf32(fsdr_filter* f, const void* d_in, size_t n_in,
                          void* d_out, size_t n_out, void* stream,
                          fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    *r = decim_status(f->fir.decim, n_in, f->fir.n_taps, n_out);
    return launch_decim_cf32(f, d_in, d_out, r->produced, n_in, st);
}

static int launch_stockham(const float2* d_in, float2* d_out,
                           float* d_mag, const float2* d_twid, int n,
                           size_t frames, int inverse, int fft_shift,
                           float norm, hipStream_t st) {
    int log2n = 0;
    while ((1 << log2n) < n) log2n++;
    int fpb = env_int("FSDR_FFT_FPB_BASE", 1024) / n;
    if (fpb < 1) fpb = 1;
    if (fpb > 16) fpb = 16;
    size_t lds = 2 * (size_t)fpb * n * sizeof(float2);
    long long blocks = ((long long)frames + fpb - 1) / fpb;
    int grid = (int)std::min<long long>(blocks, grid_cap(256 * 16));
    hipLaunchKernelGGL(k_fft_stockham, dim3(grid), dim3(256), lds, st,
                       d_in, d_out, d_mag, d_twid, n, log2n, fpb, inverse,
                       fft_shift, norm, (long long)frames);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int launch_fft(fsdr_filter* f, const void* d_in, void* d_out,
                      size_t frames, hipStream_t st,
                      float* d_mag = nullptr) {
    if (frames == 0) return FSDR_OK;
    int n = (int)f->fft.len;
    if (f->fft.m) { /* Bluestein: pre -> FFT_M -> *B -> IFFT_M -> post */
        int M = (int)f->fft.m;
        HIP_TRY(f->fft.work.ensure(2 * frames * (size_t)M * sizeof(float2)));
        float2* s1 = f->fft.work.as<float2>();
        float2* s2 = s1 + frames * (size_t)M;
        const float2* twid = f->fft.twid.as<float2>();
        long long tM = (long long)frames * M;
        hipLaunchKernelGGL(k_bluestein_pre, dim3(grid_for(tM, 256)),
                           dim3(256), 0, st, (const float2*)d_in, s1,
                           f->fft.chirp.as<float2>(), n, M, (long long)frames,
                           f->fft.inverse && f->fft.shift);
        HIP_TRY(hipGetLastError());
        int rc =
            launch_stockham(s1, s2, nullptr, twid, M, frames, 0, 0, 0.f, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bluestein_mul, dim3(grid_for(tM, 256)),
                           dim3(256), 0, st, s2, f->fft.B.as<float2>(), M,
                           (long long)frames);
        HIP_TRY(hipGetLastError());
        rc = launch_stockham(s2, s1, nullptr, twid, M, frames, 1, 0, 0.f, st);
        if (rc) return rc;
        float scale =
            (1.0f / (float)M) * (f->fft.norm != 0.f ? f->fft.norm : 1.f);
        hipLaunchKernelGGL(k_bluestein_post,
                           dim3(grid_for((long long)frames * n, 256)),
                           dim3(256), 0, st, s1, (float2*)d_out, d_mag,
                           f->fft.chirp.as<float2>(), n, M, (long long)frames,
                           (!f->fft.inverse) && f->fft.shift, scale);
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    return launch_stockham((const float2*)d_in, (float2*)d_out, d_mag,
                           f->fft.twid.as<float2>(), n, frames,
                           f->fft.inverse, f->fft.shift, f->fft.norm, st);
}

static int run_fft(fsdr_filter* f, const void* d_in, size_t n_in,
                   void* d_out, size_t n_out, void* stream,
                   fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    /* fft.rs:169-171 */
    size_t m = n_in < n_out ? n_in : n_out;
    m = (m / f->fft.len) * f->fft.len;
    size_t cap = f->fft.len * 32;
    if (m > cap) m = cap;
    r->consumed = r->produced = m;
    r->status = FSDR_BOTH_SUFFICIENT;
    return launch_fft(f, d_in, d_out, m / f->fft.len, st);
}

/* Bulk batch FFT: the GPU-native many-frames path (what the chain uses
 * internally). The 32-frames-per-work cap in fsdr_filter_dev mirrors the
 * reference block's work() quantum (fft.rs:56); a batch resident in HBM
 * has no reason to launch 512 times. d_mag optional fused |X|^2. */
extern "C" int fsdr_fft_bulk_dev(fsdr_filter* f, const void* d_in,
                                 void* d_out, void* d_mag, size_t frames,
                                 void* stream) {
    REQUIRE_GPU();
    if (!f || f->kind != K_FFT_CF32) {
        set_err("fft_bulk: not an fft filter");
        return FSDR_ERR_INVALID;
    }
    return launch_fft(f, d_in, d_out, frames, (hipStream_t)stream,
                      (float*)d_mag);
}

/* ---- f32 resampler / FM back end: launches --------------------------- */

/* Input span of one RS_TILE-output tile, and whether one padded f32 plane
 * of it plus the taps fits the 64 KiB the tiled kernels ask for. */
static bool resamp_f32_tile(const fsdr_filter* f, int* span, size_t* lds) {
    const size_t nt = f->fir.n_taps, L = f->fir.interp, D = f->fir.decim;
    const size_t tpp = nt / L;
    const size_t s = (size_t)(RS_TILE - 1) * D / L + tpp + 2;
    if (s > (1u << 20) || nt > (1u << 20) || D > (1u << 21))
        return false; /* also keeps the kernels' 32-bit tile indices exact */
    *span = (int)s;
    *lds = ((size_t)plane_floats((unsigned)s) + nt) * sizeof(float);
    return *lds <= 64 * 1024;
}

static int launch_resamp_f32(const fsdr_filter* f, const float* d_in,
                             float* d_out, size_t produced, size_t n_in,
                             hipStream_t st) {
    if (produced == 0) return FSDR_OK;
    int span = 0;
    size_t lds_t = 0;
    if (resamp_f32_tile(f, &span, &lds_t) && env_on("FSDR_RESAMP_TILED")) {
        long long tiles = ((long long)produced + RS_TILE - 1) / RS_TILE;
        int grid = (int)std::min<long long>(tiles, grid_cap(256 * 64));
        auto kern = f->fir.decim % 2 ? k_resamp_tiled_f32<false>
                                     : k_resamp_tiled_f32<true>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(RS_BLOCK), lds_t, st, d_in,
                           d_out, f->fir.taps.as<float>(), (int)f->fir.n_taps,
                           (int)f->fir.interp, (int)f->fir.decim,
                           (long long)produced, (long long)n_in, span);
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    hipLaunchKernelGGL(k_resamp_f32,
                       dim3(grid_for((long long)produced, 256)), dim3(256),
                       f->fir.n_taps * sizeof(float), st, d_in, d_out,
                       f->fir.taps.as<float>(), (int)f->fir.n_taps,
                       (int)f->fir.interp, (int)f->fir.decim,
                       (long long)produced);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int run_resamp_f32(fsdr_filter* f, const void* d_in, size_t n_in,
                          void* d_out, size_t n_out, void* stream,
                          fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    *r = resamp_status(f->fir.interp, f->fir.decim, f->fir.n_taps, n_in,
                       n_out);
    return launch_resamp_f32(f, (const float*)d_in, (float*)d_out,
                             r->produced, n_in, st);
}

/* Symbols per block of the LoRa kernel, like the Stockham kernel's frames
 * per block: 1024 samples' worth, at most 16, at least one. */
static int lora_spb(unsigned sf) {
    const int n = 1 << sf;
    return n >= 1024 ? 1 : std::min(16, 1024 / n);
}

static int launch_lora(const fsdr_filter* f, const void* d_in, void* d_out,
                       size_t n_sym, hipStream_t st) {
    if (n_sym == 0) return FSDR_OK;
    const int n = 1 << f->lora.sf, spb = lora_spb(f->lora.sf);
    const size_t lds = 2 * (size_t)spb * n * sizeof(float2) +
                       LORA_RED_DOUBLES * sizeof(double);
    const long long batches = ((long long)n_sym + spb - 1) / spb;
    const int grid = (int)std::min<long long>(batches, grid_cap(256 * 8));
    /* sf 12 needs 64 KiB + the reduction scratch: opt in past 64 KiB */
#define LORA_LAUNCH(MODE_, E_)                                               \
    do {                                                                     \
        static bool lds_opt_in = false;                                      \
        if (!lds_opt_in) {                                                   \
            HIP_TRY(hipFuncSetAttribute(                                     \
                (const void*)k_lora_demod<MODE_, E_>,                        \
                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));    \
            lds_opt_in = true;                                               \
        }                                                                    \
        hipLaunchKernelGGL((k_lora_demod<MODE_, E_>), dim3(grid),            \
                           dim3(LORA_BLOCK), lds, st, (const float2*)d_in,   \
                           d_out, f->lora.chirp.as<const float2>(),          \
                           f->lora.twid.as<const float2>(), (int)f->lora.sf, \
                           spb, f->lora.reduced, (long long)n_sym);          \
    } while (0)
#define LORA_LAUNCH_E(MODE_)                                                 \
    switch (n * spb / LORA_BLOCK) {                                          \
        case 2: LORA_LAUNCH(MODE_, 2); break;                                \
        case 4: LORA_LAUNCH(MODE_, 4); break;                                \
        case 8: LORA_LAUNCH(MODE_, 8); break;                                \
        default: LORA_LAUNCH(MODE_, 16); break;                              \
    }
    switch (f->lora.mode) {
        case LORA_RAW: LORA_LAUNCH_E(LORA_RAW); break;
        case LORA_HARD: LORA_LAUNCH_E(LORA_HARD); break;
        default: LORA_LAUNCH_E(LORA_SOFT); break;
    }
#undef LORA_LAUNCH_E
#undef LORA_LAUNCH
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int run_lora(fsdr_filter* f, const void* d_in, size_t n_in,
                    void* d_out, size_t n_out, void* stream,
                    fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    /* whole symbols only: a trailing partial one stays unconsumed */
    *r = decim_status((size_t)1 << f->lora.sf, n_in, 1, n_out);
    return launch_lora(f, d_in, d_out, r->produced, st);
}

/* n > 0 outputs of the IIR from the live memory half; the new memory goes
 * to the other half. Up to three launches (no feedback: one; one tile:
 * no tile-state pass). */
template <int NA>
static int launch_iir_na(fsdr_filter* f, const float* d_in, float* d_out,
                         long long n, hipStream_t st) {
    const long long n_tiles = (n + IIR_TILE - 1) / IIR_TILE;
    const int nb = (int)f->iir.n_b;
    const float* b = f->iir.b.as<float>();
    IirA a = {};
    for (int q = 0; q < NA; q++) a.a[q] = f->iir.plan->a[q];
    const int grid = (int)std::min<long long>(n_tiles, grid_cap(256 * 8));
    if constexpr (NA == 0) {
        hipLaunchKernelGGL(k_iir_apply<0>, dim3(grid), dim3(IIR_BLOCK), 0, st,
                           d_in, d_out, nullptr, nullptr, b, nb, a, nullptr,
                           nullptr, n, n_tiles);
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    } else {
        HIP_TRY(f->iir.tile_states.ensure(
            (size_t)(2 * n_tiles) * NA * sizeof(float)));
        float* T = f->iir.tile_states.as<float>();
        float* S = T + n_tiles * NA;
        const float* H = f->iir.tables.as<const float>();
        const float* pc = H + IIR_L * NA;
        const float* pt = pc + IIR_LEVELS * NA * NA;
        float* mem = f->iir.mem.live<float>(IIR_NA_MAX);
        float* mem_new = f->iir.mem.next<float>(IIR_NA_MAX);
        if (n_tiles > 1) {
            const int g = (int)std::min<long long>(n_tiles - 1,
                                                   grid_cap(256 * 8));
            hipLaunchKernelGGL(k_iir_tile_state<NA>, dim3(g), dim3(IIR_BLOCK),
                               0, st, d_in, T, b, nb, a, pc, n_tiles - 1);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_iir_tile_scan<NA>, dim3(1), dim3(IIR_P), 0,
                           st, (const float*)T, S, (const float*)mem, pt,
                           n_tiles);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_iir_apply<NA>, dim3(grid), dim3(IIR_BLOCK), 0, st,
                           d_in, d_out, (const float*)S, mem_new, b, nb, a, H,
                           pc, n, n_tiles);
        HIP_TRY(hipGetLastError());
        f->iir.mem.flip();
        return FSDR_OK;
    }
}

static int launch_iir(fsdr_filter* f, const float* d_in, float* d_out,
                      long long n, hipStream_t st) {
    switch (f->iir.plan->na) {
        case 0: return launch_iir_na<0>(f, d_in, d_out, n, st);
        case 1: return launch_iir_na<1>(f, d_in, d_out, n, st);
        case 2: return launch_iir_na<2>(f, d_in, d_out, n, st);
        case 3: return launch_iir_na<3>(f, d_in, d_out, n, st);
        case 4: return launch_iir_na<4>(f, d_in, d_out, n, st);
        case 5: return launch_iir_na<5>(f, d_in, d_out, n, st);
        case 6: return launch_iir_na<6>(f, d_in, d_out, n, st);
        case 7: return launch_iir_na<7>(f, d_in, d_out, n, st);
        case 8: return launch_iir_na<8>(f, d_in, d_out, n, st);
    }
    set_err("iir: no kernel for this n_a");
    return FSDR_ERR_INVALID;
}

static int run_iir(fsdr_filter* f, const void* d_in, size_t n_in,
                   void* d_out, size_t n_out, void* stream,
                   fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    if (d_in && d_in == d_out) {
        set_err("iir: in-place call (d_out == d_in)");
        return FSDR_ERR_INVALID;
    }
    const size_t filled = f->iir.filled;
    size_t filled_after;
    int status;
    fsdr_iir_count((size_t)f->iir.plan->na, f->iir.n_b, filled, n_in,
                   n_out, &filled_after, &r->consumed, &r->produced,
                   &status);
    r->status = (fsdr_status)status;
    if (filled_after > filled) {
        /* iir.rs:116: memory.push(i[memory.len()]) */
        float* mem = f->iir.mem.live<float>(IIR_NA_MAX);
        HIP_TRY(hipMemcpyAsync(mem + filled,
                               (const float*)d_in + filled,
                               (filled_after - filled) * sizeof(float),
                               hipMemcpyDeviceToDevice, st));
        f->iir.filled = filled_after;
    }
    if (r->produced == 0) return FSDR_OK;
    return launch_iir(f, (const float*)d_in, (float*)d_out,
                      (long long)r->produced, st);
}

/* `last` <- d_in[consumed-1], ordered after the kernel that read it */
static int update_demod_last(fsdr_filter* f, const void* d_in,
                             size_t consumed, hipStream_t st) {
    if (consumed == 0) return FSDR_OK;
    HIP_TRY(hipMemcpyAsync(f->demod.last.ptr,
                           (const float2*)d_in + (consumed - 1),
                           sizeof(float2), hipMemcpyDeviceToDevice, st));
    return FSDR_OK;
}

static int run_quad_demod(fsdr_filter* f, const void* d_in, size_t n_in,
                          void* d_out, size_t n_out, void* stream,
                          fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    size_t m = n_in < n_out ? n_in : n_out; /* apply.rs:108 */
    r->consumed = r->produced = m;
    r->status = FSDR_BOTH_SUFFICIENT;
    if (m == 0) return FSDR_OK;
    hipLaunchKernelGGL(k_quad_demod,
                       dim3(grid_for((long long)m, 256)), dim3(256),
                       0, st, (const float2*)d_in, (float*)d_out,
                       f->demod.last.as<const float2>(), (long long)m);
    HIP_TRY(hipGetLastError());
    return update_demod_last(f, d_in, m, st);
}

extern "C" int fsdr_fm_demod_resamp_fused(const fsdr_filter* f) {
    if (!f || f->kind != K_FM_DEMOD_RESAMP) return 0;
    int span;
    size_t lds;
    return resamp_f32_tile(f, &span, &lds) && env_on("FSDR_FM_FUSED");
}

static int launch_fm_demod_resamp(fsdr_filter* f, const void* d_in,
                                  size_t n_in, void* d_out,
                                  const fsdr_filter_result* r,
                                  hipStream_t st) {
    if (r->produced) {
        const float2* last = f->demod.last.as<const float2>();
        if (fsdr_fm_demod_resamp_fused(f)) {
            int span = 0;
            size_t lds = 0;
            (void)resamp_f32_tile(f, &span, &lds);
            long long tiles =
                ((long long)r->produced + RS_TILE - 1) / RS_TILE;
            int grid = (int)std::min<long long>(tiles, grid_cap(256 * 64));
            auto kern = f->fir.decim % 2 ? k_fm_demod_resamp<false>
                                     : k_fm_demod_resamp<true>;
            hipLaunchKernelGGL(kern, dim3(grid),
                               dim3(RS_BLOCK), lds, st, (const float2*)d_in,
                               (float*)d_out, f->fir.taps.as<float>(), last,
                               (int)f->fir.n_taps, (int)f->fir.interp,
                               (int)f->fir.decim, (long long)r->produced,
                               (long long)n_in, span);
            HIP_TRY(hipGetLastError());
        } else {
            /* staged: demodulate what the dot products read, then the
             * f32 resampler kernels on it */
            const size_t tpp = f->fir.n_taps / f->fir.interp;
            const size_t need =
                (r->produced - 1) * f->fir.decim / f->fir.interp + tpp;
            HIP_TRY(f->demod.staged.ensure(need * sizeof(float)));
            hipLaunchKernelGGL(k_quad_demod,
                               dim3(grid_for((long long)need, 256)),
                               dim3(256), 0, st, (const float2*)d_in,
                               f->demod.staged.as<float>(), last,
                               (long long)need);
            HIP_TRY(hipGetLastError());
            int rc = launch_resamp_f32(f, f->demod.staged.as<const float>(),
                                   (float*)d_out, r->produced, need, st);
            if (rc) return rc;
        }
    }
    return update_demod_last(f, d_in, r->consumed, st);
}

static int run_fm_demod_resamp(fsdr_filter* f, const void* d_in, size_t n_in,
                               void* d_out, size_t n_out, void* stream,
                               fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    /* the demodulated stream is as long as the input, so the resampler's
     * accounting applies to the Complex32 counts */
    *r = resamp_status(f->fir.interp, f->fir.decim, f->fir.n_taps, n_in,
                       n_out);
    return launch_fm_demod_resamp(f, d_in, n_in, d_out, r, st);
}

static int run_fir_f32(fsdr_filter* f, const void* d_in, size_t n_in,
                       void* d_out, size_t n_out, void* stream,
                       fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    *r = fir_status(n_in, f->fir.n_taps, n_out);
    if (r->produced == 0) return FSDR_OK;
    unsigned elems = 1024 + f->fir.n_padded - 1;
    size_t lds = (size_t)elems * sizeof(float);
    long long tiles = ((long long)r->produced + 1023) / 1024;
    int grid = (int)std::min<long long>(tiles, grid_cap(256 * 16));
    hipLaunchKernelGGL(k_fir_f32, dim3(grid), dim3(256), lds, st,
                       (const float*)d_in, (float*)d_out,
                       f->fir.taps.as<float>(), f->fir.n_padded,
                       (long long)r->produced, (long long)n_in);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int run_resamp_cf32(fsdr_filter* f, const void* d_in, size_t n_in,
                           void* d_out, size_t n_out, void* stream,
                           fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    *r = resamp_status(f->fir.interp, f->fir.decim, f->fir.n_taps, n_in,
                       n_out);
    if (r->produced == 0) return FSDR_OK;
    if (f->fir.decim4 && f->fir.decim4->fir.kk_mfma &&
        env_on("FSDR_DECIM_MFMA")) {
        /* 1:4 shape on the MFMA decim kernel: shift the window origin back
         * by D-1 (that kernel never reads rel < 3, so the rebased pointer
         * stays in bounds) */
        return launch_decim_cf32(f->fir.decim4, (const float2*)d_in - 3,
                                 d_out, r->produced, n_in + 3, st);
    }
    size_t tpp = f->fir.n_taps / f->fir.interp;
    long long span = (long long)(RS_TILE - 1) * f->fir.decim /
                         f->fir.interp + tpp + 2;
    size_t lds_t = (2 * (size_t)plane_floats((unsigned)span) +
                    f->fir.n_taps) * sizeof(float);
    if (lds_t <= 64 * 1024 && env_on("FSDR_RESAMP_TILED")) {
        long long tiles = ((long long)r->produced + RS_TILE - 1) / RS_TILE;
        int grid = (int)std::min<long long>(tiles, grid_cap(256 * 64));
        hipLaunchKernelGGL(k_resamp_tiled_cf32, dim3(grid), dim3(RS_BLOCK),
                           lds_t, st, (const float2*)d_in, (float2*)d_out,
                           f->fir.taps.as<float>(), (int)f->fir.n_taps,
                           (int)f->fir.interp, (int)f->fir.decim,
                           (long long)r->produced, (long long)n_in, (int)span);
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    size_t lds = f->fir.n_taps * sizeof(float);
    hipLaunchKernelGGL(k_resamp_cf32,
                       dim3(grid_for((long long)r->produced, 256)),
                       dim3(256), lds, st, (const float2*)d_in,
                       (float2*)d_out, f->fir.taps.as<float>(),
                       (int)f->fir.n_taps, (int)f->fir.interp,
                       (int)f->fir.decim, (long long)r->produced,
                       (long long)n_in);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int run_fir_ccf32(fsdr_filter* f, const void* d_in, size_t n_in,
                         void* d_out, size_t n_out, void* stream,
                         fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    *r = fir_status(n_in, f->fir.n_taps, n_out);
    if (r->produced == 0) return FSDR_OK;
    unsigned elems = 1024 + f->fir.n_taps - 1;
    size_t lds = ((size_t)elems + f->fir.n_taps) * sizeof(float2);
    long long tiles = ((long long)r->produced + 1023) / 1024;
    int grid = (int)std::min<long long>(tiles, grid_cap(256 * 64));
    hipLaunchKernelGGL(k_fir_ccf32, dim3(grid), dim3(256), lds, st,
                       (const float2*)d_in, (float2*)d_out,
                       f->fir.taps.as<const float2>(), (int)f->fir.n_taps,
                       (long long)r->produced, (long long)n_in);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

static int run_xlating(fsdr_filter* f, const void* d_in, size_t n_in,
                       void* d_out, size_t n_out, void* stream,
                       fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    *r = decim_status(f->fir.decim, n_in, f->fir.n_taps, n_out);
    if (r->produced == 0) return FSDR_OK;
    long long span = (long long)(XT_TILE - 1) * f->fir.decim +
                     f->fir.n_taps + 2;
    size_t lds_t = (2 * (size_t)plane_floats((unsigned)span) +
                    2 * f->fir.n_taps) * sizeof(float);
    if (lds_t <= 64 * 1024 && env_on("FSDR_XLATING_TILED")) {
        long long tiles = ((long long)r->produced + XT_TILE - 1) / XT_TILE;
        int grid = (int)std::min<long long>(tiles, grid_cap(256 * 64));
        hipLaunchKernelGGL(k_xlating_decim_tiled_ccf32, dim3(grid),
                           dim3(XT_BLOCK), lds_t, st, (const float2*)d_in,
                           (float2*)d_out, f->fir.taps.as<const float2>(),
                           (int)f->fir.n_taps, (int)f->fir.decim,
                           (long long)r->produced, (long long)n_in,
                           (double)f->xlat.theta, f->xlat.rot_re,
                           f->xlat.rot_im, (int)span);
        HIP_TRY(hipGetLastError());
    } else {
        size_t lds = f->fir.n_taps * sizeof(float2);
        hipLaunchKernelGGL(
            k_xlating_decim_ccf32, dim3(grid_for((long long)r->produced, 256)),
            dim3(256), lds, st, (const float2*)d_in, (float2*)d_out,
            f->fir.taps.as<const float2>(), (int)f->fir.n_taps,
            (long long)f->fir.decim, (long long)r->produced, (long long)n_in,
            f->xlat.theta, f->xlat.rot_re, f->xlat.rot_im);
        HIP_TRY(hipGetLastError());
    }
    { /* advance the rotator phase (closed form, f64) */
        double a = (double)f->xlat.theta * (double)r->produced;
        double cs = cos(a), sn = sin(a);
        float nr = (float)(cs * f->xlat.rot_re - sn * f->xlat.rot_im);
        float ni = (float)(cs * f->xlat.rot_im + sn * f->xlat.rot_re);
        f->xlat.rot_re = nr;
        f->xlat.rot_im = ni;
    }
    return FSDR_OK;
}

static int run_movavg(fsdr_filter* f, const void* d_in, size_t n_in,
                      void* d_out, size_t n_out, void* stream,
                      fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    auto& ma = f->movavg;
    /* the work() counting loop (consume a frame, emit every history-th one,
     * stop when input or output room runs out) in closed form: the loop
     * itself cost ~0.15 ms of host time per call at the bench's 262143
     * frames */
    size_t in_frames = n_in / ma.width;
    size_t out_frames = n_out / ma.width;
    size_t cons = 0, prod = 0, i = ma.i;
    movavg_count(in_frames, out_frames, ma.history, &cons, &prod, &i);
    r->consumed = cons * ma.width;
    r->produced = prod * ma.width;
    r->status = FSDR_BOTH_SUFFICIENT;
    if (cons == 0) return FSDR_OK;
    if (prod <= 1 && (prod == 0 || ma.i + cons == ma.history)) {
        /* parallel fast path: chunked EMA + exact composition */
        /* FSDR_MOVAVG_SKIP=0 computes every chunk */
        int cf, nch;
        const int c0 =
            movavg_plan(cons, ma.decay, env_on("FSDR_MOVAVG_SKIP"), &cf, &nch);
        HIP_TRY(ma.partials.ensure((size_t)nch * ma.width * 4));
        const long long live = (long long)(nch - c0) *
                               ((ma.width & 3) == 0 ? ma.width / 4 : ma.width);
        hipLaunchKernelGGL(k_moving_avg_chunks, dim3(grid_for(live, 256)),
                           dim3(256), 0, st, (const float*)d_in,
                           ma.partials.as<float>(), (int)ma.width,
                           (long long)cons, nch, cf, ma.decay, c0);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_moving_avg_combine,
                           dim3((unsigned)ma.width), dim3(256), 0, st,
                           ma.partials.as<const float>(), ma.avg.as<float>(),
                           prod ? (float*)d_out : nullptr, (int)ma.width,
                           (long long)cons, nch, cf, ma.decay, c0);
        HIP_TRY(hipGetLastError());
        ma.i = i;
        return FSDR_OK;
    }
    hipLaunchKernelGGL(k_moving_avg, dim3((unsigned)((ma.width + 255) / 256)),
                       dim3(256), 0, st, (const float*)d_in, (float*)d_out,
                       ma.avg.as<float>(), (int)ma.width, (long long)cons,
                       (int)ma.i, (int)ma.history, ma.decay);
    HIP_TRY(hipGetLastError());
    ma.i = i;
    return FSDR_OK;
}

/* one channel only (fsdr_filter_dev turns the others away) */
static int run_pfb_arb(fsdr_filter* f, const void* d_in, size_t n_in,
                       void* d_out, size_t n_out, void* stream,
                       fsdr_filter_result* r) {
    /* stateful block: stream semantics, like MovingAvg */
    r->status = FSDR_BOTH_SUFFICIENT;
    return fsdr_pfb_arb_resampler_stream_dev(f, d_in, n_in, n_in, d_out, n_out,
                                             n_out, stream, &r->consumed,
                                             &r->produced);
}

static int run_mag2(fsdr_filter* f, const void* d_in, size_t n_in,
                    void* d_out, size_t n_out, void* stream,
                    fsdr_filter_result* r) {
    hipStream_t st = (hipStream_t)stream;
    size_t m = n_in < n_out ? n_in : n_out; /* apply.rs:108 */
    r->consumed = r->produced = m;
    r->status = FSDR_BOTH_SUFFICIENT;
    if (m == 0) return FSDR_OK;
    hipLaunchKernelGGL(k_mag2, dim3(grid_for((long long)m, 256)), dim3(256), 0,
                       st, (const float2*)d_in, (float*)d_out, (long long)m);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

extern "C" int fsdr_filter_dev(fsdr_filter* f, const void* d_in, size_t n_in,
                               void* d_out, size_t n_out, void* stream,
                               fsdr_filter_result* r) {
    REQUIRE_GPU();
    if (!f || !r) { set_err("null argument"); return FSDR_ERR_INVALID; }
    int (*run)(fsdr_filter*, const void*, size_t, void*, size_t, void*,
               fsdr_filter_result*) = nullptr;
    switch (f->kind) {
        case K_FIR_CF32: run = run_fir_cf32; break;
        case K_FIR_F32: run = run_fir_f32; break;
        case K_DECIM_CF32: run = run_decim_cf32; break;
        case K_RESAMP_CF32: run = run_resamp_cf32; break;
        case K_FFT_CF32: run = run_fft; break;
        case K_FIR_CCF32: run = run_fir_ccf32; break;
        case K_XLATING: run = run_xlating; break;
        case K_MOVAVG: run = run_movavg; break;
        case K_RESAMP_F32: run = run_resamp_f32; break;
        case K_QUAD_DEMOD: run = run_quad_demod; break;
        case K_FM_DEMOD_RESAMP: run = run_fm_demod_resamp; break;
        case K_IIR_F32: run = run_iir; break;
        case K_LORA_DEMOD: run = run_lora; break;
        case K_MAG2: run = run_mag2; break;
        case K_PFB:
            set_err("pfb channelizer uses fsdr_pfb_channelizer_run_dev "
                    "(multi-output block)");
            return FSDR_ERR_INVALID;
        case K_PFB_SYNTH:
            set_err("pfb synthesizer uses fsdr_pfb_synthesizer_run_dev "
                    "(multi-input block)");
            return FSDR_ERR_INVALID;
        case K_PFB_ARB:
            if (f->pfb.channels != 1) {
                set_err("multi-channel pfb arb resampler uses "
                        "fsdr_pfb_arb_resampler_run_dev");
                return FSDR_ERR_INVALID;
            }
            run = run_pfb_arb;
            break;
    }
    if (!run) {
        set_err("unknown filter kind");
        return FSDR_ERR_INVALID;
    }
    return run(f, d_in, n_in, d_out, n_out, stream, r);
}

extern "C" int fsdr_filter_host(fsdr_filter* f, const void* in, size_t n_in,
                                void* out, size_t n_out,
                                fsdr_filter_result* r) {
    REQUIRE_GPU();
    if (!f || !r) { set_err("null argument"); return FSDR_ERR_INVALID; }
    HIP_TRY(f->stage_in.ensure(n_in * f->item_in + 64));
    HIP_TRY(f->stage_out.ensure(n_out * f->item_out + 64));
    if (n_in)
        HIP_TRY(hipMemcpy(f->stage_in.ptr, in, n_in * f->item_in,
                          hipMemcpyHostToDevice));
    int rc = fsdr_filter_dev(f, f->stage_in.ptr, n_in, f->stage_out.ptr, n_out,
                         nullptr, r);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (r->produced)
        HIP_TRY(hipMemcpy(out, f->stage_out.ptr, r->produced * f->item_out,
                          hipMemcpyDeviceToHost));
    return FSDR_OK;
}

extern "C" void fsdr_pfb_channelizer_window_map(size_t taps_per_filter,
                                                size_t q, long long* src) {
    if (!src) return;
    for (size_t w = 0; w < taps_per_filter; w++)
        src[w] = pfb_chan_window_src((int)taps_per_filter, (int)q, (int)w);
}

/* dots of `steps` output steps after p_before pushes into ch.dots:
 * k_pfb_dots over all of them, launched as it always was, then the
 * leading steps with fewer than 2*N*tpf pushes are rewritten through the
 * start-up map by a small launch of their own (as the synthesizer's
 * start-up rows are). d_in[0] is stream sample `bufbase`; 0 while any
 * step is a start-up one. */
static int pfb_chan_dots(fsdr_filter* f, const float2* d_in, size_t steps,
                         size_t p_before, size_t bufbase, hipStream_t st) {
    auto& ch = f->chan;
    const size_t N = f->pfb.channels, tpf = f->pfb.tpf, D = ch.decim;
    const size_t steady_at = 2 * N * tpf;
    hipLaunchKernelGGL(k_pfb_dots,
                       dim3(grid_for((long long)(steps * N), 256)),
                       dim3(256), 0, st, d_in, ch.dots.as<float2>(),
                       ch.taps.as<const float>(), (int)N, (int)tpf, (int)D,
                       (long long)steps, (long long)p_before,
                       (long long)bufbase);
    HIP_TRY(hipGetLastError());
    if (p_before + D < steady_at) {
        const size_t n_start =
            std::min(steps, (steady_at - p_before + D - 1) / D - 1);
        hipLaunchKernelGGL(k_pfb_dots_startup,
                           dim3(grid_for((long long)(n_start * N), 256)),
                           dim3(256), 0, st, d_in, ch.dots.as<float2>(),
                           ch.taps.as<const float>(), (int)N, (int)tpf,
                           (int)D, (long long)n_start, (long long)p_before,
                           (long long)bufbase);
        HIP_TRY(hipGetLastError());
    }
    return FSDR_OK;
}

extern "C" int fsdr_pfb_channelizer_run_dev(fsdr_filter* f,
                                            const void* d_in, size_t n_in,
                                            void* d_out,
                                            size_t out_cap_per_chan,
                                            void* stream,
                                            size_t* produced_per_chan) {
    REQUIRE_GPU();
    if (!f || f->kind != K_PFB) {
        set_err("not a pfb channelizer");
        return FSDR_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    auto& ch = f->chan;
    size_t N = f->pfb.channels, tpf = f->pfb.tpf, D = ch.decim;
    size_t prefill = N * tpf;
    size_t steps = n_in > prefill ? (n_in - prefill) / D : 0;
    if (steps > out_cap_per_chan) steps = out_cap_per_chan;
    if (produced_per_chan) *produced_per_chan = steps;
    if (steps == 0) return FSDR_OK;
    HIP_TRY(ch.dots.ensure(steps * N * 8));
    HIP_TRY(ch.spectra.ensure(steps * N * 8));
    int rc = pfb_chan_dots(f, (const float2*)d_in, steps, prefill, 0, st);
    if (rc) return rc;
    rc = launch_fft(f->pfb.ifft, ch.dots.ptr, ch.spectra.ptr, steps, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pfb_scatter,
                       dim3(grid_for((long long)(steps * N), 256)),
                       dim3(256), 0, st, ch.spectra.as<const float2>(),
                       (float2*)d_out, (int)N, (long long)steps,
                       (long long)out_cap_per_chan);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

/* Streaming channelizer: stateful like the reference block — carries
 * the round-robin window contents (the last N*tpf CONSUMED samples) and
 * the push count across calls, consuming in D-sample quanta after the
 * N*tpf prefill (channelizer.rs:156-212). While the stream is younger
 * than 2*N*tpf pushes it carries every consumed sample instead, since a
 * start-up step reads fill pushes back to the first. The unconsumed
 * chunk remainder stays with the caller (pair with fsdr_ring's
 * release_consumed carry). All work is enqueued on `stream`; use one
 * stream per filter. */
extern "C" int fsdr_pfb_channelizer_stream_dev(
    fsdr_filter* f, const void* d_chunk, size_t n, void* d_out,
    size_t out_cap_per_chan, void* stream, size_t* produced_per_chan,
    size_t* consumed) {
    REQUIRE_GPU();
    if (!f || f->kind != K_PFB) {
        set_err("not a pfb channelizer");
        return FSDR_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    auto& ch = f->chan;
    size_t N = f->pfb.channels, tpf = f->pfb.tpf, D = ch.decim;
    size_t prefill = N * tpf, W = N * tpf;
    size_t p = ch.pushes;
    size_t T = p < 2 * W ? p : W;
    size_t fill = p < prefill ? std::min(prefill - p, n) : 0;
    size_t steps = (p + n >= prefill) ? (p + n - prefill) / D -
                                            (p > prefill ? (p - prefill) / D
                                                         : 0)
                                      : 0;
    if (steps > out_cap_per_chan) steps = out_cap_per_chan;
    size_t cons = fill + steps * D;
    if (cons > n) cons = n; /* fill-only calls */
    if (produced_per_chan) *produced_per_chan = steps;
    if (consumed) *consumed = cons;
    if (cons == 0) return FSDR_OK;
    /* work buffer = [hist(T), chunk(cons)] */
    HIP_TRY(ch.work.ensure((T + cons) * 8));
    if (T)
        HIP_TRY(hipMemcpyAsync(ch.work.ptr, ch.hist.ptr, T * 8,
                               hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(ch.work.as<char>() + T * 8, d_chunk, cons * 8,
                           hipMemcpyDeviceToDevice, st));
    if (steps) {
        HIP_TRY(ch.dots.ensure(steps * N * 8));
        HIP_TRY(ch.spectra.ensure(steps * N * 8));
        int rc = pfb_chan_dots(f, ch.work.as<const float2>(), steps,
                               p + fill, p - T, st);
        if (rc) return rc;
        rc = launch_fft(f->pfb.ifft, ch.dots.ptr, ch.spectra.ptr, steps, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_pfb_scatter,
                           dim3(grid_for((long long)(steps * N), 256)),
                           dim3(256), 0, st, ch.spectra.as<const float2>(),
                           (float2*)d_out, (int)N, (long long)steps,
                           (long long)out_cap_per_chan);
        HIP_TRY(hipGetLastError());
    }
    /* new hist = the whole work buffer while the stream is young, its
     * last W samples from then on */
    size_t newT = p + cons < 2 * W ? T + cons : W;
    HIP_TRY(ch.hist.ensure(2 * W * 8));
    HIP_TRY(hipMemcpyAsync(ch.hist.ptr,
                           ch.work.as<char>() + (T + cons - newT) * 8,
                           newT * 8, hipMemcpyDeviceToDevice, st));
    ch.pushes = p + cons;
    return FSDR_OK;
}

/* Synthesize S consumed steps, the first `fill` of which emit nothing,
 * in front of H carried frames; writes the frames the next call needs to
 * hist_new (nullable). Fused single launch where pfb_synth_plan allows
 * (FSDR_PFB_SYNTH_FUSED=0 forces the staged gather -> IFFT -> commutator
 * path, which takes every N). */
static int pfb_synth_main(fsdr_filter* f, const float2* d_in,
                          size_t in_stride, size_t S, size_t fill,
                          float2* d_out, const float2* hist_old, size_t H,
                          float2* hist_new, hipStream_t st) {
    const size_t N = f->pfb.channels, tpf = f->pfb.tpf;
    const size_t newH = std::min(tpf - 1, H + S);
    const size_t nn = std::min(newH, S), keep = newH - nn;
    if (hist_new && keep)
        HIP_TRY(hipMemcpyAsync(hist_new, hist_old + (H - keep) * N,
                               keep * N * 8, hipMemcpyDeviceToDevice, st));
    int log2n = 0;
    while (((size_t)1 << log2n) < N) log2n++;
    SynthPlan pl;
    if (env_on("FSDR_PFB_SYNTH_FUSED") && pfb_synth_plan(N, tpf, &pl)) {
        const long long blocks = ((long long)S + pl.R - 1) / pl.R;
        const int grid = (int)std::min<long long>(blocks, 256 * 32);
#define SYN_FUSED_LAUNCH(NL_)                                                \
    do {                                                                     \
        static bool lds_opt_in = false;                                      \
        if (!lds_opt_in) {                                                   \
            HIP_TRY(hipFuncSetAttribute(                                     \
                (const void*)k_pfb_synth_fused<NL_>,                         \
                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));    \
            lds_opt_in = true;                                               \
        }                                                                    \
        hipLaunchKernelGGL(k_pfb_synth_fused<NL_>, dim3(grid),               \
                           dim3(pl.threads), pl.lds, st, d_in,               \
                           (long long)in_stride, (long long)S, hist_old,     \
                           (long long)H, hist_new, (long long)(S - nn),      \
                           (long long)keep, d_out, (long long)fill,          \
                           f->synth.taps.as<const float>(),                  \
                           f->pfb.ifft->fft.twid.as<const float2>(), (int)N, \
                           log2n, (int)tpf, pl.F, pl.G, pl.FS, pl.R, pl.hp); \
    } while (0)
        switch (pl.NL) {
            case 1: SYN_FUSED_LAUNCH(1); break;
            case 2: SYN_FUSED_LAUNCH(2); break;
            case 4: SYN_FUSED_LAUNCH(4); break;
            default: SYN_FUSED_LAUNCH(8); break;
        }
#undef SYN_FUSED_LAUNCH
        HIP_TRY(hipGetLastError());
        return FSDR_OK;
    }
    HIP_TRY(f->synth.gathered.ensure(S * N * 8));
    HIP_TRY(f->synth.frames.ensure((H + S) * N * 8));
    float2* v = f->synth.frames.as<float2>();
    if (H)
        HIP_TRY(hipMemcpyAsync(v, hist_old, H * N * 8,
                               hipMemcpyDeviceToDevice, st));
    const long long tiles =
        (long long)((N + 31) / 32) * (long long)((S + 31) / 32);
    hipLaunchKernelGGL(k_pfb_synth_gather,
                       dim3((unsigned)std::min<long long>(tiles, 256 * 32)),
                       dim3(SYN_BLOCK), 0, st, d_in,
                       f->synth.gathered.as<float2>(), (int)N,
                       (long long)in_stride, (long long)S);
    HIP_TRY(hipGetLastError());
    int rc = launch_fft(f->pfb.ifft, f->synth.gathered.ptr, v + H * N, S, st);
    if (rc) return rc;
    if (S > fill) {
        const long long runs = ((long long)(S - fill) + SYN_TT - 1) / SYN_TT;
        hipLaunchKernelGGL(k_pfb_synth_comm,
                           dim3(grid_for(runs * (long long)N, 256)),
                           dim3(256), 0, st, (const float2*)v, d_out,
                           f->synth.taps.as<const float>(), (int)N, (int)tpf,
                           (long long)H, (long long)fill,
                           (long long)(S - fill));
        HIP_TRY(hipGetLastError());
    }
    if (hist_new && nn)
        HIP_TRY(hipMemcpyAsync(hist_new + keep * N, v + (H + S - nn) * N,
                               nn * N * 8, hipMemcpyDeviceToDevice, st));
    return FSDR_OK;
}

/* pfb_synth_main plus, while the stream is within its first 2tpf-1
 * steps (`p` consumed before this call), the start-up rows: the call's
 * early columns are IFFT'd into ve[p..] (staged gather + IFFT, a few
 * frames) and k_pfb_synth_startup rewrites the emitted rows among them. */
static int pfb_synth_launch(fsdr_filter* f, const float2* d_in,
                            size_t in_stride, size_t S, size_t fill,
                            float2* d_out, const float2* hist_old, size_t H,
                            float2* hist_new, size_t p, float2* ve,
                            hipStream_t st) {
    int rc = pfb_synth_main(f, d_in, in_stride, S, fill, d_out, hist_old, H,
                            hist_new, st);
    const size_t N = f->pfb.channels, L = f->pfb.tpf;
    if (rc || L == 1 || p >= 2 * L - 1) return rc;
    const size_t eb = std::min(p + S, 2 * L - 1), ne = eb - p;
    HIP_TRY(f->synth.gathered.ensure(ne * N * 8));
    const long long tiles =
        (long long)((N + 31) / 32) * (long long)((ne + 31) / 32);
    hipLaunchKernelGGL(k_pfb_synth_gather,
                       dim3((unsigned)std::min<long long>(tiles, 256 * 32)),
                       dim3(SYN_BLOCK), 0, st, d_in,
                       f->synth.gathered.as<float2>(), (int)N,
                       (long long)in_stride, (long long)ne);
    HIP_TRY(hipGetLastError());
    rc = launch_fft(f->pfb.ifft, f->synth.gathered.ptr, ve + p * N, ne, st);
    if (rc) return rc;
    const size_t ga = std::max(p, L - 1); /* first emitting step here */
    if (ga < eb) {
        hipLaunchKernelGGL(k_pfb_synth_startup,
                           dim3(grid_for((long long)((eb - ga) * N), 256)),
                           dim3(256), 0, st, (const float2*)ve,
                           d_out + (ga - p - fill) * N,
                           f->synth.taps.as<const float>(), (int)N, (int)L,
                           (int)(ga - (L - 1)), (int)(eb - ga));
        HIP_TRY(hipGetLastError());
    }
    return FSDR_OK;
}

extern "C" int fsdr_pfb_synthesizer_run_dev(fsdr_filter* f,
                                            const void* d_in,
                                            size_t in_stride,
                                            size_t n_in_per_chan,
                                            void* d_out, size_t out_cap,
                                            void* stream,
                                            size_t* consumed_per_chan,
                                            size_t* produced) {
    REQUIRE_GPU();
    if (!f || f->kind != K_PFB_SYNTH) {
        set_err("not a pfb synthesizer");
        return FSDR_ERR_INVALID;
    }
    if (n_in_per_chan > in_stride) {
        set_err("pfb synthesizer: n_in_per_chan exceeds in_stride");
        return FSDR_ERR_INVALID;
    }
    size_t fill, steps;
    pfb_synth_count(f->pfb.channels, f->pfb.tpf, 0, n_in_per_chan, out_cap,
                    &fill, &steps);
    if (consumed_per_chan) *consumed_per_chan = fill + steps;
    if (produced) *produced = steps * f->pfb.channels;
    if (steps == 0) return FSDR_OK; /* zero state: nothing to carry */
    HIP_TRY(f->synth.early_oneshot.ensure(
        2 * f->pfb.tpf * f->pfb.channels * 8));
    return pfb_synth_launch(f, (const float2*)d_in, in_stride, fill + steps,
                            fill, (float2*)d_out, nullptr, 0, nullptr, 0,
                            f->synth.early_oneshot.as<float2>(),
                            (hipStream_t)stream);
}

/* Streaming synthesizer: carries the last tpf-1 IFFT'd frames (the
 * window contents) and the push count across calls, so any chunking
 * reproduces the one-shot stream. Unconsumed steps stay with the caller,
 * as with the channelizer. All work is enqueued on `stream`; use one
 * stream per filter. */
extern "C" int fsdr_pfb_synthesizer_stream_dev(fsdr_filter* f,
                                               const void* d_in,
                                               size_t in_stride,
                                               size_t n_in_per_chan,
                                               void* d_out, size_t out_cap,
                                               void* stream,
                                               size_t* consumed_per_chan,
                                               size_t* produced) {
    REQUIRE_GPU();
    if (!f || f->kind != K_PFB_SYNTH) {
        set_err("not a pfb synthesizer");
        return FSDR_ERR_INVALID;
    }
    if (n_in_per_chan > in_stride) {
        set_err("pfb synthesizer: n_in_per_chan exceeds in_stride");
        return FSDR_ERR_INVALID;
    }
    const size_t N = f->pfb.channels, tpf = f->pfb.tpf, p = f->synth.steps;
    size_t fill, steps;
    pfb_synth_count(N, tpf, p, n_in_per_chan, out_cap, &fill, &steps);
    const size_t S = fill + steps;
    if (consumed_per_chan) *consumed_per_chan = S;
    if (produced) *produced = steps * N;
    if (S == 0) return FSDR_OK;
    const size_t half = (tpf - 1) * N;
    HIP_TRY(f->synth.hist.buf.ensure(2 * half * 8 + 8));
    HIP_TRY(f->synth.early.ensure(2 * tpf * N * 8));
    float2* h_old = f->synth.hist.live<float2>(half);
    float2* h_new = f->synth.hist.next<float2>(half);
    int rc = pfb_synth_launch(f, (const float2*)d_in, in_stride, S, fill,
                          (float2*)d_out, h_old, std::min(p, tpf - 1),
                          tpf > 1 ? h_new : nullptr, p,
                          f->synth.early.as<float2>(), (hipStream_t)stream);
    if (rc) return rc;
    f->synth.hist.flip();
    f->synth.steps = p + S;
    return FSDR_OK;
}

/* ---- PFB arb resampler: launches ------------------------------------- */

/* `fill` window-fill pushes (the stream's pushes k0..) then n processed
 * inputs from schedule position P0 yielding M outputs per channel, on
 * the window `hist`; hist_next (nullable) receives the window after the
 * call. */
static int pfb_arb_launch(fsdr_filter* f, const float2* d_in,
                          size_t in_stride, size_t fill, size_t k0, size_t n,
                          unsigned long long P0, size_t M, float2* d_out,
                          size_t out_stride, float2* hist, float2* hist_next,
                          hipStream_t st) {
    const fsdr_pfb_arb_schedule* s = f->arb.sched;
    const int C = (int)f->pfb.channels, tpf = (int)f->pfb.tpf;
    if (fill) {
        hipLaunchKernelGGL(k_pfb_arb_fill,
                           dim3(grid_for((long long)fill * C, 256)),
                           dim3(256), 0, st, d_in, (long long)in_stride,
                           hist, C, tpf, (long long)k0, (long long)fill);
        HIP_TRY(hipGetLastError());
    }
    if (n == 0) return FSDR_OK; /* the fill wrote the window in place */
    const float2* x = d_in + fill;
    if (M) {
        ArbSt st0;
        ArbParams p;
        p.ck = f->arb.ck.as<const ArbCk>();
        p.rho = s->rho; p.lam = s->lam; p.opc = s->opc;
        p.P0 = P0; p.cum0 = arb_seek(s, P0, &st0);
        p.delay = s->delay; p.nff = s->nff;
        p.nf = s->nf; p.maxo1 = s->maxo1;
        p.tpf = tpf; p.C = C; p.RL = s->RL; p.W = s->W;
        const long long R = (long long)s->W * s->RL;
        const long long nseg = ((long long)n + R - 1) / R;
        const int grid = (int)std::min<long long>(nseg, grid_cap(256 * 8));
        bool taps_lds;
        const size_t lds = pfb_arb_lds(s, (size_t)tpf, &taps_lds);
        if (taps_lds)
            hipLaunchKernelGGL(k_pfb_arb<true>, dim3(grid), dim3(ARB_BLOCK),
                               lds, st, x, (long long)in_stride,
                               (long long)n, (const float2*)hist, d_out,
                               (long long)out_stride, (long long)M,
                               f->arb.taps.as<const float>(), p, nseg);
        else
            hipLaunchKernelGGL(k_pfb_arb<false>, dim3(grid), dim3(ARB_BLOCK),
                               lds, st, x, (long long)in_stride,
                               (long long)n, (const float2*)hist, d_out,
                               (long long)out_stride, (long long)M,
                               f->arb.taps.as<const float>(), p, nseg);
        HIP_TRY(hipGetLastError());
    }
    if (hist_next) {
        hipLaunchKernelGGL(k_pfb_arb_hist,
                           dim3(grid_for((long long)C * tpf, 256)), dim3(256),
                           0, st, x, (long long)in_stride, (long long)n,
                           (const float2*)hist, hist_next, C, tpf);
        HIP_TRY(hipGetLastError());
    }
    return FSDR_OK;
}

static int pfb_arb_check(const fsdr_filter* f, size_t in_stride,
                         size_t n_in, size_t out_stride, size_t out_cap) {
    if (!f || f->kind != K_PFB_ARB) {
        set_err("not a pfb arb resampler");
        return FSDR_ERR_INVALID;
    }
    if (f->pfb.channels > 1 && (n_in > in_stride || out_cap > out_stride)) {
        set_err("pfb arb resampler: n_in_per_chan exceeds in_stride or "
                "out_cap_per_chan exceeds out_stride");
        return FSDR_ERR_INVALID;
    }
    return FSDR_OK;
}

extern "C" int fsdr_pfb_arb_resampler_run_dev(
    fsdr_filter* f, const void* d_in, size_t in_stride, size_t n_in_per_chan,
    void* d_out, size_t out_stride, size_t out_cap_per_chan, void* stream,
    size_t* consumed_per_chan, size_t* produced_per_chan) {
    REQUIRE_GPU();
    int rc = pfb_arb_check(f, in_stride, n_in_per_chan, out_stride,
                           out_cap_per_chan);
    if (rc) return rc;
    size_t fill, n, M;
    arb_work(f->arb.sched, f->pfb.tpf, 0, n_in_per_chan, out_cap_per_chan,
             &fill, &n, &M);
    if (consumed_per_chan) *consumed_per_chan = fill + n;
    if (produced_per_chan) *produced_per_chan = M;
    if (M == 0) return FSDR_OK; /* zero state: nothing to carry */
    const size_t hb = f->pfb.channels * f->pfb.tpf * 8;
    dev_buf& win = f->arb.window_oneshot;
    HIP_TRY(win.ensure(hb));
    HIP_TRY(hipMemsetAsync(win.ptr, 0, hb, (hipStream_t)stream));
    return pfb_arb_launch(f, (const float2*)d_in, in_stride, fill, 0, n, 0, M,
                          (float2*)d_out, out_stride, win.as<float2>(),
                          nullptr, (hipStream_t)stream);
}

/* Streaming: carries the window (the last tpf samples per channel) and
 * the consumed-input count across calls, so any chunking reproduces the
 * one-shot stream. Use one stream per filter. */
extern "C" int fsdr_pfb_arb_resampler_stream_dev(
    fsdr_filter* f, const void* d_in, size_t in_stride, size_t n_in_per_chan,
    void* d_out, size_t out_stride, size_t out_cap_per_chan, void* stream,
    size_t* consumed_per_chan, size_t* produced_per_chan) {
    REQUIRE_GPU();
    int rc = pfb_arb_check(f, in_stride, n_in_per_chan, out_stride,
                           out_cap_per_chan);
    if (rc) return rc;
    const size_t tpf = f->pfb.tpf, p = f->arb.consumed;
    size_t fill, n, M;
    arb_work(f->arb.sched, tpf, p, n_in_per_chan, out_cap_per_chan, &fill, &n,
             &M);
    if (consumed_per_chan) *consumed_per_chan = fill + n;
    if (produced_per_chan) *produced_per_chan = M;
    if (fill + n == 0) return FSDR_OK;
    const size_t half = f->pfb.channels * tpf;
    float2* h_live = f->arb.window.live<float2>(half);
    float2* h_next = f->arb.window.next<float2>(half);
    rc = pfb_arb_launch(f, (const float2*)d_in, in_stride, fill, p, n,
                        p + fill - (n ? tpf : 0), M, (float2*)d_out,
                        out_stride, h_live, n ? h_next : nullptr,
                        (hipStream_t)stream);
    if (rc) return rc;
    if (n) f->arb.window.flip();
    f->arb.consumed = p + fill + n;
    return FSDR_OK;
}

extern "C" int fsdr_divide_mag_dev(const void* d_a, size_t n_a,
                                   const void* d_b, size_t n_b,
                                   void* d_out, size_t n_out, void* stream,
                                   size_t* m) {
    REQUIRE_GPU();
    size_t mm = n_a < n_b ? n_a : n_b;
    if (n_out < mm) mm = n_out;
    if (m) *m = mm;
    if (mm == 0) return FSDR_OK;
    hipLaunchKernelGGL(k_divide_mag, dim3(grid_for((long long)mm, 256)),
                       dim3(256), 0, (hipStream_t)stream,
                       (const float2*)d_a, (const float*)d_b,
                       (float*)d_out, (long long)mm);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

extern "C" int fsdr_cmul_conj_dev(const void* d_a, size_t n_a,
                                  const void* d_b, size_t n_b, void* d_out,
                                  size_t n_out, void* stream, size_t* m) {
    REQUIRE_GPU();
    size_t mm = n_a < n_b ? n_a : n_b;
    if (n_out < mm) mm = n_out;
    if (m) *m = mm;
    if (mm == 0) return FSDR_OK;
    hipLaunchKernelGGL(k_cmul_conj, dim3(grid_for((long long)mm, 256)),
                       dim3(256), 0, (hipStream_t)stream,
                       (const float2*)d_a, (const float2*)d_b,
                       (float2*)d_out, (long long)mm);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

/* WLAN MovingAverage, one-shot from fresh state: emits len-1 zero items
 * then sliding sums; is_complex selects cf32 vs f32 items. */
extern "C" int fsdr_wlan_moving_sum_dev(const void* d_in, size_t n_in,
                                        void* d_out, size_t n_out,
                                        size_t len, int is_complex,
                                        void* stream, size_t* produced) {
    REQUIRE_GPU();
    if (len == 0) { set_err("len must be > 0"); return FSDR_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    size_t w = is_complex ? 2 : 1;
    size_t pad = len - 1 < n_out ? len - 1 : n_out;
    if (pad)
        HIP_TRY(hipMemsetAsync(d_out, 0, pad * w * sizeof(float), st));
    size_t m = n_in + 1 > len ? n_in + 1 - len : 0;
    if (m > n_out - pad) m = n_out - pad;
    if (produced) *produced = pad + m;
    if (m == 0) return FSDR_OK;
    hipLaunchKernelGGL(k_moving_sum,
                       dim3(grid_for((long long)(m * w), 256)), dim3(256),
                       0, st, (const float*)d_in,
                       (float*)d_out + pad * w, (int)w, (int)len,
                       (long long)m);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

extern "C" int fsdr_cmul_dev(const void* d_a, size_t n_a, const void* d_b,
                             size_t n_b, void* d_out, size_t n_out,
                             void* stream, size_t* m) {
    REQUIRE_GPU();
    size_t mm = n_a < n_b ? n_a : n_b; /* combine.rs:115-116 */
    if (n_out < mm) mm = n_out;
    if (m) *m = mm;
    if (mm == 0) return FSDR_OK;
    hipLaunchKernelGGL(k_cmul, dim3(grid_for((long long)mm, 256)), dim3(256),
                       0, (hipStream_t)stream, (const float2*)d_a,
                       (const float2*)d_b, (float2*)d_out, (long long)mm);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

extern "C" int fsdr_cmul_host(const void* a, size_t n_a, const void* b,
                              size_t n_b, void* out, size_t n_out,
                              size_t* m) {
    REQUIRE_GPU();
    size_t mm = n_a < n_b ? n_a : n_b;
    if (n_out < mm) mm = n_out;
    dev_buf da, db, do_; /* freed on every return */
    HIP_TRY(da.ensure((mm ? mm : 1) * 8));
    HIP_TRY(db.ensure((mm ? mm : 1) * 8));
    HIP_TRY(do_.ensure((mm ? mm : 1) * 8));
    if (mm) {
        HIP_TRY(hipMemcpy(da.ptr, a, mm * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(db.ptr, b, mm * 8, hipMemcpyHostToDevice));
    }
    int rc = fsdr_cmul_dev(da.ptr, mm, db.ptr, mm, do_.ptr, mm, nullptr, m);
    if (rc == FSDR_OK && mm) {
        HIP_TRY(hipStreamSynchronize(nullptr));
        HIP_TRY(hipMemcpy(out, do_.ptr, mm * 8, hipMemcpyDeviceToHost));
    }
    return rc;
}

/* ---- device memory helpers ---- */

extern "C" int fsdr_dev_alloc(void** d_ptr, size_t bytes) {
    REQUIRE_GPU();
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return FSDR_OK;
}
extern "C" int fsdr_dev_free(void* d_ptr) {
    REQUIRE_GPU();
    HIP_TRY(hipFree(d_ptr));
    return FSDR_OK;
}
extern "C" int fsdr_memcpy_h2d(void* d_dst, const void* src, size_t bytes) {
    REQUIRE_GPU();
    HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return FSDR_OK;
}
extern "C" int fsdr_memcpy_d2h(void* dst, const void* d_src, size_t bytes) {
    REQUIRE_GPU();
    HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return FSDR_OK;
}
extern "C" int fsdr_fill_uniform_cf32(void* d_ptr, size_t n, uint64_t seed,
                                      uint64_t offset, void* stream) {
    REQUIRE_GPU();
    hipLaunchKernelGGL(k_fill_uniform_cf32,
                       dim3(grid_for((long long)(n / 2 + 1), 256)),
                       dim3(256), 0, (hipStream_t)stream, (float2*)d_ptr,
                       (long long)n, seed, offset);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

/* ================= firdes (host-side) ================================= *
 * Product restatement of the reference tap designers (host code in the
 * reference too): firdes/basic.rs:25-42,310-321,444-459, windows.rs:144,
 * special_funs.rs:22-45. Independent of oracle/ (test infra). */

static double besseli0_h(double x) {
    double t = x / 3.75;
    if (fabs(x) <= 3.75) {
        return 1.0 + 3.5156229 * pow(t, 2.0) + 3.0899424 * pow(t, 4.0) +
               1.2067492 * pow(t, 6.0) + 0.2659732 * pow(t, 8.0) +
               0.0360768 * pow(t, 10.0) + 0.0045813 * pow(t, 12.0);
    }
    return 1.0 / (sqrt(fabs(x)) * exp(-x)) *
           (0.39894228 + 0.01328592 * pow(t, -1.0) + 0.00225319 * pow(t, -2.0) -
            0.00157565 * pow(t, -3.0) + 0.00916281 * pow(t, -4.0) -
            0.02057706 * pow(t, -5.0) + 0.02635537 * pow(t, -6.0) -
            0.01647633 * pow(t, -7.0) + 0.00392377 * pow(t, -8.0));
}

extern "C" double fsdr_kaiser_beta(double max_ripple) {
    double ripple_db = -20.0 * log10(max_ripple);
    if (ripple_db > 50.0) return 0.1102 * (ripple_db - 8.7);
    if (ripple_db >= 21.0)
        return 0.5842 * pow(ripple_db - 21.0, 0.4) +
               0.07886 * (ripple_db - 21.0);
    return 0.0;
}

extern "C" void fsdr_kaiser_window(size_t len, double beta, double* out) {
    double alpha = (double)(len - 1) / 2.0;
    double denom = besseli0_h(beta);
    for (size_t n = 0; n < len; n++) {
        double q = ((double)n - alpha) / alpha;
        out[n] = besseli0_h(beta * sqrt(1.0 - q * q)) / denom;
    }
}

static void firdes_lowpass_h(double cutoff, const double* win, size_t len,
                             double* out) {
    double omega_c = 2.0 * M_PI * cutoff;
    double alpha = (double)(len - 1) / 2.0;
    for (size_t n = 0; n < len; n++) {
        double x = (double)n - alpha;
        double ft = (x == 0.0) ? omega_c / M_PI : sin(omega_c * x) / (M_PI * x);
        out[n] = win[n] * ft;
    }
}

extern "C" size_t fsdr_firdes_kaiser_lowpass_f32(double cutoff,
                                                 double transition_bw,
                                                 double max_ripple,
                                                 float* out, size_t cap) {
    double beta = fsdr_kaiser_beta(max_ripple);
    double ripple_db = -20.0 * log10(max_ripple);
    size_t num_taps =
        (size_t)(ceil((ripple_db - 7.95) / (14.36 * transition_bw)) + 1.0);
    if (!out || cap < num_taps) return num_taps;
    std::vector<double> win(num_taps), taps(num_taps);
    fsdr_kaiser_window(num_taps, beta, win.data());
    double omega_c = (2.0 * cutoff + transition_bw) / 2.0; /* basic.rs:319 */
    firdes_lowpass_h(omega_c, win.data(), num_taps, taps.data());
    for (size_t i = 0; i < num_taps; i++) out[i] = (float)taps[i];
    return num_taps;
}

/* firdes::kaiser::multirate<f32>, basic.rs:412-442: the Nyquist (L-th
 * band) filter FirBuilder::resampling designs, 2*half_polyphase_len taps
 * per polyphase arm. */
extern "C" size_t fsdr_firdes_kaiser_multirate_f32(size_t interp,
                                                   size_t decim,
                                                   size_t half_polyphase_len,
                                                   double max_ripple,
                                                   float* out, size_t cap) {
    if (interp == 0 || decim == 0 || half_polyphase_len == 0) {
        /* basic.rs:418-423 asserts */
        set_err("kaiser multirate: interp, decim and half_polyphase_len "
                "must be greater than 0");
        return 0;
    }
    if (interp == 1 && decim == 1) { /* :424-426 */
        if (out && cap >= 1) out[0] = 1.0f;
        return 1;
    }
    const size_t band = interp == 1 ? decim : interp; /* :427-430 */
    if (half_polyphase_len > ((size_t)1 << 28) / band) {
        set_err("kaiser multirate: more than 2^29 taps");
        return 0;
    }
    const size_t num_taps = 2 * half_polyphase_len * band;
    if (!out || cap < num_taps) return num_taps;
    const double beta = fsdr_kaiser_beta(max_ripple);
    /* window scaled by interp for unit gain (:433-437) */
    std::vector<double> win(num_taps + 1), taps(num_taps + 1);
    fsdr_kaiser_window(num_taps + 1, beta, win.data());
    for (double& w : win) w = (double)interp * w;
    const double omega_c = 1.0 / (2.0 * (double)std::max(interp, decim));
    firdes_lowpass_h(omega_c, win.data(), num_taps + 1, taps.data());
    for (size_t i = 0; i < num_taps; i++) /* :440 truncate */
        out[i] = (float)taps[i];
    return num_taps;
}

extern "C" int fsdr_firdes_lowpass_kaiser_n_f32(size_t n_taps, double beta,
                                                double cutoff, float* out) {
    if (!out || n_taps < 2) return FSDR_ERR_INVALID;
    std::vector<double> win(n_taps), taps(n_taps);
    fsdr_kaiser_window(n_taps, beta, win.data());
    firdes_lowpass_h(cutoff, win.data(), n_taps, taps.data());
    for (size_t i = 0; i < n_taps; i++) out[i] = (float)taps[i];
    return FSDR_OK;
}

extern "C" int fsdr_rotator_dev(const void* d_in, void* d_out, size_t n,
                                float phase_incr_angle, float phase0_re,
                                float phase0_im, void* stream,
                                float* final_re, float* final_im) {
    REQUIRE_GPU();
    if (n > 0) {
        hipLaunchKernelGGL(k_rotator, dim3(grid_for((long long)n, 256)),
                           dim3(256), 0, (hipStream_t)stream,
                           (const float2*)d_in, (float2*)d_out, (long long)n,
                           phase_incr_angle, phase0_re, phase0_im);
        HIP_TRY(hipGetLastError());
    }
    if (final_re && final_im) { /* closed-form final phase (f64) */
        double a = (double)phase_incr_angle * (double)n;
        double c = cos(a), s = sin(a);
        *final_re = (float)(c * phase0_re - s * phase0_im);
        *final_im = (float)(c * phase0_im + s * phase0_re);
    }
    return FSDR_OK;
}

/* ================= WLAN rx front end (config 5) ======================= *
 * Host-side state machines mirroring examples/wlan/src/sync_short.rs
 * (:2-5 constants THRESHOLD 0.56 / MIN_GAP 480 / MAX_SAMPLES 540*80;
 * :92-150 Search/Found/Copy loop) and sync_long.rs (:3 SEARCH_WINDOW
 * 320; :18-50 Correlator::sync; :136-178 Sync/Copy). The sequential
 * state machines run on the host exactly like the reference blocks; the
 * SyncLong correlator's 320 64-tap complex dot products run on the GPU
 * (k_fir_ccf32 through an internal filter handle). */

/* the 802.11a long-training correlator taps — sync_long.rs:188-253 */
static const float2 WLAN_LONG[64] = {
    {1.3868f, -0.0000f},  {-0.0455f, 1.0679f},  {0.3528f, 0.9865f},
    {0.8594f, -0.7348f},  {0.1874f, -0.2475f},  {0.5309f, 0.7784f},
    {-1.0218f, 0.4897f},  {-0.3401f, 0.9423f},  {0.8657f, 0.2298f},
    {0.4734f, -0.0362f},  {0.0088f, 1.0207f},   {-1.2142f, 0.4205f},
    {0.2172f, 0.5195f},   {0.5207f, 0.1326f},   {-0.1995f, -1.4259f},
    {1.0583f, 0.0363f},   {0.5547f, 0.5547f},   {0.3277f, -0.8728f},
    {-0.5077f, -0.3488f}, {-1.1650f, -0.5789f}, {0.7297f, -0.8197f},
    {0.6173f, -0.1253f},  {-0.5353f, -0.7214f}, {-0.5011f, 0.1935f},
    {-0.3110f, 1.3392f},  {-1.0818f, 0.1470f},  {-1.1300f, 0.1820f},
    {0.6663f, 0.6571f},   {-0.0249f, -0.4773f}, {-0.8155f, -1.0218f},
    {0.8140f, -0.9396f},  {0.1090f, -0.8662f},  {-1.3868f, -0.0000f},
    {0.1090f, 0.8662f},   {0.8140f, 0.9396f},   {-0.8155f, 1.0218f},
    {-0.0249f, 0.4773f},  {0.6663f, -0.6571f},  {-1.1300f, -0.1820f},
    {-1.0818f, -0.1470f}, {-0.3110f, -1.3392f}, {-0.5011f, -0.1935f},
    {-0.5353f, 0.7214f},  {0.6173f, 0.1253f},   {0.7297f, 0.8197f},
    {-1.1650f, 0.5789f},  {-0.5077f, 0.3488f},  {0.3277f, 0.8728f},
    {0.5547f, -0.5547f},  {1.0583f, -0.0363f},  {-0.1995f, 1.4259f},
    {0.5207f, -0.1326f},  {0.2172f, -0.5195f},  {-1.2142f, -0.4205f},
    {0.0088f, -1.0207f},  {0.4734f, 0.0362f},   {0.8657f, -0.2298f},
    {-0.3401f, -0.9423f}, {-1.0218f, -0.4897f}, {0.5309f, -0.7784f},
    {0.1874f, 0.2475f},   {0.8594f, 0.7348f},   {0.3528f, -0.9865f},
    {-0.0455f, -1.0679f},
};

#define WLAN_THRESHOLD 0.56f
#define WLAN_MIN_GAP 480
#define WLAN_MAX_SAMPLES (540 * 80)
#define WLAN_SEARCH_WINDOW 320

struct fsdr_wlan_rx {
    /* SyncShort state (sync_short.rs:8-12,34) */
    int ss_state = 0;      /* 0 Search, 1 Found, 2 Copy */
    size_t ss_copied = 0;
    float ss_foffset = 0.f;
    bool ss_above = false;
    bool ss_pending = false;
    float ss_pending_freq = 0.f;
    /* SyncLong GPU correlator, its input window and its output */
    fsdr_filter* corr = nullptr;
    dev_buf win, cor;
    ~fsdr_wlan_rx() { delete corr; }
};

extern "C" fsdr_wlan_rx* fsdr_wlan_rx_create(void) {
    if (!have_gpu()) { set_err("no HIP device"); return nullptr; }
    fsdr_wlan_rx* rx = new fsdr_wlan_rx();
    /* FirCC computes y[i] = sum_t in[i+t]*taps[63-t]; the reference
     * correlator is sum_k in[i+k]*LONG[k] (sync_long.rs:21-27), so the
     * filter taps are LONG reversed. */
    fsdr_cf32 rev[64];
    for (int i = 0; i < 64; i++) {
        rev[i].re = WLAN_LONG[63 - i].x;
        rev[i].im = WLAN_LONG[63 - i].y;
    }
    rx->corr = fsdr_fir_ccf32_create(rev, 64);
    if (!rx->corr ||
        rx->win.ensure((WLAN_SEARCH_WINDOW + 64) * sizeof(float2)) !=
            hipSuccess ||
        rx->cor.ensure(WLAN_SEARCH_WINDOW * sizeof(float2)) != hipSuccess) {
        set_err("wlan rx alloc failed");
        delete rx;
        return nullptr;
    }
    return rx;
}

extern "C" void fsdr_wlan_rx_destroy(fsdr_wlan_rx* rx) {
    if (rx) delete rx;
}

/* SyncShort actor loop (sync_short.rs:92-150) over aligned spans of the
 * delayed signal, the 48-sample complex autocorrelation average, and
 * the correlation metric. Emits the frame-sample stream plus
 * "wifi_start" tags (output index + coarse freq offset). Returns
 * produced; *consumed_out = input samples consumed (== n unless out or
 * tag capacity limited). */
extern "C" size_t fsdr_wlan_sync_short_run(
    fsdr_wlan_rx* rx, const fsdr_cf32* sig, const fsdr_cf32* abs48,
    const float* cor, size_t n, fsdr_cf32* out, size_t out_cap,
    size_t* tag_idx, float* tag_freq, size_t tag_cap, size_t* n_tags,
    size_t* consumed_out) {
    size_t i = 0, o = 0, nt = 0;
    while (i < n && o < out_cap) {
        switch (rx->ss_state) {
            case 0: /* Search */
                if (cor[i] > WLAN_THRESHOLD) rx->ss_state = 1;
                break;
            case 1: /* Found */
                if (cor[i] > WLAN_THRESHOLD) {
                    float fo = -atan2f(abs48[i].im, abs48[i].re) / 16.0f;
                    rx->ss_state = 2;
                    rx->ss_copied = 0;
                    rx->ss_foffset = fo;
                    rx->ss_above = false;
                    rx->ss_pending = true;
                    rx->ss_pending_freq = fo;
                } else {
                    rx->ss_state = 0;
                }
                break;
            case 2: { /* Copy(n_copied, f_offset, last_above) */
                if (cor[i] > WLAN_THRESHOLD) {
                    if (rx->ss_above && rx->ss_copied > WLAN_MIN_GAP) {
                        /* resync (sync_short.rs:110-117) */
                        float fo =
                            -atan2f(abs48[i].im, abs48[i].re) / 16.0f;
                        rx->ss_copied = 0;
                        rx->ss_foffset = fo;
                        rx->ss_above = false;
                        rx->ss_pending = true;
                        rx->ss_pending_freq = fo;
                        i++;
                        continue;
                    }
                    rx->ss_above = true;
                } else {
                    rx->ss_above = false;
                }
                if (rx->ss_copied == 0 && rx->ss_pending) {
                    if (nt < tag_cap) {
                        tag_idx[nt] = o;
                        tag_freq[nt] = rx->ss_pending_freq;
                        nt++;
                    }
                    rx->ss_pending = false;
                }
                float ang = rx->ss_foffset * (float)rx->ss_copied;
                float s, c;
                __builtin_sincosf(ang, &s, &c);
                out[o].re = sig[i].re * c - sig[i].im * s;
                out[o].im = sig[i].re * s + sig[i].im * c;
                o++;
                if (rx->ss_copied + 1 == WLAN_MAX_SAMPLES)
                    rx->ss_state = 0;
                else
                    rx->ss_copied++;
                break;
            }
        }
        i++;
    }
    if (n_tags) *n_tags = nt;
    if (consumed_out) *consumed_out = i;
    return o;
}

/* SyncLong over a tagged span (sync_long.rs:96-185): for each
 * "wifi_start" tag, run the GPU 64-tap correlator over the
 * SEARCH_WINDOW, pick the top-2 |cor|^2 peaks (stable order, pair
 * sorted by index — :38-48), copy 128 samples rotated by the fine freq
 * offset, then strip the 16-sample CP from each 80-sample symbol until
 * the next tag (leftover < 80 dropped, like the reference's m<80
 * consume). Needs a GPU. Returns symbols*64 (+128/frame) samples
 * written; frame_off[f] = the correlator offset chosen for frame f. */
extern "C" size_t fsdr_wlan_sync_long_run(
    fsdr_wlan_rx* rx, const fsdr_cf32* in, size_t n,
    const size_t* tag_idx, const float* tag_freq, size_t num_tags,
    fsdr_cf32* out, size_t out_cap, size_t* frame_off, float* frame_freq,
    size_t frame_cap, size_t* num_frames) {
    (void)tag_freq;
    size_t o = 0, nf = 0;
    for (size_t t = 0; t < num_tags; t++) {
        size_t T = tag_idx[t];
        size_t T2 = (t + 1 < num_tags) ? tag_idx[t + 1] : n;
        if (T2 - T < WLAN_SEARCH_WINDOW + 128) continue; /* :143 */
        /* Correlator::sync on in[T .. T+SEARCH_WINDOW+63] (GPU) */
        if (hipMemcpy(rx->win.ptr, in + T,
                      (WLAN_SEARCH_WINDOW + 63) * sizeof(float2),
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_err("wlan h2d failed");
            break;
        }
        fsdr_filter_result r;
        if (fsdr_filter_dev(rx->corr, rx->win.ptr, WLAN_SEARCH_WINDOW + 63,
                            rx->cor.ptr, WLAN_SEARCH_WINDOW, nullptr,
                            &r) != FSDR_OK)
            break;
        (void)hipStreamSynchronize(nullptr);
        float2 corv[WLAN_SEARCH_WINDOW];
        if (hipMemcpy(corv, rx->cor.ptr,
                      WLAN_SEARCH_WINDOW * sizeof(float2),
                      hipMemcpyDeviceToHost) != hipSuccess)
            break;
        /* top-2 by |cor|^2, stable (first occurrence wins ties), pair
         * ordered by index (:38-44) */
        int i0 = 0, i1 = -1;
        float m0 = -1.f, m1 = -1.f;
        for (int i = 0; i < WLAN_SEARCH_WINDOW; i++) {
            float m = corv[i].x * corv[i].x + corv[i].y * corv[i].y;
            if (m > m0) {
                m1 = m0; i1 = i0;
                m0 = m; i0 = i;
            } else if (m > m1) {
                m1 = m; i1 = i;
            }
        }
        int first = i0 < i1 ? i0 : i1;
        int second = i0 < i1 ? i1 : i0;
        /* freq = arg(cor[first] * conj(cor[second])) / 64  (:46-48) */
        float2 a = corv[first], b = corv[second];
        float pr = a.x * b.x + a.y * b.y;
        float pi = a.y * b.x - a.x * b.y;
        float freq = atan2f(pi, pr) / 64.0f;
        size_t off = (size_t)first;
        if (o + 128 > out_cap) break;
        for (int i = 0; i < 128; i++) { /* :147-151 */
            float s, c;
            __builtin_sincosf((float)i * freq, &s, &c);
            fsdr_cf32 x = in[T + off + i];
            out[o + i].re = x.re * c - x.im * s;
            out[o + i].im = x.re * s + x.im * c;
        }
        o += 128;
        if (nf < frame_cap) {
            if (frame_off) frame_off[nf] = off;
            if (frame_freq) frame_freq[nf] = freq;
            nf++;
        }
        /* Copy state (:162-177): 80-sample symbols -> 64 samples each */
        size_t cur = T + off + 128;
        size_t n_copied = 0;
        while (cur + 80 <= T2 && o + 64 <= out_cap) {
            for (int k = 0; k < 64; k++) {
                float ang =
                    (float)(n_copied * 80 + 128 + 16 + (size_t)k) * freq;
                float s, c;
                __builtin_sincosf(ang, &s, &c);
                fsdr_cf32 x = in[cur + 16 + k];
                out[o + k].re = x.re * c - x.im * s;
                out[o + k].im = x.re * s + x.im * c;
            }
            o += 64;
            cur += 80;
            n_copied++;
        }
    }
    if (num_frames) *num_frames = nf;
    return o;
}

/* ================= WLAN frame decoder ==================================
 * The bit work of examples/wlan Decoder (src/decoder.rs:47-115) and
 * ViterbiDecoder (src/viterbi_decoder.rs) for a batch of frames: one frame
 * per wavefront, one trellis state per lane ("WLAN frame
 * decoder"). No LDS, no block barrier: the symbols of 32 trellis steps are
 * two wave-wide ballots held in scalar registers, the traceback ring is
 * three VGPRs per lane read with v_readlane, and a wave that runs out of
 * frames simply leaves. */

#define WLAN_DEC_WAVES 4   /* frames (waves) per block */
#define WLAN_MAX_PSDU 1528 /* lib.rs:43-44 */
#define WLAN_MAX_SYM 511   /* lib.rs:45 */
#define WLAN_SRC_ERASURE (-1)
#define WLAN_SRC_PAST (-2)
#define WLAN_CRC_RESIDUE 558161692u /* decoder.rs:89 */

/* mcs 0..7: Bpsk_1_2, Bpsk_3_4, Qpsk_1_2, Qpsk_3_4, Qam16_1_2, Qam16_3_4,
 * Qam64_2_3, Qam64_3_4 (lib.rs:223-282). punct: 0 rate 1/2 (no
 * puncturing), 1 rate 2/3 (pattern 1110), 2 rate 3/4 (pattern 111001). */
__host__ __device__ static inline unsigned wlan_n_bpsc(unsigned mcs) {
    return mcs < 2 ? 1 : mcs < 4 ? 2 : mcs < 6 ? 4 : 6;
}
__host__ __device__ static inline unsigned wlan_punct(unsigned mcs) {
    return (mcs & 1) ? 2 : mcs == 6 ? 1 : 0;
}
__host__ __device__ static inline unsigned wlan_n_dbps(unsigned mcs) {
    const unsigned n_cbps = 48 * wlan_n_bpsc(mcs), p = wlan_punct(mcs);
    return p == 0 ? n_cbps / 2 : p == 1 ? n_cbps / 3 * 2 : n_cbps / 4 * 3;
}
/* viterbi_decoder.rs:68-78 */
__host__ __device__ static inline unsigned wlan_n_traceback(unsigned mcs) {
    const unsigned p = wlan_punct(mcs);
    return p == 0 ? 5 : p == 1 ? 9 : 10;
}
/* lib.rs:324-343 */
__host__ __device__ static inline unsigned wlan_n_symbols(unsigned mcs,
                                                          size_t psdu) {
    const size_t bits = 16 + 8 * psdu + 6, d = wlan_n_dbps(mcs);
    return (unsigned)((bits + d - 1) / d);
}

/* Where depunctured value p of a frame comes from: 8 * (index byte) + bit,
 * WLAN_SRC_ERASURE for a punctured position (the reference's value 2), or
 * WLAN_SRC_PAST beyond the frame's own bits (reads 0, the tail rule). This
 * is decoder.rs:69-76 (bits), :47-67 (deinterleave) and viterbi_decoder.rs:
 * 81-107 (depuncture) composed and inverted: pattern position -> coded bit
 * c; c -> symbol and deinterleaved position d; d -> received position k by
 * the interleaver's two permutations (the inverses of second[] and first[]);
 * k -> byte k / n_bpsc, bit k % n_bpsc. n_coded = n_symbols * n_cbps is a
 * multiple of the pattern's ones, so the depunctured length is whole
 * patterns. */
template <unsigned BPSC, unsigned PUNCT>
__host__ __device__ static inline int wlan_src_tpl(unsigned p,
                                                   unsigned n_coded) {
    constexpr unsigned N = 48 * BPSC, S = BPSC >= 2 ? BPSC / 2 : 1;
    unsigned c;
    if (PUNCT == 0) {
        if (p >= n_coded) return WLAN_SRC_PAST;
        c = p;
    } else if (PUNCT == 1) {
        const unsigned q = p >> 2, r = p & 3;
        if (q * 3 >= n_coded) return WLAN_SRC_PAST;
        if (r == 3) return WLAN_SRC_ERASURE;
        c = q * 3 + r;
    } else {
        const unsigned q = p / 6, r = p - q * 6;
        if (q * 4 >= n_coded) return WLAN_SRC_PAST;
        if (r == 3 || r == 4) return WLAN_SRC_ERASURE;
        c = q * 4 + (r == 5 ? 3 : r);
    }
    const unsigned sym = c / N, d = c - sym * N;
    const unsigned i = (N / 16) * (d & 15) + (d >> 4);
    const unsigned k = S * (i / S) + (i + N - 16 * i / N) % S;
    return (int)(((sym * 48 + k / BPSC) << 3) | (k % BPSC));
}

__host__ __device__ static inline int wlan_src(unsigned bpsc, unsigned punct,
                                               unsigned p, unsigned n_coded) {
#define WLAN_SRC_P(B_)                                                       \
    (punct == 0   ? wlan_src_tpl<B_, 0>(p, n_coded)                          \
     : punct == 1 ? wlan_src_tpl<B_, 1>(p, n_coded)                          \
                  : wlan_src_tpl<B_, 2>(p, n_coded))
    switch (bpsc) {
        case 1: return WLAN_SRC_P(1);
        case 2: return WLAN_SRC_P(2);
        case 4: return WLAN_SRC_P(4);
        default: return WLAN_SRC_P(6);
    }
#undef WLAN_SRC_P
}

/* byte-wise table of the reflected CRC-32 (polynomial 0xedb88320) */
struct WlanCrcTab {
    unsigned v[256];
    constexpr WlanCrcTab() : v() {
        for (unsigned i = 0; i < 256; i++) {
            unsigned c = i;
            for (int b = 0; b < 8; b++)
                c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1)));
            v[i] = c;
        }
    }
};
__constant__ WlanCrcTab wlan_crc_tab = WlanCrcTab();

struct WlanFrameDesc {
    unsigned mcs, psdu, n_sym, n_bytes; /* n_bytes = ceil(n_data_bits / 8) */
    unsigned long long sym_off, out_off, dec_off;
};

/* max over the wave, in every lane's view a scalar: four rotate-and-max
 * steps leave each row of 16 lanes holding its maximum, the four rows are
 * read out with v_readlane. */
__device__ __forceinline__ int wlan_wave_max(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));
    return max(max(__builtin_amdgcn_readlane(v, 0),
                   __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32),
                   __builtin_amdgcn_readlane(v, 48)));
}

/* One frame per wave; frames strided over the grid's waves.
 *
 * Lane L is trellis state L, which is also the reference's storage index:
 * its new entry comes from old entries j = L >> 1 and j + 32 with
 * branch-table index j (viterbi_decoder.rs:184-189, 240-258). Per step a
 * lane first forms the reference's shifted path byte for its OWN old
 * entry -- the 16-bit pair shift hands bit 7 of an even entry to bit 0 of
 * its odd neighbour (:216-228), and the upper half adds 1 mod 256
 * (:233-235) -- packs it with its metric, and two ds_bpermute fetch the
 * pair for j and j + 32. The decision is the reference's strict m0 > m1.
 *
 * Depunctured values are numbered p' = p + 4, so that output group g (6
 * steps for g = 0, then 8 each, :504-523) owns p' in [16 g, 16 g + 16). A
 * chunk is 64 values, one per lane: every lane maps its p to an index
 * byte and bit (wlan_src), loads it, and two ballots turn the chunk into
 * a 64-bit value mask and a 64-bit erasure mask, both wave-uniform. The
 * next chunk's bytes are loaded before the current chunk's 32 steps run.
 *
 * The traceback ring (ppresult, :435-484) is the last 10 path bytes of
 * each lane in r0..r2, newest in the low byte of r0; the walk reads them
 * with v_readlane at the wave-uniform state. Descrambling and the CRC-32
 * run per output byte on wave-uniform values; bytes are collected one per
 * lane and stored 64 at a time. */
__global__ __launch_bounds__(64 * WLAN_DEC_WAVES) void k_wlan_decode(
    const unsigned char* __restrict__ syms,
    const WlanFrameDesc* __restrict__ frames, int n_frames,
    unsigned char* __restrict__ out, unsigned char* __restrict__ dec,
    unsigned char* __restrict__ crc_ok) {
    const unsigned lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool odd = lane & 1, upper = lane >= 32;
    const unsigned bt0 = __popc((lane & ~1u) & 0x6d) & 1; /* :56-60 */
    const unsigned bt1 = __popc((lane & ~1u) & 0x4f) & 1;
    const int addr_lo = (int)(lane >> 1) * 4, addr_hi = addr_lo + 32 * 4;

    for (int f = (int)blockIdx.x * WLAN_DEC_WAVES + wave; f < n_frames;
         f += (int)gridDim.x * WLAN_DEC_WAVES) {
        const WlanFrameDesc fr = frames[f];
        const unsigned bpsc = wlan_n_bpsc(fr.mcs), punct = wlan_punct(fr.mcs);
        const unsigned T = wlan_n_traceback(fr.mcs);
        const unsigned n_coded = fr.n_sym * 48 * bpsc;
        const unsigned G = T + fr.n_bytes; /* get_output calls */
        const unsigned char* s = syms + fr.sym_off;

        int metric = 0;
        unsigned path = 0, r0 = 0, r1 = 0, r2 = 0;
        unsigned state = 0, crc = 0xffffffffu; /* wave-uniform */
        unsigned obyte = 0, dbyte = 0;         /* this lane's pending bytes */

        auto fetch = [&](unsigned ch, int& src) -> unsigned {
            const unsigned pp = ch * 64 + lane;
            src = pp < 4 ? WLAN_SRC_PAST
                         : wlan_src(bpsc, punct, pp - 4, n_coded);
            return src >= 0 ? s[src >> 3] : 0u;
        };
        int src;
        unsigned byte = fetch(0, src);

        for (unsigned ch = 0; ch * 4 < G; ch++) {
            const unsigned long long vm = __ballot((byte >> (src & 7)) & 1);
            const unsigned long long em = __ballot(src == WLAN_SRC_ERASURE);
            byte = fetch(ch + 1, src); /* nothing is loaded past the frame */
            const unsigned g_end = min(4u, G - ch * 4);
            for (unsigned gg = 0; gg < g_end; gg++) {
                const unsigned g = ch * 4 + gg;
                const unsigned v16 = (unsigned)(vm >> (16 * gg)) & 0xffffu;
                const unsigned e16 = (unsigned)(em >> (16 * gg)) & 0xffffu;
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    if (t < 2 && g == 0) continue; /* p' 0..3 do not exist */
                    const unsigned s0 = (v16 >> (2 * t)) & 1;
                    const unsigned s1 = (v16 >> (2 * t + 1)) & 1;
                    const unsigned w0 = ~(e16 >> (2 * t)) & 1;
                    const unsigned w1 = ~(e16 >> (2 * t + 1)) & 1;
                    /* shifted path of this lane's old entry */
                    const unsigned up = (unsigned)__builtin_amdgcn_update_dpp(
                        0, (int)path, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
                    unsigned sh = (path << 1) | (odd ? (up >> 7) & 1 : 0u);
                    sh = (sh + (upper ? 1u : 0u)) & 0xffu;
                    const int pack = metric | (int)(sh << 16);
                    const int lo = __builtin_amdgcn_ds_bpermute(addr_lo, pack);
                    const int hi = __builtin_amdgcn_ds_bpermute(addr_hi, pack);
                    /* branch metrics, :161-189: an erased symbol drops out */
                    const int bm = (int)((w0 & (bt0 ^ s0)) + (w1 & (bt1 ^ s1)));
                    const int mx = (int)(w0 + w1);
                    const int add_lo = odd ? bm : mx - bm;
                    const int m_lo = (lo & 0xffff) + add_lo;
                    const int m_hi = (hi & 0xffff) + (mx - add_lo);
                    const bool d = m_lo > m_hi; /* strict, :198-199 */
                    metric = d ? m_lo : m_hi;
                    path = (unsigned)(d ? lo : hi) >> 16;
                }

                /* viterbi_get_output_generic, :435-484 */
                r2 = (r2 << 8) | (r1 >> 24);
                r1 = (r1 << 8) | (r0 >> 24);
                r0 = (r0 << 8) | path;
                const int kmax = wlan_wave_max((metric << 6) | (int)(63 - lane));
                const int mmin = -wlan_wave_max(-metric);
                int best = 63 - (kmax & 63); /* first strict maximum */
#pragma unroll
                for (unsigned k = 0; k < 9; k++) {
                    if (k < T - 1) {
                        const unsigned w = (unsigned)__builtin_amdgcn_readlane(
                            (int)(k < 4 ? r0 : k < 8 ? r1 : r2), best);
                        best = (int)(((w >> (8 * (k & 3))) & 0xffu) >> 2);
                    }
                }
                /* entry T-1 back: byte 0 of r1 (T 5), byte 0 or 1 of r2 */
                const unsigned c =
                    ((unsigned)__builtin_amdgcn_readlane((int)(T == 5 ? r1 : r2),
                                                         best) >>
                     (T == 10 ? 8 : 0)) & 0xffu;
                path = 0;
                metric -= mmin;

                if (g < T) continue; /* the first T bytes are dropped */
                const unsigned n = g - T, slot = n & 63;
                if (lane == slot) dbyte = c;
                if (dec && (slot == 63 || n == fr.n_bytes - 1) && lane <= slot)
                    dec[fr.dec_off + (n - slot) + lane] = (unsigned char)dbyte;
                if (n >= fr.psdu + 2) continue;

                /* descramble, decoder.rs:92-115: decoded bit 8n+b is bit
                 * 7-b of c; bits 0..6 are the scrambler state itself */
                unsigned ob;
                if (n == 0) {
                    state = c >> 1;
                    const unsigned fb = ((state >> 6) ^ (state >> 3)) & 1;
                    ob = state | ((fb ^ (c & 1)) << 7);
                    state = ((state << 1) & 0x7e) | fb;
                } else {
                    /* four feedback bits at a time: x6^x3, x5^x2, x4^x1,
                     * x3^x0 of the state x read only bits the four shifts
                     * have not replaced, and end up as its low nibble */
                    const unsigned t0 = ((state >> 3) ^ state) & 0xf;
                    state = ((state << 4) & 0x70) | t0;
                    const unsigned t1 = ((state >> 3) ^ state) & 0xf;
                    state = ((state << 4) & 0x70) | t1;
                    ob = __brev(c ^ ((t0 << 4) | t1)) >> 24;
                }
                if (n >= 2) /* reflected CRC-32 over out_bytes[2..] */
                    crc = wlan_crc_tab.v[(crc ^ ob) & 0xff] ^ (crc >> 8);
                if (lane == slot) obyte = ob;
                if ((slot == 63 || n == fr.psdu + 1) && lane <= slot)
                    out[fr.out_off + (n - slot) + lane] = (unsigned char)obyte;
            }
        }
        if (lane == 0) crc_ok[f] = (unsigned char)(~crc == WLAN_CRC_RESIDUE);
    }
}

/* ---- WLAN frame decoder: host-only helpers and the handle -------------- */

static bool wlan_mcs_ok(unsigned mcs) {
    if (mcs > 7) {
        set_err("wlan: mcs must be in [0,7]");
        return false;
    }
    return true;
}

extern "C" int fsdr_wlan_frame_param(unsigned mcs, size_t psdu_size,
                                     size_t* n_symbols, size_t* n_data_bits,
                                     size_t* n_pad) {
    if (!wlan_mcs_ok(mcs)) return FSDR_ERR_INVALID;
    if (psdu_size > 4095) { /* the SIGNAL length field has 12 bits */
        set_err("wlan: psdu_size must be at most 4095");
        return FSDR_ERR_INVALID;
    }
    const size_t ns = wlan_n_symbols(mcs, psdu_size);
    const size_t nd = ns * wlan_n_dbps(mcs);
    if (n_symbols) *n_symbols = ns;
    if (n_data_bits) *n_data_bits = nd;
    if (n_pad) *n_pad = nd - (16 + 8 * psdu_size + 6);
    return FSDR_OK;
}

extern "C" int fsdr_wlan_deinterleave_map(unsigned mcs, uint16_t* out) {
    if (!wlan_mcs_ok(mcs) || !out) {
        if (mcs <= 7) set_err("wlan: null argument");
        return FSDR_ERR_INVALID;
    }
    /* read off the kernel's own map, without puncturing: deinterleaved
     * position d of symbol 0 comes from received bit k */
    const unsigned bpsc = wlan_n_bpsc(mcs), n_cbps = 48 * bpsc;
    for (unsigned d = 0; d < n_cbps; d++) {
        const int src = wlan_src(bpsc, 0, d, n_cbps);
        out[(unsigned)(src >> 3) * bpsc + (unsigned)(src & 7)] = (uint16_t)d;
    }
    return FSDR_OK;
}

extern "C" int fsdr_wlan_depuncture_map(unsigned mcs, size_t n_symbols,
                                        size_t first, size_t count,
                                        int32_t* out) {
    if (!wlan_mcs_ok(mcs)) return FSDR_ERR_INVALID;
    if (n_symbols > WLAN_MAX_SYM || first + count > ((size_t)1 << 24) ||
        (count && !out)) {
        set_err("wlan: depuncture map range");
        return FSDR_ERR_INVALID;
    }
    const unsigned bpsc = wlan_n_bpsc(mcs);
    for (size_t i = 0; i < count; i++)
        out[i] = wlan_src(bpsc, wlan_punct(mcs), (unsigned)(first + i),
                          (unsigned)n_symbols * 48 * bpsc);
    return FSDR_OK;
}

/* frame_equalizer.rs:142-174 on a word whose bit i is decoded bit i: parity
 * over bits 0..16 against bit 17, rate in bits 0..3 (8..15 are the known
 * ones: mcs 6, 4, 2, 0, 7, 5, 3, 1), length in bits 5..16. Shared by
 * fsdr_wlan_signal_field and k_wlan_eq_data. */
__host__ __device__ static inline bool wlan_signal_parse(unsigned bits,
                                                         unsigned* mcs,
                                                         unsigned* psdu) {
    unsigned parity = bits & 0x1ffffu;
    parity ^= parity >> 16;
    parity ^= parity >> 8;
    parity ^= parity >> 4;
    parity ^= parity >> 2;
    parity ^= parity >> 1;
    const unsigned r = bits & 0xfu;
    if ((parity & 1u) != ((bits >> 17) & 1u) || r < 8) return false;
    *mcs = (0x13570246u >> (4 * (r - 8))) & 0xfu;
    *psdu = (bits >> 5) & 0xfffu;
    return true;
}

extern "C" int fsdr_wlan_signal_field(const uint8_t* bits24, int* found,
                                      unsigned* mcs, size_t* psdu_size) {
    if (!bits24 || !found) {
        set_err("wlan: null argument");
        return FSDR_ERR_INVALID;
    }
    unsigned bits = 0, m = 0, p = 0;
    for (int i = 0; i < 18; i++) bits |= (unsigned)(bits24[i] > 0) << i;
    *found = wlan_signal_parse(bits, &m, &p) ? 1 : 0;
    if (!*found) return FSDR_OK;
    if (mcs) *mcs = m;
    if (psdu_size) *psdu_size = p;
    return FSDR_OK;
}

struct fsdr_wlan_decoder {
    dev_buf desc; /* the frame descriptors the kernel reads */
    /* pinned image of them; `uploaded` fires once the copy has read it */
    WlanFrameDesc* pinned = nullptr;
    size_t pinned_cap = 0;
    hipEvent_t uploaded = nullptr;
    /* staging of fsdr_wlan_decode_host */
    dev_buf st_syms, st_out, st_dec, st_crc;
    ~fsdr_wlan_decoder() {
        if (uploaded) {
            (void)hipEventSynchronize(uploaded);
            (void)hipEventDestroy(uploaded);
        }
        if (pinned) (void)hipHostFree(pinned);
    }
};

extern "C" fsdr_wlan_decoder* fsdr_wlan_decoder_create(void) {
    return new fsdr_wlan_decoder(); /* buffers come with the first call */
}

extern "C" void fsdr_wlan_decoder_destroy(fsdr_wlan_decoder* dec) {
    delete dec;
}

/* Validates the batch; fills the three span lengths when asked. */
static int wlan_check_frames(const fsdr_wlan_decoder* dec,
                             const fsdr_wlan_frame* frames, size_t n_frames,
                             size_t* sym_span, size_t* out_span,
                             size_t* dec_span) {
    if (!dec) {
        set_err("wlan: null decoder");
        return FSDR_ERR_INVALID;
    }
    if (n_frames && !frames) {
        set_err("wlan: null frame array");
        return FSDR_ERR_INVALID;
    }
    if (n_frames > (size_t)1 << 30) {
        set_err("wlan: too many frames");
        return FSDR_ERR_INVALID;
    }
    size_t ss = 0, os = 0, ds = 0;
    for (size_t i = 0; i < n_frames; i++) {
        const fsdr_wlan_frame& f = frames[i];
        if (!wlan_mcs_ok(f.mcs)) return FSDR_ERR_INVALID;
        if (f.psdu_size > WLAN_MAX_PSDU) {
            set_err("wlan: psdu_size must be at most 1528");
            return FSDR_ERR_INVALID;
        }
        const size_t ns = wlan_n_symbols(f.mcs, f.psdu_size);
        if (ns > WLAN_MAX_SYM) {
            set_err("wlan: frame has more than 511 symbols");
            return FSDR_ERR_INVALID;
        }
        ss = std::max(ss, f.sym_off + 48 * ns);
        os = std::max(os, f.out_off + f.psdu_size + 2);
        ds = std::max(ds, f.dec_off + (ns * wlan_n_dbps(f.mcs) + 7) / 8);
    }
    if (sym_span) *sym_span = ss;
    if (out_span) *out_span = os;
    if (dec_span) *dec_span = ds;
    return FSDR_OK;
}

static int wlan_launch(fsdr_wlan_decoder* dec, const void* d_syms,
                       const fsdr_wlan_frame* frames, size_t n_frames,
                       void* d_out, void* d_dec, void* d_crc,
                       hipStream_t st) {
    if (!dec->uploaded)
        HIP_TRY(hipEventCreateWithFlags(&dec->uploaded,
                                        hipEventDisableTiming));
    /* the previous call's copy may still be reading the pinned image */
    HIP_TRY(hipEventSynchronize(dec->uploaded));
    if (dec->pinned_cap < n_frames) {
        if (dec->pinned) HIP_TRY(hipHostFree(dec->pinned));
        dec->pinned = nullptr;
        dec->pinned_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&dec->pinned,
                              n_frames * sizeof(WlanFrameDesc)));
        dec->pinned_cap = n_frames;
    }
    for (size_t i = 0; i < n_frames; i++) {
        const fsdr_wlan_frame& f = frames[i];
        WlanFrameDesc& d = dec->pinned[i];
        d.mcs = f.mcs;
        d.psdu = (unsigned)f.psdu_size;
        d.n_sym = wlan_n_symbols(f.mcs, f.psdu_size);
        d.n_bytes = (d.n_sym * wlan_n_dbps(f.mcs) + 7) / 8;
        d.sym_off = f.sym_off;
        d.out_off = f.out_off;
        d.dec_off = f.dec_off;
    }
    HIP_TRY(dec->desc.ensure(n_frames * sizeof(WlanFrameDesc)));
    HIP_TRY(hipMemcpyAsync(dec->desc.ptr, dec->pinned,
                           n_frames * sizeof(WlanFrameDesc),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(dec->uploaded, st));
    const long long blocks =
        ((long long)n_frames + WLAN_DEC_WAVES - 1) / WLAN_DEC_WAVES;
    const int grid = (int)std::min<long long>(blocks, grid_cap(256 * 8));
    hipLaunchKernelGGL(k_wlan_decode, dim3(grid), dim3(64 * WLAN_DEC_WAVES),
                       0, st, (const unsigned char*)d_syms,
                       dec->desc.as<const WlanFrameDesc>(), (int)n_frames,
                       (unsigned char*)d_out, (unsigned char*)d_dec,
                       (unsigned char*)d_crc);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

extern "C" int fsdr_wlan_decode_dev(fsdr_wlan_decoder* dec,
                                    const void* d_syms,
                                    const fsdr_wlan_frame* frames,
                                    size_t n_frames, void* d_out_bytes,
                                    void* d_dec_bytes, void* d_crc_ok,
                                    void* stream) {
    int rc = wlan_check_frames(dec, frames, n_frames, nullptr, nullptr,
                               nullptr);
    if (rc) return rc;
    if (n_frames == 0) return FSDR_OK;
    if (!d_syms || !d_out_bytes || !d_crc_ok) {
        set_err("wlan: null device pointer");
        return FSDR_ERR_INVALID;
    }
    REQUIRE_GPU();
    return wlan_launch(dec, d_syms, frames, n_frames, d_out_bytes,
                       d_dec_bytes, d_crc_ok, (hipStream_t)stream);
}

extern "C" int fsdr_wlan_decode_host(fsdr_wlan_decoder* dec,
                                     const uint8_t* syms,
                                     const fsdr_wlan_frame* frames,
                                     size_t n_frames, uint8_t* out_bytes,
                                     uint8_t* dec_bytes, uint8_t* crc_ok) {
    size_t ss = 0, os = 0, ds = 0;
    int rc = wlan_check_frames(dec, frames, n_frames, &ss, &os, &ds);
    if (rc) return rc;
    if (n_frames == 0) return FSDR_OK;
    if (!syms || !out_bytes || !crc_ok) {
        set_err("wlan: null argument");
        return FSDR_ERR_INVALID;
    }
    REQUIRE_GPU();
    HIP_TRY(dec->st_syms.ensure(ss));
    HIP_TRY(dec->st_out.ensure(os));
    HIP_TRY(dec->st_crc.ensure(n_frames));
    if (dec_bytes) HIP_TRY(dec->st_dec.ensure(ds));
    HIP_TRY(hipMemcpy(dec->st_syms.ptr, syms, ss, hipMemcpyHostToDevice));
    rc = wlan_launch(dec, dec->st_syms.ptr, frames, n_frames, dec->st_out.ptr,
                     dec_bytes ? dec->st_dec.ptr : nullptr, dec->st_crc.ptr,
                     nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    /* only the frames' own ranges reach the caller's spans */
    std::vector<uint8_t> h(std::max(os, ds));
    HIP_TRY(hipMemcpy(h.data(), dec->st_out.ptr, os, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_frames; i++)
        memcpy(out_bytes + frames[i].out_off, h.data() + frames[i].out_off,
               frames[i].psdu_size + 2);
    if (dec_bytes) {
        HIP_TRY(hipMemcpy(h.data(), dec->st_dec.ptr, ds,
                          hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n_frames; i++) {
            const fsdr_wlan_frame& f = frames[i];
            const size_t nb = (wlan_n_symbols(f.mcs, f.psdu_size) *
                                   (size_t)wlan_n_dbps(f.mcs) + 7) / 8;
            memcpy(dec_bytes + f.dec_off, h.data() + f.dec_off, nb);
        }
    }
    HIP_TRY(hipMemcpy(crc_ok, dec->st_crc.ptr, n_frames,
                      hipMemcpyDeviceToHost));
    return FSDR_OK;
}

/* ================= WLAN frame equalizer ================================
 * examples/wlan FrameEqualizer (src/frame_equalizer.rs) for a batch of
 * frames: channel estimate from the two long-training symbols, common pilot
 * phase of every symbol, SIGNAL field, equalize and demap ("WLAN
 * frame equalizer"). Lane = carrier: a 64-bin symbol is one wavefront. Three
 * launches on the caller's stream: k_wlan_eq_head (one wave per frame),
 * k_wlan_decode over the SIGNAL fields at (mcs 0, psdu 0), k_wlan_eq_data
 * (waves over the data symbols). No LDS, no barrier. */

#define WLAN_EQ_WAVES 4      /* waves per block, both kernels */
#define WLAN_EQ_SLOT_BLOCKS 8 /* blocks sharing one frame's data symbols */
#define WLAN_EQ_MAX_SYM 1366  /* FrameParam::new at Bpsk_1_2, psdu 4095 */

/* lib.rs:365: 1 - 2*bit of the x^7+x^4+1 scrambler seeded with all ones,
 * 127 entries; bit i of {lo, hi} is set where the entry is -1. */
struct WlanPolarity {
    unsigned long long lo, hi;
    constexpr WlanPolarity() : lo(0), hi(0) {
        unsigned state = 0x7f;
        for (int i = 0; i < 127; i++) {
            const unsigned fb = ((state >> 6) ^ (state >> 3)) & 1;
            state = ((state << 1) & 0x7e) | fb;
            if (fb) (i < 64 ? lo : hi) |= 1ull << (i & 63);
        }
    }
};
__host__ __device__ static inline float wlan_polarity(unsigned i) {
    constexpr WlanPolarity p = WlanPolarity();
    i %= 127;
    return (((i < 64 ? p.lo : p.hi) >> (i & 63)) & 1) ? -1.0f : 1.0f;
}

/* lib.rs:495, the frequency-domain long-training sequence L(-26..26) on
 * carriers 6..58: half its sign (the reference divides by LONG + LONG), 0
 * on the other carriers. */
__host__ __device__ static inline float wlan_long_half(unsigned m) {
    /* '-' entries of "++--++-+-++++++--++-+-++++0+--++-+-+-----++--+-+-++++",
     * bit m - 6 */
    constexpr unsigned long long neg =
        (1ull << 2) | (1ull << 3) | (1ull << 6) | (1ull << 8) |
        (1ull << 15) | (1ull << 16) | (1ull << 19) | (1ull << 21) |
        (1ull << 28) | (1ull << 29) | (1ull << 32) | (1ull << 34) |
        (1ull << 36) | (1ull << 37) | (1ull << 38) | (1ull << 39) |
        (1ull << 40) | (1ull << 43) | (1ull << 44) | (1ull << 46) |
        (1ull << 48);
    if (m < 6 || m > 58 || m == 32) return 0.0f;
    return ((neg >> (m - 6)) & 1) ? -0.5f : 0.5f;
}

/* frame_equalizer.rs:55-57: output position of carrier m, -1 for the
 * guards, DC and the four pilots. */
__host__ __device__ static inline int wlan_carrier_out(unsigned m) {
    if (m < 6 || m > 58 || m == 11 || m == 25 || m == 32 || m == 39 ||
        m == 53)
        return -1;
    return (int)m - 6 - (m > 11) - (m > 25) - (m > 32) - (m > 39) - (m > 53);
}

/* Modulation::demap, lib.rs:177-218, strict comparisons; the thresholds are
 * f32 products of the f32 constants. NaN gives 0. */
__host__ __device__ static inline unsigned wlan_demap(unsigned bpsc, float re,
                                                      float im) {
    if (bpsc == 1) return re > 0.0f;
    if (bpsc == 2) return 2u * (im > 0.0f) + (re > 0.0f);
    const float are = fabsf(re), aim = fabsf(im);
    if (bpsc == 4) {
        const float l = 0.6324555320336759f;
        return (unsigned)(re > 0.0f) | (unsigned)(are < l) << 1 |
               (unsigned)(im > 0.0f) << 2 | (unsigned)(aim < l) << 3;
    }
    const float l = 0.1543033499620919f;
    const float l2 = 2.0f * l, l4 = 4.0f * l, l6 = 6.0f * l;
    return (unsigned)(re > 0.0f) | (unsigned)(are < l4) << 1 |
           (unsigned)(are < l6 && are > l2) << 2 |
           (unsigned)(im > 0.0f) << 3 | (unsigned)(aim < l4) << 4 |
           (unsigned)(aim < l6 && aim > l2) << 5;
}

/* num-complex's division: (a * conj(b)) / |b|^2, componentwise. */
__device__ __forceinline__ float2 wlan_cdiv(float2 a, float2 b) {
    const float n = b.x * b.x + b.y * b.y;
    return make_float2((a.x * b.x + a.y * b.y) / n,
                       (a.y * b.x - a.x * b.y) / n);
}

__device__ __forceinline__ float2 wlan_eq_lane(float2 v, int l) {
    return make_float2(
        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), l)),
        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), l)));
}

/* frame_equalizer.rs:241-246: training symbols, s11 - s25 + s39 + s53 */
__device__ __forceinline__ float2 wlan_pilots_training(float2 s) {
    const float2 a = wlan_eq_lane(s, 11), b = wlan_eq_lane(s, 25),
                 c = wlan_eq_lane(s, 39), d = wlan_eq_lane(s, 53);
    return make_float2(((a.x - b.x) + c.x) + d.x, ((a.y - b.y) + c.y) + d.y);
}

/* :249-254, :260-265: SIGNAL and data, p*s11 + p*s39 + p*s25 - p*s53 */
__device__ __forceinline__ float2 wlan_pilots_data(float2 s, float p) {
    const float2 a = wlan_eq_lane(s, 11), b = wlan_eq_lane(s, 39),
                 c = wlan_eq_lane(s, 25), d = wlan_eq_lane(s, 53);
    return make_float2(((a.x * p + b.x * p) + c.x * p) + d.x * -p,
                       ((a.y * p + b.y * p) + c.y * p) + d.y * -p);
}

/* s * from_polar(1, -arg(sum)); the angle is wave-uniform */
__device__ __forceinline__ float2 wlan_derotate(float2 s, float2 sum) {
    const float beta = atan2f(sum.y, sum.x);
    float sn, cs;
    sincosf(-beta, &sn, &cs);
    return make_float2(s.x * cs - s.y * sn, s.x * sn + s.y * cs);
}

__device__ __forceinline__ float wlan_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct WlanEqDesc {
    unsigned long long sym_off, idx_off, eq_off;
    unsigned n_avail, pad;
};

/* One wave per frame; frames strided over the grid's waves. Lane m loads
 * FFT bin (m + 32) % 64 of the three leading symbols (:234-237), so the
 * shift costs nothing. Writes h (64 values), snr and the 48 BPSK indices of
 * the SIGNAL symbol to the workspace; a frame with fewer than 3 symbols
 * gets indices 0 (its SIGNAL field is then decoded but never looked at),
 * one with fewer than 2 also h = 0 and snr = 0. */
__global__ __launch_bounds__(64 * WLAN_EQ_WAVES) void k_wlan_eq_head(
    const float2* __restrict__ spec, const WlanEqDesc* __restrict__ frames,
    int n_frames, float2* __restrict__ h_ws, float* __restrict__ snr_ws,
    unsigned char* __restrict__ sig_ws) {
    const unsigned lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned bin = (lane + 32) & 63;
    const float lh = wlan_long_half(lane);
    const int o = wlan_carrier_out(lane);

    for (int f = (int)blockIdx.x * WLAN_EQ_WAVES + wave; f < n_frames;
         f += (int)gridDim.x * WLAN_EQ_WAVES) {
        const WlanEqDesc fr = frames[f];
        const float2* s = spec + fr.sym_off;
        float2 h = make_float2(0.0f, 0.0f);
        float snr = 0.0f;
        unsigned idx = 0;
        if (fr.n_avail >= 2) {
            float2 a = s[bin], b = s[64 + bin];
            float2 c = make_float2(0.0f, 0.0f);
            if (fr.n_avail >= 3) c = s[128 + bin];
            a = wlan_derotate(a, wlan_pilots_training(a));
            b = wlan_derotate(b, wlan_pilots_training(b));
            /* sync2, :31-46 */
            float nz = 0.0f, sg = 0.0f;
            h = a;
            if (lh != 0.0f) {
                const float2 d = make_float2(a.x - b.x, a.y - b.y);
                const float2 e = make_float2(a.x + b.x, a.y + b.y);
                nz = d.x * d.x + d.y * d.y;
                sg = e.x * e.x + e.y * e.y;
                h = make_float2(e.x * lh, e.y * lh);
            }
            nz = wlan_wave_sum(nz);
            sg = wlan_wave_sum(sg);
            snr = 10.0f * log10f(sg / nz / 2.0f);
            if (fr.n_avail >= 3) {
                c = wlan_derotate(c, wlan_pilots_data(c, wlan_polarity(0)));
                const float2 z = wlan_cdiv(c, h);
                idx = wlan_demap(1, z.x, z.y);
            }
        }
        h_ws[(size_t)f * 64 + lane] = h;
        if (lane == 0) snr_ws[f] = snr;
        if (o >= 0) sig_ws[(size_t)f * 48 + o] = (unsigned char)idx;
    }
}

/* A frame is shared by `fblocks` consecutive blocks of the 1-D grid, so
 * that the blocks running side by side read one contiguous stretch of the
 * spectra; (frame, block of the frame) pairs are strided over the grid and
 * a frame's data symbols over its fblocks * WLAN_EQ_WAVES waves. Every
 * wave parses its frame's three raw SIGNAL bytes (wave-uniform; MSB =
 * earlier bit) and leaves unless the field was found and it has a symbol
 * below n_copied; h is loaded once per wave. The frame's first wave writes the info record, found or not. */
__global__ __launch_bounds__(64 * WLAN_EQ_WAVES) void k_wlan_eq_data(
    const float2* __restrict__ spec, const WlanEqDesc* __restrict__ frames,
    int n_frames, const float2* __restrict__ h_ws,
    const float* __restrict__ snr_ws, const unsigned* __restrict__ dec_ws,
    unsigned char* __restrict__ idx, float2* __restrict__ eq,
    fsdr_wlan_eq_info* __restrict__ info, unsigned fblocks) {
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave =
        (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned bin = (lane + 32) & 63;
    const int o = wlan_carrier_out(lane);
    const unsigned stride = fblocks * WLAN_EQ_WAVES;
    const long long total = (long long)n_frames * fblocks;

    for (long long vb = blockIdx.x; vb < total; vb += gridDim.x) {
        const int f = (int)(vb / fblocks);
        const unsigned slot0 =
            (unsigned)(vb - (long long)f * fblocks) * WLAN_EQ_WAVES + wave;
        const WlanEqDesc fr = frames[f];
        const unsigned have = fr.n_avail >= 3 ? fr.n_avail - 3 : 0;
        if (slot0 != 0 && slot0 >= have) continue;
        unsigned mcs = 0, psdu = 0, n_sym = 0;
        bool found = false;
        if (fr.n_avail >= 3) {
            const unsigned w = dec_ws[f]; /* bytes 0..2, little endian */
            const unsigned bits = (__brev(w & 0xffu) >> 24) |
                                  (__brev(w & 0xff00u) >> 8) |
                                  (__brev(w & 0xff0000u) << 8);
            found = wlan_signal_parse(bits, &mcs, &psdu);
        }
        if (found) n_sym = wlan_n_symbols(mcs, psdu);
        const unsigned n_copied = min(n_sym, have);
        if (slot0 == 0 && lane == 0) {
            fsdr_wlan_eq_info r;
            r.found = found;
            r.mcs = found ? mcs : 0;
            r.psdu_size = found ? psdu : 0;
            r.n_symbols = n_sym;
            r.n_copied = n_copied;
            r.snr_db = snr_ws[f];
            info[f] = r;
        }
        if (slot0 >= n_copied) continue;
        const unsigned bpsc = wlan_n_bpsc(mcs);
        const float2 h = h_ws[(size_t)f * 64 + lane];
        const float2* s = spec + fr.sym_off + 3 * 64;
        float2 next = s[(size_t)slot0 * 64 + bin];
        for (unsigned slot = slot0; slot < n_copied; slot += stride) {
            float2 v = next; /* the next symbol is loaded before this one's
                                arithmetic */
            if (slot + stride < n_copied)
                next = s[(size_t)(slot + stride) * 64 + bin];
            v = wlan_derotate(v, wlan_pilots_data(v, wlan_polarity(slot + 1)));
            const float2 z = wlan_cdiv(v, h);
            if (o >= 0) {
                const size_t at = (size_t)slot * 48 + (unsigned)o;
                idx[fr.idx_off + at] =
                    (unsigned char)wlan_demap(bpsc, z.x, z.y);
                if (eq) eq[fr.eq_off + at] = z;
            }
        }
    }
}

/* ---- WLAN frame equalizer: host-only helpers and the handle ------------ */

extern "C" int fsdr_wlan_demap(unsigned mcs, const fsdr_cf32* z, size_t n,
                               uint8_t* out) {
    if (!wlan_mcs_ok(mcs)) return FSDR_ERR_INVALID;
    if (n && (!z || !out)) {
        set_err("wlan: null argument");
        return FSDR_ERR_INVALID;
    }
    const unsigned bpsc = wlan_n_bpsc(mcs);
    for (size_t i = 0; i < n; i++)
        out[i] = (uint8_t)wlan_demap(bpsc, z[i].re, z[i].im);
    return FSDR_OK;
}

extern "C" int fsdr_wlan_pilot_polarity(size_t first, size_t count,
                                        int8_t* out) {
    if (count && !out) {
        set_err("wlan: null argument");
        return FSDR_ERR_INVALID;
    }
    for (size_t i = 0; i < count; i++)
        out[i] = (int8_t)wlan_polarity((unsigned)((first + i) % 127));
    return FSDR_OK;
}

extern "C" int fsdr_wlan_carrier_map(int8_t out[64]) {
    if (!out) {
        set_err("wlan: null argument");
        return FSDR_ERR_INVALID;
    }
    for (unsigned m = 0; m < 64; m++) out[m] = (int8_t)wlan_carrier_out(m);
    return FSDR_OK;
}

struct fsdr_wlan_equalizer {
    fsdr_wlan_decoder* dec = nullptr; /* the SIGNAL fields' own decoder */
    dev_buf desc;                     /* the frame descriptors */
    /* per frame: h (64 cf32), snr, 48 SIGNAL indices, and the SIGNAL
     * decode's 3 raw bytes (one word), 2 out bytes and crc byte */
    dev_buf ws_h, ws_snr, ws_sig, ws_dec, ws_out, ws_crc;
    WlanEqDesc* pinned = nullptr;
    size_t pinned_cap = 0;
    hipEvent_t uploaded = nullptr;
    /* staging of fsdr_wlan_equalize_host */
    dev_buf st_spec, st_idx, st_eq, st_info;
    ~fsdr_wlan_equalizer() {
        if (uploaded) {
            (void)hipEventSynchronize(uploaded);
            (void)hipEventDestroy(uploaded);
        }
        if (pinned) (void)hipHostFree(pinned);
        delete dec;
    }
};

extern "C" fsdr_wlan_equalizer* fsdr_wlan_equalizer_create(void) {
    fsdr_wlan_equalizer* eq = new fsdr_wlan_equalizer();
    eq->dec = fsdr_wlan_decoder_create(); /* buffers come with the first call */
    return eq;
}

extern "C" void fsdr_wlan_equalizer_destroy(fsdr_wlan_equalizer* eq) {
    delete eq;
}

static unsigned wlan_eq_slots(const fsdr_wlan_eq_frame& f) {
    return f.n_avail >= 3 ? f.n_avail - 3 : 0;
}

static int wlan_eq_check(const fsdr_wlan_equalizer* eq,
                         const fsdr_wlan_eq_frame* frames, size_t n_frames) {
    if (!eq) {
        set_err("wlan: null equalizer");
        return FSDR_ERR_INVALID;
    }
    if (n_frames && !frames) {
        set_err("wlan: null frame array");
        return FSDR_ERR_INVALID;
    }
    if (n_frames > (size_t)1 << 30) {
        set_err("wlan: too many frames");
        return FSDR_ERR_INVALID;
    }
    return FSDR_OK;
}

static int wlan_eq_launch(fsdr_wlan_equalizer* eq, const void* d_spec,
                          const fsdr_wlan_eq_frame* frames, size_t n_frames,
                          void* d_idx, void* d_eq, void* d_info,
                          hipStream_t st) {
    if (!eq->uploaded)
        HIP_TRY(hipEventCreateWithFlags(&eq->uploaded,
                                        hipEventDisableTiming));
    /* the previous call's copy may still be reading the pinned image */
    HIP_TRY(hipEventSynchronize(eq->uploaded));
    if (eq->pinned_cap < n_frames) {
        if (eq->pinned) HIP_TRY(hipHostFree(eq->pinned));
        eq->pinned = nullptr;
        eq->pinned_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&eq->pinned,
                              n_frames * sizeof(WlanEqDesc)));
        eq->pinned_cap = n_frames;
    }
    unsigned max_slots = 1; /* every frame needs the wave of slot 0 */
    std::vector<fsdr_wlan_frame> sig(n_frames);
    for (size_t i = 0; i < n_frames; i++) {
        const fsdr_wlan_eq_frame& f = frames[i];
        WlanEqDesc& d = eq->pinned[i];
        d.sym_off = f.sym_off;
        d.idx_off = f.idx_off;
        d.eq_off = f.eq_off;
        d.n_avail = f.n_avail;
        d.pad = 0;
        max_slots = std::max(
            max_slots, std::min<unsigned>(wlan_eq_slots(f), WLAN_EQ_MAX_SYM));
        sig[i].mcs = 0;
        sig[i].psdu_size = 0;
        sig[i].sym_off = 48 * i;
        sig[i].out_off = 2 * i;
        sig[i].dec_off = 4 * i;
    }
    HIP_TRY(eq->desc.ensure(n_frames * sizeof(WlanEqDesc)));
    HIP_TRY(eq->ws_h.ensure(n_frames * 64 * sizeof(float2)));
    HIP_TRY(eq->ws_snr.ensure(n_frames * sizeof(float)));
    HIP_TRY(eq->ws_sig.ensure(n_frames * 48));
    HIP_TRY(eq->ws_dec.ensure(n_frames * 4));
    HIP_TRY(eq->ws_out.ensure(n_frames * 2));
    HIP_TRY(eq->ws_crc.ensure(n_frames));
    HIP_TRY(hipMemcpyAsync(eq->desc.ptr, eq->pinned,
                           n_frames * sizeof(WlanEqDesc),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(eq->uploaded, st));

    const long long hblocks =
        ((long long)n_frames + WLAN_EQ_WAVES - 1) / WLAN_EQ_WAVES;
    const int hgrid = (int)std::min<long long>(hblocks, grid_cap(256 * 8));
    hipLaunchKernelGGL(k_wlan_eq_head, dim3(hgrid), dim3(64 * WLAN_EQ_WAVES),
                       0, st, (const float2*)d_spec,
                       eq->desc.as<const WlanEqDesc>(), (int)n_frames,
                       eq->ws_h.as<float2>(), eq->ws_snr.as<float>(),
                       eq->ws_sig.as<unsigned char>());
    HIP_TRY(hipGetLastError());

    int rc = fsdr_wlan_decode_dev(eq->dec, eq->ws_sig.ptr, sig.data(),
                                  n_frames, eq->ws_out.ptr, eq->ws_dec.ptr,
                                  eq->ws_crc.ptr, st);
    if (rc) return rc;

    const unsigned fblocks = std::min<unsigned>(
        (max_slots + WLAN_EQ_WAVES - 1) / WLAN_EQ_WAVES, WLAN_EQ_SLOT_BLOCKS);
    const int dgrid = (int)std::min<long long>(
        (long long)n_frames * fblocks, grid_cap(1 << 20));
    hipLaunchKernelGGL(k_wlan_eq_data, dim3(dgrid),
                       dim3(64 * WLAN_EQ_WAVES), 0, st,
                       (const float2*)d_spec, eq->desc.as<const WlanEqDesc>(),
                       (int)n_frames, eq->ws_h.as<const float2>(),
                       eq->ws_snr.as<const float>(),
                       eq->ws_dec.as<const unsigned>(),
                       (unsigned char*)d_idx, (float2*)d_eq,
                       (fsdr_wlan_eq_info*)d_info, fblocks);
    HIP_TRY(hipGetLastError());
    return FSDR_OK;
}

extern "C" int fsdr_wlan_equalize_dev(fsdr_wlan_equalizer* eq,
                                      const void* d_spec,
                                      const fsdr_wlan_eq_frame* frames,
                                      size_t n_frames, void* d_idx,
                                      void* d_eq, void* d_info,
                                      void* stream) {
    int rc = wlan_eq_check(eq, frames, n_frames);
    if (rc) return rc;
    if (n_frames == 0) return FSDR_OK;
    if (!d_spec || !d_idx || !d_info) {
        set_err("wlan: null device pointer");
        return FSDR_ERR_INVALID;
    }
    REQUIRE_GPU();
    return wlan_eq_launch(eq, d_spec, frames, n_frames, d_idx, d_eq, d_info,
                          (hipStream_t)stream);
}

extern "C" int fsdr_wlan_equalize_host(fsdr_wlan_equalizer* eq,
                                       const fsdr_cf32* spec,
                                       const fsdr_wlan_eq_frame* frames,
                                       size_t n_frames, uint8_t* idx,
                                       fsdr_cf32* eq_syms,
                                       fsdr_wlan_eq_info* info) {
    int rc = wlan_eq_check(eq, frames, n_frames);
    if (rc) return rc;
    if (n_frames == 0) return FSDR_OK;
    if (!spec || !idx || !info) {
        set_err("wlan: null argument");
        return FSDR_ERR_INVALID;
    }
    REQUIRE_GPU();
    size_t ss = 1, is = 1, es = 1;
    for (size_t i = 0; i < n_frames; i++) {
        const fsdr_wlan_eq_frame& f = frames[i];
        const size_t out = 48 * (size_t)wlan_eq_slots(f);
        ss = std::max(ss, f.sym_off + 64 * (size_t)f.n_avail);
        is = std::max(is, f.idx_off + out);
        es = std::max(es, f.eq_off + out);
    }
    HIP_TRY(eq->st_spec.ensure(ss * sizeof(float2)));
    HIP_TRY(eq->st_idx.ensure(is));
    HIP_TRY(eq->st_info.ensure(n_frames * sizeof(fsdr_wlan_eq_info)));
    if (eq_syms) HIP_TRY(eq->st_eq.ensure(es * sizeof(float2)));
    HIP_TRY(hipMemcpy(eq->st_spec.ptr, spec, ss * sizeof(float2),
                      hipMemcpyHostToDevice));
    rc = wlan_eq_launch(eq, eq->st_spec.ptr, frames, n_frames,
                        eq->st_idx.ptr, eq_syms ? eq->st_eq.ptr : nullptr,
                        eq->st_info.ptr, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(info, eq->st_info.ptr,
                      n_frames * sizeof(fsdr_wlan_eq_info),
                      hipMemcpyDeviceToHost));
    /* only what the frames' info records say was written reaches the
     * caller's spans */
    std::vector<uint8_t> hi(is);
    HIP_TRY(hipMemcpy(hi.data(), eq->st_idx.ptr, is, hipMemcpyDeviceToHost));
    std::vector<fsdr_cf32> he;
    if (eq_syms) {
        he.resize(es);
        HIP_TRY(hipMemcpy(he.data(), eq->st_eq.ptr, es * sizeof(float2),
                          hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < n_frames; i++) {
        const size_t n = 48 * (size_t)info[i].n_copied;
        memcpy(idx + frames[i].idx_off, hi.data() + frames[i].idx_off, n);
        if (eq_syms)
            memcpy(eq_syms + frames[i].eq_off, he.data() + frames[i].eq_off,
                   n * sizeof(fsdr_cf32));
    }
    return FSDR_OK;
}

/* ================= chain ============================================== */

struct fsdr_chain {
    fsdr_filter* fir1 = nullptr;
    fsdr_filter* fir2 = nullptr;
    fsdr_filter* fused = nullptr; /* combined-taps decimating FIR */
    fsdr_filter* fft = nullptr;
    dev_buf y1, y2;     /* unfused path: the stage outputs */
    dev_buf null_sink;  /* NullSink scratch when the caller passes NULL */
    ~fsdr_chain() { delete fir1; delete fir2; delete fused; delete fft; }
};

extern "C" fsdr_chain* fsdr_chain_create(const float* taps1, size_t n_taps1,
                                         const float* taps2, size_t n_taps2,
                                         size_t decim, size_t fft_len) {
    fsdr_chain* c = new fsdr_chain();
    c->fir1 = fsdr_fir_cf32_create(taps1, n_taps1);
    c->fir2 = fsdr_decim_fir_cf32_create(decim, taps2, n_taps2);
    c->fft = fsdr_fft_cf32_create(fft_len, 0, 0, nullptr);
    /* Algebraic fusion (default on, FSDR_CHAIN_FUSED=0 for the two-stage
     * path): Fir(h1) then DecimatingFir(D, h2) is one DecimatingFir(D, g)
     * with g = h1 (*) h2 (composition of LTI filters; combined taps in
     * f64). Output count is identical: (n+1-(T1+T2-1))/D == the composed
     * two-stage count. Parity vs the two-stage oracle is covered by the
     * chain tests (rel l2 1e-4). Cuts chain arithmetic from
     * (T1*4 + T2) to ~(T1+T2)*1 flops per input sample and removes the
     * y1 HBM round trip (30 -> ~12 B/sample). */
    if (env_on("FSDR_CHAIN_FUSED")) {
        size_t tg = n_taps1 + n_taps2 - 1;
        std::vector<double> g(tg, 0.0);
        for (size_t a = 0; a < n_taps1; a++)
            for (size_t b = 0; b < n_taps2; b++)
                g[a + b] += (double)taps1[a] * (double)taps2[b];
        std::vector<float> gf(tg);
        for (size_t i = 0; i < tg; i++) gf[i] = (float)g[i];
        c->fused = fsdr_decim_fir_cf32_create(decim, gf.data(), tg);
    }
    if (!c->fir1 || !c->fir2 || !c->fft) {
        delete c;
        return nullptr;
    }
    return c;
}

extern "C" int fsdr_chain_variant(const fsdr_chain* c, int* fused_kk_mfma) {
    if (!c) { set_err("null chain"); return FSDR_ERR_INVALID; }
    if (fused_kk_mfma) *fused_kk_mfma = c->fused ? c->fused->fir.kk_mfma : 0;
    return FSDR_OK;
}

extern "C" void fsdr_chain_destroy(fsdr_chain* c) {
    if (c) delete c;
}

extern "C" int fsdr_chain_run_dev(fsdr_chain* c, const void* d_in,
                                  size_t n_in, void* d_out, size_t out_cap,
                                  void* d_mag, size_t mag_cap, void* stream,
                                  size_t* consumed, size_t* produced) {
    REQUIRE_GPU();
    if (!c) { set_err("null chain"); return FSDR_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    const size_t nt1 = c->fir1->fir.n_taps, nt2 = c->fir2->fir.n_taps;
    const size_t D = c->fir2->fir.decim, L = c->fft->fft.len;
    size_t y1 = sat_sub(n_in + 1, nt1);
    size_t y2 = sat_sub(y1 + 1, nt2) / D;
    size_t frames = y2 / L;
    if (d_out && out_cap < frames * L) frames = out_cap / L;
    if (d_mag && mag_cap < frames * L) frames = mag_cap / L;
    size_t prod = frames * L;
    if (consumed) *consumed = prod * D; /* chain-input samples per frame set */
    if (produced) *produced = prod;
    if (frames == 0) return FSDR_OK;
    int rc;
    const bool fft_fusable =
        (L == 64 || L == 128 || L == 256 || L == 512 || L == 1024);
    if (c->fused && fft_fusable && c->fused->fir.kk_mfma &&
        !c->fft->fft.inverse && !c->fft->fft.shift &&
        c->fft->fft.norm == 0.f && env_on("FSDR_CHAIN_FFTFUSE")) {
        /* single kernel: fused decimating filter + in-block per-frame
         * FFT (+ optional |X|^2) — y2 never touches HBM. Tile = 1024
         * decimated outputs = 1024/L frames. */
        const int KK = c->fused->fir.kk_mfma;
        const float* mtaps = c->fused->fir.mtaps.as<float>();
        const float2* twid = c->fft->fft.twid.as<float2>();
        long long tiles = ((long long)prod + MDFIR_TILE - 1) / MDFIR_TILE;
        /* ~2 tiles/block at 2^26: best measured */
        long long cap = grid_cap(8192);
        int grid = (int)std::min<long long>(tiles, cap);
        /* a launch of one of the family's kernels at this filter's K */
        auto chain_launch = [&](auto&& launch) -> int {
            if (!tpl_dispatch(decim4_mfma_ks{}, KK, launch)) {
                set_err("bad chain mfma K");
                return FSDR_ERR_INVALID;
            }
            HIP_TRY(hipGetLastError());
            return FSDR_OK;
        };
        float2* spec_dst = (float2*)d_out; /* null + mag-only: skip the
                                              discarded spectra write */
        if (!spec_dst && !d_mag) { /* NullSink scratch keeps work observable */
            HIP_TRY(c->null_sink.ensure((prod + 8) * sizeof(float2)));
            spec_dst = c->null_sink.as<float2>();
        }
        if (env_int("FSDR_CHAIN_BLOCK512", 0) != 0 && L == 1024 && KK == 80 &&
            prod % 2048 == 0) {
            long long tiles2 = (long long)prod / 2048;
            int grid2 = (int)std::min<long long>(tiles2, cap);
            using G2 = ChainGeom<80, 512, 2048>;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_decim4_fft_mfma2_tpl<80>),
                               dim3(grid2), dim3(G2::BLOCK),
                               G2::halves_bytes, st, (const float2*)d_in,
                               spec_dst, mtaps, (long long)prod,
                               (long long)n_in, twid, (float*)d_mag);
            HIP_TRY(hipGetLastError());
            return FSDR_OK;
        }
        /* software-pipelined FFT-in-MFMA-shadow variant: measured ~4%
         * faster than the ap kernel at fft_len 1024 (the serial FFT
         * issues inside the MFMA pipe shadow) — default for the
         * aligned 1024 case; FSDR_CHAIN_WS=0 disables. */
        if (env_on("FSDR_CHAIN_WS") && L == 1024 &&
            ((uintptr_t)d_in & 15u) == 0) {
            return chain_launch([&](auto K) {
                using G = ChainGeom<decltype(K)::value>;
                hipLaunchKernelGGL(
                    HIP_KERNEL_NAME(k_decim4_fft_mfma_ws_tpl<G::KKD>),
                    dim3(grid), dim3(G::BLOCK), G::ws_bytes, st,
                    (const float2*)d_in, spec_dst, mtaps, (long long)prod,
                    (long long)n_in, twid, (float*)d_mag);
            });
        }
        /* all-phase + aligned-group staging is the default (measured
         * ~2% faster: fewer barriers and half the staging-load
         * instructions; see profiles/pmc_sq_r02.txt). The ap kernel's
         * group staging needs a 16B-aligned input base — ring carry
         * offsets can be 8B-odd — so unaligned inputs (and
         * FSDR_CHAIN_ALLPHASE=0) take the 2-phase-halves kernel. */
        if (env_on("FSDR_CHAIN_ALLPHASE") && ((uintptr_t)d_in & 15u) == 0) {
            return chain_launch([&](auto K) {
                using G = ChainGeom<decltype(K)::value>;
                hipLaunchKernelGGL(
                    HIP_KERNEL_NAME(k_decim4_fft_mfma_ap_tpl<G::KKD>),
                    dim3(grid), dim3(G::BLOCK), G::ap_bytes, st,
                    (const float2*)d_in, spec_dst, mtaps, (long long)prod,
                    (long long)n_in, twid, (float*)d_mag, (int)L);
            });
        }
        if (env_int("FSDR_CHAIN_OCC8", 0) != 0 && KK == 80) {
            /* experiment: force 8 waves/SIMD occupancy (VGPR capped to
             * 64 by the compiler; some spill risk) */
            hipLaunchKernelGGL(
                HIP_KERNEL_NAME((k_decim4_fft_mfma_tpl<80, 8>)),
                dim3(grid), dim3(MDFIR_BLOCK), ChainGeom<80>::halves_bytes,
                st, (const float2*)d_in, spec_dst, mtaps, (long long)prod,
                (long long)n_in, twid, (float*)d_mag, (int)L, 0);
            HIP_TRY(hipGetLastError());
            return FSDR_OK;
        }
        const int stagger = env_int("FSDR_CHAIN_STAGGER", 0);
        return chain_launch([&](auto K) {
            using G = ChainGeom<decltype(K)::value>;
            hipLaunchKernelGGL(
                HIP_KERNEL_NAME(k_decim4_fft_mfma_tpl<G::KKD>), dim3(grid),
                dim3(G::BLOCK), G::halves_bytes, st, (const float2*)d_in,
                spec_dst, mtaps, (long long)prod, (long long)n_in, twid,
                (float*)d_mag, (int)L, stagger);
        });
    }
    HIP_TRY(c->y2.ensure((prod + 8) * sizeof(float2)));
    float2* out2 = (float2*)d_out;
    if (!out2) {
        HIP_TRY(c->null_sink.ensure((prod + 8) * sizeof(float2)));
        out2 = c->null_sink.as<float2>();
    }
    if (c->fused) {
        rc = launch_decim_cf32(c->fused, d_in, c->y2.ptr, prod, n_in, st);
        if (rc) return rc;
    } else {
        /* two-stage path: y1 covers the y2 window
         * (y2 needs y1[D-1 + (prod-1)*D + nt2-1]) */
        size_t y1_need = D - 1 + (prod - 1) * D + nt2;
        HIP_TRY(c->y1.ensure((y1_need + 8) * sizeof(float2)));
        rc = launch_fir_cf32(c->fir1, d_in, c->y1.ptr, y1_need, n_in, st);
        if (rc) return rc;
        rc = launch_decim_cf32(c->fir2, c->y1.ptr, c->y2.ptr, prod, y1_need,
                               st);
        if (rc) return rc;
    }
    rc = launch_fft(c->fft, c->y2.ptr, out2, frames, st, (float*)d_mag);
    return rc;
}

/* ================= ring (Slab-style) ================================== */

struct RingBuf {
    void* host = nullptr;  /* pinned; carry capacity + payload */
    void* dev = nullptr;
    size_t items = 0;      /* valid payload items (after the carry region) */
    hipEvent_t ev = nullptr;      /* copy (H2D [+ carry D2D]) complete */
    hipEvent_t free_ev = nullptr; /* consumer done reading dev */
};

/* Slab-exact streaming ring (slab.rs:110-152,369-399): the reader reports
 * how many items it CONSUMED and the ring carries the unconsumed
 * remainder in front of the next buffer — device-side (one small D2D on
 * the copy stream), so arbitrary chunk sizes stream exactly like the
 * reference block leaving leftovers in the slab buffer. `reserved`
 * is the carry CAPACITY (>= the consumer's worst-case leftover; for a
 * FIR chain that is taps-1 + decim*fft_len). */
struct fsdr_ring {
    size_t n_buffers, items_per_buffer, item_bytes, reserved;
    std::vector<RingBuf> bufs;
    std::deque<int> empty_q, full_q;
    int writer_cur = -1, reader_cur = -1;
    int prev_buf = -1;          /* released buffer still holding the tail */
    size_t prev_tail_off = 0;   /* byte offset of the tail in prev dev buf */
    size_t carry_items = 0;     /* items to prepend at the next acquire */
    size_t presented_items = 0; /* what the current reader_acquire returned */
    size_t presented_off = 0;   /* byte offset of presented span start */
    std::mutex mu;
    std::condition_variable cv;
    hipStream_t copy_stream = nullptr;
};

extern "C" fsdr_ring* fsdr_ring_create(size_t n_buffers,
                                       size_t items_per_buffer,
                                       size_t item_bytes,
                                       size_t reserved_items) {
    if (!have_gpu()) { set_err("no HIP device"); return nullptr; }
    if (n_buffers < 2 || items_per_buffer == 0 || item_bytes == 0) {
        set_err("invalid ring parameters");
        return nullptr;
    }
    fsdr_ring* r = new fsdr_ring();
    r->n_buffers = n_buffers;
    r->items_per_buffer = items_per_buffer;
    r->item_bytes = item_bytes;
    r->reserved = reserved_items;
    if (hipStreamCreate(&r->copy_stream) != hipSuccess) {
        set_err("stream create failed");
        delete r;
        return nullptr;
    }
    size_t bytes = (items_per_buffer + reserved_items) * item_bytes;
    for (size_t i = 0; i < n_buffers; i++) {
        RingBuf b;
        if (hipHostMalloc(&b.host, bytes) != hipSuccess ||
            hipMalloc(&b.dev, bytes) != hipSuccess ||
            hipEventCreate(&b.ev) != hipSuccess ||
            hipEventCreate(&b.free_ev) != hipSuccess) {
            set_err("ring buffer alloc failed");
            r->bufs.push_back(b);
            fsdr_ring_destroy(r);
            return nullptr;
        }
        r->bufs.push_back(b);
        r->empty_q.push_back((int)i);
    }
    return r;
}

extern "C" int fsdr_ring_writer_acquire(fsdr_ring* r, void** host_ptr,
                                        size_t* items) {
    if (!r) return FSDR_ERR_INVALID;
    std::unique_lock<std::mutex> lk(r->mu);
    r->cv.wait(lk, [&] { return !r->empty_q.empty(); });
    r->writer_cur = r->empty_q.front();
    r->empty_q.pop_front();
    RingBuf& b = r->bufs[r->writer_cur];
    *host_ptr = (char*)b.host + r->reserved * r->item_bytes;
    *items = r->items_per_buffer;
    return FSDR_OK;
}

extern "C" int fsdr_ring_writer_commit(fsdr_ring* r, size_t items) {
    if (!r || r->writer_cur < 0) return FSDR_ERR_INVALID;
    RingBuf& b = r->bufs[r->writer_cur];
    b.items = items;
    size_t off = r->reserved * r->item_bytes;
    /* don't overwrite dev while the consumer may still read it (a
     * never-recorded free_ev makes this wait a no-op) */
    HIP_TRY(hipStreamWaitEvent(r->copy_stream, b.free_ev, 0));
    HIP_TRY(hipMemcpyAsync((char*)b.dev + off, (char*)b.host + off,
                           items * r->item_bytes, hipMemcpyHostToDevice,
                           r->copy_stream));
    HIP_TRY(hipEventRecord(b.ev, r->copy_stream));
    {
        std::lock_guard<std::mutex> lk(r->mu);
        r->full_q.push_back(r->writer_cur);
        r->writer_cur = -1;
    }
    r->cv.notify_all();
    return FSDR_OK;
}

extern "C" int fsdr_ring_reader_acquire(fsdr_ring* r, void** dev_ptr,
                                        size_t* items) {
    if (!r) return FSDR_ERR_INVALID;
    std::unique_lock<std::mutex> lk(r->mu);
    r->cv.wait(lk, [&] { return !r->full_q.empty(); });
    r->reader_cur = r->full_q.front();
    r->full_q.pop_front();
    lk.unlock();
    RingBuf& b = r->bufs[r->reader_cur];
    size_t ib = r->item_bytes;
    size_t off = (r->reserved - r->carry_items) * ib;
    if (r->carry_items > 0 && r->prev_buf >= 0) {
        /* prepend the previous buffer's unconsumed tail (slab.rs:369-399),
         * after the consumer's reads of it have drained */
        RingBuf& pb = r->bufs[r->prev_buf];
        HIP_TRY(hipStreamWaitEvent(r->copy_stream, pb.free_ev, 0));
        HIP_TRY(hipMemcpyAsync((char*)b.dev + off,
                               (char*)pb.dev + r->prev_tail_off,
                               r->carry_items * ib,
                               hipMemcpyDeviceToDevice, r->copy_stream));
        HIP_TRY(hipEventRecord(b.ev, r->copy_stream));
    }
    if (r->prev_buf >= 0) {
        std::lock_guard<std::mutex> lk2(r->mu);
        r->empty_q.push_back(r->prev_buf);
        r->prev_buf = -1;
        r->cv.notify_all();
    }
    HIP_TRY(hipEventSynchronize(b.ev));
    r->presented_items = r->carry_items + b.items;
    r->presented_off = off;
    r->carry_items = 0;
    *dev_ptr = (char*)b.dev + off;
    *items = r->presented_items;
    return FSDR_OK;
}

/* Reader reports how much of the presented span it consumed; the
 * remainder is carried in front of the next buffer. `stream` is the
 * consumer's compute stream (the carry copy and buffer reuse are ordered
 * after work already enqueued there); NULL = default stream. */
extern "C" int fsdr_ring_reader_release_consumed(fsdr_ring* r,
                                                 size_t consumed,
                                                 void* stream) {
    if (!r || r->reader_cur < 0) return FSDR_ERR_INVALID;
    if (consumed > r->presented_items) {
        set_err("release_consumed: consumed > presented");
        return FSDR_ERR_INVALID;
    }
    size_t un = r->presented_items - consumed;
    if (un > r->reserved) {
        set_err("release_consumed: unconsumed tail exceeds ring "
                "reserved capacity");
        return FSDR_ERR_INVALID;
    }
    RingBuf& b = r->bufs[r->reader_cur];
    HIP_TRY(hipEventRecord(b.free_ev, (hipStream_t)stream));
    r->prev_buf = r->reader_cur;
    r->prev_tail_off = r->presented_off + consumed * r->item_bytes;
    r->carry_items = un;
    r->reader_cur = -1;
    return FSDR_OK;
}

extern "C" int fsdr_ring_reader_release(fsdr_ring* r) {
    return fsdr_ring_reader_release_consumed(r, r ? r->presented_items : 0,
                                             nullptr);
}

extern "C" void fsdr_ring_destroy(fsdr_ring* r) {
    if (!r) return;
    for (auto& b : r->bufs) {
        if (b.host) (void)hipHostFree(b.host);
        if (b.dev) (void)hipFree(b.dev);
        if (b.ev) (void)hipEventDestroy(b.ev);
        if (b.free_ev) (void)hipEventDestroy(b.free_ev);
    }
    if (r->copy_stream) (void)hipStreamDestroy(r->copy_stream);
    delete r;
}

/* ================= D2H return ring ==================================== *
 * The reverse direction of fsdr_ring: a device-side producer fills ring
 * buffers, async D2H on the ring's copy stream hands them to a pinned
 * host consumer — the vulkan d2h.rs Writer::submit / host Reader pair
 * (d2h.rs:66,247-268) with the circuit's empty-buffer recirculation
 * (d2h.rs:284-299). Writer: acquire(stream) (returns a device buffer;
 * the caller's stream is made to wait for that buffer's previous D2H)
 * -> fill on the stream -> commit(items, stream) (enqueues D2H after
 * the producer's work). Reader: acquire (waits for the copy; yields the
 * pinned host span) -> release (recycles). SPSC. */

struct fsdr_ring_d2h {
    size_t n_buffers, items_per_buffer, item_bytes;
    std::vector<RingBuf> bufs; /* free_ev = producer-done event */
    std::deque<int> empty_q, full_q;
    int writer_cur = -1, reader_cur = -1;
    std::mutex mu;
    std::condition_variable cv;
    hipStream_t copy_stream = nullptr;
};

extern "C" fsdr_ring_d2h* fsdr_ring_d2h_create(size_t n_buffers,
                                               size_t items_per_buffer,
                                               size_t item_bytes) {
    if (!have_gpu()) { set_err("no HIP device"); return nullptr; }
    if (n_buffers < 2 || items_per_buffer == 0 || item_bytes == 0) {
        set_err("invalid ring parameters");
        return nullptr;
    }
    fsdr_ring_d2h* r = new fsdr_ring_d2h();
    r->n_buffers = n_buffers;
    r->items_per_buffer = items_per_buffer;
    r->item_bytes = item_bytes;
    if (hipStreamCreate(&r->copy_stream) != hipSuccess) {
        set_err("stream create failed");
        delete r;
        return nullptr;
    }
    size_t bytes = items_per_buffer * item_bytes;
    for (size_t i = 0; i < n_buffers; i++) {
        RingBuf b;
        if (hipHostMalloc(&b.host, bytes) != hipSuccess ||
            hipMalloc(&b.dev, bytes) != hipSuccess ||
            hipEventCreate(&b.ev) != hipSuccess ||
            hipEventCreate(&b.free_ev) != hipSuccess) {
            set_err("ring buffer alloc failed");
            r->bufs.push_back(b);
            fsdr_ring_d2h_destroy(r);
            return nullptr;
        }
        r->bufs.push_back(b);
        r->empty_q.push_back((int)i);
    }
    return r;
}

extern "C" int fsdr_ring_d2h_writer_acquire(fsdr_ring_d2h* r,
                                            void** dev_ptr, size_t* items,
                                            void* stream) {
    if (!r) return FSDR_ERR_INVALID;
    std::unique_lock<std::mutex> lk(r->mu);
    r->cv.wait(lk, [&] { return !r->empty_q.empty(); });
    r->writer_cur = r->empty_q.front();
    r->empty_q.pop_front();
    lk.unlock();
    RingBuf& b = r->bufs[r->writer_cur];
    /* the producer must not overwrite dev before its previous D2H is
     * drained (no-op for a never-recorded event) */
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, b.ev, 0));
    *dev_ptr = b.dev;
    *items = r->items_per_buffer;
    return FSDR_OK;
}

extern "C" int fsdr_ring_d2h_writer_commit(fsdr_ring_d2h* r, size_t items,
                                           void* stream) {
    if (!r || r->writer_cur < 0) return FSDR_ERR_INVALID;
    RingBuf& b = r->bufs[r->writer_cur];
    b.items = items;
    HIP_TRY(hipEventRecord(b.free_ev, (hipStream_t)stream));
    HIP_TRY(hipStreamWaitEvent(r->copy_stream, b.free_ev, 0));
    HIP_TRY(hipMemcpyAsync(b.host, b.dev, items * r->item_bytes,
                           hipMemcpyDeviceToHost, r->copy_stream));
    HIP_TRY(hipEventRecord(b.ev, r->copy_stream));
    {
        std::lock_guard<std::mutex> lk(r->mu);
        r->full_q.push_back(r->writer_cur);
        r->writer_cur = -1;
    }
    r->cv.notify_all();
    return FSDR_OK;
}

extern "C" int fsdr_ring_d2h_reader_acquire(fsdr_ring_d2h* r,
                                            void** host_ptr,
                                            size_t* items) {
    if (!r) return FSDR_ERR_INVALID;
    std::unique_lock<std::mutex> lk(r->mu);
    r->cv.wait(lk, [&] { return !r->full_q.empty(); });
    r->reader_cur = r->full_q.front();
    r->full_q.pop_front();
    lk.unlock();
    RingBuf& b = r->bufs[r->reader_cur];
    HIP_TRY(hipEventSynchronize(b.ev));
    *host_ptr = b.host;
    *items = b.items;
    return FSDR_OK;
}

extern "C" int fsdr_ring_d2h_reader_release(fsdr_ring_d2h* r) {
    if (!r || r->reader_cur < 0) return FSDR_ERR_INVALID;
    {
        std::lock_guard<std::mutex> lk(r->mu);
        r->empty_q.push_back(r->reader_cur);
        r->reader_cur = -1;
    }
    r->cv.notify_all();
    return FSDR_OK;
}

extern "C" void fsdr_ring_d2h_destroy(fsdr_ring_d2h* r) {
    if (!r) return;
    for (auto& b : r->bufs) {
        if (b.host) (void)hipHostFree(b.host);
        if (b.dev) (void)hipFree(b.dev);
        if (b.ev) (void)hipEventDestroy(b.ev);
        if (b.free_ev) (void)hipEventDestroy(b.free_ev);
    }
    if (r->copy_stream) (void)hipStreamDestroy(r->copy_stream);
    delete r;
}
