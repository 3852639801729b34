// K17: reverberation with a drawn room impulse response (include/ctcasr.h).  One launch over the
// PCM of a batch: a drawn row is convolved with its response in exact 32-bit integers, scaled and
// rounded once; every other row, and the padding behind n in every row, is copied.  The draws are
// the integer functions of (seed, row) pinned in the header; tests/reverb_reference.py restates
// them and the arithmetic in numpy.
//
// A workgroup serves CHUNK output samples [c0, c0 + CHUNK) of one row.  It stages the input it
// needs in LDS BACKWARDS: w[j] = x[c0 + CHUNK - 1 + delay - j] (zero outside [0, n)), so that
//     out[c0 + CHUNK - 1 - u] = sum_k h[k] * w[u + k]
// is a correlation with the taps in the order the bank holds them.  A lane owns the 8 outputs
// u0 .. u0 + 7 (u0 = 8 * thread) and walks the taps 8 at a time: the 16 samples w[u0 + k0 ..] sit
// in 8 registers, of which every step keeps 4 and reads 4 (one 16-byte LDS read).  Outputs at an
// even distance take their sample pairs as those dwords, outputs at an odd distance from the 7
// dwords between them (one v_alignbit each, 4 new ones per step), and the pairs of taps are the
// same for all lanes: a workgroup-uniform read that the compiler keeps on the scalar side (loads
// through the scalar cache, taps as scalar operands of the dot instructions).  8 outputs x 8 taps
// are 32 v_dot2 instructions against one LDS read and 4 shuffles.
#include "common.h"

#include <limits.h>

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = CTCASR_REVERB_CHUNK;           // output samples per workgroup
constexpr int MAX_TAPS = CTCASR_REVERB_MAX_TAPS;
constexpr int TAP_ALIGN = CTCASR_REVERB_TAP_ALIGN;
constexpr int TAP_BLOCK = CTCASR_REVERB_TAP_BLOCK;   // taps per round of the unrolled inner loop
constexpr int WINDOW = CHUNK + MAX_TAPS;             // staged samples, at most
static_assert(CHUNK == 8 * THREADS, "a lane owns 8 outputs");
static_assert(TAP_ALIGN == 8 && TAP_BLOCK % 8 == 0 && MAX_TAPS % TAP_BLOCK == 0, "tap steps of 8");

typedef short short2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
// the taps are read-only for the whole launch and their address is the same in every lane
typedef const __attribute__((address_space(4))) u32x4 *tap_ptr;

__device__ __forceinline__ int below(uint64_t seed, uint64_t idx, int64_t n) {
    return (int)(((uint64_t)splitmix64_r24(seed, idx) * (uint64_t)n) >> 24);
}

__device__ __forceinline__ int dot2(u32 taps, u32 samples, int acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, taps),
                                  __builtin_bit_cast(short2_t, samples), acc, false);
}

// the pair that starts at the upper half of lo: (lo >> 16) | (hi << 16)
__device__ __forceinline__ u32 between(u32 lo, u32 hi) {
    return __builtin_amdgcn_alignbit(hi, lo, 16);
}

// 8 taps h[0..7] (4 dwords) against the 16 samples in w[0..7]: acc[e] += sum_k h[k] * s[e + k]
__device__ __forceinline__ void step8(const u32x4 h, const u32 (&w)[8], const u32 (&o)[7],
                                      int (&acc)[8]) {
    const u32 hp[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            acc[2 * m] = dot2(hp[p], w[m + p], acc[2 * m]);
            acc[2 * m + 1] = dot2(hp[p], o[m + p], acc[2 * m + 1]);
        }
    }
}

// grid = B x chunks
__global__ void __launch_bounds__(THREADS)
reverb_kernel(const int16_t *__restrict__ pcm, const int32_t *__restrict__ num_samples,
              int max_samples, const int16_t *__restrict__ taps,
              const int64_t *__restrict__ rir_offsets, const int32_t *__restrict__ rir_delay,
              const float *__restrict__ rir_scale, int num_rirs, uint64_t seed, int permille,
              int16_t *__restrict__ out, int32_t *__restrict__ draws, int chunks) {
    __shared__ __attribute__((aligned(16))) int16_t s_w[WINDOW];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int n = num_samples[b];
    const uint64_t idx = 8ull * (uint64_t)b;
    int status = 0, r = 0, K = 0, delay = 0;
    int64_t start = 0;
    if (n >= 1 && n <= max_samples && below(seed, idx, 1000) < permille) {
        r = below(seed, idx + 1, num_rirs);
        start = rir_offsets[r];
        const int64_t len = rir_offsets[r + 1] - start;
        delay = rir_delay[r];
        const bool served = len >= TAP_ALIGN && len <= MAX_TAPS && len % TAP_ALIGN == 0 &&
                            start >= 0 && start % TAP_ALIGN == 0 && delay >= 0 && delay < len;
        status = served ? 1 : 2;
        K = served ? (int)len : 0;
    }
    if (chunk == 0 && tid == 0 && draws) {
        draws[2 * (size_t)b] = status;
        draws[2 * (size_t)b + 1] = r;
    }
    const int16_t *x = pcm + (size_t)b * max_samples;
    int16_t *y = out + (size_t)b * max_samples;
    const int c0 = chunk * CHUNK;                                    // < max_samples <= 2^30
    const int live = status == 1 ? n : 0;                            // samples to compute
    // the copy: everything of this chunk at or beyond `live`
    {
        const int lo = c0 > live ? c0 : live;
        const int hi = c0 + CHUNK < max_samples ? c0 + CHUNK : max_samples;
        for (int i = lo + tid; i < hi; i += THREADS) y[i] = x[i];
    }
    if (c0 >= live) return;

    // the window, backwards: w[j] = x[top - j] for j < CHUNK + K (the last one is read, not used)
    const int top = c0 + CHUNK - 1 + delay;
    for (int j = tid; j < CHUNK + K; j += THREADS) {
        const int i = top - j;
        s_w[j] = (i >= 0 && i < n) ? x[i] : (int16_t)0;
    }
    __syncthreads();

    const int u0 = 8 * tid;
    const int i_lo = c0 + CHUNK - 8 - u0;                            // this lane's lowest output
    if (i_lo >= n) return;
    const float scale = rir_scale[r];
    const u32x4 *win = reinterpret_cast<const u32x4 *>(s_w + u0);    // 16-byte steps of 8 samples
    tap_ptr h = (tap_ptr)(taps + start);
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u32 w[8], o[7];
    {
        const u32x4 first = win[0];
        w[4] = first.x, w[5] = first.y, w[6] = first.z, w[7] = first.w;
        o[4] = between(w[4], w[5]), o[5] = between(w[5], w[6]), o[6] = between(w[6], w[7]);
    }
    // round q: taps [8 q, 8 q + 8) against w[u0 + 8 q .. u0 + 8 q + 15]
    auto round8 = [&](int q) {
        const u32x4 next = win[q + 1];
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = w[t + 4];
#pragma unroll
        for (int t = 0; t < 3; ++t) o[t] = o[t + 4];
        w[4] = next.x, w[5] = next.y, w[6] = next.z, w[7] = next.w;
        o[3] = between(w[3], w[4]);
        o[4] = between(w[4], w[5]), o[5] = between(w[5], w[6]), o[6] = between(w[6], w[7]);
        step8(h[q], w, o, acc);
    };
    const int rounds = K / 8;
    int q = 0;
    for (; q + TAP_BLOCK / 8 <= rounds; q += TAP_BLOCK / 8) {
#pragma unroll
        for (int t = 0; t < TAP_BLOCK / 8; ++t) round8(q + t);
    }
    for (; q < rounds; ++q) round8(q);

    // acc[e] belongs to output i_lo + 7 - e
    int v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = rintf((float)acc[7 - e] * scale);
        v[e] = (int)fminf(fmaxf(f, -32768.0f), 32767.0f);
    }
    if (i_lo + 8 <= n && (reinterpret_cast<uintptr_t>(y + i_lo) & 15) == 0) {
        u32x4 packed;
        packed.x = (u32)(uint16_t)v[0] | ((u32)(uint16_t)v[1] << 16);
        packed.y = (u32)(uint16_t)v[2] | ((u32)(uint16_t)v[3] << 16);
        packed.z = (u32)(uint16_t)v[4] | ((u32)(uint16_t)v[5] << 16);
        packed.w = (u32)(uint16_t)v[6] | ((u32)(uint16_t)v[7] << 16);
        *reinterpret_cast<u32x4 *>(y + i_lo) = packed;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (i_lo + e < n) y[i_lo + e] = (int16_t)v[e];
    }
}

}  // namespace

extern "C" int ctcasr_reverb(const int16_t *pcm, const int32_t *num_samples, int B,
                             int max_samples, const int16_t *taps, const int64_t *rir_offsets,
                             const int32_t *rir_delay, const float *rir_scale, int num_rirs,
                             uint64_t seed, int prob_permille, int16_t *out, int32_t *draws,
                             ctcasr_stream_t stream) {
    if (!pcm || !num_samples || !taps || !rir_offsets || !rir_delay || !rir_scale || !out ||
        out == pcm || B < 1 || max_samples < 1 || num_rirs < 1 || prob_permille < 0 ||
        prob_permille > 1000)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (max_samples > 1 << 30 || num_rirs > 1 << 24) return CTCASR_ERR_UNSUPPORTED;
    const int64_t chunks = ((int64_t)max_samples + CHUNK - 1) / CHUNK;
    if (chunks * B > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (prob_permille == 0) {
        // no row can be drawn: no kernel, only the copy and zeroed draws
        bool ok = hipMemcpyAsync(out, pcm, (size_t)B * max_samples * sizeof(int16_t),
                                 hipMemcpyDeviceToDevice, s) == hipSuccess;
        if (draws) ok &= hipMemsetAsync(draws, 0, (size_t)B * 2 * sizeof(int32_t), s) == hipSuccess;
        return ok ? CTCASR_OK : CTCASR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(reverb_kernel, dim3((unsigned)(chunks * B)), dim3(THREADS), 0, s, pcm,
                       num_samples, max_samples, taps, rir_offsets, rir_delay, rir_scale, num_rirs,
                       seed, prob_permille, out, draws, (int)chunks);
    return ctcasr_launch_status();
}
