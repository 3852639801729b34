// K18: speech segmentation of a long recording (include/ctcasr.h).  Two entry points around the
// host-side decision of ctc_asr_amd/vad.py: the one pass over the PCM - energy per 10 ms hop as an
// exact 64-bit integer, and the histogram of the hops' quarter-octave levels - and the gather
// that lays the chosen pieces out as the rows of a batch for ctcasr_features.  Integer sums and
// integer atomics only: the results depend on nothing but the data.
// tests/vad_reference.py restates both in numpy.
//
// Addresses.  The energy pass cuts the recording into groups of 8 samples counted from its first
// sample: a hop is 20 whole groups, so no group belongs to two hops.  With a 16-byte aligned base
// every group is one 16-byte load; any other base reads the one or two aligned 16-byte words that
// hold the group and shifts them into place.  The gather cuts a row by the address of what it
// STORES, as ctcasr_noise_mix does, and reads its source, which starts anywhere, the same way.
#include "common.h"

#include <limits.h>

namespace {

constexpr int THREADS = 256;
constexpr int HOP = CTCASR_VAD_HOP;
constexpr int LEVELS = CTCASR_VAD_LEVELS;
constexpr int CHUNK = CTCASR_VAD_CHUNK;            // samples per workgroup of the energy pass
constexpr int HOPS = CHUNK / HOP;                  // hops per workgroup
constexpr int HOP_GROUPS = HOP / 8;                // groups of 8 samples per hop
constexpr int GROUPS = CHUNK / 8;
constexpr int HOP_STRIDE = HOP_GROUPS + 1;         // partial sums of a hop in LDS, padded by one
constexpr int GATHER_CHUNK = 8192;                 // samples of a row per workgroup of the gather
constexpr int GATHER_GROUPS = GATHER_CHUNK / 8;
static_assert(CHUNK % HOP == 0 && HOP % 8 == 0, "a chunk is whole hops, a hop whole groups");
static_assert(HOPS == THREADS, "one thread sums one hop");
static_assert(GROUPS % THREADS == 0 && GATHER_GROUPS % THREADS == 0, "whole rounds");
static_assert(LEVELS <= THREADS, "one thread flushes one bin");

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int misalignment(const int16_t *p) {      // in samples, 0..7
    return (int)((reinterpret_cast<uintptr_t>(p) >> 1) & 7);
}

__device__ __forceinline__ int sample_of(u64 lo, u64 hi, int j) {    // j is a constant after unrolling
    return (int)(int16_t)((j < 4 ? lo : hi) >> (16 * (j & 3)));
}

// the 8 samples at p (any 2-byte aligned address): the one or two aligned 16-byte words that hold
// them - both hold at least one of the 8, so no byte outside their 16-byte granules is touched -
// shifted into place
__device__ __forceinline__ void load8_any(const int16_t *p, u64 &lo, u64 &hi) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    const u64x2 *q = reinterpret_cast<const u64x2 *>(addr & ~(uintptr_t)15);
    unsigned shift = (unsigned)(addr & 15) * 8;
    const u64x2 first = q[0];
    lo = first.x;
    hi = first.y;
    if (shift == 0) return;
    const u64x2 second = q[1];
    u64 a0 = first.x, a1 = first.y, a2 = second.x;
    if (shift >= 64) {
        a0 = a1;
        a1 = a2;
        a2 = second.y;
        shift -= 64;
    }
    if (shift) {
        lo = (a0 >> shift) | (a1 << (64 - shift));
        hi = (a1 >> shift) | (a2 << (64 - shift));
    } else {
        lo = a0;
        hi = a1;
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void load8(const int16_t *p, u64 &lo, u64 &hi) {
    if (ALIGNED) {
        const u64x2 v = *reinterpret_cast<const u64x2 *>(p);
        lo = v.x;
        hi = v.y;
    } else {
        load8_any(p, lo, hi);
    }
}

__device__ __forceinline__ u64 squares8(u64 lo, u64 hi) {
    u64 sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int x = sample_of(lo, hi, j);
        sum += (u64)(x * x);                       // at most 2^30: the product fits an int
    }
    return sum;
}

// the quarter-octave level of an energy (pinned in the header)
__device__ __forceinline__ int level_of(u64 e) {
    const int b = e ? 64 - __clzll((long long)e) : 0;
    return b <= 2 ? (int)e : 4 * (b - 2) + (int)((e >> (b - 3)) & 3);
}

// grid = ceil(n / CHUNK).  A workgroup sums the squares of its CHUNK samples per group of 8 into
// LDS, one thread per hop adds the hop's 20 partial sums (a hop's partials lie HOP_STRIDE = 21
// 64-bit words apart: 42 dwords, so the 32 lanes of half a wave read 32 different bank pairs),
// stores the energy and counts its level in the workgroup's histogram; the non-empty bins go to
// `hist` with one integer atomic each.  `hist` is zeroed on the stream before the launch.
template <bool ALIGNED>
__global__ void __launch_bounds__(THREADS)
vad_energy_kernel(const int16_t *__restrict__ pcm, int64_t n, int64_t *__restrict__ energy,
                  uint32_t *__restrict__ hist) {
    __shared__ u64 s_part[HOPS * HOP_STRIDE];
    __shared__ uint32_t s_hist[LEVELS];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * CHUNK;               // first sample of this chunk
    if (tid < LEVELS) s_hist[tid] = 0;
    if (first + CHUNK <= n) {
        // a whole chunk: nothing to decide per group, so the loads of several rounds are in flight
#pragma unroll 5
        for (int r = 0; r < GROUPS / THREADS; ++r) {
            const int g = r * THREADS + tid;
            u64 lo, hi;
            load8<ALIGNED>(pcm + first + 8 * g, lo, hi);
            s_part[g + g / HOP_GROUPS] = squares8(lo, hi);
        }
    } else {
        for (int r = 0; r < GROUPS / THREADS; ++r) {
            const int g = r * THREADS + tid;
            const int64_t s = first + 8 * (int64_t)g;
            u64 sum = 0;
            if (s + 8 <= n) {
                u64 lo, hi;
                load8<ALIGNED>(pcm + s, lo, hi);
                sum = squares8(lo, hi);
            } else {
                for (int64_t i = s; i < n; ++i) {      // (no trip at all when s >= n)
                    const int x = pcm[i];
                    sum += (u64)(x * x);
                }
            }
            s_part[g + g / HOP_GROUPS] = sum;
        }
    }
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * HOPS + tid;
    if (f * HOP < n) {
        u64 e = 0;
#pragma unroll
        for (int k = 0; k < HOP_GROUPS; ++k) e += s_part[tid * HOP_STRIDE + k];
        energy[f] = (int64_t)e;
        atomicAdd(&s_hist[level_of(e)], 1u);
    }
    __syncthreads();
    if (tid < LEVELS && s_hist[tid]) atomicAdd(hist + tid, s_hist[tid]);
}

// grid = B x chunks, groups cut by the address of the row of `out`.  Every workgroup of a row
// clips the row's range the same way; the first one reports the clipped length.
__global__ void __launch_bounds__(THREADS)
gather_segments_kernel(const int16_t *__restrict__ pcm, int64_t n,
                       const int64_t *__restrict__ seg_start, const int32_t *__restrict__ seg_len,
                       int max_samples, int16_t *__restrict__ out,
                       int32_t *__restrict__ num_samples, int chunks) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int64_t start = seg_start[b];
    int64_t len = seg_len[b];
    if (start < 0 || start >= n || len < 1) {
        len = 0;
    } else {
        if (len > n - start) len = n - start;
        if (len > max_samples) len = max_samples;
    }
    if (chunk == 0 && tid == 0) num_samples[b] = (int32_t)len;
    const int16_t *x = pcm + (len ? start : 0);
    int16_t *y = out + (size_t)b * max_samples;
    const int64_t head = (int64_t)chunk * GATHER_CHUNK - misalignment(y);
#pragma unroll 2
    for (int r = 0; r < GATHER_GROUPS / THREADS; ++r) {
        const int64_t s = head + 8 * (int64_t)(r * THREADS + tid);
        if (s >= max_samples) break;
        if (s >= 0 && s + 8 <= max_samples && (s + 8 <= len || s >= len)) {
            u64x2 v;
            v.x = 0;
            v.y = 0;
            if (s < len) {
                u64 lo, hi;
                load8_any(x + s, lo, hi);
                v.x = lo;
                v.y = hi;
            }
            *reinterpret_cast<u64x2 *>(y + s) = v;
            continue;
        }
        const int lo = s < 0 ? 0 : (int)s, hi = (int)(s + 8 < max_samples ? s + 8 : max_samples);
        for (int i = lo; i < hi; ++i) y[i] = i < len ? x[i] : (int16_t)0;
    }
}

}  // namespace

extern "C" int ctcasr_vad_energy(const int16_t *pcm, int64_t n, int64_t *energy, uint32_t *hist,
                                 ctcasr_stream_t stream) {
    if (!pcm || !energy || !hist || n < 1) return CTCASR_ERR_BAD_ARGUMENT;
    if (n > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, LEVELS * sizeof(uint32_t), s) != hipSuccess)
        return CTCASR_ERR_LAUNCH;
    const dim3 grid((unsigned)((n + CHUNK - 1) / CHUNK));
    if (reinterpret_cast<uintptr_t>(pcm) % 16 == 0)
        hipLaunchKernelGGL(vad_energy_kernel<true>, grid, dim3(THREADS), 0, s, pcm, n, energy, hist);
    else
        hipLaunchKernelGGL(vad_energy_kernel<false>, grid, dim3(THREADS), 0, s, pcm, n, energy,
                           hist);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_gather_segments(const int16_t *pcm, int64_t n, const int64_t *seg_start,
                                      const int32_t *seg_len, int B, int max_samples,
                                      int16_t *out, int32_t *num_samples,
                                      ctcasr_stream_t stream) {
    if (!pcm || !seg_start || !seg_len || !out || !num_samples || B < 1 || max_samples < 1)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (max_samples > 1 << 30) return CTCASR_ERR_UNSUPPORTED;
    // (+ 7: a row that starts behind a 16-byte boundary has a short first group)
    const int64_t chunks = ((int64_t)max_samples + 7 + GATHER_CHUNK - 1) / GATHER_CHUNK;
    if (chunks * B > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gather_segments_kernel, dim3((unsigned)(chunks * B)), dim3(THREADS), 0,
                       (hipStream_t)stream, pcm, n, seg_start, seg_len, max_samples, out,
                       num_samples, (int)chunks);
    return ctcasr_launch_status();
}
