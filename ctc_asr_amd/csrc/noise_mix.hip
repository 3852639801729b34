// K16: additive noise at a drawn SNR (include/ctcasr.h).  Two launches over the PCM of a batch:
// the first sums the squares of the speech and of the noise under it per row - exact 64-bit
// integers, one atomic per workgroup and sum, so the sums depend on nothing but the data - the
// second recomputes the row's gain from the two sums in every workgroup and stores the mix.  The
// draws are the integer functions of (seed, row) pinned in the header;
// tests/noise_reference.py restates them, the powers and the gain in numpy.
//
// Addresses.  Rows start anywhere (max_samples may be odd) and the noise starts anywhere in its
// clip, so a row is cut into GROUPS of 8 samples by the ADDRESS of the stream that is stored (the
// speech in the first launch): group q of a row whose first sample sits `mis` samples behind a
// 16-byte boundary covers samples [8 q - mis, 8 q - mis + 8).  A group that lies inside the row,
// below n, and whose noise does not wrap is one 16-byte access per stream - the noise through two
// aligned loads and a funnel shift, since its phase against the speech is arbitrary.  Every other
// group - the head and the tail of a row, the group that straddles n, a group that crosses the
// clip's end, all of a clip shorter than 8 - walks its samples one by one.  No sample belongs to
// two groups and no group to two workgroups, which is what makes `out == pcm` safe.
#include "common.h"

#include <limits.h>

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = CTCASR_NOISE_MIX_CHUNK;      // samples per workgroup
constexpr int GROUPS = CHUNK / 8;                  // groups per workgroup
constexpr int MAX_CLIP = 1 << 24;
static_assert(GROUPS % THREADS == 0, "a chunk is a whole number of rounds of the workgroup");

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int below(uint64_t seed, uint64_t idx, int64_t n) {
    return (int)(((uint64_t)splitmix64_r24(seed, idx) * (uint64_t)n) >> 24);
}

// What row b drew.  status: 0 = not drawn or a bad row (k = o = snr = 0), 1 = to be mixed if
// neither power is zero, 2 = drawn a clip whose length is not served (o = 0).
struct Draw {
    int status, k, o, snr, n;
    uint32_t len;
    const int16_t *clip;
};

__device__ Draw draw_row(const int32_t *num_samples, int b, int max_samples, const int16_t *bank,
                         const int64_t *clip_offsets, int num_clips, uint64_t seed, int snr_lo,
                         int snr_hi, int permille) {
    Draw d = {0, 0, 0, 0, num_samples[b], 0u, bank};
    const uint64_t idx = 8ull * (uint64_t)b;
    if (d.n < 1 || d.n > max_samples || below(seed, idx, 1000) >= permille) return d;
    d.k = below(seed, idx + 1, num_clips);
    d.snr = snr_lo + below(seed, idx + 3, snr_hi - snr_lo + 1);
    const int64_t start = clip_offsets[d.k], len = clip_offsets[d.k + 1] - start;
    if (len < 1 || len > MAX_CLIP) {
        d.status = 2;
        return d;
    }
    d.status = 1;
    d.len = (uint32_t)len;
    d.o = below(seed, idx + 2, len);
    d.clip = bank + start;
    return d;
}

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

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// grid = B x chunks.  sums[2 b] += squares of the speech, sums[2 b + 1] += squares of the noise
// under it, over the samples below n of this workgroup's groups; rows that drew nothing read
// nothing.  `sums` is zeroed on the stream before the launch.
__global__ void __launch_bounds__(THREADS)
noise_power_kernel(const int16_t *__restrict__ pcm, const int32_t *__restrict__ num_samples,
                   int max_samples, const int16_t *__restrict__ bank,
                   const int64_t *__restrict__ clip_offsets, int num_clips, uint64_t seed,
                   int snr_lo, int snr_hi, int permille, u64 *__restrict__ sums, int chunks) {
    __shared__ u64 s_part[2][THREADS / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const Draw d = draw_row(num_samples, b, max_samples, bank, clip_offsets, num_clips, seed,
                            snr_lo, snr_hi, permille);
    if (d.status != 1) return;
    const int16_t *x = pcm + (size_t)b * max_samples;
    const int mis = misalignment(x);
    const int64_t first = (int64_t)chunk * CHUNK - mis;            // first sample of this chunk
    if (first >= d.n) return;
    u64 ps = 0, pn = 0;
#pragma unroll 2
    for (int r = 0; r < GROUPS / THREADS; ++r) {
        const int64_t s = first + 8 * (int64_t)(r * THREADS + tid);
        if (s >= d.n) break;
        const uint32_t p = ((uint32_t)d.o + (uint32_t)(s < 0 ? 0 : s)) % d.len;   // o + s < 2^31
        if (s >= 0 && s + 8 <= d.n && p + 8 <= d.len) {
            const u64x2 xv = *reinterpret_cast<const u64x2 *>(x + s);
            u64 nlo, nhi;
            load8_any(d.clip + p, nlo, nhi);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int xs = sample_of(xv.x, xv.y, j), vs = sample_of(nlo, nhi, j);
                ps += (u64)(xs * xs);          // at most 2^30: the product fits an int
                pn += (u64)(vs * vs);
            }
        } else {
            const int lo = s < 0 ? 0 : (int)s, hi = (int)(s + 8 < d.n ? s + 8 : d.n);
            uint32_t q = p;
            for (int i = lo; i < hi; ++i) {
                const int xs = x[i], vs = d.clip[q];
                ps += (u64)(xs * xs);
                pn += (u64)(vs * vs);
                if (++q == d.len) q = 0;
            }
        }
    }
    ps = wave_sum_u64(ps);
    pn = wave_sum_u64(pn);
    if ((tid & 63) == 0) {
        s_part[0][tid >> 6] = ps;
        s_part[1][tid >> 6] = pn;
    }
    __syncthreads();
    if (tid < 2) {
        const u64 total = s_part[tid][0] + s_part[tid][1] + s_part[tid][2] + s_part[tid][3];
        if (total) atomicAdd(sums + 2 * b + tid, total);
    }
}

__device__ __forceinline__ int mix_one(int xs, int vs, float g) {
    const float y = rintf(fmaf(g, (float)vs, (float)xs));
    return (int)fminf(fmaxf(y, -32768.0f), 32767.0f);
}

// grid = B x chunks, groups cut by the address of `out`.  Every workgroup of a row computes the
// same gain from the same two sums.  Stores: the mixed samples below n of a mixed row; when
// out != pcm also a copy of everything else.  pcm and out may be the same buffer: a thread reads
// the samples of its group before it stores them, and nobody else touches them.
__global__ void __launch_bounds__(THREADS)
noise_mix_kernel(const int16_t *pcm, const int32_t *__restrict__ num_samples, int max_samples,
                 const int16_t *__restrict__ bank, const int64_t *__restrict__ clip_offsets,
                 int num_clips, uint64_t seed, int snr_lo, int snr_hi, int permille,
                 const u64 *__restrict__ sums, int16_t *out, int32_t *__restrict__ draws,
                 int64_t *__restrict__ powers, float *__restrict__ gain, int chunks) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    Draw d = draw_row(num_samples, b, max_samples, bank, clip_offsets, num_clips, seed, snr_lo,
                      snr_hi, permille);
    u64 ps = 0, pn = 0;
    float g = 0.0f;
    if (d.status == 1) {
        ps = sums[2 * b];
        pn = sums[2 * b + 1];
        if (ps == 0 || pn == 0) {
            d.status = 2;
        } else {
            // (uniform over the workgroup: the compiler keeps it on the scalar side where it can)
            g = (float)(sqrt((double)ps / (double)pn) * pow(10.0, -(double)d.snr / 20.0));
        }
    }
    if (chunk == 0 && tid == 0) {
        if (draws) {
            int32_t *dst = draws + 4 * (size_t)b;
            dst[0] = d.status;
            dst[1] = d.k;
            dst[2] = d.o;
            dst[3] = d.snr;
        }
        if (powers) {
            powers[2 * (size_t)b] = (int64_t)ps;
            powers[2 * (size_t)b + 1] = (int64_t)pn;
        }
        if (gain) gain[b] = g;
    }
    const bool mixed = d.status == 1, copy = out != pcm;
    if (!mixed && !copy) return;
    const int n = mixed ? d.n : 0;                                   // samples to mix
    const int64_t stored = copy ? max_samples : n;                   // samples to store
    const int16_t *x = pcm + (size_t)b * max_samples;
    int16_t *y = out + (size_t)b * max_samples;
    const int mis = misalignment(y);
    const bool x_aligned = misalignment(x) == mis;
    const int64_t first = (int64_t)chunk * CHUNK - mis;
    if (first >= stored) return;
#pragma unroll 2
    for (int r = 0; r < GROUPS / THREADS; ++r) {
        const int64_t s = first + 8 * (int64_t)(r * THREADS + tid);
        if (s >= stored) break;
        const bool whole = s >= 0 && s + 8 <= max_samples && x_aligned;
        if (whole && s >= n) {                                       // (copy only)
            *reinterpret_cast<u64x2 *>(y + s) = *reinterpret_cast<const u64x2 *>(x + s);
            continue;
        }
        const uint32_t p = mixed ? ((uint32_t)d.o + (uint32_t)(s < 0 ? 0 : s)) % d.len : 0u;
        if (whole && s + 8 <= n && p + 8 <= d.len) {
            const u64x2 xv = *reinterpret_cast<const u64x2 *>(x + s);
            u64 nlo, nhi;
            load8_any(d.clip + p, nlo, nhi);
            u64 w[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int v = mix_one(sample_of(xv.x, xv.y, j), sample_of(nlo, nhi, j), g);
                w[j >> 2] |= (u64)(uint16_t)v << (16 * (j & 3));
            }
            u64x2 yv;
            yv.x = w[0];
            yv.y = w[1];
            *reinterpret_cast<u64x2 *>(y + s) = yv;
            continue;
        }
        const int lo = s < 0 ? 0 : (int)s, hi = (int)(s + 8 < stored ? s + 8 : stored);
        uint32_t q = p;
        for (int i = lo; i < hi; ++i) {
            int v = x[i];
            if (i < n) {
                v = mix_one(v, d.clip[q], g);
                if (++q == d.len) q = 0;
            }
            y[i] = (int16_t)v;
        }
    }
}

int64_t chunks_of(int max_samples) {
    // (+ 7: a row that starts behind a 16-byte boundary has a short first group)
    return ((int64_t)max_samples + 7 + CHUNK - 1) / CHUNK;
}

}  // namespace

extern "C" size_t ctcasr_noise_mix_workspace_bytes(int B) {
    return B < 1 ? 0 : (size_t)B * 2 * sizeof(u64);
}

extern "C" int ctcasr_noise_mix(const int16_t *pcm, const int32_t *num_samples, int B,
                                int max_samples, const int16_t *bank, const int64_t *clip_offsets,
                                int num_clips, uint64_t seed, int snr_lo_db, int snr_hi_db,
                                int prob_permille, int16_t *out, int32_t *draws, int64_t *powers,
                                float *gain, void *workspace, size_t workspace_bytes,
                                ctcasr_stream_t stream) {
    if (!pcm || !num_samples || !bank || !clip_offsets || !out || B < 1 || max_samples < 1 ||
        num_clips < 1)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (snr_lo_db > snr_hi_db || snr_lo_db < CTCASR_NOISE_MIX_MIN_SNR_DB ||
        snr_hi_db > CTCASR_NOISE_MIX_MAX_SNR_DB || prob_permille < 0 || prob_permille > 1000)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (max_samples > 1 << 30 || num_clips > MAX_CLIP) return CTCASR_ERR_UNSUPPORTED;
    const int64_t chunks = chunks_of(max_samples);
    if (chunks * B > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ctcasr_noise_mix_workspace_bytes(B) ||
        reinterpret_cast<uintptr_t>(workspace) % sizeof(u64) != 0)
        return CTCASR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (prob_permille == 0) {
        // no row can be drawn: no kernel, only the copy the caller asked for and zeroed reports
        bool ok = true;
        if (out != pcm)
            ok &= hipMemcpyAsync(out, pcm, (size_t)B * max_samples * sizeof(int16_t),
                                 hipMemcpyDeviceToDevice, s) == hipSuccess;
        if (draws) ok &= hipMemsetAsync(draws, 0, (size_t)B * 4 * sizeof(int32_t), s) == hipSuccess;
        if (powers) ok &= hipMemsetAsync(powers, 0, (size_t)B * 2 * sizeof(int64_t), s) == hipSuccess;
        if (gain) ok &= hipMemsetAsync(gain, 0, (size_t)B * sizeof(float), s) == hipSuccess;
        return ok ? CTCASR_OK : CTCASR_ERR_LAUNCH;
    }
    u64 *sums = static_cast<u64 *>(workspace);
    if (hipMemsetAsync(sums, 0, (size_t)B * 2 * sizeof(u64), s) != hipSuccess)
        return CTCASR_ERR_LAUNCH;
    const dim3 grid((unsigned)(chunks * B));
    hipLaunchKernelGGL(noise_power_kernel, grid, dim3(THREADS), 0, s, pcm, num_samples,
                       max_samples, bank, clip_offsets, num_clips, seed, snr_lo_db, snr_hi_db,
                       prob_permille, sums, (int)chunks);
    hipLaunchKernelGGL(noise_mix_kernel, grid, dim3(THREADS), 0, s, pcm, num_samples, max_samples,
                       bank, clip_offsets, num_clips, seed, snr_lo_db, snr_hi_db, prob_permille,
                       sums, out, draws, powers, gain, (int)chunks);
    return ctcasr_launch_status();
}
