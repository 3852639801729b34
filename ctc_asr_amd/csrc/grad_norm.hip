// Gradient norms over the flat gradient arena: one read of it, squares summed in fp64 in an order
// that the data layout alone fixes, then per-segment norms, the global norm, the clip factor and
// the guard word - all on the device (include/ctcasr.h, "K14").
//
// Two launches.  The first gives every chunk of CTCASR_GRAD_NORM_CHUNK floats - counted from its
// SEGMENT's start - to one workgroup, which writes the chunk's sum of squares to the workspace.
// The second is one workgroup that adds the chunk sums per segment, the segment sums in index order,
// and writes the results.  (The alternative, "the last workgroup to finish does the rest", needs a
// ticket counter, release / acquire fences around it and somebody to zero it again; a launch of one
// workgroup needs none of that and costs a few microseconds behind a read of hundreds.)
#include "common.h"

namespace {

constexpr int CHUNK = CTCASR_GRAD_NORM_CHUNK;
constexpr int MAX_SEGMENTS = CTCASR_GRAD_NORM_MAX_SEGMENTS;
constexpr int THREADS = 256;
constexpr int V4_PER_THREAD = CHUNK / 4 / THREADS;
constexpr int FINISH_THREADS = 1024;
static_assert(V4_PER_THREAD * 4 * THREADS == CHUNK, "a chunk is a whole number of float4 rounds");

// 256 CUs x 8 resident workgroups of 256 threads; the rest of the chunks by grid stride.
// ctcasr_set_option("grad_norm_blocks", k) overrides it (0: back to this) - for the microbenchmark
// and for the test that the results do not depend on it.
constexpr int DEFAULT_BLOCKS = 2048;

// The offset table as the kernels use it: start[i] clamped into [0, n], made ascending, every entry
// but the last rounded down to a multiple of 4 (no change to a table that keeps the contract; one
// that does not can make the sums meaningless, but never an address outside grad[0, n) and never a
// misaligned 16-byte load).  first_chunk[s] = chunks of the segments before s.
struct SegTable {
    int64_t start[MAX_SEGMENTS + 1];
    int64_t first_chunk[MAX_SEGMENTS + 1];
};

__device__ void load_table(const int64_t *__restrict__ seg_offsets, int segments, int64_t n,
                           SegTable &t) {
    for (int i = threadIdx.x; i <= segments; i += blockDim.x) {
        int64_t o = seg_offsets[i];
        o = o < 0 ? 0 : o > n ? n : o;
        if (i < segments) o &= ~(int64_t)3;
        t.start[i] = o;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t prev = 0, chunks = 0;
        for (int i = 0; i <= segments; ++i) {
            int64_t o = t.start[i];
            if (o < prev) o = prev;
            t.start[i] = o;
            if (i > 0) {
                t.first_chunk[i - 1] = chunks;
                chunks += (o - prev + CHUNK - 1) / CHUNK;
            }
            prev = o;
        }
        t.first_chunk[segments] = chunks;
    }
    __syncthreads();
}

// every lane ends with the same sum: a + b == b + a, so the butterfly is one fixed tree
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

#define SQ_ADD(acc, v4)                                     \
    {                                                       \
        acc = fma((double)(v4).x, (double)(v4).x, acc);     \
        acc = fma((double)(v4).y, (double)(v4).y, acc);     \
        acc = fma((double)(v4).z, (double)(v4).z, acc);     \
        acc = fma((double)(v4).w, (double)(v4).w, acc);     \
    }

// partial[c] = sum of squares of chunk c (chunks numbered segment by segment).  Within a chunk
// thread t owns the float4s t, t + 256, ..., adds their squares in that order (x, y, z, w inside
// one) - the product of two floats is exact in fp64, so the fma rounds once, as a multiply and an
// add would - then the 64 lanes of a wave by butterfly, then the four waves in order.  Elements past
// the end of a short chunk count as +0, which changes no sum.
__global__ void __launch_bounds__(THREADS)
grad_sumsq_kernel(const float *__restrict__ grad, int64_t n,
                  const int64_t *__restrict__ seg_offsets, int segments,
                  double *__restrict__ partial) {
    __shared__ SegTable t;
    __shared__ double wave_part[THREADS / 64];
    load_table(seg_offsets, segments, n, t);
    const int tid = threadIdx.x;
    const int64_t total = t.first_chunk[segments];
    for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
        // the segment of chunk c: first_chunk[lo] <= c < first_chunk[hi] (empty segments drop out)
        int lo = 0, hi = segments;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (t.first_chunk[mid] <= c) lo = mid; else hi = mid;
        }
        const int64_t base = t.start[lo] + (c - t.first_chunk[lo]) * CHUNK;
        const int64_t left = t.start[lo + 1] - base;
        const int len = left < CHUNK ? (int)left : CHUNK;
        const float *x = grad + base;
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        float4 v[V4_PER_THREAD];
        if (len == CHUNK) {
#pragma unroll
            for (int j = 0; j < V4_PER_THREAD; ++j) v[j] = x4[j * THREADS + tid];
        } else {
#pragma unroll
            for (int j = 0; j < V4_PER_THREAD; ++j) {
                const int e = 4 * (j * THREADS + tid);
                v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e + 4 <= len) {
                    v[j] = x4[j * THREADS + tid];
                } else {
                    if (e < len) v[j].x = x[e];
                    if (e + 1 < len) v[j].y = x[e + 1];
                    if (e + 2 < len) v[j].z = x[e + 2];
                }
            }
        }
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < V4_PER_THREAD; ++j) SQ_ADD(acc, v[j])
        acc = wave_sum_f64(acc);
        if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0)
            partial[c] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
        __syncthreads();
    }
}
#undef SQ_ADD

// One workgroup.  A wave per segment: lane l adds the segment's chunk sums l, l + 64, ... in that
// order, the lanes by butterfly - an order that depends on the segment's chunk count alone.  Then
// one thread: segment sums in index order for the total, one rounding to fp32 per norm, the factor
// by one fp32 division, the guard word.
__global__ void __launch_bounds__(FINISH_THREADS)
grad_norm_finish_kernel(const double *__restrict__ partial, int64_t n,
                        const int64_t *__restrict__ seg_offsets, int segments, float grad_scale,
                        float max_norm, float *__restrict__ norms,
                        float *__restrict__ clip_factor, int32_t *__restrict__ skip) {
    __shared__ SegTable t;
    __shared__ double seg_sum[MAX_SEGMENTS];
    load_table(seg_offsets, segments, n, t);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < segments; s += FINISH_THREADS / 64) {
        double acc = 0.0;
        for (int64_t c = t.first_chunk[s] + lane; c < t.first_chunk[s + 1]; c += 64)
            acc += partial[c];
        acc = wave_sum_f64(acc);
        if (lane == 0) seg_sum[s] = acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int s = 0; s < segments; ++s) {
        total += seg_sum[s];
        norms[s] = (float)((double)grad_scale * sqrt(seg_sum[s]));
    }
    const float gnorm = (float)((double)grad_scale * sqrt(total));
    norms[segments] = gnorm;
    float factor = 1.0f;
    if (!isfinite(gnorm)) {
        // gradients that hold an inf or a NaN (or overflow fp32 as a norm) behind a finite loss:
        // the step is dropped like one whose loss is not finite (ctcasr_step_guard's word)
        factor = 0.0f;
        if (skip) skip[0] = 1;
    } else if (max_norm > 0.0f && gnorm > max_norm) {
        factor = __fdiv_rn(max_norm, gnorm);
    }
    clip_factor[0] = factor;
}

int64_t chunk_bound(int64_t n, int segments) { return n / CHUNK + segments; }

}  // namespace

int g_grad_norm_blocks = 0;     // ctcasr_set_option("grad_norm_blocks", k); 0 = DEFAULT_BLOCKS

extern "C" size_t ctcasr_grad_norm_workspace_bytes(int64_t n, int segments) {
    if (n < 0 || segments < 1 || segments > MAX_SEGMENTS) return 0;
    // sum over segments of ceil(len / CHUNK) <= n / CHUNK + segments
    return (size_t)chunk_bound(n, segments) * sizeof(double);
}

extern "C" int ctcasr_grad_norm(const float *grad, int64_t n, const int64_t *seg_offsets,
                                int segments, float grad_scale, float max_norm, float *norms,
                                float *clip_factor, int32_t *skip, void *workspace,
                                size_t workspace_bytes, ctcasr_stream_t stream) {
    if ((!grad && n > 0) || !seg_offsets || !norms || !clip_factor || n < 0 || segments < 1 ||
        reinterpret_cast<uintptr_t>(grad) % 16 != 0)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (segments > MAX_SEGMENTS) return CTCASR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ctcasr_grad_norm_workspace_bytes(n, segments) ||
        reinterpret_cast<uintptr_t>(workspace) % sizeof(double) != 0)
        return CTCASR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cap = g_grad_norm_blocks > 0 ? g_grad_norm_blocks : DEFAULT_BLOCKS;
    const int64_t bound = chunk_bound(n, segments);
    double *partial = static_cast<double *>(workspace);
    grad_sumsq_kernel<<<(int)(bound < cap ? bound : cap), THREADS, 0, s>>>(grad, n, seg_offsets,
                                                                          segments, partial);
    grad_norm_finish_kernel<<<1, FINISH_THREADS, 0, s>>>(partial, n, seg_offsets, segments,
                                                         grad_scale, max_norm, norms, clip_factor,
                                                         skip);
    return ctcasr_launch_status();
}
