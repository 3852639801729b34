// Sequence-wise batch normalisation of a recurrent layer's input (include/ctcasr.h, "K20"):
// per-channel statistics over every counted frame of the batch in fp64, in an order that the row
// numbers alone fix, then a streaming apply pass; the backward pass has the same shape.
//
// A channel row is contiguous, so a lane owns four adjacent channels (one 16-byte access per row)
// and walks the CTCASR_SEQ_BN_ROWS rows of its chunk with fp64 accumulators of its own: the
// statistics pass needs no cross-lane step, no LDS and no barrier, and the pinned order falls out
// by itself.  A workgroup of 256 lanes covers 1024 channels of one chunk; the work items are the
// (chunk, channel tile) pairs, taken by grid stride.  A finish launch (one lane per channel) adds
// the chunk sums in ascending order and writes the per-channel results; the apply / dx launch is
// an elementwise stream over the same work items with its channel constants loaded once.
//
// Every fp32 / fp64 operation below rounds on its own unless it is written as fma / fmaf: the
// restatement the tests hold this to (tests/batchnorm_reference.py) follows it operation by
// operation.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ROWS = CTCASR_SEQ_BN_ROWS;
constexpr int THREADS = 256;
constexpr int TILE = 4 * THREADS;       // channels per workgroup
// the finish launches: one lane per channel, one wave per workgroup - 2048 channels walk their
// chunk sums on 32 CUs instead of 8
constexpr int FINISH_THREADS = 64;
// 256 CUs x 8 resident workgroups of 256 lanes; further work items by grid stride
constexpr int DEFAULT_BLOCKS = 2048;

__device__ __forceinline__ int counted_len(const int32_t *__restrict__ lengths, int b, int T) {
    if (!lengths) return T;
    const int l = lengths[b];
    return l < 0 ? 0 : l > T ? T : l;
}

// the number of counted rows (B scalar loads; every lane of a finish launch gets the same value)
__device__ __forceinline__ int64_t counted_rows(const int32_t *__restrict__ lengths, int T, int B) {
    if (!lengths) return (int64_t)T * B;
    int64_t n = 0;
    for (int b = 0; b < B; ++b) n += counted_len(lengths, b, T);
    return n;
}

struct Item {
    int64_t row0;       // first row of the chunk
    int rows;           // rows of the chunk (the last one may be short)
    int c0;             // this lane's first channel; >= C: the lane idles
    int64_t chunk;
};

__device__ __forceinline__ Item work_item(int64_t w, int ctiles, int64_t total_rows) {
    Item it;
    it.chunk = w / ctiles;
    it.c0 = (int)(w % ctiles) * TILE + 4 * (int)threadIdx.x;
    it.row0 = it.chunk * ROWS;
    const int64_t left = total_rows - it.row0;
    it.rows = left < ROWS ? (int)left : ROWS;
    return it;
}

// partial[chunk][0][c] = sum over the chunk's counted rows of a, [chunk][1][c] = of a * b, where
//   BWD = false: a = b = x                         (S1, S2)
//   BWD = true:  a = dy, b = (x - mean) * rstd     (s1, s2)
template <bool BWD>
__global__ void __launch_bounds__(THREADS)
seq_bn_sums_kernel(const float *__restrict__ a_in, const float *__restrict__ x,
                   const int32_t *__restrict__ lengths, int T, int B, int C,
                   const float *__restrict__ mean, const float *__restrict__ rstd,
                   double *__restrict__ partial) {
    const int ctiles = (C + TILE - 1) / TILE;
    const int64_t total_rows = (int64_t)T * B;
    const int64_t items = (total_rows + ROWS - 1) / ROWS * ctiles;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const Item it = work_item(w, ctiles, total_rows);
        if (it.c0 >= C) continue;
        float mu[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
        if (BWD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { mu[k] = mean[it.c0 + k]; rs[k] = rstd[it.c0 + k]; }
        }
        double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
        int t = (int)(it.row0 / B), b = (int)(it.row0 % B);
#pragma unroll 8
        for (int j = 0; j < it.rows; ++j) {
            if (t < counted_len(lengths, b, T)) {
                const size_t at = (size_t)(it.row0 + j) * C + it.c0;
                const float4 av = *reinterpret_cast<const float4 *>(a_in + at);
                const float a[4] = {av.x, av.y, av.z, av.w};
                float bb[4] = {av.x, av.y, av.z, av.w};
                if (BWD) {
                    const float4 xv = *reinterpret_cast<const float4 *>(x + at);
                    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) bb[k] = (xs[k] - mu[k]) * rs[k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s1[k] += (double)a[k];
                    s2[k] = fma((double)a[k], (double)bb[k], s2[k]);
                }
            }
            if (++b == B) { b = 0; ++t; }
        }
        double *out = partial + (size_t)it.chunk * 2 * C + it.c0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { out[k] = s1[k]; out[C + k] = s2[k]; }
    }
}

// the chunk sums of channel c in ascending chunk order
__device__ __forceinline__ void add_chunks(const double *__restrict__ partial, int64_t chunks,
                                           int C, int c, double &s1, double &s2) {
    s1 = 0.0;
    s2 = 0.0;
    // (eight chunks' loads in flight at a time; the additions keep their order)
    int64_t k = 0;
    for (; k + 8 <= chunks; k += 8) {
        double a[8], b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a[j] = partial[(size_t)(k + j) * 2 * C + c];
            b[j] = partial[(size_t)(k + j) * 2 * C + C + c];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { s1 += a[j]; s2 += b[j]; }
    }
    for (; k < chunks; ++k) {
        s1 += partial[(size_t)k * 2 * C + c];
        s2 += partial[(size_t)k * 2 * C + C + c];
    }
}

__global__ void __launch_bounds__(FINISH_THREADS)
seq_bn_fwd_finish_kernel(const double *__restrict__ partial, const int32_t *__restrict__ lengths,
                         int T, int B, int C, double decay, double eps,
                         float *__restrict__ running_mean, float *__restrict__ running_var,
                         float *__restrict__ mean, float *__restrict__ rstd) {
    const int c = blockIdx.x * FINISH_THREADS + threadIdx.x;
    if (c >= C) return;
    const int64_t n = counted_rows(lengths, T, B);
    if (n == 0) {
        mean[c] = 0.f;
        rstd[c] = 0.f;
        return;
    }
    double s1, s2;
    add_chunks(partial, ((int64_t)T * B + ROWS - 1) / ROWS, C, c, s1, s2);
    const double mean64 = s1 / (double)n;
    const double sq = mean64 * mean64;
    double var64 = s2 / (double)n - sq;
    if (var64 < 0.0) var64 = 0.0;           // (a NaN stays a NaN)
    const double rstd64 = 1.0 / sqrt(var64 + eps);
    mean[c] = (float)mean64;
    rstd[c] = (float)rstd64;
    if (isfinite(mean64) && isfinite(var64)) {
        const double keep = decay * (double)running_mean[c], take = (1.0 - decay) * mean64;
        running_mean[c] = (float)(keep + take);
        const double keep_v = decay * (double)running_var[c], take_v = (1.0 - decay) * var64;
        running_var[c] = (float)(keep_v + take_v);
    }
}

__global__ void __launch_bounds__(FINISH_THREADS)
seq_bn_bwd_finish_kernel(const double *__restrict__ partial, const int32_t *__restrict__ lengths,
                         int T, int B, int C, float *__restrict__ dgamma,
                         float *__restrict__ dbeta, float *__restrict__ m12) {
    const int c = blockIdx.x * FINISH_THREADS + threadIdx.x;
    if (c >= C) return;
    const int64_t n = counted_rows(lengths, T, B);
    if (n == 0) {
        m12[c] = 0.f;
        m12[C + c] = 0.f;
        return;
    }
    double s1, s2;
    add_chunks(partial, ((int64_t)T * B + ROWS - 1) / ROWS, C, c, s1, s2);
    dbeta[c] += (float)s1;
    dgamma[c] += (float)s2;
    m12[c] = (float)(s1 / (double)n);
    m12[C + c] = (float)(s2 / (double)n);
}

// MODE 0: y = fmaf(x - mean, gamma * rstd, beta), rstd given
// MODE 1: the same with rstd = (float)(1 / sqrt((double)var + eps)) (`rstd` points at the variance)
// MODE 2: dx = a * ((dy - m1) - xhat * m2); `in` is dy, `m12` holds m1 [C] then m2 [C]
template <int MODE>
__global__ void __launch_bounds__(THREADS)
seq_bn_apply_kernel(const float *__restrict__ in, const float *__restrict__ x,
                    const int32_t *__restrict__ lengths, int T, int B, int C,
                    const float *__restrict__ mean, const float *__restrict__ rstd,
                    const float *__restrict__ gamma, const float *__restrict__ beta,
                    const float *__restrict__ m12, double eps, float *__restrict__ out) {
    const int ctiles = (C + TILE - 1) / TILE;
    const int64_t total_rows = (int64_t)T * B;
    const int64_t items = (total_rows + ROWS - 1) / ROWS * ctiles;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const Item it = work_item(w, ctiles, total_rows);
        if (it.c0 >= C) continue;
        float mu[4], rs[4], a[4], sh[4], m1[4], m2[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = it.c0 + k;
            mu[k] = mean[c];
            rs[k] = MODE == 1 ? (float)(1.0 / sqrt((double)rstd[c] + eps)) : rstd[c];
            a[k] = gamma[c] * rs[k];
            sh[k] = MODE == 2 ? 0.f : beta[c];
            m1[k] = MODE == 2 ? m12[c] : 0.f;
            m2[k] = MODE == 2 ? m12[C + c] : 0.f;
        }
        int t = (int)(it.row0 / B), b = (int)(it.row0 % B);
#pragma unroll 4
        for (int j = 0; j < it.rows; ++j) {
            const size_t at = (size_t)(it.row0 + j) * C + it.c0;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < counted_len(lengths, b, T)) {
                const float4 xv = *reinterpret_cast<const float4 *>(x + at);
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
                float r[4];
                if (MODE == 2) {
                    const float4 dv = *reinterpret_cast<const float4 *>(in + at);
                    const float ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float xhat = (xs[k] - mu[k]) * rs[k];
                        const float left = ds[k] - m1[k], right = xhat * m2[k];
                        r[k] = a[k] * (left - right);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) r[k] = fmaf(xs[k] - mu[k], a[k], sh[k]);
                }
                o = make_float4(r[0], r[1], r[2], r[3]);
            }
            *reinterpret_cast<float4 *>(out + at) = o;
            if (++b == B) { b = 0; ++t; }
        }
    }
}

int64_t chunk_count(int64_t rows) { return (rows + ROWS - 1) / ROWS; }

bool bad_shape(int T, int B, int C) {
    return T < 1 || B < 1 || (int64_t)T * B > 0x7FFFFFFFll || C < 4 || C % 4 != 0;
}

bool misaligned(const void *p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace

int g_seq_bn_blocks = 0;        // ctcasr_set_option("seq_bn_blocks", k); 0 = DEFAULT_BLOCKS

namespace {
int stream_blocks(int T, int B, int C) {
    const int64_t items = chunk_count((int64_t)T * B) * ((C + TILE - 1) / TILE);
    const int64_t cap = g_seq_bn_blocks > 0 ? g_seq_bn_blocks : DEFAULT_BLOCKS;
    return (int)(items < cap ? items : cap);
}
}  // namespace

extern "C" size_t ctcasr_seq_bn_workspace_bytes(int64_t rows, int C) {
    if (rows < 1 || rows > 0x7FFFFFFFll || C < 4 || C % 4 != 0) return 0;
    // chunk sums [chunks][2][C] fp64, then m1 [C] and m2 [C] fp32 of the backward pass
    return (size_t)chunk_count(rows) * 2 * C * sizeof(double) + (size_t)2 * C * sizeof(float);
}

extern "C" int ctcasr_seq_bn_fwd(const float *x, const int32_t *lengths, int T, int B, int C,
                                 const float *gamma, const float *beta, float *running_mean,
                                 float *running_var, double decay, double eps, float *y,
                                 float *mean, float *rstd, void *workspace,
                                 size_t workspace_bytes, ctcasr_stream_t stream) {
    if (!x || !gamma || !beta || !running_mean || !running_var || !y || !mean || !rstd ||
        bad_shape(T, B, C) || misaligned(x, 16) || misaligned(y, 16) ||
        !(decay >= 0.0 && decay <= 1.0) || !(eps > 0.0 && isfinite(eps)))
        return CTCASR_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < ctcasr_seq_bn_workspace_bytes((int64_t)T * B, C) ||
        misaligned(workspace, sizeof(double)))
        return CTCASR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *partial = static_cast<double *>(workspace);
    const int blocks = stream_blocks(T, B, C);
    seq_bn_sums_kernel<false><<<blocks, THREADS, 0, s>>>(x, x, lengths, T, B, C, nullptr, nullptr,
                                                         partial);
    seq_bn_fwd_finish_kernel<<<(C + FINISH_THREADS - 1) / FINISH_THREADS, FINISH_THREADS, 0, s>>>(
        partial, lengths, T, B, C, decay, eps, running_mean, running_var, mean, rstd);
    seq_bn_apply_kernel<0><<<blocks, THREADS, 0, s>>>(nullptr, x, lengths, T, B, C, mean, rstd,
                                                      gamma, beta, nullptr, eps, y);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_seq_bn_infer(const float *x, const int32_t *lengths, int T, int B, int C,
                                   const float *gamma, const float *beta,
                                   const float *running_mean, const float *running_var,
                                   double eps, float *y, ctcasr_stream_t stream) {
    if (!x || !gamma || !beta || !running_mean || !running_var || !y || bad_shape(T, B, C) ||
        misaligned(x, 16) || misaligned(y, 16) || !(eps > 0.0 && isfinite(eps)))
        return CTCASR_ERR_BAD_ARGUMENT;
    seq_bn_apply_kernel<1><<<stream_blocks(T, B, C), THREADS, 0, (hipStream_t)stream>>>(
        nullptr, x, lengths, T, B, C, running_mean, running_var, gamma, beta, nullptr, eps, y);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_seq_bn_bwd(const float *dy, const float *x, const int32_t *lengths, int T,
                                 int B, int C, const float *mean, const float *rstd,
                                 const float *gamma, float *dgamma, float *dbeta, float *dx,
                                 void *workspace, size_t workspace_bytes,
                                 ctcasr_stream_t stream) {
    if (!dy || !x || !mean || !rstd || !gamma || !dgamma || !dbeta || !dx ||
        bad_shape(T, B, C) || misaligned(dy, 16) || misaligned(x, 16) || misaligned(dx, 16))
        return CTCASR_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < ctcasr_seq_bn_workspace_bytes((int64_t)T * B, C) ||
        misaligned(workspace, sizeof(double)))
        return CTCASR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *partial = static_cast<double *>(workspace);
    float *m12 = reinterpret_cast<float *>(partial + (size_t)chunk_count((int64_t)T * B) * 2 * C);
    const int blocks = stream_blocks(T, B, C);
    seq_bn_sums_kernel<true><<<blocks, THREADS, 0, s>>>(dy, x, lengths, T, B, C, mean, rstd,
                                                        partial);
    seq_bn_bwd_finish_kernel<<<(C + FINISH_THREADS - 1) / FINISH_THREADS, FINISH_THREADS, 0, s>>>(
        partial, lengths, T, B, C, dgamma, dbeta, m12);
    seq_bn_apply_kernel<2><<<blocks, THREADS, 0, s>>>(dy, x, lengths, T, B, C, mean, rstd, gamma,
                                                      nullptr, m12, 0.0, dx);
    return ctcasr_launch_status();
}
