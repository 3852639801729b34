// K19: sampling-rate conversion and channel downmix of one recording (include/ctcasr.h).  Any
// interleaved uint8 / int16 / int32 / float32 PCM of 1..8 channels at rate_in becomes int16 mono
// at rate_out: the Hann-windowed sinc of ctcasr_speed_perturb at the ratio M : L of the two rates
// in lowest terms, positions in integers, weights in fp64 rounded once.
// tests/resample_reference.py restates it in numpy.
//
// The weights.  A pair of rates reaches L phases of `taps` weights each: 160 x 70 at 44 100 ->
// 16 000, 640 x 26 at 11 025.  ctcasr_resample_table evaluates them once, in a launch of its own,
// into global memory; every workgroup of the resampler copies the table into LDS (16 bytes per
// lane) and never evaluates a sine.  (ctcasr_speed_perturb rebuilds its at most 100 x 52 weights in
// every workgroup, because each row of a batch has its own ratio; here one ratio serves the
// whole recording and the table may be 40 times as large.)
//
// The samples.  A workgroup owns `chunk` consecutive outputs and so a span of chunk * M / L + taps
// input frames.  The span's bytes come through LDS: aligned 16-byte loads, RAW_BYTES per pass,
// land in a raw image that keeps every byte's address modulo 16, so an element is read from the
// image at its natural alignment whatever the base pointer and the frame size are; each frame is
// then downmixed ONCE to the fp32 frame value of the header and stored in the tile.  The taps run
// from the tile.  Frames outside [0, n) are zeros in the tile, and a tap on a zero leaves the
// accumulator as it was, so the ends of the recording need no other care.
//
// `chunk` (ctcasr_resample_chunk) is the largest of 2048, 1024, 512 and 256 outputs whose table
// and tile fit SMALL_FLOATS of LDS (four workgroups per CU next to the raw image), or, for the
// tables that alone are larger than that, LARGE_FLOATS (two per CU).  Every output is computed
// from the same frame values, weights and order of additions whichever workgroup it falls into.
#include "common.h"

#include <limits.h>

namespace {

constexpr int THREADS = 256;
constexpr int MAX_CHUNK = 2048, MIN_CHUNK = 256;
constexpr int MAX_FRAME_BYTES = 32;                   // 8 channels of 4 bytes
constexpr int RAW_BYTES = 8192;                       // input bytes per pass: two loads per lane
// a frame that starts inside a pass ends inside the slack behind it
constexpr int RAW_WORDS = (RAW_BYTES + MAX_FRAME_BYTES) / 16;
constexpr int SMALL_FLOATS = 7680;                    // 30 KiB + raw image: 4 workgroups per CU
constexpr int LARGE_FLOATS = 18400;                   // 71.9 KiB + raw image: 2 workgroups per CU
constexpr int MIN_RATE = 4000, MAX_RATE = 192000;
static_assert(RAW_BYTES % 16 == 0 && MAX_FRAME_BYTES % 16 == 0, "whole 16-byte words");
static_assert(4 * (SMALL_FLOATS * 4 + RAW_WORDS * 16) <= 160 * 1024, "four per CU");
static_assert(2 * (LARGE_FLOATS * 4 + RAW_WORDS * 16) <= 160 * 1024, "two per CU");
static_assert(CTCASR_RESAMPLE_MAX_TABLE + MIN_CHUNK <= LARGE_FLOATS, "the largest table fits");
// p_base + q * M of the output loop stays a uint32
static_assert((int64_t)MAX_CHUNK * MAX_RATE + MAX_RATE < INT_MAX, "32-bit phase arithmetic");

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

struct Plan {
    int M, L, radius, taps;
    int table_floats;       // L * taps rounded up to 4; 0 when M == L (no filter)
    int chunk;              // outputs per workgroup
    bool large;             // LARGE_FLOATS of LDS
};

// frames a run of `chunk` outputs reaches: floor((chunk - 1) M / L) + 1 first taps, taps - 1 more
inline int64_t span_bound(int chunk, int M, int L, int taps) {
    return ((int64_t)(chunk - 1) * M) / L + 1 + (taps > 0 ? taps - 1 : 0) + 1;
}

int make_plan(int rate_in, int rate_out, Plan *plan) {
    if (rate_in < MIN_RATE || rate_in > MAX_RATE || rate_out < MIN_RATE || rate_out > MAX_RATE)
        return CTCASR_ERR_BAD_ARGUMENT;
    int g = rate_in, r = rate_out;
    while (r) { const int q = g % r; g = r; r = q; }
    Plan p;
    p.M = rate_in / g;
    p.L = rate_out / g;
    const int64_t S = p.M > p.L ? p.M : p.L;
    p.radius = (int)((1200 * S) / (95 * (int64_t)p.L));
    p.taps = 2 * p.radius + 2;
    if ((int64_t)p.L * p.taps > CTCASR_RESAMPLE_MAX_TABLE) return CTCASR_ERR_UNSUPPORTED;
    const bool filter = p.M != p.L;
    p.table_floats = filter ? (p.L * p.taps + 3) & ~3 : 0;
    p.chunk = 0;
    for (int pass = 0; pass < 2 && !p.chunk; ++pass) {
        const int cap = pass ? LARGE_FLOATS : SMALL_FLOATS;
        for (int chunk = MAX_CHUNK; chunk >= MIN_CHUNK; chunk >>= 1)
            if (p.table_floats + span_bound(chunk, p.M, p.L, filter ? p.taps : 0) <= cap) {
                p.chunk = chunk;
                p.large = pass == 1;
                break;
            }
    }
    if (!p.chunk) return CTCASR_ERR_UNSUPPORTED;      // (a long filter next to a large table)
    *plan = p;
    return CTCASR_OK;
}

inline int64_t out_samples(int64_t n, const Plan &p) {
    if (n < 1 || n > INT_MAX) return 0;
    const int64_t out = n * p.L / p.M;                // n < 2^31, L < 2^18
    return out < 1 ? 1 : out;
}

// h(d) of the ctcasr_speed_perturb block of the header, in fp64
__device__ double tap_weight(double c, double d) {
    const double pi = 3.14159265358979323846;
    const double u = c * d;
    if (fabs(u) >= 12.0) return 0.0;
    const double s = u == 0.0 ? 1.0 : sin(pi * u) / (pi * u);
    return c * s * 0.5 * (1.0 + cos(pi * u / 12.0));
}

// table[p][i] = h(p / L - (i - R)); entries behind L * taps (the pad to 16 bytes) are zero
__global__ void __launch_bounds__(THREADS)
resample_table_kernel(float *__restrict__ table, int M, int L, int radius, int taps, int floats) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= floats) return;
    const int p = e / taps, i = e - p * taps;
    const double S = (double)(M > L ? M : L);
    const double c = (95.0 * (double)L) / (100.0 * S);
    table[e] = p < L ? (float)tap_weight(c, (double)p / (double)L - (double)(i - radius)) : 0.0f;
}

// the frame value of the header: the fp32 sum over the channels, in ascending order, of each
// sample on the int16 scale.  `p` points into the raw LDS image, at the element's own alignment.
__device__ __forceinline__ float frame_value(const unsigned char *p, int format, int channels,
                                             bool &bad) {
    float s = 0.0f;
    switch (format) {
    case CTCASR_PCM_S16: {
        const int16_t *x = reinterpret_cast<const int16_t *>(p);
        s = (float)x[0];
        for (int c = 1; c < channels; ++c) s += (float)x[c];
        break;
    }
    case CTCASR_PCM_U8: {
        s = (float)(((int)p[0] - 128) * 256);
        for (int c = 1; c < channels; ++c) s += (float)(((int)p[c] - 128) * 256);
        break;
    }
    case CTCASR_PCM_S32: {
        const int32_t *x = reinterpret_cast<const int32_t *>(p);
        s = (float)x[0] * 0x1p-16f;
        for (int c = 1; c < channels; ++c) s += (float)x[c] * 0x1p-16f;
        break;
    }
    default: {
        const float *x = reinterpret_cast<const float *>(p);
        for (int c = 0; c < channels; ++c) bad |= !isfinite(x[c]);
        s = x[0] * 32768.0f;
        for (int c = 1; c < channels; ++c) s += x[c] * 32768.0f;
        break;
    }
    }
    return s;
}

// grid = ceil(n_out / chunk).  taps == 0: no filter (M == L), out[j] is the scaled frame value.
template <int LDS_FLOATS>
__global__ void __launch_bounds__(THREADS)
resample_kernel(const unsigned char *__restrict__ in, int format, int channels, int64_t n, int M,
                int L, int radius, int taps, int table_floats, int chunk,
                const float *__restrict__ table, int16_t *__restrict__ out, int64_t n_out,
                float gain, int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) float s_mem[LDS_FLOATS];
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[RAW_WORDS * 16];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * chunk;
    const int count = (int)(n_out - j0 < chunk ? n_out - j0 : chunk);
    const u64 pos0 = (u64)j0 * (u64)M;
    const int64_t t_base = (int64_t)(pos0 / (u64)L);           // t0 of the first output
    const uint32_t p_base = (uint32_t)(pos0 % (u64)L);         // its phase
    const int64_t k_lo = t_base - radius;                      // the frame tile[0] holds
    const int span = (int)((p_base + (uint32_t)(count - 1) * (uint32_t)M) / (uint32_t)L) +
        (taps > 0 ? taps : 1);
    if (count < 1 || table_floats + span > LDS_FLOATS) return;  // (ruled out by the host's plan)
    float *s_w = s_mem, *s_x = s_mem + table_floats;

    for (int e = tid; e < table_floats / 4; e += THREADS)
        reinterpret_cast<f32x4 *>(s_w)[e] = reinterpret_cast<const f32x4 *>(table)[e];
    for (int e = tid; e < span; e += THREADS) {
        const int64_t k = k_lo + e;
        if (k < 0 || k >= n) s_x[e] = 0.0f;
    }

    // frames [ka, kb) of the span lie inside the recording; their bytes are [ka * fb, kb * fb)
    const int fb = channels * (format == CTCASR_PCM_U8 ? 1 : format == CTCASR_PCM_S16 ? 2 : 4);
    const int64_t ka = k_lo > 0 ? k_lo : 0, kb = k_lo + span < n ? k_lo + span : n;
    bool bad = false;
    if (ka < kb) {
        const int64_t end = kb * fb;
        // the window starts at the 16-byte boundary at or below the first byte: up to 15 bytes
        // below it (and below `in` itself, inside the granule that holds in[0])
        const int64_t first = ka * fb - (int64_t)(reinterpret_cast<uintptr_t>(in + ka * fb) & 15);
        for (int64_t w = first; w < end; w += RAW_BYTES) {
            for (int q = tid; q < RAW_WORDS; q += THREADS) {
                const int64_t b = w + 16 * q;                  // w <= b: the word holds a byte of
                if (b < end)                                   // [ka * fb, end), so it may be read
                    reinterpret_cast<u64x2 *>(s_raw)[q] = *reinterpret_cast<const u64x2 *>(in + b);
            }
            __syncthreads();
            // the frames that START in [w, w + RAW_BYTES)
            const int64_t kf = w <= ka * fb ? ka : (w + fb - 1) / fb;
            const int64_t stop = (w + RAW_BYTES + fb - 1) / fb;
            const int64_t ke = stop < kb ? stop : kb;
            for (int64_t k = kf + tid; k < ke; k += THREADS)
                s_x[k - k_lo] = frame_value(s_raw + (k * fb - w), format, channels, bad);
            __syncthreads();
        }
    } else {
        __syncthreads();
    }
    if (bad) atomicOr(status, 1);

    for (int q = tid; q < count; q += THREADS) {
        const uint32_t a = p_base + (uint32_t)q * (uint32_t)M;
        const uint32_t t = a / (uint32_t)L, p = a - t * (uint32_t)L;
        const float *x = s_x + t;
        float acc = 0.0f;
        if (taps > 0) {
            const float *wt = s_w + p * taps;
#pragma unroll 2
            for (int i = 0; i < taps; ++i) acc = fmaf(x[i], wt[i], acc);
        } else {
            acc = x[0];
        }
        out[j0 + q] = (int16_t)fminf(fmaxf(rintf(acc * gain), -32768.0f), 32767.0f);
    }
}

}  // namespace

extern "C" int ctcasr_resample_plan(int rate_in, int rate_out, int *M, int *L, int *radius,
                                    int *taps) {
    if (!M || !L || !radius || !taps) return CTCASR_ERR_BAD_ARGUMENT;
    Plan p;
    const int rc = make_plan(rate_in, rate_out, &p);
    if (rc != CTCASR_OK) return rc;
    *M = p.M;
    *L = p.L;
    *radius = p.radius;
    *taps = p.taps;
    return CTCASR_OK;
}

extern "C" int ctcasr_resample_chunk(int rate_in, int rate_out) {
    Plan p;
    return make_plan(rate_in, rate_out, &p) == CTCASR_OK ? p.chunk : 0;
}

extern "C" int64_t ctcasr_resample_out_samples(int64_t n, int rate_in, int rate_out) {
    Plan p;
    return make_plan(rate_in, rate_out, &p) == CTCASR_OK ? out_samples(n, p) : 0;
}

extern "C" size_t ctcasr_resample_table_bytes(int rate_in, int rate_out) {
    Plan p;
    if (make_plan(rate_in, rate_out, &p) != CTCASR_OK) return 0;
    return (size_t)((p.L * p.taps + 3) & ~3) * sizeof(float);
}

extern "C" int ctcasr_resample_table(int rate_in, int rate_out, float *table,
                                     ctcasr_stream_t stream) {
    if (!table || reinterpret_cast<uintptr_t>(table) % 16) return CTCASR_ERR_BAD_ARGUMENT;
    Plan p;
    const int rc = make_plan(rate_in, rate_out, &p);
    if (rc != CTCASR_OK) return rc;
    const int floats = (p.L * p.taps + 3) & ~3;
    hipLaunchKernelGGL(resample_table_kernel, dim3((unsigned)((floats + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, (hipStream_t)stream, table, p.M, p.L, p.radius, p.taps,
                       floats);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_resample(const void *in, int format, int channels, int64_t n, int rate_in,
                               int rate_out, const float *table, int16_t *out, int64_t n_out,
                               int32_t *status, ctcasr_stream_t stream) {
    if (!in || !table || !out || !status || format < 0 || format > 3 || channels < 1 ||
        channels > 8 || n < 1)
        return CTCASR_ERR_BAD_ARGUMENT;
    const int element = format == CTCASR_PCM_U8 ? 1 : format == CTCASR_PCM_S16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(in) % element || reinterpret_cast<uintptr_t>(table) % 16 ||
        reinterpret_cast<uintptr_t>(out) % 2 || reinterpret_cast<uintptr_t>(status) % 4)
        return CTCASR_ERR_BAD_ARGUMENT;
    Plan p;
    const int rc = make_plan(rate_in, rate_out, &p);
    if (rc != CTCASR_OK) return rc;
    if (n > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    if (n_out != out_samples(n, p)) return CTCASR_ERR_BAD_ARGUMENT;
    const int64_t groups = (n_out + p.chunk - 1) / p.chunk;
    if (groups > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return CTCASR_ERR_LAUNCH;
    const bool filter = p.M != p.L;
    const float gain = (float)(1.0 / channels);
    const unsigned char *bytes = static_cast<const unsigned char *>(in);
    const int radius = filter ? p.radius : 0, taps = filter ? p.taps : 0;
    if (p.large)
        hipLaunchKernelGGL(resample_kernel<LARGE_FLOATS>, dim3((unsigned)groups), dim3(THREADS),
                           0, s, bytes, format, channels, n, p.M, p.L, radius, taps,
                           p.table_floats, p.chunk, table, out, n_out, gain, status);
    else
        hipLaunchKernelGGL(resample_kernel<SMALL_FLOATS>, dim3((unsigned)groups), dim3(THREADS),
                           0, s, bytes, format, channels, n, p.M, p.L, radius, taps,
                           p.table_floats, p.chunk, table, out, n_out, gain, status);
    return ctcasr_launch_status();
}
