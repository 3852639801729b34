// K15: augmentation of training batches (include/ctcasr.h): SpecAugment masks stored into the
// features, band-limited speed perturbation of the PCM.  Every draw and every tap position is
// integer arithmetic pinned in the header; tests/augment_reference.py restates both in numpy.
#include "common.h"

#include <limits.h>

namespace {

constexpr int SA_COLS = 80;          // feature columns
constexpr int SA_TILE = 64;          // frames per workgroup
constexpr int SA_THREADS = 256;
constexpr int SA_MAX_MASKS = CTCASR_SPEC_AUGMENT_MAX_MASKS;

__device__ __forceinline__ int below(uint64_t seed, uint64_t idx, int64_t n) {
    return (int)(((uint64_t)splitmix64_r24(seed, idx) * (uint64_t)n) >> 24);
}

// grid = B x ceil(out_frames / SA_TILE) workgroups (at least one per row: it writes `intervals`).
// Every workgroup redoes the <= 32 draws of its row - 64 integer multiplies - instead of reading
// them from a table a launch of its own would have to fill.  Stores only: a tile's cells are
// walked in memory order and a masked cell is stored +0, so a wave's stores inside a time span
// are 256 contiguous bytes and inside a frequency band one run per frame.
__global__ void __launch_bounds__(SA_THREADS)
spec_augment_kernel(float *__restrict__ feat, const int32_t *__restrict__ lengths, int out_frames,
                    uint64_t seed, int n_freq, int freq_width, int n_time, int time_width,
                    int time_permille, int32_t *__restrict__ intervals, int tiles) {
    __shared__ int s_start[2 * SA_MAX_MASKS], s_width[2 * SA_MAX_MASKS];
    __shared__ unsigned char s_col[SA_COLS], s_frame[SA_TILE];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int masks = n_freq + n_time;
    const int L = min(max(lengths[b], 0), out_frames);
    if (tid < masks) {
        int start = 0, width = 0;
        if (L > 0 && tid < n_freq) {
            const uint64_t idx = 64ull * (uint64_t)b + 2ull * (uint64_t)tid;
            width = below(seed, idx, min(freq_width, SA_COLS) + 1);
            start = below(seed, idx + 1, SA_COLS - width + 1);
        } else if (L > 0) {
            const uint64_t idx = 64ull * (uint64_t)b + 32ull + 2ull * (uint64_t)(tid - n_freq);
            const int64_t cap = min((int64_t)time_width, (int64_t)L * time_permille / 1000);
            width = below(seed, idx, cap + 1);
            start = below(seed, idx + 1, (int64_t)L - width + 1);
        }
        s_start[tid] = start;
        s_width[tid] = width;
        if (tile == 0 && intervals) {
            int32_t *dst = intervals + ((size_t)b * masks + tid) * 2;
            dst[0] = start;
            dst[1] = width;
        }
    }
    __syncthreads();
    const int t_lo = tile * SA_TILE;
    if (t_lo >= L) return;                                   // (uniform over the workgroup)
    const int t_hi = min(t_lo + SA_TILE, L);
    if (tid < SA_COLS) {
        bool hit = false;
        for (int i = 0; i < n_freq; ++i) hit |= tid >= s_start[i] && tid < s_start[i] + s_width[i];
        s_col[tid] = hit;
    } else if (tid < SA_COLS + SA_TILE) {
        const int t = t_lo + tid - SA_COLS;
        bool hit = false;
        for (int i = n_freq; i < masks; ++i) hit |= t >= s_start[i] && t < s_start[i] + s_width[i];
        s_frame[tid - SA_COLS] = hit;
    }
    __syncthreads();
    float *base = feat + ((size_t)b * out_frames + t_lo) * SA_COLS;
    const int cells = (t_hi - t_lo) * SA_COLS;
    for (int e = tid; e < cells; e += SA_THREADS) {
        const int t = e / SA_COLS, f = e - t * SA_COLS;
        if (s_frame[t] | s_col[f]) base[e] = 0.0f;
    }
}

constexpr int SP_THREADS = 256;
constexpr int SP_CHUNK = 2048;       // output samples per workgroup
constexpr int SP_MAX_TAPS = 52;      // 2 R + 2 at P = 200
constexpr int SP_MAX_PHASES = 100;

__host__ __device__ inline int resample_count(int n, int percent) {
    if (n < 1 || percent < 50 || percent > 200) return 0;
    const int64_t out = (int64_t)n * 100 / percent;
    return out < 1 ? 1 : (out > INT_MAX ? INT_MAX : (int)out);
}

// h(d) of the header, in fp64
__device__ double tap_weight(double c, double d) {
    const double pi = 3.14159265358979323846;
    const double u = c * d;
    if (fabs(u) >= 12.0) return 0.0;
    const double s = u == 0.0 ? 1.0 : sin(pi * u) / (pi * u);
    return c * s * 0.5 * (1.0 + cos(pi * u / 12.0));
}

// grid = B x ceil(max_out / SP_CHUNK) workgroups; a workgroup writes EVERY column of its chunk
// (samples, then zeros).  Tap weights: one LDS table per workgroup, [phase][tap], built in fp64
// from the row's own percent - a row reaches 100 / gcd(P, 100) phases (10 at P = 90 and 110, so
// 280 weights, about one per thread, against 2048 x 28 multiply-adds); no table outlives the
// launch and the percents never have to be known on the host.  The PCM is read
// through the caches: neighbouring outputs share all but one or two of their taps.
__global__ void __launch_bounds__(SP_THREADS)
speed_perturb_kernel(const int16_t *__restrict__ pcm, const int32_t *__restrict__ num_samples,
                     const int32_t *__restrict__ percent, int max_in, int16_t *__restrict__ out,
                     int max_out, int32_t *__restrict__ out_samples, int chunks) {
    __shared__ float s_w[SP_MAX_PHASES * SP_MAX_TAPS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int n = num_samples[b], P = percent[b];
    const bool ok = n >= 1 && n <= max_in && P >= 50 && P <= 200;
    const int n_out = ok ? min(resample_count(n, P), max_out) : 0;
    if (chunk == 0 && tid == 0) out_samples[b] = n_out;
    const int j0 = chunk * SP_CHUNK, j1 = min(j0 + SP_CHUNK, max_out);
    const int16_t *x = pcm + (size_t)b * max_in;
    int16_t *y = out + (size_t)b * max_out;
    if (!ok || P == 100 || j0 >= n_out) {
        // a bad row (n_out = 0: no PCM is read), the tail of a row, or the bit copy of P = 100
        // (n_out <= n there)
        for (int j = j0 + tid; j < j1; j += SP_THREADS) y[j] = j < n_out ? x[j] : (int16_t)0;
        return;
    }
    int g = P, r = 100;                                      // gcd(P, 100)
    while (r) { const int q = g % r; g = r; r = q; }
    const int radius = 12 * max(P, 100) / 95, taps = 2 * radius + 2;
    const double c = 95.0 / (double)max(P, 100);
    for (int e = tid; e < (100 / g) * taps; e += SP_THREADS) {
        const int q = e / taps, i = e - q * taps;
        s_w[e] = (float)tap_weight(c, (double)(q * g) / 100.0 - (double)(i - radius));
    }
    __syncthreads();
    for (int j = j0 + tid; j < j1; j += SP_THREADS) {
        int16_t v = 0;
        if (j < n_out) {
            const uint64_t pos = (uint64_t)j * (uint64_t)P;
            const int t0 = (int)(pos / 100), phase = (int)(pos % 100);   // t0 <= n - 1
            const float *w = s_w + (phase / g) * taps;
            const int k_lo = t0 - radius;
            const int i_lo = max(0, -k_lo), i_hi = min(taps, n - k_lo);  // 0 <= k_lo + i < n
            float acc = 0.0f;
            for (int i = i_lo; i < i_hi; ++i) acc = fmaf((float)x[k_lo + i], w[i], acc);
            v = (int16_t)fminf(fmaxf(rintf(acc), -32768.0f), 32767.0f);
        }
        y[j] = v;
    }
}

}  // namespace

extern "C" int ctcasr_spec_augment(float *features, const int32_t *lengths, int B, int out_frames,
                                   uint64_t seed, int n_freq, int freq_width, int n_time,
                                   int time_width, int time_permille, int32_t *intervals,
                                   ctcasr_stream_t stream) {
    // an empty [B, 0, 80] buffer has no address to give: no cell of it is ever stored to
    if ((!features && out_frames != 0) || !lengths || B < 1 || out_frames < 0)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (n_freq < 0 || n_freq > SA_MAX_MASKS || n_time < 0 || n_time > SA_MAX_MASKS)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (freq_width < 0 || time_width < 0 || time_permille < 0 || time_permille > 1000)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (out_frames >= 1 << 24) return CTCASR_ERR_UNSUPPORTED;      // below() draws from n <= 2^24
    if (n_freq + n_time == 0) return CTCASR_OK;
    const int64_t tiles = out_frames > 0 ? ((int64_t)out_frames + SA_TILE - 1) / SA_TILE : 1;
    if (tiles * B > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(spec_augment_kernel, dim3((unsigned)(tiles * B)), dim3(SA_THREADS), 0,
                       (hipStream_t)stream, features, lengths, out_frames, seed, n_freq,
                       freq_width, n_time, time_width, time_permille, intervals, (int)tiles);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_resample_num_samples(int num_samples, int percent) {
    return resample_count(num_samples, percent);
}

extern "C" int ctcasr_speed_perturb(const int16_t *pcm, const int32_t *num_samples,
                                    const int32_t *percent, int B, int max_in, int16_t *out,
                                    int max_out, int32_t *out_samples, ctcasr_stream_t stream) {
    if (!pcm || !num_samples || !percent || !out || !out_samples || B < 1 || max_in < 1 ||
        max_out < 1)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (max_in > 1 << 30 || max_out > 1 << 30) return CTCASR_ERR_UNSUPPORTED;
    const int64_t chunks = ((int64_t)max_out + SP_CHUNK - 1) / SP_CHUNK;
    if (chunks * B > INT_MAX) return CTCASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(speed_perturb_kernel, dim3((unsigned)(chunks * B)), dim3(SP_THREADS), 0,
                       (hipStream_t)stream, pcm, num_samples, percent, max_in, out, max_out,
                       out_samples, (int)chunks);
    return ctcasr_launch_status();
}
