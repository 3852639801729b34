// K11: CTC forced alignment - the Viterbi (max-sum) form of the alpha recursion of ctc.hip.
//
// One workgroup per utterance, as the loss's ctc_sweep_kernel: the extended-label lattice (two
// fp64 rows, 384 threads x 3 states) and the per-utterance fp32 log-softmax table live in LDS.
// The new part is the back-pointer slab: every step records for each state which predecessor won
// (0: s, 1: s - 1, 2: s - 2), 2 bits per (t, s).  Within a wave the 64 consecutive states give
// two __ballot words (low bit, high bit), and lane 0 stores the pair as 16 bytes: the slab is
// T x ceil(s_pad / 64) x 16 B per utterance, in LDS when table + lattice + slab fit, in the
// workspace otherwise.  Both are written and read by the same workgroup: a workgroup barrier
// orders them.
//
// Backtrace without T dependent round trips: a step moves at most 2 states, so over 64 frames the
// path touches at most 3 of the 64-state words (the word of the state it starts the chunk in and
// the two below).  Lane j of wave 0 copies the words frame t0 - j could need into an LDS stage,
// then one lane walks the 64 frames from the stage: ceil(len / 64) round trips instead of len.
#include "common.h"

#define ALIGN_THREADS 384
#define ALIGN_MAX_PER_THREAD 3   // extended labels per thread: S = 2L+1 <= 1152
#define ALIGN_WAVES (ALIGN_THREADS / 64)
#define ALIGN_CHUNK 64           // frames walked per backtrace round trip
#define ALIGN_LDS_MAX (150 * 1024)

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// LDS layout (bytes), shared by the launcher and the kernel; every offset is 16-byte aligned:
//   two fp64 lattice rows | int ext[s_pad] | 16 int words | int path stage[64] |
//   back-pointer stage [64][3] x 16 B | (slab T x words x 16 B) | (log-softmax table T x C f32)
struct AlignLds {
    size_t ext, misc, spath, stage, fixed;
    __host__ __device__ AlignLds(int s_pad) {
        ext = (size_t)2 * s_pad * sizeof(double);
        misc = ext + ((size_t)s_pad * sizeof(int) + 15) / 16 * 16;
        spath = misc + 16 * sizeof(int);
        stage = spath + ALIGN_CHUNK * sizeof(int);
        fixed = stage + (size_t)ALIGN_CHUNK * 3 * sizeof(u64x2);
    }
};

static __host__ __device__ inline int align_words(int s_pad) { return (s_pad + 63) / 64; }

// misc words
#define M_BAD_LABEL 0
#define M_REPEATS 1
#define M_NONFINITE 2
#define M_STATE 3    // state of the path at the frame the next backtrace chunk starts from

template <bool LOGP_IN_LDS, bool BP_IN_LDS>
__global__ void __launch_bounds__(ALIGN_THREADS)
ctc_align_kernel(const float *__restrict__ logits, const int *__restrict__ labels,
                 const int *__restrict__ label_offsets, const int *__restrict__ seq_len, int T,
                 int B, int C, int blank, int s_pad, int *__restrict__ path,
                 float *__restrict__ score, float *__restrict__ frame_logp,
                 int *__restrict__ status, float *__restrict__ logp_ws,
                 u64x2 *__restrict__ bp_ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const AlignLds lay(s_pad);
    const int nw = align_words(s_pad);
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = label_offsets[b + 1] - label_offsets[b];
    const int S = 2 * L + 1;
    const int len = seq_len[b];
    const int *lab = labels + label_offsets[b];
    // a row longer than max_label_len (or with decreasing offsets) does not fit the lattice and
    // the slab sized from s_pad: refuse it before anything is read
    const bool unfit = L < 0 || S > s_pad;

    double *lat0 = reinterpret_cast<double *>(smem);
    double *lat1 = lat0 + s_pad;
    int *ext = reinterpret_cast<int *>(smem + lay.ext);
    int *misc = reinterpret_cast<int *>(smem + lay.misc);
    int *spath = reinterpret_cast<int *>(smem + lay.spath);
    u64x2 *stage = reinterpret_cast<u64x2 *>(smem + lay.stage);
    u64x2 *bp = BP_IN_LDS ? reinterpret_cast<u64x2 *>(smem + lay.fixed)
                          : bp_ws + (size_t)b * T * nw;
    float *logp = LOGP_IN_LDS
        ? reinterpret_cast<float *>(smem + lay.fixed + (BP_IN_LDS ? (size_t)T * nw * 16 : 0))
        : logp_ws + (size_t)b * T * C;
    int *path_row = path + (size_t)b * T;
    float *flp_row = frame_logp ? frame_logp + (size_t)b * T : nullptr;

    if (tid < 16) misc[tid] = 0;
    __syncthreads();
    for (int u = tid; u < (unfit ? 0 : S); u += ALIGN_THREADS) {
        int sym = blank;
        if (u & 1) {
            sym = lab[u >> 1];
            if (sym < 0 || sym >= C || sym == blank) atomicOr(&misc[M_BAD_LABEL], 1);
            if (u >= 3 && lab[(u >> 1) - 1] == sym) atomicAdd(&misc[M_REPEATS], 1);
        }
        ext[u] = sym;
    }
    __syncthreads();
    int st = 0;
    if (unfit || misc[M_BAD_LABEL] || len > T || len < 0) st = 2;
    else if (len < L + misc[M_REPEATS]) st = 1;

    // ---- per-utterance log-softmax table; any non-finite logit in the first len frames -> 3 ----
    if (st == 0) {
        for (int t = tid; t < len; t += ALIGN_THREADS) {
            const float *row = logits + ((size_t)t * B + b) * C;
            float mx = row[0];
            bool finite = true;
            for (int c = 0; c < C; ++c) {
                finite = finite && fabsf(row[c]) <= 3.4028235e38f;
                mx = fmaxf(mx, row[c]);
            }
            float sum = 0.f;
            for (int c = 0; c < C; ++c) sum += expf(row[c] - mx);
            const float lz = mx + logf(sum);
            if (!finite || !(fabsf(lz) <= 3.4028235e38f)) atomicOr(&misc[M_NONFINITE], 1);
            for (int c = 0; c < C; ++c) logp[t * C + c] = row[c] - lz;
        }
        __syncthreads();
        if (misc[M_NONFINITE]) st = 3;
    }

    // ---- rows without a path: every output written, then done ---------------------------------
    const int live = st == 0 ? len : 0;
    for (int t = live + tid; t < T; t += ALIGN_THREADS) {
        path_row[t] = -1;
        if (flp_row) flp_row[t] = 0.f;
    }
    if (tid == 0 && (st != 0 || len == 0)) {
        status[b] = st;
        score[b] = st == 3 ? __uint_as_float(0x7FC00000u) : (st != 0 ? -INFINITY : 0.f);
    }
    if (st != 0 || len == 0) return;

    int my_ext[ALIGN_MAX_PER_THREAD];
    bool skip_ok[ALIGN_MAX_PER_THREAD];   // may take the u-2 -> u transition
#pragma unroll
    for (int i = 0; i < ALIGN_MAX_PER_THREAD; ++i) {
        const int u = tid + i * ALIGN_THREADS;
        my_ext[i] = u < S ? ext[u] : blank;
        skip_ok[i] = u < S && u >= 2 && ext[u] != blank && ext[u] != ext[u - 2];
    }
    const int live_words = (S + 63) >> 6;

    // ---- forward max-sum sweep with back-pointers ---------------------------------------------
#pragma unroll
    for (int i = 0; i < ALIGN_MAX_PER_THREAD; ++i) {
        const int u = tid + i * ALIGN_THREADS;
        if (u < S) lat0[u] = u == 0 ? (double)logp[blank]
                                    : (u == 1 ? (double)logp[my_ext[i]] : -INFINITY);
    }
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        double *cur = (t & 1) ? lat1 : lat0;
        const double *prev = (t & 1) ? lat0 : lat1;
        const float *lp = logp + t * C;
#pragma unroll
        for (int i = 0; i < ALIGN_MAX_PER_THREAD; ++i) {
            const int u = tid + i * ALIGN_THREADS;
            int move = 0;
            if (u < S) {
                // tie rule: strict > in the order s, s - 1, s - 2 (the smallest move wins a tie)
                double best = prev[u];
                if (u >= 1 && prev[u - 1] > best) { best = prev[u - 1]; move = 1; }
                if (skip_ok[i] && prev[u - 2] > best) { best = prev[u - 2]; move = 2; }
                cur[u] = best + (double)lp[my_ext[i]];
            }
            const unsigned long long lo = __ballot(move & 1);
            const unsigned long long hi = __ballot(move >> 1);
            const int word = i * ALIGN_WAVES + wave;
            if (lane == 0 && word < live_words) bp[(size_t)t * nw + word] = u64x2{lo, hi};
        }
        __syncthreads();
    }

    // ---- end state: S - 1 wins over S - 2 unless S - 2 is strictly better ---------------------
    if (tid == 0) {
        const double *fin = ((len - 1) & 1) ? lat1 : lat0;
        double best = fin[S - 1];
        int end = S - 1;
        if (S > 1 && fin[S - 2] > best) { best = fin[S - 2]; end = S - 2; }
        misc[M_STATE] = end;
        status[b] = 0;
        score[b] = (float)best;
    }
    __syncthreads();

    // ---- backtrace: ceil(len / 64) chunks of frames t0, t0 - 1, ..., t0 - 63 ------------------
    for (int t0 = len - 1; t0 >= 0; t0 -= ALIGN_CHUNK) {
        const int top = misc[M_STATE] >> 6;   // word of the path's state at frame t0
        if (tid < ALIGN_CHUNK) {
            const int t = t0 - tid;
            if (t >= 1) {
                for (int k = 0; k < 3; ++k)
                    if (top - k >= 0) stage[tid * 3 + k] = bp[(size_t)t * nw + top - k];
            }
        }
        __syncthreads();
        if (tid == 0) {
            int s = misc[M_STATE];
            for (int j = 0; j < ALIGN_CHUNK && t0 - j >= 0; ++j) {
                spath[j] = s;
                if (t0 - j >= 1) {
                    const u64x2 w = stage[j * 3 + top - (s >> 6)];
                    const int bit = s & 63;
                    s -= (int)((w.x >> bit) & 1ull) | ((int)((w.y >> bit) & 1ull) << 1);
                }
            }
            misc[M_STATE] = s;
        }
        __syncthreads();
        if (tid < ALIGN_CHUNK && t0 - tid >= 0) {
            const int t = t0 - tid, s = spath[tid];
            path_row[t] = s;
            if (flp_row) flp_row[t] = logp[t * C + ext[s]];
        }
        __syncthreads();
    }
}

extern "C" size_t ctcasr_ctc_align_workspace_bytes(int T, int B, int C, int max_label_len) {
    if (T <= 0 || B <= 0 || C <= 0 || max_label_len < 0) return 0;
    // log-softmax tables when they leave LDS; back-pointer slabs when they leave LDS
    const int nw = align_words(2 * max_label_len + 1);
    return ctcasr_align_up((size_t)B * T * C * sizeof(float), 256) +
           ctcasr_align_up((size_t)B * T * nw * sizeof(u64x2), 256);
}

template <bool LOGP_IN_LDS, bool BP_IN_LDS>
static int launch_align(size_t lds, int B, hipStream_t s, const float *logits,
                        const int32_t *labels, const int32_t *label_offsets,
                        const int32_t *seq_len, int T, int C, int blank, int s_pad,
                        int32_t *path, float *score, float *frame_logp, int32_t *status,
                        float *logp_ws, u64x2 *bp_ws) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(
            reinterpret_cast<const void *>(&ctc_align_kernel<LOGP_IN_LDS, BP_IN_LDS>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return CTCASR_ERR_LAUNCH;
    }
    ctc_align_kernel<LOGP_IN_LDS, BP_IN_LDS><<<B, ALIGN_THREADS, lds, s>>>(
        logits, labels, label_offsets, seq_len, T, B, C, blank, s_pad, path, score, frame_logp,
        status, logp_ws, bp_ws);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_ctc_align(const float *logits, const int32_t *labels,
                                const int32_t *label_offsets, const int32_t *seq_len, int T,
                                int B, int C, int blank, int max_label_len, int32_t *path,
                                float *score, float *frame_logp, int32_t *status, void *workspace,
                                size_t workspace_bytes, ctcasr_stream_t stream) {
    if (!logits || !labels || !label_offsets || !seq_len || !path || !score || !status)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (T <= 0 || B <= 0 || C <= 1 || blank < 0 || blank >= C || max_label_len < 0)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (C > 64) return CTCASR_ERR_UNSUPPORTED;
    const int s_pad = 2 * max_label_len + 1;
    if (s_pad > ALIGN_THREADS * ALIGN_MAX_PER_THREAD) return CTCASR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ctcasr_ctc_align_workspace_bytes(T, B, C, max_label_len))
        return CTCASR_ERR_WORKSPACE;
    const int nw = align_words(s_pad);
    float *logp_ws = reinterpret_cast<float *>(workspace);
    u64x2 *bp_ws = reinterpret_cast<u64x2 *>(
        reinterpret_cast<char *>(workspace) +
        ctcasr_align_up((size_t)B * T * C * sizeof(float), 256));
    const size_t fixed = AlignLds(s_pad).fixed;
    const size_t table = (size_t)T * C * sizeof(float);
    const size_t slab = (size_t)T * nw * sizeof(u64x2);
    hipStream_t s = (hipStream_t)stream;
    if (fixed + table + slab <= ALIGN_LDS_MAX)
        return launch_align<true, true>(fixed + table + slab, B, s, logits, labels,
                                        label_offsets, seq_len, T, C, blank, s_pad, path, score,
                                        frame_logp, status, logp_ws, bp_ws);
    if (fixed + table <= ALIGN_LDS_MAX)
        return launch_align<true, false>(fixed + table, B, s, logits, labels, label_offsets,
                                         seq_len, T, C, blank, s_pad, path, score, frame_logp,
                                         status, logp_ws, bp_ws);
    return launch_align<false, false>(fixed, B, s, logits, labels, label_offsets, seq_len, T, C,
                                      blank, s_pad, path, score, frame_logp, status, logp_ws,
                                      bp_ws);
}
