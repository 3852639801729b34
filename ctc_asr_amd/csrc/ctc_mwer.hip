// K23: the gradient of the expected error count over an n-best list (minimum word error rate
// training).  Per utterance b with valid hypotheses y_1..y_n, scores s_i = ln p(y_i | x) and
// risks W_i: P = softmax(s), R = sum_i P_i W_i, c_i = P_i (W_i - R), and since d s_i / d logit =
// occ_i - softmax, with sum_i c_i = 0 the softmax terms cancel:
//     grad[t, b, k] = scale * sum_i c_i * occ_i[t, k].
//
// Three launches behind K8's log-softmax table:
//  (a) mwer_sweep_kernel, grid (ceil(B N / 4), 2): K14's kernel (ctc_score.hip) with the lattice
//      written out.  ONE WAVEFRONT runs one (hypothesis, direction); the extended-label lattice
//      stays in registers, NS consecutive states per lane, the neighbour states cross lanes by
//      two shuffles per frame - no LDS, no barrier.  The alpha wave is K14's code line for line
//      (the same table, lse3 operand order and precision), so its score is K14's bit for bit; the
//      beta wave is its mirror image (u + 1 / u + 2 from the lane above).  A frame's row of the
//      lattice goes to the workspace as fp64 [NS][64]: state u = lane * NS + i sits at i * 64 +
//      lane, so each of the NS stores of a frame is one contiguous 512-byte run.
//  (b) mwer_weights_kernel, one thread per utterance: P, R, c in fp64 from the fp32 scores.
//  (c) mwer_fold_kernel, one wavefront per (t, b): walks the utterance's hypotheses in rank order,
//      forms exp(alpha + beta - s) per state, sums the blank states by a fixed butterfly and the
//      label states per class from LDS in ascending state order, and adds c_i * occ_i into a
//      per-lane fp64 accumulator.  Lane k owns class k: every output element has one owner, there
//      is no atomic anywhere, and the result is a pure function of the utterance's own inputs.
#include "common.h"

#define MWER_WAVES 4                  // (hypothesis, direction) pairs per workgroup of the sweep
#define MWER_FOLD_WAVES 4             // (t, b) rows per workgroup of the fold
#define MWER_MAX_STATES 1152          // K9's limit: 2 * max_label_len + 1
#define MWER_MAX_LABELS ((MWER_MAX_STATES - 1) / 2)

namespace {

// K14's score_lse3 / K9's lse3: the same operand order, fp64 state, fp32 exp / log
__device__ __forceinline__ double mwer_lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    if (m == -INFINITY) return -INFINITY;
    const float s = __expf((float)(a - m)) + __expf((float)(b - m)) + __expf((float)(c - m));
    return m + (double)__logf(s);
}

__device__ __forceinline__ int mwer_list_size(const int *n_hyps, int b, int N) {
    const int n = n_hyps[b];
    return n < 0 ? 0 : (n > N ? N : n);
}

template <int NS>
__global__ void __launch_bounds__(64 * MWER_WAVES)
mwer_sweep_kernel(const float *__restrict__ logp, const int *__restrict__ seq_len, int T, int B,
                  int C, int blank, const int *__restrict__ labels,
                  const int *__restrict__ label_offsets, const int *__restrict__ n_hyps, int N,
                  int max_label_len, float *__restrict__ score, int *__restrict__ status,
                  double *__restrict__ alpha_ws, double *__restrict__ beta_ws,
                  double *__restrict__ log_pyx_ws) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * MWER_WAVES + (threadIdx.x >> 6);
    const bool beta_sweep = blockIdx.y == 1;
    if (h >= B * N) return;                               // wave-uniform: no barrier below
    const int b = h / N;
    if (h - b * N >= mwer_list_size(n_hyps, b, N)) {      // an unused row: nothing of it is read
        if (!beta_sweep && lane == 0) { status[h] = -1; score[h] = -INFINITY; }
        return;
    }
    const int begin = label_offsets[h];
    const int L = label_offsets[h + 1] - begin;
    const bool fits = L >= 0 && L <= max_label_len;
    const int S = fits ? 2 * L + 1 : 1;
    const int len = fits ? seq_len[b] : 0;
    const int *lab = labels + begin;

    // extended labels of this lane's states u = lane * NS + i; whether u - 2 -> u (alpha) and
    // u -> u + 2 (beta) are allowed
    int sym[NS];
    bool skip[NS], skip_fw[NS];
    bool bad = false;
    int repeats = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int u = lane * NS + i;
        sym[i] = blank;
        skip[i] = false;
        skip_fw[i] = false;
        if (u < S && (u & 1)) {
            const int c = lab[u >> 1];
            const int before = u >= 3 ? lab[(u >> 1) - 1] : -1;
            bad |= c < 0 || c >= C || c == blank;
            repeats += before == c;
            skip[i] = u >= 3 && before != c;
            skip_fw[i] = u + 2 < S && lab[(u >> 1) + 1] != c;
            sym[i] = c < 0 || c >= C ? blank : c;         // never index the table outside a row
        }
    }
    bad = __any(bad);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) repeats += __shfl_xor(repeats, off, 64);

    int st = 0;
    if (!fits || bad || len > T || len < 0) st = 2;
    else if (len < L + repeats) st = 1;
    if (st != 0) {
        if (!beta_sweep && lane == 0) { status[h] = st; score[h] = -INFINITY; }
        return;
    }

    const float *row = logp + (size_t)b * C;
    const size_t stride = (size_t)B * C;
    const size_t slab = (size_t)h * T * (NS * 64);        // this hypothesis' [T][NS][64] lattice

    if (!beta_sweep) {
        // ---- alpha: K14's loop, plus the stores ------------------------------------------------
        double *aw = alpha_ws + slab;
        double a[NS];
        float e[NS];
        bool poisoned = false;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            a[i] = -INFINITY;
            e[i] = len > 0 ? row[sym[i]] : 0.f;
        }
        for (int t = 0; t < len; ++t) {
            // the next frame's emissions are on their way while this frame computes
            float e_next[NS];
            const float *next = row + (size_t)(t + 1 < len ? t + 1 : t) * stride;
#pragma unroll
            for (int i = 0; i < NS; ++i) e_next[i] = next[sym[i]];
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const int u = lane * NS + i;
                    if (u <= 1 && u < S) a[i] = (double)e[i];
                }
            } else {
                double below1 = __shfl_up(a[NS - 1], 1, 64);
                double below2 = NS >= 2 ? __shfl_up(a[NS >= 2 ? NS - 2 : 0], 1, 64)
                                        : __shfl_up(a[0], 2, 64);
                if (lane == 0) below1 = -INFINITY;
                if (lane * NS < 2) below2 = -INFINITY;
                // top down, so a[i - 1] and a[i - 2] still hold the previous frame
#pragma unroll
                for (int i = NS - 1; i >= 0; --i) {
                    const double a1 = i >= 1 ? a[i >= 1 ? i - 1 : 0] : below1;
                    const double a2 = i >= 2 ? a[i >= 2 ? i - 2 : 0] : (i == 1 ? below1 : below2);
                    double v = mwer_lse3(a[i], a1, skip[i] ? a2 : -INFINITY);
                    if (v != -INFINITY) v += (double)e[i];
                    a[i] = v;
                }
            }
            double *out = aw + (size_t)t * (NS * 64) + lane;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                out[i * 64] = a[i];
                poisoned |= e[i] != e[i];
                e[i] = e_next[i];
            }
        }

        double last = -INFINITY, last2 = -INFINITY;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int u = lane * NS + i;
            if (u == S - 1) last = a[i];
            if (u == S - 2) last2 = a[i];
        }
        last = __shfl(last, (S - 1) / NS, 64);
        last2 = S > 1 ? __shfl(last2, (S - 2) / NS, 64) : -INFINITY;
        const double log_pyx = len > 0 ? mwer_lse3(last, last2, -INFINITY) : 0.0;
        poisoned = __any(poisoned);
        if (lane == 0) {
            status[h] = poisoned ? 3 : 0;
            score[h] = poisoned ? __uint_as_float(0x7FC00000u) : (float)log_pyx;
            log_pyx_ws[h] = log_pyx;
        }
        return;
    }

    // ---- beta: beta(t, u) excludes the emission at t, so alpha + beta is the joint log-prob -----
    if (len == 0) return;
    double *bw = beta_ws + slab;
    double bt[NS];
    float e[NS];                                          // the emissions of frame t
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int u = lane * NS + i;
        bt[i] = u < S && u >= S - 2 ? 0.0 : -INFINITY;    // states at or above S stay -inf
        e[i] = row[(size_t)(len - 1) * stride + sym[i]];
        bw[(size_t)(len - 1) * (NS * 64) + i * 64 + lane] = bt[i];
    }
    for (int t = len - 1; t > 0; --t) {
        float e_next[NS];
        const float *next = row + (size_t)(t - 1) * stride;
#pragma unroll
        for (int i = 0; i < NS; ++i) e_next[i] = next[sym[i]];
        double g[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) g[i] = bt[i] + (double)e[i];
        // the two states above this lane's last: the first two of the lane above (NS = 1: of the
        // two lanes above); the lattice's top has none
        double above1 = __shfl_down(g[0], 1, 64);
        double above2 = NS >= 2 ? __shfl_down(g[NS >= 2 ? 1 : 0], 1, 64) : __shfl_down(g[0], 2, 64);
        if (lane == 63) above1 = -INFINITY;
        if (NS >= 2 ? lane == 63 : lane >= 62) above2 = -INFINITY;
        double *out = bw + (size_t)(t - 1) * (NS * 64) + lane;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const double g1 = i + 1 < NS ? g[i + 1 < NS ? i + 1 : 0] : above1;
            const double g2 = i + 2 < NS ? g[i + 2 < NS ? i + 2 : 0]
                                         : (i + 1 < NS ? above1 : above2);
            bt[i] = mwer_lse3(g[i], g1, skip_fw[i] ? g2 : -INFINITY);
            out[i * 64] = bt[i];
            e[i] = e_next[i];
        }
    }
}

// P, R, c of one utterance per thread, in fp64 from the fp32 scores.  mode: 0 fewer than two valid
// hypotheses (gradient +0), 1 the sum of (c), 2 a non-finite logit (NaN).
__global__ void __launch_bounds__(64)
mwer_weights_kernel(const int *__restrict__ n_hyps, int B, int N, const float *__restrict__ risk,
                    const float *__restrict__ score, const int *__restrict__ status,
                    float *__restrict__ posterior, float *__restrict__ expected_risk,
                    double *__restrict__ weight, int *__restrict__ mode) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n = mwer_list_size(n_hyps, b, N);
    const size_t base = (size_t)b * N;
    const float nan32 = __uint_as_float(0x7FC00000u);
    int valid = 0;
    bool poisoned = false;
    double peak = -INFINITY;
    for (int i = 0; i < n; ++i) {
        const int st = status[base + i];
        poisoned |= st == 3;
        if (st == 0) {
            ++valid;
            peak = fmax(peak, (double)score[base + i]);
        }
    }
    for (int i = n; i < N; ++i) {
        posterior[base + i] = 0.f;
        weight[base + i] = 0.0;
    }
    if (poisoned) {
        for (int i = 0; i < n; ++i) {
            const int st = status[base + i];
            posterior[base + i] = st == 0 || st == 3 ? nan32 : 0.f;
            weight[base + i] = 0.0;
        }
        expected_risk[b] = nan32;
        mode[b] = 2;
        return;
    }
    // every valid score -inf: they share the mass (CTCModel.nbest_posteriors)
    double z = 0.0;
    for (int i = 0; i < n; ++i)
        if (status[base + i] == 0)
            z += peak == -INFINITY ? 1.0 : exp((double)score[base + i] - peak);
    double expected = 0.0;
    for (int i = 0; i < n; ++i)
        if (status[base + i] == 0) {
            const double w = peak == -INFINITY ? 1.0 : exp((double)score[base + i] - peak);
            expected += w / z * (double)risk[base + i];
        }
    for (int i = 0; i < n; ++i) {
        double p = 0.0, c = 0.0;
        if (status[base + i] == 0) {
            const double w = peak == -INFINITY ? 1.0 : exp((double)score[base + i] - peak);
            p = w / z;
            if (valid >= 2) c = p * ((double)risk[base + i] - expected);
        }
        posterior[base + i] = (float)p;
        weight[base + i] = c;
    }
    expected_risk[b] = (float)expected;
    mode[b] = valid >= 2 ? 1 : 0;
}

__global__ void __launch_bounds__(64 * MWER_FOLD_WAVES)
mwer_fold_kernel(const int *__restrict__ seq_len, int T, int B, int C, int blank,
                 const int *__restrict__ labels, const int *__restrict__ label_offsets,
                 const int *__restrict__ n_hyps, int N, int NS, float scale, int accumulate,
                 const int *__restrict__ status, const double *__restrict__ alpha_ws,
                 const double *__restrict__ beta_ws, const double *__restrict__ log_pyx_ws,
                 const double *__restrict__ weight, const int *__restrict__ mode,
                 float *__restrict__ grad) {
    __shared__ float vals_s[MWER_FOLD_WAVES][MWER_MAX_LABELS + 1];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * MWER_FOLD_WAVES + wave;
    if (t >= T) return;                                    // wave-uniform; no workgroup barrier
    int len = seq_len[b];
    if (len < 0 || len > T) len = 0;                       // status 2 throughout: no live row
    float *out = grad + ((size_t)t * B + b) * C + lane;
    if (t >= len) {                                        // accumulate: the row keeps grad_in
        if (!accumulate && lane < C) *out = 0.f;
        return;
    }
    const int m = mode[b];
    float *vals = vals_s[wave];
    double acc = 0.0;
    if (m == 2) acc = (double)__uint_as_float(0x7FC00000u);
    const int n = m == 1 ? mwer_list_size(n_hyps, b, N) : 0;
    const size_t row = (size_t)NS * 64;
    for (int i = 0; i < n; ++i) {
        const int h = b * N + i;
        if (status[h] != 0) continue;
        const double c = weight[h], log_pyx = log_pyx_ws[h];
        const int begin = label_offsets[h];
        const int L = label_offsets[h + 1] - begin;
        const int S = 2 * L + 1;
        const int *lab = labels + begin;
        const double *aw = alpha_ws + ((size_t)h * T + t) * row + lane;
        const double *bw = beta_ws + ((size_t)h * T + t) * row + lane;
        double blank_sum = 0.0;
        for (int j = 0; j < NS; ++j) {
            const int u = lane * NS + j;
            if (u < S) {
                const double joint = aw[j * 64] + bw[j * 64];
                const float v = joint != -INFINITY && log_pyx != -INFINITY
                                    ? expf((float)(joint - log_pyx)) : 0.f;
                if (u & 1) vals[u >> 1] = v;
                else blank_sum += (double)v;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) blank_sum += __shfl_xor(blank_sum, off, 64);
        // the wave's LDS writes are ordered before its reads (one in-order LDS queue per wave)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double occ = 0.0;
        for (int j = 0; j < L; ++j) {
            const float v = *reinterpret_cast<volatile float *>(&vals[j]);
            if (lab[j] == lane) occ += (double)v;
        }
        if (lane == blank) occ = blank_sum;
        acc += c * occ;
        // ... and these reads before the next hypothesis' writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane < C) {
        // (the plain call adds to +0.0: it is the accumulating call onto zeros, bit for bit)
        const double total = m == 0 ? 0.0 : (double)scale * acc;
        *out = (float)((accumulate ? (double)*out : 0.0) + total);
    }
}

int mwer_states_per_lane(int max_label_len) {
    const int per_lane = (2 * max_label_len + 1 + 63) / 64;
    return per_lane <= 3 ? per_lane : (per_lane <= 6 ? 6 : 18);
}

size_t mwer_table_bytes(int T, int B, int C) {
    return ctcasr_align_up((size_t)T * B * C * sizeof(float), 256);
}
size_t mwer_lattice_bytes(int T, int B, int N, int max_label_len) {
    return ctcasr_align_up((size_t)B * N * T * mwer_states_per_lane(max_label_len) * 64 *
                               sizeof(double), 256);
}
size_t mwer_per_hyp_bytes(int B, int N) {
    return ctcasr_align_up((size_t)B * N * sizeof(double), 256);
}

}  // namespace

extern "C" size_t ctcasr_ctc_mwer_workspace_bytes(int T, int B, int C, int N, int max_label_len) {
    if (T <= 0 || B <= 0 || C <= 0 || N <= 0 || max_label_len < 0 ||
        max_label_len > MWER_MAX_LABELS)
        return 0;
    // the table; the alpha and beta lattices; ln p and c per hypothesis; the mode per utterance
    return mwer_table_bytes(T, B, C) + 2 * mwer_lattice_bytes(T, B, N, max_label_len) +
           2 * mwer_per_hyp_bytes(B, N) + ctcasr_align_up((size_t)B * sizeof(int), 256);
}

extern "C" int ctcasr_ctc_mwer(const float *logits, const int32_t *seq_len, int T, int B, int C,
                               int blank, const int32_t *labels, const int32_t *label_offsets,
                               const int32_t *n_hyps, const float *risk, int N, int max_label_len,
                               float scale, int accumulate, float *grad, float *expected_risk,
                               float *score, float *posterior, int32_t *status, void *workspace,
                               size_t workspace_bytes, ctcasr_stream_t stream) {
    if (!logits || !seq_len || !labels || !label_offsets || !n_hyps || !risk || !grad ||
        !expected_risk || !score || !posterior || !status)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (T <= 0 || B <= 0 || C <= 1 || blank < 0 || blank >= C || N <= 0 || max_label_len < 0)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (C > 64 || max_label_len > MWER_MAX_LABELS || B > 65535) return CTCASR_ERR_UNSUPPORTED;
    if ((size_t)T * B > 0x7fffffffu || (size_t)B * N > 0x7fffffffu) return CTCASR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ctcasr_ctc_mwer_workspace_bytes(T, B, C, N, max_label_len))
        return CTCASR_ERR_WORKSPACE;
    char *ws = reinterpret_cast<char *>(workspace);
    const size_t lattice = mwer_lattice_bytes(T, B, N, max_label_len);
    const size_t per_hyp = mwer_per_hyp_bytes(B, N);
    float *logp = reinterpret_cast<float *>(ws);
    ws += mwer_table_bytes(T, B, C);
    double *alpha_ws = reinterpret_cast<double *>(ws);
    double *beta_ws = reinterpret_cast<double *>(ws + lattice);
    double *log_pyx_ws = reinterpret_cast<double *>(ws + 2 * lattice);
    double *weight_ws = reinterpret_cast<double *>(ws + 2 * lattice + per_hyp);
    int *mode_ws = reinterpret_cast<int *>(ws + 2 * lattice + 2 * per_hyp);
    const int rc = ctcasr_log_softmax_fwd(logits, logp, T * B, C, stream);
    if (rc != CTCASR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int H = B * N;
    const int per_lane = mwer_states_per_lane(max_label_len);
    const dim3 sweeps((H + MWER_WAVES - 1) / MWER_WAVES, 2);
#define MWER_LAUNCH(NS)                                                                       \
    mwer_sweep_kernel<NS><<<sweeps, 64 * MWER_WAVES, 0, s>>>(                                 \
        logp, seq_len, T, B, C, blank, labels, label_offsets, n_hyps, N, max_label_len, score, \
        status, alpha_ws, beta_ws, log_pyx_ws)
    if (per_lane == 1) MWER_LAUNCH(1);
    else if (per_lane == 2) MWER_LAUNCH(2);
    else if (per_lane == 3) MWER_LAUNCH(3);
    else if (per_lane == 6) MWER_LAUNCH(6);
    else MWER_LAUNCH(18);
#undef MWER_LAUNCH
    mwer_weights_kernel<<<(B + 63) / 64, 64, 0, s>>>(n_hyps, B, N, risk, score, status, posterior,
                                                     expected_risk, weight_ws, mode_ws);
    const dim3 rows((T + MWER_FOLD_WAVES - 1) / MWER_FOLD_WAVES, B);
    mwer_fold_kernel<<<rows, 64 * MWER_FOLD_WAVES, 0, s>>>(
        seq_len, T, B, C, blank, labels, label_offsets, n_hyps, N, per_lane, scale, accumulate,
        status, alpha_ws, beta_ws, log_pyx_ws, weight_ws, mode_ws, grad);
    return ctcasr_launch_status();
}
