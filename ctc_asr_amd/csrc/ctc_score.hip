// K14: forward-only CTC log-likelihood of many label sequences against few utterances - the
// exact ln p(y | x) of every hypothesis of an n-best list (ctcasr_ctc_beam_decode_nbest), where
// the beam's own totals sum only the alignments that survived pruning.
//
// K9's sweep spends a 384-thread workgroup, a log-softmax table in LDS and one s_barrier per frame
// on one label row, and writes the lattice out for the gradient.  Here the rows are many and
// short and one float per row leaves the chip: the log-softmax of every frame is taken once into
// the workspace (K8's kernel), then ONE WAVEFRONT runs one hypothesis.  Its extended-label
// lattice (S = 2L + 1 states) stays in registers, NS = ceil(S_max / 64) consecutive states per
// lane, so the u - 1 / u - 2 neighbours are the lane's own registers except for its first two
// states, which come from the lane below by two shuffles per frame: a frame costs no barrier and
// no LDS.  The waves of a workgroup take consecutive hypotheses - those of one utterance in the
// n-best layout - so a frame's row of the table (<= 256 B) is fetched from HBM once and then
// served by the cache; nothing is shared between waves, so the result of a hypothesis does not
// depend on its neighbours.  State in fp64, exp / log of the O(1) differences in fp32, for the
// reason given at `lse3` in ctc.hip, and with the same operand order: a row's score is bit for bit
// the same under every NS.
#include "common.h"

#define SCORE_WAVES 4                 // hypotheses per workgroup
#define SCORE_MAX_STATES 1152         // K9's limit: 2 * max_label_len + 1

namespace {

__device__ __forceinline__ double score_lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    if (m == -INFINITY) return -INFINITY;
    const float s = __expf((float)(a - m)) + __expf((float)(b - m)) + __expf((float)(c - m));
    return m + (double)__logf(s);
}

template <int NS>
__global__ void __launch_bounds__(64 * SCORE_WAVES)
ctc_score_kernel(const float *__restrict__ logp, const int *__restrict__ seq_len, int T, int B,
                 int C, int blank, const int *__restrict__ labels,
                 const int *__restrict__ label_offsets, const int *__restrict__ utt, int H,
                 int max_label_len, float *__restrict__ score, int *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6);
    if (h >= H) return;                                   // wave-uniform: no barrier below
    const int begin = label_offsets[h];
    const int L = label_offsets[h + 1] - begin;
    const int b = utt[h];
    const bool fits = L >= 0 && L <= max_label_len && b >= 0 && b < B;
    const int S = fits ? 2 * L + 1 : 1;
    const int len = fits ? seq_len[b] : 0;
    const int *lab = labels + begin;

    // extended labels of this lane's states u = lane * NS + i, and whether u - 2 -> u is allowed
    int sym[NS];
    bool skip[NS];
    bool bad = false;
    int repeats = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int u = lane * NS + i;
        sym[i] = blank;
        skip[i] = false;
        if (u < S && (u & 1)) {
            const int c = lab[u >> 1];
            const int before = u >= 3 ? lab[(u >> 1) - 1] : -1;
            bad |= c < 0 || c >= C || c == blank;
            repeats += before == c;
            skip[i] = u >= 3 && before != c;
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
        if (lane == 0) { status[h] = st; score[h] = -INFINITY; }
        return;
    }

    double a[NS];
    float e[NS];
    bool poisoned = false;
    const float *row = logp + (size_t)b * C;
    const size_t stride = (size_t)B * C;
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
            // the two states below this lane's first: the last two of the lane below (NS = 1:
            // of the two lanes below); the lattice's bottom has none
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
                double v = score_lse3(a[i], a1, skip[i] ? a2 : -INFINITY);
                if (v != -INFINITY) v += (double)e[i];
                a[i] = v;
            }
        }
        // a non-finite logit makes its frame's whole log-softmax row NaN: any state sees it
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            poisoned |= e[i] != e[i];
            e[i] = e_next[i];
        }
    }

    // ln p = lse(alpha(S - 1), alpha(S - 2)), fetched from the lanes that hold them
    double last = -INFINITY, last2 = -INFINITY;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int u = lane * NS + i;
        if (u == S - 1) last = a[i];
        if (u == S - 2) last2 = a[i];
    }
    last = __shfl(last, (S - 1) / NS, 64);
    last2 = S > 1 ? __shfl(last2, (S - 2) / NS, 64) : -INFINITY;
    double log_pyx = len > 0 ? score_lse3(last, last2, -INFINITY) : 0.0;   // len 0: L is 0 too
    poisoned = __any(poisoned);
    if (lane == 0) {
        status[h] = 0;
        score[h] = poisoned ? __uint_as_float(0x7FC00000u) : (float)log_pyx;
    }
}

}  // namespace

extern "C" size_t ctcasr_ctc_score_workspace_bytes(int T, int B, int C, int H,
                                                   int max_label_len) {
    if (T <= 0 || B <= 0 || C <= 0 || H < 0 || max_label_len < 0) return 0;
    return ctcasr_align_up((size_t)T * B * C * sizeof(float), 256);   // the log-softmax table
}

extern "C" int ctcasr_ctc_score(const float *logits, const int32_t *seq_len, int T, int B, int C,
                                int blank, const int32_t *labels, const int32_t *label_offsets,
                                const int32_t *utt, int H, int max_label_len, float *score,
                                int32_t *status, void *workspace, size_t workspace_bytes,
                                ctcasr_stream_t stream) {
    if (!logits || !seq_len || !labels || !label_offsets || !utt || !score || !status)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (T <= 0 || B <= 0 || C <= 1 || blank < 0 || blank >= C || H < 0 || max_label_len < 0)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (C > 64 || max_label_len > (SCORE_MAX_STATES - 1) / 2) return CTCASR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ctcasr_ctc_score_workspace_bytes(T, B, C, H, max_label_len))
        return CTCASR_ERR_WORKSPACE;
    if (H == 0) return CTCASR_OK;
    if ((size_t)T * B > 0x7fffffffu) return CTCASR_ERR_UNSUPPORTED;
    float *logp = reinterpret_cast<float *>(workspace);
    const int rc = ctcasr_log_softmax_fwd(logits, logp, T * B, C, stream);
    if (rc != CTCASR_OK) return rc;
    const int per_lane = (2 * max_label_len + 1 + 63) / 64;
    const int blocks = (H + SCORE_WAVES - 1) / SCORE_WAVES;
#define SCORE_LAUNCH(NS)                                                                     \
    ctc_score_kernel<NS><<<blocks, 64 * SCORE_WAVES, 0, (hipStream_t)stream>>>(              \
        logp, seq_len, T, B, C, blank, labels, label_offsets, utt, H, max_label_len, score,  \
        status)
    if (per_lane <= 1) SCORE_LAUNCH(1);
    else if (per_lane <= 2) SCORE_LAUNCH(2);
    else if (per_lane <= 3) SCORE_LAUNCH(3);
    else if (per_lane <= 6) SCORE_LAUNCH(6);
    else SCORE_LAUNCH(18);
#undef SCORE_LAUNCH
    return ctcasr_launch_status();
}
