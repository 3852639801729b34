// K22: CTC phrase spotting - is this phrase said in here, and where?  (include/ctcasr.h has the
// contract and the pinned arithmetic.)
//
// K14's shape (ctc_score.hip) with another lattice in it: the log-softmax of every frame is taken
// once into the workspace (K8's kernel), a small pre-pass takes each frame's maximum ("fill", the
// greedy path's emission), then ONE WAVEFRONT runs one (utterance, phrase) pair.  The lattice is
// Viterbi (max-sum, fp64) over S = 2L - 1 states - no blank in front of the phrase and none
// behind it - with a free start (state 0 may be entered at any frame at value 0) and a free end
// (state S - 1 is read at every frame).  Each state carries its value and the frame at which its
// path entered state 0, NS = ceil(S_max / 64) consecutive states per lane in registers; the two
// states below a lane's first come from the lane below by shuffle (a double and an int each): a
// frame costs no barrier and no LDS.  The lane that owns state S - 1 runs the hit pass on what
// that state holds frame by frame and writes the hits in order, so an hour of audio against a
// few hundred phrases leaves a few KB and not pairs x frames scores.  Nothing is shared between
// waves: a pair's result does not depend on its neighbours.  The waves of a workgroup take
// consecutive pairs - those of one utterance when the caller groups them so - and a frame's row
// of the table is then fetched from HBM once and served by the cache.  Max, add and subtract in
// fp64 have one answer: every output is bit for bit the same under every NS.
#include "common.h"

#define SEARCH_WAVES 4                // pairs per workgroup
#define SEARCH_MAX_STATES 1151        // 2 * max_label_len - 1
#define SEARCH_MAX_HITS 1024

namespace {

// fill[r] = fmaxf over the table's row r: one wave per row.  Lanes beyond C repeat column 0, so
// that a row of NaN (all of it is, or none) keeps its NaN through fmaxf.
__global__ void __launch_bounds__(256) ctc_search_fill_kernel(const float *__restrict__ logp,
                                                              float *__restrict__ fill, int rows,
                                                              int C) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int r = wave; r < rows; r += nwaves) {
        const float v = wave_max(logp[(size_t)r * C + (lane < C ? lane : 0)]);
        if (lane == 0) fill[r] = v;
    }
}

// what the owner of state S - 1 carries through the frames
struct SearchHits {
    double pend_score, best;
    int pend_start, pend_end, flushed_end, count, best_start, best_end;
    bool pending;
};

__device__ __forceinline__ void search_flush(SearchHits &k, int max_hits, int *__restrict__ hits,
                                             double *__restrict__ hit_score) {
    if (k.count < max_hits) {
        hits[2 * k.count] = k.pend_start;
        hits[2 * k.count + 1] = k.pend_end;
        hit_score[k.count] = k.pend_score;
    }
    ++k.count;
    k.flushed_end = k.pend_end;
}

template <int NS>
__global__ void __launch_bounds__(64 * SEARCH_WAVES)
ctc_search_kernel(const float *__restrict__ logp, const float *__restrict__ fill,
                  const int *__restrict__ seq_len, int T, int B, int C, int blank,
                  const int *__restrict__ labels, const int *__restrict__ label_offsets, int P,
                  int max_label_len, const double *__restrict__ min_score,
                  const int *__restrict__ pair_utt, const int *__restrict__ pair_phrase, int H,
                  int max_hits, int *__restrict__ hits, double *__restrict__ hit_score,
                  int *__restrict__ n_hits, double *__restrict__ best_score,
                  int *__restrict__ best_span, double *__restrict__ end_score,
                  int *__restrict__ end_start, int *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * SEARCH_WAVES + (threadIdx.x >> 6);
    if (h >= H) return;                                   // wave-uniform: no barrier below
    const int b = pair_utt[h];
    const int p = pair_phrase[h];
    const bool named = b >= 0 && b < B && p >= 0 && p < P;
    const int begin = named ? label_offsets[p] : 0;
    const int L = named ? label_offsets[p + 1] - begin : 0;
    const bool fits = named && begin >= 0 && L >= 1 && L <= max_label_len;
    const int S = fits ? 2 * L - 1 : 1;
    const int len = fits ? seq_len[b] : 0;
    const int *lab = labels + (fits ? begin : 0);

    // extended labels of this lane's states u = lane * NS + i (even u: a label, odd u: the
    // blank), and whether u - 2 -> u is allowed
    int sym[NS];
    bool skip[NS];
    bool bad = false;
    int repeats = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int u = lane * NS + i;
        sym[i] = blank;
        skip[i] = false;
        if (fits && u < S && !(u & 1)) {
            const int c = lab[u >> 1];
            const int before = u >= 2 ? lab[(u >> 1) - 1] : -1;
            bad |= c < 0 || c >= C || c == blank;
            repeats += before == c;
            skip[i] = u >= 2 && before != c;
            sym[i] = c < 0 || c >= C ? blank : c;         // never index the table outside a row
        }
    }
    bad = __any(bad);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) repeats += __shfl_xor(repeats, off, 64);

    int st = 0;
    if (!fits || bad || len > T || len < 0) st = 2;
    else if (len < L + repeats) st = 1;
    // a NaN in `fill` among the utterance's own frames, found before the sweep so that nothing
    // has to be rewritten: 64 frames at a time
    if (st == 0) {
        bool nan = false;
        for (int t = lane; t < len; t += 64) {
            const float f = fill[(size_t)t * B + b];
            nan |= f != f;
        }
        if (__any(nan)) st = 3;
    }

    int *my_hits = hits ? hits + (size_t)h * max_hits * 2 : nullptr;
    double *my_hit_score = hit_score ? hit_score + (size_t)h * max_hits : nullptr;
    double *my_end_score = end_score ? end_score + (size_t)h * T : nullptr;
    int *my_end_start = end_start ? end_start + (size_t)h * T : nullptr;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);

    if (st != 0) {
        const double none = st == 3 ? qnan : -INFINITY;
        for (int k = lane; k < max_hits; k += 64) {
            my_hits[2 * k] = -1;
            my_hits[2 * k + 1] = -1;
            my_hit_score[k] = -INFINITY;
        }
        for (int t = lane; t < T; t += 64) {
            if (my_end_score) my_end_score[t] = none;
            if (my_end_start) my_end_start[t] = -1;
        }
        if (lane == 0) {
            status[h] = st;
            n_hits[h] = 0;
            best_score[h] = none;
            best_span[2 * h] = -1;
            best_span[2 * h + 1] = -1;
        }
        return;
    }

    // from here on len >= L + repeats >= 1
    const double threshold = min_score[p];
    const int owner = (S - 1) / NS;                       // the lane that holds state S - 1
    double a[NS];                                         // d_t(u)
    int s[NS];                                            // s_t(u)
    float e[NS];
    const float *row = logp + (size_t)b * C;
    const float *frow = fill + b;
    const size_t stride = (size_t)B * C;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        a[i] = -INFINITY;
        s[i] = -1;
        e[i] = row[sym[i]];
    }
    float f = frow[0];
    SearchHits k;
    k.pending = false;
    k.pend_score = -INFINITY;
    k.pend_start = k.pend_end = -1;
    k.flushed_end = -1;
    k.count = 0;
    k.best = -INFINITY;
    k.best_start = k.best_end = -1;

    for (int t = 0; t < len; ++t) {
        // the next frame's emissions and filler are on their way while this frame computes
        float e_next[NS];
        const int tn = t + 1 < len ? t + 1 : t;
        const float *next = row + (size_t)tn * stride;
#pragma unroll
        for (int i = 0; i < NS; ++i) e_next[i] = next[sym[i]];
        const float f_next = frow[(size_t)tn * B];

        // the two states below this lane's first: the last two of the lane below (NS = 1: of the
        // two lanes below); the lattice's bottom has none.  At t = 0 every state is still -inf,
        // which is "stay, step and skip do not exist".
        double below1 = __shfl_up(a[NS - 1], 1, 64);
        int sbelow1 = __shfl_up(s[NS - 1], 1, 64);
        double below2 = NS >= 2 ? __shfl_up(a[NS >= 2 ? NS - 2 : 0], 1, 64)
                                : __shfl_up(a[0], 2, 64);
        int sbelow2 = NS >= 2 ? __shfl_up(s[NS >= 2 ? NS - 2 : 0], 1, 64)
                              : __shfl_up(s[0], 2, 64);
        if (lane == 0) { below1 = -INFINITY; sbelow1 = -1; }
        if (lane * NS < 2) { below2 = -INFINITY; sbelow2 = -1; }
        const double fd = (double)f;
        // top down, so a[i - 1] and a[i - 2] still hold the previous frame.  (States at and
        // above S hold values nobody reads: every move goes upwards.)
#pragma unroll
        for (int i = NS - 1; i >= 0; --i) {
            const double a1 = i >= 1 ? a[i >= 1 ? i - 1 : 0] : below1;
            const int s1 = i >= 1 ? s[i >= 1 ? i - 1 : 0] : sbelow1;
            const double a2 = i >= 2 ? a[i >= 2 ? i - 2 : 0] : (i == 1 ? below1 : below2);
            const int s2 = i >= 2 ? s[i >= 2 ? i - 2 : 0] : (i == 1 ? sbelow1 : sbelow2);
            // stay first (a state at -inf carries start -1 already), then strict >
            double best = a[i];
            int from = s[i];
            if (a1 > best) { best = a1; from = s1; }
            if (skip[i] && a2 > best) { best = a2; from = s2; }
            if (i == 0 && lane == 0 && 0.0 > best) { best = 0.0; from = t; }
            const double v = best + ((double)e[i] - fd);
            a[i] = v;
            s[i] = v == -INFINITY ? -1 : from;
        }

        if (lane == owner) {
            double v = -INFINITY;
            int from = -1;
#pragma unroll
            for (int i = 0; i < NS; ++i)
                if (lane * NS + i == S - 1) { v = a[i]; from = s[i]; }
            if (my_end_score) my_end_score[t] = v;
            if (my_end_start) my_end_start[t] = from;
            if (v > k.best) { k.best = v; k.best_start = from; k.best_end = t; }
            if (v > -INFINITY && v >= threshold && from > k.flushed_end) {
                if (!k.pending) {
                    k.pending = true;
                    k.pend_score = v; k.pend_start = from; k.pend_end = t;
                } else if (from <= k.pend_end) {
                    if (v > k.pend_score || (v == k.pend_score && from == k.pend_start)) {
                        k.pend_score = v; k.pend_start = from; k.pend_end = t;
                    }
                } else {
                    search_flush(k, max_hits, my_hits, my_hit_score);
                    k.pend_score = v; k.pend_start = from; k.pend_end = t;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) e[i] = e_next[i];
        f = f_next;
    }

    if (lane == owner) {
        if (k.pending) search_flush(k, max_hits, my_hits, my_hit_score);
        status[h] = 0;
        n_hits[h] = k.count;
        best_score[h] = k.best;
        best_span[2 * h] = k.best_start;
        best_span[2 * h + 1] = k.best_end;
    }
    // the rows no hit took, and the frames behind the utterance
    const int stored = min(__shfl(k.count, owner, 64), max_hits);
    for (int j = stored + lane; j < max_hits; j += 64) {
        my_hits[2 * j] = -1;
        my_hits[2 * j + 1] = -1;
        my_hit_score[j] = -INFINITY;
    }
    for (int t = len + lane; t < T; t += 64) {
        if (my_end_score) my_end_score[t] = -INFINITY;
        if (my_end_start) my_end_start[t] = -1;
    }
}

}  // namespace

extern "C" size_t ctcasr_ctc_search_workspace_bytes(int T, int B, int C) {
    if (T <= 0 || B <= 0 || C <= 0) return 0;
    return ctcasr_align_up((size_t)T * B * C * sizeof(float), 256) +     // the log-softmax table
           ctcasr_align_up((size_t)T * B * sizeof(float), 256);          // fill
}

extern "C" int ctcasr_ctc_search(const float *logits, const int32_t *seq_len, int T, int B, int C,
                                 int blank, const int32_t *labels, const int32_t *label_offsets,
                                 int P, int max_label_len, const double *min_score,
                                 const int32_t *pair_utt, const int32_t *pair_phrase, int H,
                                 int max_hits, int32_t *hits, double *hit_score, int32_t *n_hits,
                                 double *best_score, int32_t *best_span, double *end_score,
                                 int32_t *end_start, int32_t *status, void *workspace,
                                 size_t workspace_bytes, ctcasr_stream_t stream) {
    if (T < 0 || B < 0 || C < 2 || blank < 0 || blank >= C || P < 0 || max_label_len < 0 ||
        H < 0 || max_hits < 0)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (H == 0) return CTCASR_OK;
    if (!seq_len || !labels || !label_offsets || !min_score || !pair_utt || !pair_phrase ||
        !n_hits || !best_score || !best_span || !status || (!logits && T > 0 && B > 0))
        return CTCASR_ERR_BAD_ARGUMENT;
    if (max_hits > 0 && (!hits || !hit_score)) return CTCASR_ERR_BAD_ARGUMENT;
    if (C > 64 || 2 * (long long)max_label_len - 1 > SEARCH_MAX_STATES ||
        max_hits > SEARCH_MAX_HITS || (size_t)T * B > 0x7fffffffu)
        return CTCASR_ERR_UNSUPPORTED;
    const size_t need = ctcasr_ctc_search_workspace_bytes(T, B, C);
    if (workspace_bytes < need || (need > 0 && !workspace)) return CTCASR_ERR_WORKSPACE;
    float *logp = reinterpret_cast<float *>(workspace);
    float *fill = reinterpret_cast<float *>(
        reinterpret_cast<char *>(workspace) + ctcasr_align_up((size_t)T * B * C * sizeof(float), 256));
    if (need > 0) {
        const int rows = T * B;
        const int rc = ctcasr_log_softmax_fwd(logits, logp, rows, C, stream);
        if (rc != CTCASR_OK) return rc;
        int fill_blocks = (rows + 3) / 4;
        if (fill_blocks > 4096) fill_blocks = 4096;
        ctc_search_fill_kernel<<<fill_blocks, 256, 0, (hipStream_t)stream>>>(logp, fill, rows, C);
    }
    const int per_lane = (2 * max_label_len - 1 + 63) / 64;
    const int blocks = (H + SEARCH_WAVES - 1) / SEARCH_WAVES;
#define SEARCH_LAUNCH(NS)                                                                     \
    ctc_search_kernel<NS><<<blocks, 64 * SEARCH_WAVES, 0, (hipStream_t)stream>>>(             \
        logp, fill, seq_len, T, B, C, blank, labels, label_offsets, P, max_label_len,         \
        min_score, pair_utt, pair_phrase, H, max_hits, hits, hit_score, n_hits, best_score,   \
        best_span, end_score, end_start, status)
    if (per_lane <= 1) SEARCH_LAUNCH(1);
    else if (per_lane <= 2) SEARCH_LAUNCH(2);
    else if (per_lane <= 3) SEARCH_LAUNCH(3);
    else if (per_lane <= 6) SEARCH_LAUNCH(6);
    else SEARCH_LAUNCH(18);
#undef SEARCH_LAUNCH
    return ctcasr_launch_status();
}
