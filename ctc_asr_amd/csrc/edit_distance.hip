// K13: batched edit distance with error counts (substitutions, deletions, insertions).
//
// One wavefront per pair, up to four pairs per workgroup, the whole batch in one launch.  The DP
// matrix has a row per reference symbol and a column per hypothesis symbol; the 64 lanes lie
// across 64 consecutive columns (a strip) and sweep the rows along anti-diagonals: at step s lane
// l owns cell (row s - l + 1, column base + l + 1).  What a cell needs from the column to its
// left - that lane's cell of the previous step, and the reference symbol it compared - moves one
// lane up by a DPP wave shift whose lane 0 takes the value the previous strip left for that row;
// the diagonal neighbour is the value that arrived one step earlier.  No LDS round trip and no
// barrier sits between two steps.
//
// A cell is the packed pair distance << 16 | substitutions, compared as one unsigned integer:
// delete and insert add 1 << 16, substitute adds (1 << 16) + 1, match adds 0, and a plain min
// over the three moves yields the lexicographic minimum of (distance, substitutions) - the
// alignment with the fewest substitutions among those of minimum distance, whatever the order
// of evaluation.  Lengths up to 32767 keep every candidate inside 32 bits.
//
// LDS per wave: the reference symbols, staged once (the hypothesis symbols need no staging: a
// lane reads the one symbol of its column when a strip begins, so each is read once), and the
// carry column - cell (row, last column of the strip) for every row, read by lane 0 of the next
// strip one step ahead of its use and overwritten in place by lane 63, 63 steps after the read.
// When four carry columns do not fit beside the symbols they live in the workspace; when four
// symbol arrays do not fit, a workgroup takes two pairs or one.  Waves of a workgroup never wait
// for each other: a long pair keeps its own wave busy and nothing else.
#include "common.h"

#define ED_MAX_LEN 32767
#define ED_MAX_WAVES 4
#define ED_LDS_MAX (150 * 1024)
#define ED_STEP (1u << 16)            // delete / insert
#define ED_SUBSTITUTE ((1u << 16) + 1u)
#define ED_DPP_WAVE_SHR1 0x138        // lane l reads lane l - 1; lane 0 keeps `old`

// ints of one wave's symbol array and of one carry column (16-byte multiples)
static __host__ __device__ inline int ed_stride(int max_ref_len) {
    return (max_ref_len + 3) / 4 * 4;
}

struct EdPlan {
    int waves;         // pairs per workgroup
    bool col_in_lds;   // carry columns beside the symbols, else in the workspace
    size_t lds;
};

static EdPlan ed_plan(int max_ref_len) {
    const size_t row = (size_t)ed_stride(max_ref_len) * sizeof(int);
    EdPlan p;
    p.waves = ED_MAX_WAVES;
    while (p.waves > 1 && p.waves * row > ED_LDS_MAX) p.waves >>= 1;
    p.col_in_lds = 2 * p.waves * row <= ED_LDS_MAX;
    p.lds = (p.col_in_lds ? 2 : 1) * p.waves * row;
    return p;
}

__device__ __forceinline__ unsigned ed_shift_up(unsigned lane0, unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)lane0, (int)v, ED_DPP_WAVE_SHR1, 0xf, 0xf,
                                                 false);
}

template <bool COL_IN_LDS>
__global__ void __launch_bounds__(ED_MAX_WAVES * 64)
edit_distance_kernel(const int *hyp, const int *hyp_offsets, const int *hyp_len, const int *ref,
                     const int *ref_offsets, const int *ref_len, int B, int max_hyp_len,
                     int max_ref_len, int *__restrict__ distance, int *__restrict__ substitutions,
                     int *__restrict__ deletions, int *__restrict__ insertions,
                     int *__restrict__ status, unsigned *__restrict__ col_ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    // (readfirstlane: the pair and its lengths are wave-uniform, so the loops branch on scalars)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * waves + wave;
    if (b >= B) return;   // the kernel has no workgroup barrier
    const int H = __builtin_amdgcn_readfirstlane(hyp_len[b]);
    const int R = __builtin_amdgcn_readfirstlane(ref_len[b]);
    if (H < 0 || H > max_hyp_len || R < 0 || R > max_ref_len) {
        if (lane == 0) {
            status[b] = 2;
            distance[b] = -1;
            if (substitutions) substitutions[b] = -1;
            if (deletions) deletions[b] = -1;
            if (insertions) insertions[b] = -1;
        }
        return;
    }
    const int stride = ed_stride(max_ref_len);
    int *sym = reinterpret_cast<int *>(smem) + wave * stride;
    // col[k]: cell (row k + 1, last column before the current strip); row 0 is known: column << 16
    unsigned *col = COL_IN_LDS
        ? reinterpret_cast<unsigned *>(smem) + (waves + wave) * stride
        : col_ws + (size_t)b * stride;

    unsigned packed = (unsigned)(R + H) << 16;   // one side empty: all deletions or all insertions
    if (R > 0 && H > 0) {
        const int *h = hyp + hyp_offsets[b];
        const int *r = ref + ref_offsets[b];
        for (int k = lane; k < R; k += 64) {
            sym[k] = r[k];
            col[k] = (unsigned)(k + 1) << 16;
        }
        unsigned cur = 0;
        for (int base = 0; base < H; base += 64) {
            // lanes of this wave wrote sym / col for each other (above, or in the last strip)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const int width = min(64, H - base);
            const bool carry_out = base + 64 < H;
            const int h_sym = lane < width ? h[base + lane] : 0;
            cur = (unsigned)(base + lane + 1) << 16;         // cell (0, own column)
            unsigned diag = (unsigned)(base + lane) << 16;   // cell (0, column to the left)
            unsigned r_sym = 0;
            unsigned next_sym = (unsigned)sym[0], next_col = col[0];
            const int steps = R + width - 1;
            for (int s = 0; s < steps; ++s) {
                // lane 0 enters row s + 1 now; fetch what it needs for row s + 2
                const unsigned in_sym = next_sym, in_col = next_col;
                const int k = min(s + 1, R - 1);
                next_sym = (unsigned)sym[k];
                next_col = col[k];
                const unsigned left = ed_shift_up(in_col, cur);
                r_sym = ed_shift_up(in_sym, r_sym);
                const int row = s - lane + 1;
                const unsigned best = min(min(left, cur) + ED_STEP,
                                          diag + (r_sym == (unsigned)h_sym ? 0u : ED_SUBSTITUTE));
                diag = left;
                const bool live = (unsigned)(row - 1) < (unsigned)R;
                cur = live ? best : cur;
                if (carry_out && lane == 63 && live) col[row - 1] = best;
            }
        }
        packed = (unsigned)__shfl((int)cur, (H - 1) & 63, 64);   // cell (R, H)
    }
    if (lane == 0) {
        const int d = (int)(packed >> 16), s = (int)(packed & 0xFFFFu);
        const int del = (d - s + R - H) / 2;   // D + I = d - S, D - I = R - H
        status[b] = 0;
        distance[b] = d;
        if (substitutions) substitutions[b] = s;
        if (deletions) deletions[b] = del;
        if (insertions) insertions[b] = d - s - del;
    }
}

extern "C" size_t ctcasr_edit_distance_workspace_bytes(int B, int max_hyp_len, int max_ref_len) {
    (void)max_hyp_len;   // the lanes lie across the hypothesis: nothing is kept per column
    if (B < 1 || max_ref_len < 0 || ed_plan(max_ref_len).col_in_lds) return 0;
    return ctcasr_align_up((size_t)B * ed_stride(max_ref_len) * sizeof(unsigned), 256);
}

template <bool COL_IN_LDS>
static int launch_edit_distance(const EdPlan &plan, hipStream_t s, const int32_t *hyp,
                                const int32_t *hyp_offsets, const int32_t *hyp_len,
                                const int32_t *ref, const int32_t *ref_offsets,
                                const int32_t *ref_len, int B, int max_hyp_len, int max_ref_len,
                                int32_t *distance, int32_t *substitutions, int32_t *deletions,
                                int32_t *insertions, int32_t *status, unsigned *col_ws) {
    if (plan.lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(
            reinterpret_cast<const void *>(&edit_distance_kernel<COL_IN_LDS>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds);
        if (e != hipSuccess) return CTCASR_ERR_LAUNCH;
    }
    const int blocks = (B + plan.waves - 1) / plan.waves;
    edit_distance_kernel<COL_IN_LDS><<<blocks, plan.waves * 64, plan.lds, s>>>(
        hyp, hyp_offsets, hyp_len, ref, ref_offsets, ref_len, B, max_hyp_len, max_ref_len,
        distance, substitutions, deletions, insertions, status, col_ws);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_edit_distance(const int32_t *hyp, const int32_t *hyp_offsets,
                                    const int32_t *hyp_len, const int32_t *ref,
                                    const int32_t *ref_offsets, const int32_t *ref_len, int B,
                                    int max_hyp_len, int max_ref_len, int32_t *distance,
                                    int32_t *substitutions, int32_t *deletions,
                                    int32_t *insertions, int32_t *status, void *workspace,
                                    size_t workspace_bytes, ctcasr_stream_t stream) {
    if (!hyp || !hyp_offsets || !hyp_len || !ref || !ref_offsets || !ref_len || !distance ||
        !status)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (B < 1 || max_hyp_len < 0 || max_ref_len < 0) return CTCASR_ERR_BAD_ARGUMENT;
    if (max_hyp_len > ED_MAX_LEN || max_ref_len > ED_MAX_LEN) return CTCASR_ERR_UNSUPPORTED;
    const EdPlan plan = ed_plan(max_ref_len);
    const size_t need = ctcasr_edit_distance_workspace_bytes(B, max_hyp_len, max_ref_len);
    if (need > 0 && (!workspace || workspace_bytes < need)) return CTCASR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned *col_ws = reinterpret_cast<unsigned *>(workspace);
    if (plan.col_in_lds)
        return launch_edit_distance<true>(plan, s, hyp, hyp_offsets, hyp_len, ref, ref_offsets,
                                          ref_len, B, max_hyp_len, max_ref_len, distance,
                                          substitutions, deletions, insertions, status, col_ws);
    return launch_edit_distance<false>(plan, s, hyp, hyp_offsets, hyp_len, ref, ref_offsets,
                                       ref_len, B, max_hyp_len, max_ref_len, distance,
                                       substitutions, deletions, insertions, status, col_ws);
}
