// K21: CTC forced alignment of ONE long sequence - K11's lattice (ctc_align.hip) tiled in HBM.
//
// K11 keeps a whole lattice in one workgroup's LDS (S = 2L + 1 <= 1152).  An hour of audio against
// its text is T ~ 180 000 frames x S ~ 110 000 states, 2e10 cells: here the lattice is cut into
// tiles of ALONG_TILE_STATES states x tile_frames frames, one workgroup per tile, and the host
// enqueues one launch per anti-diagonal of tiles.  Tile (i, j) - tile row i of frames, tile column
// j of states - reads
//   * the values of its own states at the frame before its first      (row boundary of (i-1, j)),
//   * per frame, the value of the state just below its first state at the frame before
//                                             (column halo of (i, j-1), and of (i-1, j-1) for the
//                                              tile's first frame),
// all written by launches d - 1 and d - 2 of diagonal d = i + j.  NO WORKGROUP WAITS FOR ANOTHER:
// no flag, no spin, no grid barrier - stream order between the launches is the only dependency.
// Every boundary value has a slot of its own, written once per call (row boundaries [rows][S_pad],
// column halos [cols][T]), so no tile of a launch overwrites what another tile of it reads.
//
// A thread owns 4 CONSECUTIVE states 4k .. 4k+3 (blank, label, blank, label): the predecessors
// s - 1 and s - 2 of all four are its own registers except one, the state 4k - 1, which the
// blank 4k takes as s - 1 and the label 4k + 1 as s - 2 (a blank takes no skip, so 4k - 2 is
// never read).  That one value crosses from the neighbouring lane by a shuffle, between waves
// through LDS, between tile columns through the halo.  The tile width is a multiple of 4, hence
// the halo is one value per frame.
//
// Arithmetic is K11's operation for operation (pinned in include/ctcasr.h): the same fp32
// log-softmax table, delta = max(...) + (double)lp in fp64, strict > in the order s, s-1, s-2,
// S-1 over S-2 at the end.  Max and add do not care how the lattice is tiled: every output is a
// pure function of the table, bit for bit, for any tile_frames.
//
// Back-pointers: 2 bits per cell, a thread's 4 states make one byte, a tile's frame 256
// consecutive bytes: bp[(col * T + t) * 256 + thread].  Backtrace as K11: stage the bytes 64
// frames can touch (the path drops at most 126 states: 33 bytes per frame), walk with one lane.
//
// Tiles no path can pass through are skipped: every state above 2t + 1 (not reachable from the
// start) or below S - 2 - 2(T - 1 - t) (cannot reach the end).  A reader substitutes -inf for what
// a skipped tile would have written.  That is the true value for the first kind; a cell of the
// second kind has only successors of the second kind, so no cell of a path to the end reads one.
//
// K25 (ctcasr_ctc_align_partial) is the same kernels with WILD = true: a label may be
// CTCASR_ALIGN_WILDCARD, one more class whose log-probability at frame t is fill[t], the fmaxf over
// the table's row.  It is an ordinary label state - a blank on either side, at least one frame,
// different from every label, so the skip into and out of it is allowed - and nothing of the
// lattice, the tiling or live() changes.  fill has no region in the workspace (the sizes are
// K21's): a tile that holds a wildcard computes it per staged frame from s_lp, in LDS; a tile
// that holds none does K21's work.  labels[] == -1 never indexes the table: the emission is
// selected.  K21 launches the WILD = false forms, which are the kernels it always had.
#include "common.h"

#define ALONG_THREADS 256
#define ALONG_PER_THREAD 4
#define ALONG_TILE_STATES (ALONG_THREADS * ALONG_PER_THREAD)
#define ALONG_WAVES (ALONG_THREADS / 64)
#define ALONG_STAGE_FRAMES 64     // frames of the table (and of the halo) staged in LDS at a time
#define ALONG_CHUNK 64            // frames walked per backtrace round trip
#define ALONG_CHUNK_BYTES 33      // back-pointer bytes per frame that such a walk can touch
static_assert(ALONG_THREADS == 4 * ALONG_CHUNK, "K25's backtrace puts 4 threads on a frame");
#define ALONG_MAX_C 64
#define ALONG_MAX_T (1ll << 22)
#define ALONG_MAX_L (1ll << 20)
#define ALONG_MAX_ROWS 65536      // tile rows (launches ~ rows + cols)

static_assert(ALONG_TILE_STATES == CTCASR_ALIGN_LONG_TILE_STATES, "header and kernel disagree");
static_assert(ALONG_TILE_STATES % 4 == 0, "one halo value per frame needs columns of 4k states");

// control words (int32) at the head of the workspace
#define LC_BAD_LABEL 0
#define LC_REPEATS 1
#define LC_NONFINITE 2
#define LC_STATUS 3
#define LC_WORDS 64

// The geometry of one call, the same on the host and in every kernel.
struct AlongGeom {
    long long T, L, S;
    int C, tf;
    long long rows, cols, s_pad;
    size_t off_table, off_rowb, off_halo, off_bp, total;
    __host__ __device__ AlongGeom(long long T_, int C_, long long L_, int tile_frames)
        : T(T_), L(L_), S(2 * L_ + 1), C(C_) {
        long long f = tile_frames > 0 ? tile_frames : CTCASR_ALIGN_LONG_TILE_FRAMES;
        if (f > T) f = T;
        if (f < 1) f = 1;
        tf = (int)f;
        rows = (T + f - 1) / f;
        cols = (S + ALONG_TILE_STATES - 1) / ALONG_TILE_STATES;
        s_pad = cols * ALONG_TILE_STATES;
        off_table = LC_WORDS * sizeof(int);
        off_rowb = off_table + up((size_t)T * C * sizeof(float));
        off_halo = off_rowb + up((size_t)rows * s_pad * sizeof(double));
        off_bp = off_halo + up((size_t)cols * T * sizeof(double));
        total = off_bp + up((size_t)cols * T * ALONG_THREADS);
    }
    static __host__ __device__ size_t up(size_t v) { return (v + 255) / 256 * 256; }
    // does any path from the start to the end pass through tile (i, j)?
    __host__ __device__ bool live(long long i, long long j) const {
        if (i < 0 || j < 0 || i >= rows || j >= cols) return false;
        const long long t_first = i * tf;
        const long long t_last = (t_first + tf < T ? t_first + tf : T) - 1;
        const long long s_min = j * ALONG_TILE_STATES;
        const long long s_max = (s_min + ALONG_TILE_STATES < S ? s_min + ALONG_TILE_STATES : S) - 1;
        return s_min <= 2 * t_last + 1 && s_max + 2 * (T - 1 - t_first) >= S - 2;
    }
};

// ---- launch 1: the table, the label check, the repeat count --------------------------------
// Thread g takes frame g and label g.  The row arithmetic is ctc_align_kernel's, line for line.
// WILD: a wildcard is a label and no repeat; two of them side by side are refused as a bad label.
template <bool WILD>
__global__ void __launch_bounds__(ALONG_THREADS)
ctc_align_long_prep_kernel(const float *__restrict__ logits, const int *__restrict__ labels,
                           long long T, int C, int blank, long long L, int *__restrict__ ctrl,
                           float *__restrict__ table, float *__restrict__ logp_out) {
    const long long g = (long long)blockIdx.x * ALONG_THREADS + threadIdx.x;
    if (g < L) {
        const int sym = labels[g];
        if (WILD && sym == CTCASR_ALIGN_WILDCARD) {
            if (g >= 1 && labels[g - 1] == sym) atomicOr(&ctrl[LC_BAD_LABEL], 1);
        } else {
            if (sym < 0 || sym >= C || sym == blank) atomicOr(&ctrl[LC_BAD_LABEL], 1);
            if (g >= 1 && labels[g - 1] == sym) atomicAdd(&ctrl[LC_REPEATS], 1);
        }
    }
    if (g < T) {
        const float *row = logits + (size_t)g * C;
        float mx = row[0];
        bool finite = true;
        for (int c = 0; c < C; ++c) {
            finite = finite && fabsf(row[c]) <= 3.4028235e38f;
            mx = fmaxf(mx, row[c]);
        }
        float sum = 0.f;
        for (int c = 0; c < C; ++c) sum += expf(row[c] - mx);
        const float lz = mx + logf(sum);
        if (!finite || !(fabsf(lz) <= 3.4028235e38f)) atomicOr(&ctrl[LC_NONFINITE], 1);
        for (int c = 0; c < C; ++c) {
            const float v = row[c] - lz;
            table[(size_t)g * C + c] = v;
            if (logp_out) logp_out[(size_t)g * C + c] = v;
        }
    }
}

// ---- launch 2: the status word; the outputs of a sequence without a path -------------------
__global__ void __launch_bounds__(ALONG_THREADS)
ctc_align_long_status_kernel(long long T, long long L, int *__restrict__ ctrl,
                             int *__restrict__ path, double *__restrict__ score,
                             float *__restrict__ frame_logp, int *__restrict__ status) {
    // K11's order: labels and lengths, then feasibility, then the logits
    int st = 0;
    if (ctrl[LC_BAD_LABEL]) st = 2;
    else if (T < L + ctrl[LC_REPEATS]) st = 1;
    else if (ctrl[LC_NONFINITE]) st = 3;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctrl[LC_STATUS] = st;      // (the other blocks of this launch read the three counters)
        if (st != 0 || T == 0) {
            status[0] = st;
            score[0] = st == 3 ? __longlong_as_double(0x7FF8000000000000ll)
                               : (st != 0 ? -(double)INFINITY : 0.0);
        }
    }
    if (st == 0) return;
    for (long long t = (long long)blockIdx.x * ALONG_THREADS + threadIdx.x; t < T;
         t += (long long)gridDim.x * ALONG_THREADS) {
        path[t] = -1;
        if (frame_logp) frame_logp[t] = 0.f;
    }
}

// ---- one anti-diagonal of tiles ------------------------------------------------------------
// The body of a tile is ctc_align_long_tile.h, included twice: as K21's kernel, and as the device
// function below, which K25's kernel calls with FILL = does a thread of this tile hold a wildcard.
#define ALONG_TILE_ARGS                                                                        \
    const int *__restrict__ labels, long long T, int C, int blank, long long L,                \
    int tile_frames, long long diag, long long i_lo, const int *__restrict__ ctrl,             \
    const float *__restrict__ table, double *__restrict__ rowb, double *__restrict__ halo,     \
    unsigned char *__restrict__ bp

__global__ void __launch_bounds__(ALONG_THREADS) ctc_align_long_tile_kernel(ALONG_TILE_ARGS) {
    constexpr bool WILD = false, FILL = false;
#include "ctc_align_long_tile.h"
}

template <bool FILL>
__device__ __forceinline__ void along_partial_tile(ALONG_TILE_ARGS) {
    constexpr bool WILD = true;
#include "ctc_align_long_tile.h"
}

__global__ void __launch_bounds__(ALONG_THREADS) ctc_align_partial_tile_kernel(ALONG_TILE_ARGS) {
    // Does a thread of this tile hold a wildcard?  A tile without one runs K21's loop: the vote
    // is all that it pays.  (Every test before the vote is uniform over the block.)
    if (ctrl[LC_STATUS] != 0) return;
    const AlongGeom g(T, C, L, tile_frames);
    const long long i = i_lo + blockIdx.x, j = diag - i;
    if (!g.live(i, j)) return;
    const long long k0 = (j * ALONG_TILE_STATES + (long long)threadIdx.x * ALONG_PER_THREAD) >> 1;
    const bool mine = (k0 < L && labels[k0] == CTCASR_ALIGN_WILDCARD) ||
                      (k0 + 1 < L && labels[k0 + 1] == CTCASR_ALIGN_WILDCARD);
    if (__syncthreads_or(mine))
        along_partial_tile<true>(labels, T, C, blank, L, tile_frames, diag, i_lo, ctrl, table,
                                 rowb, halo, bp);
    else
        along_partial_tile<false>(labels, T, C, blank, L, tile_frames, diag, i_lo, ctrl, table,
                                  rowb, halo, bp);
}

// ---- last launch: end state, score, backtrace ----------------------------------------------
template <bool WILD>
__global__ void __launch_bounds__(ALONG_THREADS)
ctc_align_long_backtrace_kernel(const int *__restrict__ labels, long long T, int C, int blank,
                                long long L, int tile_frames, const int *__restrict__ ctrl,
                                const float *__restrict__ table,
                                const double *__restrict__ rowb,
                                const unsigned char *__restrict__ bp, int *__restrict__ path,
                                double *__restrict__ score, float *__restrict__ frame_logp,
                                int *__restrict__ status) {
    __shared__ unsigned char s_stage[ALONG_CHUNK * ALONG_CHUNK_BYTES];
    __shared__ int s_path[ALONG_CHUNK];
    __shared__ int s_state;

    if (ctrl[LC_STATUS] != 0 || T == 0) return;
    const AlongGeom g(T, C, L, tile_frames);
    const int tid = threadIdx.x;
    if (tid == 0) {
        // end state: S - 1 wins over S - 2 unless S - 2 is strictly better
        const double ninf = -(double)INFINITY;
        const double *fin = rowb + (size_t)(g.rows - 1) * g.s_pad;
        const long long S = g.S;
        double best = g.live(g.rows - 1, (S - 1) / ALONG_TILE_STATES) ? fin[S - 1] : ninf;
        long long end = S - 1;
        if (S > 1) {
            const double other = g.live(g.rows - 1, (S - 2) / ALONG_TILE_STATES) ? fin[S - 2] : ninf;
            if (other > best) { best = other; end = S - 2; }
        }
        s_state = (int)end;
        status[0] = 0;
        score[0] = best;
    }
    __syncthreads();
    for (long long t0 = T - 1; t0 >= 0; t0 -= ALONG_CHUNK) {
        const int q_top = s_state >> 2;       // byte of the path's state at frame t0
        for (int e = tid; e < ALONG_CHUNK * ALONG_CHUNK_BYTES; e += ALONG_THREADS) {
            const long long t = t0 - e / ALONG_CHUNK_BYTES;
            const int q = q_top - e % ALONG_CHUNK_BYTES;
            if (t >= 1 && q >= 0)
                s_stage[e] = bp[((size_t)(q >> 8) * T + t) * ALONG_THREADS + (q & 255)];
        }
        __syncthreads();
        if (tid == 0) {
            int s = s_state;
            for (int f = 0; f < ALONG_CHUNK && t0 - f >= 0; ++f) {
                s_path[f] = s;
                if (t0 - f >= 1) {
                    const int byte = s_stage[f * ALONG_CHUNK_BYTES + q_top - (s >> 2)];
                    s -= (byte >> ((s & 3) * 2)) & 3;
                }
            }
            s_state = s;
        }
        __syncthreads();
        if constexpr (!WILD) {
            if (tid < ALONG_CHUNK && t0 - tid >= 0) {
                const long long t = t0 - tid;
                const int s = s_path[tid];
                path[t] = s;
                if (frame_logp) frame_logp[t] = table[(size_t)t * C + ((s & 1) ? labels[s >> 1] : blank)];
            }
        } else {
            // 4 threads per frame (ALONG_THREADS = 4 ALONG_CHUNK): on a wildcard frame they take
            // the columns q, q + 4, ... of the table's row in HBM and fold to fill[t]
            const int f = tid >> 2, q = tid & 3;
            const bool in = t0 - f >= 0;
            const long long t = in ? t0 - f : 0;
            const int s = in ? s_path[f] : 0;
            const int sym = (s & 1) ? labels[s >> 1] : blank;
            const bool wild = in && sym == CTCASR_ALIGN_WILDCARD;
            const float *row = table + (size_t)t * C;
            float mx = row[wild ? 0 : sym];
            if (wild && frame_logp)
                for (int c = q; c < C; c += 4) mx = fmaxf(mx, row[c]);
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            if (in && q == 0) {
                path[t] = s;
                if (frame_logp) frame_logp[t] = mx;
            }
        }
        __syncthreads();
    }
}

static bool along_args_ok(long long T, int C, long long L, int tile_frames) {
    return T >= 0 && C > 1 && L >= 0 && tile_frames >= 0;
}

static bool along_supported(long long T, int C, long long L, int tile_frames) {
    if (C > ALONG_MAX_C || T > ALONG_MAX_T || L > ALONG_MAX_L) return false;
    return AlongGeom(T, C, L, tile_frames).rows <= ALONG_MAX_ROWS;
}

extern "C" size_t ctcasr_ctc_align_long_workspace_bytes(int64_t T, int C, int64_t L,
                                                        int tile_frames) {
    if (!along_args_ok(T, C, L, tile_frames) || !along_supported(T, C, L, tile_frames)) return 0;
    return AlongGeom(T, C, L, tile_frames).total;
}

template <bool WILD>
static int along_run(const float *logits, const int32_t *labels, int64_t T, int C, int blank,
                     int64_t L, int tile_frames, int32_t *path, double *score, float *frame_logp,
                     float *logp, int32_t *status, void *workspace, size_t workspace_bytes,
                     ctcasr_stream_t stream) {
    if (!score || !status) return CTCASR_ERR_BAD_ARGUMENT;
    if (!along_args_ok(T, C, L, tile_frames) || blank < 0 || blank >= C)
        return CTCASR_ERR_BAD_ARGUMENT;
    // (a tensor without elements has no address: T = 0 needs no logits, L = 0 no labels)
    if ((T > 0 && (!logits || !path)) || (L > 0 && !labels)) return CTCASR_ERR_BAD_ARGUMENT;
    if (!along_supported(T, C, L, tile_frames)) return CTCASR_ERR_UNSUPPORTED;
    const AlongGeom g(T, C, L, tile_frames);
    if (!workspace || workspace_bytes < g.total || ((uintptr_t)workspace & 7))
        return CTCASR_ERR_WORKSPACE;

    char *ws = reinterpret_cast<char *>(workspace);
    int *ctrl = reinterpret_cast<int *>(ws);
    float *table = reinterpret_cast<float *>(ws + g.off_table);
    double *rowb = reinterpret_cast<double *>(ws + g.off_rowb);
    double *halo = reinterpret_cast<double *>(ws + g.off_halo);
    unsigned char *bp = reinterpret_cast<unsigned char *>(ws + g.off_bp);
    hipStream_t s = (hipStream_t)stream;

    if (hipMemsetAsync(ctrl, 0, LC_WORDS * sizeof(int), s) != hipSuccess) return CTCASR_ERR_LAUNCH;
    const long long n = T > L ? T : L;
    if (n > 0) {
        ctc_align_long_prep_kernel<WILD><<<(unsigned)((n + ALONG_THREADS - 1) / ALONG_THREADS),
                                     ALONG_THREADS, 0, s>>>(logits, labels, T, C, blank, L, ctrl,
                                                            table, logp);
        if (ctcasr_launch_status() != CTCASR_OK) return CTCASR_ERR_LAUNCH;
    }
    long long fill = (T + ALONG_THREADS - 1) / ALONG_THREADS;
    fill = fill < 1 ? 1 : (fill > 1024 ? 1024 : fill);
    ctc_align_long_status_kernel<<<(unsigned)fill, ALONG_THREADS, 0, s>>>(T, L, ctrl, path, score,
                                                                         frame_logp, status);
    if (ctcasr_launch_status() != CTCASR_OK) return CTCASR_ERR_LAUNCH;
    if (T == 0) return CTCASR_OK;

    for (long long d = 0; d < g.rows + g.cols - 1; ++d) {
        // tiles (i, d - i) of the diagonal, trimmed to its first and last live one (a skipped
        // tile in between returns at once)
        long long lo = d - (g.cols - 1) > 0 ? d - (g.cols - 1) : 0;
        long long hi = d < g.rows - 1 ? d : g.rows - 1;
        while (lo <= hi && !g.live(lo, d - lo)) ++lo;
        while (hi >= lo && !g.live(hi, d - hi)) --hi;
        if (lo > hi) continue;
        if constexpr (WILD)
            ctc_align_partial_tile_kernel<<<(unsigned)(hi - lo + 1), ALONG_THREADS, 0, s>>>(
                labels, T, C, blank, L, tile_frames, d, lo, ctrl, table, rowb, halo, bp);
        else
            ctc_align_long_tile_kernel<<<(unsigned)(hi - lo + 1), ALONG_THREADS, 0, s>>>(
                labels, T, C, blank, L, tile_frames, d, lo, ctrl, table, rowb, halo, bp);
        if (ctcasr_launch_status() != CTCASR_OK) return CTCASR_ERR_LAUNCH;
    }
    ctc_align_long_backtrace_kernel<WILD><<<1, ALONG_THREADS, 0, s>>>(
        labels, T, C, blank, L, tile_frames, ctrl, table, rowb, bp, path, score, frame_logp,
        status);
    return ctcasr_launch_status();
}

extern "C" int ctcasr_ctc_align_long(const float *logits, const int32_t *labels, int64_t T, int C,
                                     int blank, int64_t L, int tile_frames, int32_t *path,
                                     double *score, float *frame_logp, float *logp,
                                     int32_t *status, void *workspace, size_t workspace_bytes,
                                     ctcasr_stream_t stream) {
    return along_run<false>(logits, labels, T, C, blank, L, tile_frames, path, score, frame_logp,
                            logp, status, workspace, workspace_bytes, stream);
}

// K25: the same call with CTCASR_ALIGN_WILDCARD accepted among the labels.
extern "C" int ctcasr_ctc_align_partial(const float *logits, const int32_t *labels, int64_t T,
                                        int C, int blank, int64_t L, int tile_frames,
                                        int32_t *path, double *score, float *frame_logp,
                                        float *logp, int32_t *status, void *workspace,
                                        size_t workspace_bytes, ctcasr_stream_t stream) {
    return along_run<true>(logits, labels, T, C, blank, L, tile_frames, path, score, frame_logp,
                           logp, status, workspace, workspace_bytes, stream);
}
