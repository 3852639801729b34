// K4/K5, persistent variant: ONE launch runs all T time steps of a bidirectional layer.
//
// The recurrence is bound by latency and by re-reading the recurrent weights every step
// (SURVEY.md 7.2): R is 16.8 MB per direction at H=1024 fp32, more than a 4 MB XCD L2 holds.
// Here every workgroup keeps its slice of R in LDS for the whole sequence — 128 KB per CU, both
// directions across the 256 CUs of the chip — laid out in MFMA fragment order so the B operand
// is a conflict-free lane-linear ds_read_b128.  Per step a workgroup then only (1) reads the
// previous hidden state (forward: 64 KB at B=16) straight into A fragments with every load in
// flight at once, (2) issues its share of v_mfma_f32_16x16x4_f32, (3) reduces over its 4 waves
// through LDS and applies the gate math for the units it owns (cell state stays in registers),
// and (4) meets the other workgroups of ITS direction at a two-level counter barrier.
// The two directions are independent chains and never wait for each other.
//
// Inter-workgroup visibility uses the write-through form of the guide's placement-independent
// protocol (no fences on the critical path): the values other workgroups consume (h_t forward,
// dgates_t backward) are stored with 16-byte `sc1` buffer stores, every storing wave drains
// them (vmcnt(0)), a workgroup barrier, then ONE lane posts a relaxed agent-scope arrival on its
// group's counter (8 counters per direction).  Waiters poll the 8 counters with relaxed
// agent-scope loads from 8 lanes, and read the published rows with `sc1` buffer loads (L1 is
// bypassed, so no acquire invalidation is needed).  Stores that only the host-side backward
// pass needs (the LSTM reserve) are plain and issued after the arrival.  Published rows live in
// the output tensors themselves, whose addresses are unique per time step.  Every spin is
// bounded; a timeout raises an error word that the host reports (ctcasr_rnn_poll_error).
#include "common.h"
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

#define PRNN_THREADS 256
#define PRNN_BLOCK_ROWS 32          // rows one persistent launch covers (two 16-row tiles)
#ifndef PRNN_GROUPS
#define PRNN_GROUPS 8
#endif
#define PRNN_SPIN_LIMIT (1u << 22)
#ifndef PRNN_PROBE_HALF_LOADS
#define PRNN_PROBE_HALF_LOADS 0
#endif
#ifndef PRNN_XCD_AWARE
#define PRNN_XCD_AWARE 0
#endif
#ifndef PRNN_CHAIN_LB
#define PRNN_CHAIN_LB 4
#endif
#ifndef PRNN_CHAIN_REGW
#define PRNN_CHAIN_REGW 32
#endif
#ifndef PRNN_CHAIN0_PRIO
#define PRNN_CHAIN0_PRIO 1
#endif
#ifndef PRNN_XCD_TILE_PAIRS
#define PRNN_XCD_TILE_PAIRS 1
#endif
#ifndef PRNN_POLL_SLEEP
#define PRNN_POLL_SLEEP 1
#endif

namespace {

// Every arrival counter sits in its own 256-byte block: the 16 counters of a launch then map to
// different memory channels instead of serialising 256 arrivals + all polls on one line.
#define PRNN_CNT_STRIDE 64
#define PRNN_MAX_CHAINS 2
struct SyncWords {
    // [direction][chain][group]: a chain is one 16-row batch tile running its own recurrence
    unsigned group_cnt[2][PRNN_MAX_CHAINS][PRNN_GROUPS][PRNN_CNT_STRIDE];
    // workgroups of a (direction, chain) that are through their LAST wait of the launch; the last
    // one zeroes that group's counters again, so a launch needs no memset before it
    unsigned done[2][PRNN_MAX_CHAINS][PRNN_CNT_STRIDE];
    unsigned error;
    unsigned pad[63];
    unsigned long long prof[16];   // CTCASR_RNN_PROF=1: per-phase 100 MHz ticks of workgroup 0
    unsigned long long prof_all[256][4];   // ... and of every workgroup (forward pass)
    // residency hand-shake (ctcasr_rnn_resident_gate): workgroups of a launch that carries a
    // ticket count themselves in at entry; the one that completes the grid posts the ticket
    unsigned resident[PRNN_CNT_STRIDE];
    unsigned resident_ticket[PRNN_CNT_STRIDE];
};

struct PArgs {
    const float *xw;       // [T, B, 2, G*H]
    const float *w;        // fwd: w_hh [2, G*H, H]; bwd: w_hh_t [2, H, G*H]
    const int *seq_len;
    float *y;              // [T, B, 2H]
    unsigned short *y16;   // forward, fp16 kernel (optional): the pieces of y, [T, B, 3, 2H] halves
    const float *dy;
    float *dxw;
    float *gates;          // LSTM reserve [T, B, 2, 4H]
    float *cells;          // LSTM reserve [T, B, 2, H]
    SyncWords *sync;
    float *xchg;           // exchange buffer [T steps][2][K/16 chunks][B][16] (see below)
    const float *bias;     // forward: [2, G*H] added to xw (NULL: none)
    const float *b_hh;     // GRU forward: recurrent bias [2, 3H] (its candidate-gate third is read)
    float *drec;           // GRU backward: d(recurrent pre-activations) [T, B, 2, 3H]
    float *dbias;          // backward (optional): bias gradients accumulate here: [2][G * H] column
                           // sums of dxw, then (GRU only) [2][3 * H] column sums of drec
    int T, B, H, nwg;      // nwg = workgroups per direction (and chain); B = rows of this launch
    int BS;                // batch stride of the [T, batch, ...] tensors (>= B: a launch may cover a
                           // block of at most 32 rows of a bigger batch, pointers offset by the host)
    int ndir, dir0;        // directions in this launch (2, or 1 when they run one after the other)
    int chain0;            // first batch tile of this launch
    int s_lo, s_hi;        // backward: this launch runs steps s_hi-1 ... s_lo (a whole pass: 0, T)
    float *carry;          // backward, LSTM: dc [2, B, H] handed from one launch to the next
    float *rs;             // backward, fp16 form: the inverse scales (prnn_b16_scale_bytes)
    unsigned *colmax;      // backward, fp16 form (optional): [2][G * H] maxima of |dxw| (bit patterns);
                           // reduced with fmaxf, which skips a NaN: max over nan_to_num(|dxw|, 0),
                           // what colmax_kernel (split.hip) finds in a pass over dxw (inf stays inf)
    int prof;              // record phase timings of workgroup 0
    unsigned ticket;       // != 0: post it once every workgroup of this launch is running
    int xcd_split;         // fp16 kernels: direction 0 on XCDs 0 - 3, direction 1 on XCDs 4 - 7
    unsigned *kp;          // backward, K-pair form (H = 2048): KPairWords + the hand-off slots
                           // (prnn_w16_kp_bytes)
};

__device__ __forceinline__ float4 ldg4(const float *p) {
    return *reinterpret_cast<const float4 *>(p);
}
__device__ __forceinline__ void mma4(f32x4 &acc, const float4 &a, const float4 &b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}
// Two independent accumulators, alternated: v_mfma_f32_16x16x4_f32 issues every 32 cycles but a
// dependent accumulate needs 40, so back-to-back MFMAs on ONE accumulator run 25 % slower.
__device__ __forceinline__ void mma4x2(f32x4 &acc0, f32x4 &acc1, const float4 &a0,
                                       const float4 &b0, const float4 &a1, const float4 &b1) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc1, 0, 0, 0);
}
__device__ __forceinline__ int row_steps(const int *seq_len, int b, int T) {
    return seq_len ? min(max(seq_len[b], 0), T) : T;
}
__device__ __forceinline__ int row_time(int dir, int s, int steps) {
    return dir == 0 ? s : steps - 1 - s;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 16-byte write-through store / L1-bypassing load (buffer_*_dwordx4 ... sc1)
__device__ __forceinline__ void store16_sc1(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off,
                                            float a, float b, float c, float d) {
    u32x4 v = {__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)};
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)byte_off, 0, 16);
}
// Exchange-buffer read.  Plain (L1/L2-allocating) load: every exchange row has an address that
// is written exactly once per launch (the buffer is indexed by step), always with write-through
// stores and always before the direction barrier that precedes its first read, so no cache on
// the reading side can hold an older copy of it - and the 15 other workgroups of the direction
// on the same XCD then hit in L2 instead of going back to the Infinity Cache (sc1 loads did:
// ~9 TB/s chip-wide, 7 us per backward step).  AUX selects the cache policy (0 plain, 16 sc1).
template <int AUX = 0>
__device__ __forceinline__ float4 load16_sc1(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
    u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, AUX);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                       __uint_as_float(v.w));
}

// Two chains per workgroup (CHAINS = 2, batches of 17..32 rows).  The two 16-row batch tiles of
// such a batch are INDEPENDENT recurrences that share the weights.  Run through one barrier
// (the MT = 2 kernels of round 1) each step costs wait + 2 x MFMA work; here every workgroup has
// 8 waves instead - waves 0-3 carry tile 0, waves 4-7 tile 1, two waves per SIMD - and each tile
// has its own arrival counters, so while one tile's waves wait for their exchange round trip the
// SIMD issues the other tile's MFMAs: the hardware interleaves the chains, no software
// pipelining.  The LDS weight slice is shared by both chains.  A workgroup-wide s_barrier would
// couple the chains again, so the three per-step synchronisations among the 4 waves of a chain
// go through LDS words instead (LDS executes a wave's DS instructions in issue order, so a
// counter update issued after a wave's ds_writes is seen only after them):
//   chain_flag_*   one-way: the polling wave tells the other three that the direction barrier
//                  has been passed
//   chain_barrier  all four waves have written their partial tiles before any of them reads
//   chain_arrive   non-blocking: every wave drains its published stores, the LAST one to get
//                  there posts the workgroup's arrival on the global counter.
struct ChainSync {          // in LDS, one per chain
    unsigned flag;          // steps whose direction barrier the poller has seen complete
    unsigned bar;           // chain_barrier arrivals
    unsigned arrive;        // chain_arrive arrivals
    unsigned pad;
};
__device__ __forceinline__ unsigned lds_load(unsigned *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void chain_barrier(ChainSync *cs, unsigned &epoch, int lane) {
    epoch += 4;
    asm volatile("" ::: "memory");          // (compiler) LDS writes above stay above
    if (lane == 0)
        __hip_atomic_fetch_add(&cs->bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (lds_load(&cs->bar) < epoch) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");          // LDS reads below stay below
}

// Direction-wide barrier, split in two so that the arrival is posted as soon as a step's
// published stores are out and the wait happens at the top of the next step.
// `step` counts arrivals (0-based).  CHAINS = 1: `ctid` is threadIdx.x and the workgroup barrier
// separates the phases; CHAINS = 2: `ctid` is the thread index within the chain's 4 waves.
template <int CHAINS>
__device__ __forceinline__ void dir_arrive(SyncWords *sy, ChainSync *cs, int dir, int chain,
                                           int grp, int ctid, unsigned &arrivals) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its stores
    if constexpr (CHAINS == 1) {
        __syncthreads();
        if (ctid == 0)
            __hip_atomic_fetch_add(&sy->group_cnt[dir][chain][grp][0], 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    } else {
        arrivals += 4;
        if ((ctid & 63) == 0) {
            const unsigned before = __hip_atomic_fetch_add(
                &cs->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (before + 1 == arrivals)     // the last of the chain's four waves
                __hip_atomic_fetch_add(&sy->group_cnt[dir][chain][grp][0], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Wait until every workgroup of this direction (and chain) has posted arrival number `step`
// (0-based).  Only one wave polls (8 lanes, one counter each): more pollers measurably slow the
// arrivals down.
// (One flag word per workgroup - a plain write-through store instead of the atomic, every poller
// reading all 128 flags - was measured too: 5.4 / 7.6 us per step against 5.3 / 7.2.  So was
// running the forward pass as 2 x 256 four-unit workgroups, two per CU, so that one's MFMAs
// overlap the other's barrier: the barrier over twice as many arrivals costs 4 us, 7.5 us/step.
// And software-pipelined polling, 2 / 3 loads in flight per poller: wait 1.40 -> 1.64 / 1.90 us.
// The round trip (arrival atomic out, poll load back) is 1.3 us even for the last workgroup to
// arrive; every extra access to the counter lines makes it longer.)
// On timeout the error word is raised and the workgroup carries on with whatever it reads
// (results are invalid, the host reports CTCASR_ERR_TIMEOUT) so that no barrier is abandoned.
template <int CHAINS>
__device__ __forceinline__ void dir_wait(SyncWords *sy, ChainSync *cs, int dir, int chain,
                                         int group_size, unsigned step, int ctid) {
    if (ctid < 64) {
        const unsigned target = (unsigned)group_size * (step + 1);
        unsigned spins = 0;
        for (;;) {
            bool ready = true;
            if (ctid < PRNN_GROUPS)
                ready = __hip_atomic_load(&sy->group_cnt[dir][chain][ctid][0], __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT) >= target;
            if (__all(ready)) break;
            __builtin_amdgcn_s_sleep(PRNN_POLL_SLEEP);
            if (++spins > PRNN_SPIN_LIMIT ||
                ((spins & 1023u) == 0 &&
                 __hip_atomic_load(&sy->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                if (ctid == 0)
                    __hip_atomic_store(&sy->error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
        if constexpr (CHAINS > 1) {
            asm volatile("" ::: "memory");
            if (ctid == 0)
                __hip_atomic_store(&cs->flag, step + 1, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    } else if constexpr (CHAINS > 1) {
        while (lds_load(&cs->flag) < step + 1) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    }
    if constexpr (CHAINS == 1) __syncthreads();
}

// Called by a workgroup (thread 0 of the chain) after its LAST dir_wait of a launch: none of its
// threads touches the arrival counters again.  The last workgroup of the (direction, chain) group
// to get here - by then every poller of the group has finished - zeroes the group's counters, so
// the next launch on this workspace finds them clean without a memset on the critical path (a
// 4 KB hipMemsetAsync between two launches measured 0.26-0.43 ms when GEMMs of another stream
// were holding the CUs).
__device__ __forceinline__ void counters_done(SyncWords *sy, int dir, int chain, int nwg) {
    const unsigned before = __hip_atomic_fetch_add(&sy->done[dir][chain][0], 1u, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1 == (unsigned)nwg) {
        for (int g = 0; g < PRNN_GROUPS; ++g)
            __hip_atomic_store(&sy->group_cnt[dir][chain][g][0], 0u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sy->done[dir][chain][0], 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Residency hand-shake.  Work on another stream that should fill the CUs a persistent launch
// leaves free (weight-gradient GEMMs beside the half-chip backward recurrence) must not get to
// the chip first: the persistent kernel's workgroups would then wait for CUs until the first
// GEMM has drained (measured: it starts 1.9 ms late).  Round 1/2 idled the side stream with a
// timed spacer kernel (70-100 us, a guess that a kernel trace showed losing its race up to
// 3.6 ms).  Now every workgroup of a launch that carries a ticket counts itself in when it
// STARTS - by then it holds its CU - and the one that completes the grid posts the ticket; a
// one-lane gate kernel on the other stream (ctcasr_rnn_resident_gate) waits for that ticket,
// with a bound.  Tickets are 24-bit launch numbers chosen by the caller, compared modulo 2^24.
__device__ __forceinline__ void resident_signal(SyncWords *sy, unsigned ticket) {
    if (ticket == 0 || threadIdx.x != 0) return;
    const unsigned before = __hip_atomic_fetch_add(&sy->resident[0], 1u, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1 == gridDim.x) {
        __hip_atomic_store(&sy->resident[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sy->resident_ticket[0], ticket, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A time-out word that is already set when a launch starts (sticky until the host polls it): every
// result since is invalid anyway - the workgroup leaves at once instead of running its steps with
// waits that each give up only after another 1024 polls (a release mode that
// wedges one barrier at N > 1 must not turn the rest of a benchmark leg into minutes of spinning).
// Workgroups of the SAME launch that are already waiting for this one time out within 1024 polls
// per step, as before.
__device__ __forceinline__ bool launch_poisoned(SyncWords *sy) {
    return __hip_atomic_load(&sy->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

__global__ void resident_gate_kernel(SyncWords *sy, unsigned ticket, unsigned long long ticks) {
    const unsigned long long start = wall_clock64();
    for (;;) {
        const unsigned seen = __hip_atomic_load(&sy->resident_ticket[0], __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
        // seen >= ticket (mod 2^24); 0 = nothing posted yet (tickets are 1 .. 2^24 - 1: a freshly
        // zeroed workspace must not pass a ticket above 2^23 at once)
        if (seen != 0u && ((seen - ticket) & 0xFFFFFFu) < 0x800000u) break;
        if (wall_clock64() - start >= ticks) break;
        __builtin_amdgcn_s_sleep(8);
    }
}

// ---------------------------------------------------------------------------------------------
// forward.  NT N-tiles of 16 gate columns per workgroup (cols = 16*NT = G * UPB), QW = 16-float
// K chunks per wave (H = 64 * QW), MT = batch tiles of 16 rows.
// LDS: fragments [NT][4*QW][64] float4, then reduction scratch [4][NT][MT*16][17], then a flag.
// ---------------------------------------------------------------------------------------------
// REGW > 0: the last REGW of a wave's QW * NT B-fragment slots (slot = chunk * NT + tile) live in
// registers instead of LDS - the variant for 64 workgroups per direction (half of the chip), whose
// 256 KB weight slice does not fit LDS alone.
template <int CELL, int NT, int QW, int MT, int REGW = 0, int CHAINS = 1>
__global__ void __launch_bounds__(PRNN_THREADS * CHAINS) prnn_fwd_kernel(PArgs p) {
    static_assert(CHAINS == 1 || (MT == 1 && REGW == 0), "two chains: one batch tile each");
    // G = gate slots in the column layout, GR = gates that exist: the GRU's three gates use the
    // LSTM's four-slot layout with an all-zero fourth slot (24 real columns per 8 units do not
    // tile into 16-column MFMA tiles; a quarter of the MFMAs and of the weight slice is padding)
    constexpr bool GRU = CELL == CTCASR_CELL_GRU;
    constexpr int G = (CELL == CTCASR_CELL_LSTM || GRU) ? 4 : 1;
    constexpr int GR = GRU ? 3 : G;
    constexpr int COLS = 16 * NT;
    constexpr int UPB = COLS / G;
    constexpr int QS = QW * NT;          // B-fragment slots per wave
    constexpr int QL = QS - REGW;        // ... of which in LDS
    constexpr int ITEMS = (16 * MT * UPB + PRNN_THREADS - 1) / PRNN_THREADS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    resident_signal(p.sync, p.ticket);
    if (launch_poisoned(p.sync)) return;
    float4 *frag = reinterpret_cast<float4 *>(smem);
    constexpr int RED_FLOATS = 4 * NT * MT * 16 * 17;
    // chain = batch tile with its own barrier (CHAINS = 2: waves 0-3 / 4-7); `tid` and `wave`
    // count within the chain, `row0` is the tile's first batch row
    // (readfirstlane: wave-uniform, so that branches on it are scalar branches - s_setprio is a
    // scalar instruction and ignores the exec mask of a predicated block)
    // CHAINS = 1 with a grid of 2 x (2 * nwg) workgroups: the two tiles run as separate groups of
    // workgroups (each tile on its own CUs, nothing shared but the launch)
    const int chain =
        CHAINS > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / PRNN_THREADS)
                   : p.chain0 + (int)blockIdx.x / (p.ndir * p.nwg);
    const int row0 = chain * 16;
    const int lchain = CHAINS > 1 ? chain : 0;      // chain index WITHIN the workgroup (LDS carve)
    float *red = reinterpret_cast<float *>(smem + (size_t)4 * QL * 64 * sizeof(float4)) +
                 lchain * RED_FLOATS;
    ChainSync *cs = reinterpret_cast<ChainSync *>(
                        smem + (size_t)4 * QL * 64 * sizeof(float4) +
                        (size_t)CHAINS * RED_FLOATS * sizeof(float)) + lchain;
    unsigned bar_epoch = 0, arrivals = 0;
    // Two chains left alone run in lockstep (both wait, then both want the matrix pipe, sharing
    // it 50:50 - measured 8.5 us per forward step against 7.3 with one barrier): a static
    // priority for chain 0 lets it through first, after which the chains stay out of phase and
    // each one's exchange round trip hides behind the other's MFMAs.
    // (Round 3: both tiles as two chains in every workgroup of a WHOLE-chip launch - 128
    // workgroups per direction, 8 units each, 1.7 us of MFMA per chain and step - with the
    // chains' MFMA phases taking turns through an LDS lock (one holder at a time; the code is
    // gone): 7.2 us per step with the lock holder at s_setprio 2, 6.96 at equal
    // priority, 7.14 without the lock, against 6.1 for one group of workgroups per tile - the
    // other chain's gate math (VALU, transcendentals) crawls while a chain issues MFMAs on the
    // same SIMD: reduce + gates + publish 0.56 -> 1.85 - 2.46 us.  Not kept.)
    if constexpr (CHAINS > 1) {
        if (chain == 0) __builtin_amdgcn_s_setprio(PRNN_CHAIN0_PRIO);
    }

    const int tid = threadIdx.x % PRNN_THREADS, lane = tid & 63, wave = tid >> 6;
    // PRNN_XCD_AWARE (off): workgroup b runs on XCD b % 8 in practice, so direction 0 could take
    // XCDs 0-3 and direction 1 XCDs 4-7 - every line of the exchange buffer an XCD pulls in from
    // the Infinity Cache is then used by twice as many workgroups of that XCD.  Measured: no
    // difference at B = 16 or 32, forward or backward (4.5 / 7.2 / 6.1 / 11.3 us per step either
    // way), so the plain mapping stays.
    const int wg = blockIdx.x % (p.ndir * p.nwg);
#if PRNN_XCD_AWARE
    const int xcd = wg & 7, rank = wg >> 3;
    const int dir = p.dir0 + (xcd >> 2), slice = rank * 4 + (xcd & 3);    // (ndir = 2 only)
    // arrival counters: two per XCD of the direction
    const int group_size = p.nwg / PRNN_GROUPS, grp = (xcd & 3) * 2 + (rank & 1);
#else
    const int dir = p.dir0 + wg / p.nwg, slice = wg % p.nwg;
    const int group_size = p.nwg / PRNN_GROUPS, grp = slice / group_size;
#endif
    const int H = p.H, B = p.B, T = p.T, BS = p.BS;
    const int u0 = slice * UPB;
    const int kq = 4 * (lane >> 4);

    // ---- stage this workgroup's slice of R in fragment order (once): LDS, then registers -------
    float4 wreg[REGW > 0 ? REGW : 1];
    {
        auto slot = [&](int sl) -> float4 {
            const int i = sl / NT, c = (sl % NT) * 16 + (lane & 15);
            if (GRU && c / UPB >= GR) return make_float4(0.f, 0.f, 0.f, 0.f);
            const float *wrow =
                p.w + ((size_t)dir * GR * H + (c / UPB) * H + u0 + (c % UPB)) * H + kq;
            return ldg4(wrow + 16 * (wave * QW + i));
        };
        // (two chains share the LDS copy: each stages every other slot)
        for (int sl = lchain; sl < QL; sl += CHAINS) frag[(wave * QL + sl) * 64 + lane] = slot(sl);
        if (CHAINS > 1 && tid == 0) *cs = ChainSync{0u, 0u, 0u, 0u};
#pragma unroll
        for (int sl = 0; sl < REGW; ++sl) wreg[sl] = slot(QL + sl);
    }
    __syncthreads();

    // Published rows go to an exchange buffer laid out [step][dir][16-float K chunk][k group of
    // 4][b][4 floats]: the A-fragment load of a chunk (lane l: batch row l & 15, k group l >> 4)
    // is then LANE-LINEAR - lane l reads bytes [16 l, 16 l + 16) of one contiguous 1 KB block.
    // Reading fragments from y itself (rows 8 KB apart: 16 half-used lines per instruction) ran
    // at ~25 GB/s per CU, and a contiguous block with lanes permuted inside it (4 address cycles
    // per lane quad) was still texture-addresser bound at ~37 GB/s per CU.
    // The buffer starts with an all-zero block of 2*B*G*H floats that no kernel ever writes (rows
    // that are not running read it; zero-filled once with the workspace), the steps follow.
    const size_t x_base = (size_t)2 * B * GR * H;     // floats of the all-zero block
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.xchg, 0, (int)((x_base + (size_t)T * 2 * B * H) * sizeof(float)), 0x00020000);
    const size_t x_step = (size_t)2 * B * H;          // floats per step
    // every workgroup of a direction reads the same rows: start each one at a different chunk so
    // that the 16 workgroups sharing an XCD's L2 do not all hit the same channel at once
    // (register-resident fragments need a static chunk -> register map: no rotation then)
    const int rot = REGW == 0 ? (slice % QW) : 0;

    // ---- per-item state ----------------------------------------------------------------------
    float c_state[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        c_state[it] = 0.f;
        if constexpr (CELL == CTCASR_CELL_LSTM || GRU) {
            // continuing a pass that an earlier launch started: pick up its cell state (LSTM) /
            // hidden state (GRU: h_{t-1} of the units this thread owns enters z * h_{t-1})
            const int item = tid + it * PRNN_THREADS;
            if (p.s_lo > 0 && item < 16 * MT * UPB && row0 + item / UPB < B)
                c_state[it] = p.carry[((size_t)dir * B + row0 + item / UPB) * H + u0 + item % UPB];
        }
    }

    int a_steps[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = row0 + mt * 16 + (lane & 15);
        a_steps[mt] = row < B ? row_steps(p.seq_len, row, T) : 0;
    }
    // the input projection's bias: an item's unit is the same in every step, so its G bias
    // values live in registers (saves the bias epilogue of the xw GEMM: 0.23 ms of 4.16 at C3)
    float xb[ITEMS][GR], bq[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int item = tid + it * PRNN_THREADS;
#pragma unroll
        for (int g = 0; g < GR; ++g)
            xb[it][g] = p.bias && item < 16 * MT * UPB
                            ? p.bias[(size_t)dir * GR * H + (size_t)g * H + u0 + item % UPB] : 0.f;
        // GRU: the candidate gate's recurrent bias stays inside r * (R_n h + b_Rn)
        bq[it] = GRU && item < 16 * MT * UPB
                     ? p.b_hh[(size_t)dir * 3 * H + 2 * H + u0 + item % UPB] : 0.f;
    }

    unsigned long long pt[5] = {0, 0, 0, 0, 0};
    // phase timings: thread 0 of each chain (chain 1's go to prof[8..12] of workgroup 0)
    const bool prof = p.prof && tid == 0;
    for (int s = p.s_lo; s < p.s_hi; ++s) {
        unsigned long long c0 = prof ? wall_clock64() : 0;
        // gate pre-activations from the input projection: independent of the recurrence, so
        // they are requested before waiting for the other workgroups
        float xw[ITEMS][GR];
        int it_t[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int item = tid + it * PRNN_THREADS;
            it_t[it] = -1;
            if (item < 16 * MT * UPB) {
                const int b = row0 + item / UPB, u = item % UPB;
                if (b < B) {
                    const int steps = row_steps(p.seq_len, b, T);
                    if (s < steps) {
                        const int t = row_time(dir, s, steps);
                        it_t[it] = t;
                        const float *x = p.xw + (((size_t)t * BS + b) * 2 + dir) * GR * H + u0 + u;
#pragma unroll
                        for (int g = 0; g < GR; ++g) xw[it][g] = x[(size_t)g * H] + xb[it][g];
                    }
                }
            }
        }

        f32x4 acc[MT][NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

        if (s > 0) {
            // (the first step of a continued pass reads what the previous launch published)
            if (s > p.s_lo) {
                dir_wait<CHAINS>(p.sync, cs, dir, chain, group_size, (unsigned)(s - 1 - p.s_lo),
                                 tid);
                if (s == p.s_hi - 1 && tid == 0) counters_done(p.sync, dir, chain, p.nwg);
            }
            if (prof) { unsigned long long c = wall_clock64(); pt[0] += c - c0; c0 = c; }
            // A fragments: h_{s-1} rows straight from y, every load issued before the first MFMA
            float4 a[MT][QW];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = row0 + mt * 16 + (lane & 15);
                // rows that are not running (beyond B, or past their length) read the all-zero
                // block at the start of the exchange buffer: the loads stay unconditional, so the compiler
                // can count them (vmcnt(N)) and start the MFMAs as the first ones land
                const bool ok = s < a_steps[mt];     // row still running (implies s-1 ran too)
                const unsigned aoff = (unsigned)(((ok ? x_base + (size_t)(s - 1) * x_step : 0) +
                                                  (size_t)dir * B * H +
                                                  (size_t)(wave * QW) * B * 16 +
                                                  (size_t)(lane >> 4) * B * 4 +
                                                  (size_t)(ok ? row : 0) * 4) *
                                                 sizeof(float));
#pragma unroll
                for (int i = 0; i < QW; ++i)
                    a[mt][i] = load16_sc1(x_rsrc, aoff + (unsigned)(((i + rot) % QW) *
                                                                    B * 64));
            }
            // keep every exchange load above the MFMA loop: hipcc otherwise sinks each load next to
            // its first use and the step degenerates to load -> wait -> 8 MFMAs -> load ...
            __builtin_amdgcn_sched_barrier(0);
            // B fragments one chunk ahead of the MFMAs that consume them (see the backward kernel)
            auto bfrag = [&](int i, int nt) -> float4 {     // compile-time slot when REGW > 0
                if constexpr (REGW == 0) {
                    return frag[(wave * QL + ((i + rot) % QW) * NT + nt) * 64 + lane];
                } else {
                    const int sl = i * NT + nt;
                    return sl < QL ? frag[(wave * QL + sl) * 64 + lane] : wreg[sl - QL];
                }
            };
            float4 bf[NT], nf[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bf[nt] = bfrag(0, nt);
#pragma unroll
            for (int i = 0; i < QW; ++i) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    nf[nt] = bf[nt];
                    if (i + 1 < QW) nf[nt] = bfrag(i + 1, nt);
                }
                // pin the order: next chunk's ds_reads, THEN this chunk's MFMAs (hipcc otherwise
                // sinks each read to one or two MFMAs before its first use).  Measured: plain RNN
                // (NT = 1, 4 MFMAs per read) 5.57 -> 5.28 us per step; LSTM (NT = 2, 8 MFMAs per
                // pair of reads) 5.29 -> 5.39, so only the former is pinned.
                if constexpr (NT == 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if constexpr (NT == 2) {
                        mma4x2(acc[mt][0], acc[mt][1], a[mt][i], bf[0], a[mt][i], bf[1]);
                    } else if constexpr (NT == 4) {
                        mma4x2(acc[mt][0], acc[mt][1], a[mt][i], bf[0], a[mt][i], bf[1]);
                        mma4x2(acc[mt][2], acc[mt][3], a[mt][i], bf[2], a[mt][i], bf[3]);
                    } else {
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) mma4(acc[mt][nt], a[mt][i], bf[nt]);
                    }
                }
                if constexpr (NT == 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bf[nt] = nf[nt];
            }
        }
        // cross-wave reduction of the K split
        if (prof) {
            asm volatile("" ::"v"(acc[0][0][0]));
            unsigned long long c = wall_clock64(); pt[1] += c - c0; c0 = c;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    red[((wave * NT + nt) * MT * 16 + mt * 16 + 4 * (lane >> 4) + r) * 17 +
                        (lane & 15)] = acc[mt][nt][r];
        if constexpr (CHAINS == 1) __syncthreads();
        else chain_barrier(cs, bar_epoch, lane);
        if (prof) { unsigned long long c = wall_clock64(); pt[4] += c - c0; }

        float hv[ITEMS], rsv[ITEMS][5];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            hv[it] = 0.f;
            if (it_t[it] >= 0) {
                const int item = tid + it * PRNN_THREADS;
                const int b = item / UPB, u = item % UPB;      // row within the tile
                float rec[GR];
#pragma unroll
                for (int g = 0; g < GR; ++g) {
                    const int c = g * UPB + u;
                    float sum = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        sum += red[((w * NT + (c >> 4)) * MT * 16 + b) * 17 + (c & 15)];
                    rec[g] = sum;
                }
                if constexpr (CELL == CTCASR_CELL_LSTM) {
                    const float gi = sigmoidf_(xw[it][0] + rec[0]);
                    const float gf = sigmoidf_(xw[it][1] + rec[1]);
                    const float gg = tanhf_(xw[it][2] + rec[2]);
                    const float go = sigmoidf_(xw[it][3] + rec[3]);
                    const float c = gf * c_state[it] + gi * gg;
                    c_state[it] = c;
                    hv[it] = go * tanhf_(c);
                    rsv[it][0] = gi; rsv[it][1] = gf; rsv[it][2] = gg; rsv[it][3] = go;
                    rsv[it][4] = c;
                } else if constexpr (GRU) {
                    // cuDNN GRU: n = tanh(W_n x + b_Wn + r * (R_n h + b_Rn)); h = (1-z) n + z h'
                    const float gr_ = sigmoidf_(xw[it][0] + rec[0]);
                    const float gz = sigmoidf_(xw[it][1] + rec[1]);
                    const float q = rec[2] + bq[it];
                    const float gn = tanhf_(xw[it][2] + gr_ * q);
                    hv[it] = (1.f - gz) * gn + gz * c_state[it];
                    c_state[it] = hv[it];
                    rsv[it][0] = gr_; rsv[it][1] = gz; rsv[it][2] = gn; rsv[it][3] = q;
                } else {
                    const float pre = xw[it][0] + rec[0];
                    hv[it] = CELL == CTCASR_CELL_RNN_RELU ? relu_keep_nan(pre) : tanhf_(pre);
                }
            }
            // publish h: lanes of 4 consecutive units gather into one 16-byte sc1 store
            const float h1 = __shfl_down(hv[it], 1, 64), h2 = __shfl_down(hv[it], 2, 64),
                        h3 = __shfl_down(hv[it], 3, 64);
            if (it_t[it] >= 0 && (tid & 3) == 0) {
                const int item = tid + it * PRNN_THREADS;
                const int b = row0 + item / UPB, unit = u0 + item % UPB;
                store16_sc1(x_rsrc, (unsigned)((x_base + (size_t)s * x_step + (size_t)dir * B * H +
                                                (size_t)(unit >> 4) * B * 16 +
                                                (size_t)((unit & 15) >> 2) * B * 4 +
                                                (size_t)b * 4) * sizeof(float)),
                            hv[it], h1, h2, h3);
            }
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[2] += c - c0; c0 = c; }
        if (s + 1 < p.s_hi) dir_arrive<CHAINS>(p.sync, cs, dir, chain, grp, tid, arrivals);
        // y and the reserve for the backward pass: nobody inside this launch reads them
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            if (it_t[it] < 0) continue;
            const int item = tid + it * PRNN_THREADS;
            const int b = row0 + item / UPB, unit = u0 + item % UPB;
            p.y[((size_t)it_t[it] * BS + b) * 2 * H + dir * H + unit] = hv[it];
        }
        if constexpr (CELL == CTCASR_CELL_LSTM || GRU) {
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                if (it_t[it] < 0) continue;
                const int item = tid + it * PRNN_THREADS;
                const int b = row0 + item / UPB, unit = u0 + item % UPB;
                float *gr = p.gates + (((size_t)it_t[it] * BS + b) * 2 + dir) * 4 * H + unit;
                gr[0] = rsv[it][0]; gr[H] = rsv[it][1]; gr[2 * H] = rsv[it][2];
                gr[3 * H] = rsv[it][3];
                if constexpr (!GRU)
                    p.cells[(((size_t)it_t[it] * BS + b) * 2 + dir) * H + unit] = rsv[it][4];
            }
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[3] += c - c0; c0 = c; }
    }
    if constexpr (CELL == CTCASR_CELL_LSTM || GRU) {
        if (p.s_hi < T) {
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                const int item = tid + it * PRNN_THREADS;
                if (item < 16 * MT * UPB && row0 + item / UPB < B)
                    p.carry[((size_t)dir * B + row0 + item / UPB) * H + u0 + item % UPB] =
                        c_state[it];
            }
        }
    }
    if (prof) {
        for (int i = 0; i < 4; ++i) {
            if (blockIdx.x == 0) p.sync->prof[chain * 8 + i] = pt[i];
            if (blockIdx.x < 256 && chain == 0) p.sync->prof_all[blockIdx.x][i] = pt[i];
        }
        // (of which, inside phase 2: partial-tile writes + the barrier of the chain's 4 waves)
        if (blockIdx.x == 0) p.sync->prof[chain * 8 + 4] = pt[4];
    }
}

// ---------------------------------------------------------------------------------------------
// forward on the fp16 matrix pipe (round 4; LSTM / GRU, `flags` bit CTCASR_RNN_F16).
//
// prnn_fwd_kernel is bound by the issue rate of v_mfma_f32_16x16x4_f32 (3.4 of its 6.1 us per
// step at B = 32: 256 MFMAs of 32 cycles per wave), and gfx950 runs the 16-bit MFMAs at 16 x that
// rate.  Both operands of THIS product are bounded - |h| <= 1, and a workgroup's slice of W_hh by
// its own largest magnitude - so each is held as TWO fp16 pieces after a power-of-two scale,
//     x s = x1 + x2,   x1 = rne_f16(x s),  x2 = rne_f16(x s - x1)        (11 + 11 mantissa bits)
// and the product is the three piece products h1 w1 + h1 w2 + h2 w1 accumulated in fp32 by
// v_mfma_f32_16x16x32_f16 (dropped: h2 w2 <= 2^-22 |h w|; the same form as the forward projection
// GEMMs) - 3 MFMAs of K = 32 where the fp32 kernel issues 8 of K = 4.
// Nothing else changes size: W_hh as two fp16 pieces is the 4 bytes per weight of the fp32 slice
// (same LDS / register split), and h is PUBLISHED as its two pieces - per 32 units one 1 KB block
// of first pieces and one of second pieces, [k group of 8 units][b][8 halves], where the fp32
// kernel has two blocks of 16 units - so the exchange moves the same bytes, and a lane's 16-byte
// load from a block IS the A-fragment register quadruple of a K = 32 MFMA: no conversion and no
// re-arranging at the consumer.
//   scale of h: 2^15 (|h| <= 1); scale of W_hh: per workgroup, found while staging - the largest
//   magnitude of the slice lands in [2^14, 2^15) - so no weight can overflow whatever its size
//   (a per-workgroup scale is a per-output-column scale: it leaves through the accumulator).
// K chunk c of wave w = 32 units; lane l of a fragment holds units 8 (l >> 4) + e of it, for A
// and B alike.
// B-fragment slots per wave: (c * NT + nt) * 2 + piece; the last REGW of them live in registers.
// ---------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
union Frag16 {
    u32x4 u;
    f16x8 h;
};
#define PRNN_F16_H_SCALE 32768.0f
// the two pieces of s (already scaled): first piece in the low half, second in the high half
__device__ __forceinline__ unsigned f16_pieces(float s) {
    const _Float16 h1 = (_Float16)s;
    const _Float16 h2 = (_Float16)(s - (float)h1);
    return (unsigned)__builtin_bit_cast(unsigned short, h1) |
           ((unsigned)__builtin_bit_cast(unsigned short, h2) << 16);
}
__device__ __forceinline__ u32x4 load16u(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0);
}
// per-lane offset + wave-uniform offset (an SGPR: no address arithmetic or register per load)
__device__ __forceinline__ u32x4 load16u(__amdgpu_buffer_rsrc_t rsrc, unsigned lane_off,
                                         unsigned uniform_off) {
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)lane_off, (int)uniform_off, 0);
}
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// q = f16_pieces() of this lane's value; in the first lane of every group of 8 (lanes of 8
// consecutive units): the 8 first pieces and the 8 second pieces of the group as two 16-byte
// granules - each one IS the fragment register quadruple of an MFMA operand (lane l of a K = 32
// step holds 8 consecutive k), so the consumer loads operands, not data to re-arrange
__device__ __forceinline__ void gather8_pieces(unsigned q0, u32x4 &first, u32x4 &second) {
    const unsigned q1 = dpp_u32<0x101>(q0), q2 = dpp_u32<0x102>(q0), q3 = dpp_u32<0x103>(q0),
                   q4 = dpp_u32<0x104>(q0), q5 = dpp_u32<0x105>(q0), q6 = dpp_u32<0x106>(q0),
                   q7 = dpp_u32<0x107>(q0);                       // row_shl: lane i <- lane i + n
    first = (u32x4){(q0 & 0xFFFFu) | (q1 << 16), (q2 & 0xFFFFu) | (q3 << 16),
                    (q4 & 0xFFFFu) | (q5 << 16), (q6 & 0xFFFFu) | (q7 << 16)};
    second = (u32x4){(q0 >> 16) | (q1 & 0xFFFF0000u), (q2 >> 16) | (q3 & 0xFFFF0000u),
                     (q4 >> 16) | (q5 & 0xFFFF0000u), (q6 >> 16) | (q7 & 0xFFFF0000u)};
}

template <int CELL, int NT, int KC, int REGW = 0>
__global__ void __launch_bounds__(PRNN_THREADS) prnn_fwd16_kernel(PArgs p) {
    constexpr bool GRU = CELL == CTCASR_CELL_GRU;
    constexpr int G = 4;
    constexpr int GR = GRU ? 3 : G;
    constexpr int COLS = 16 * NT;
    constexpr int UPB = COLS / G;
    constexpr int QS = KC * NT * 2;      // B-fragment slots per wave (two pieces per tile and chunk)
    constexpr int QL = QS - REGW;        // ... of which in LDS
    constexpr int QW = 2 * KC;           // 16-unit exchange chunks per wave
    static_assert(16 * UPB <= PRNN_THREADS, "one item per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    resident_signal(p.sync, p.ticket);
    if (launch_poisoned(p.sync)) return;
    u32x4 *frag = reinterpret_cast<u32x4 *>(smem);
    float *red = reinterpret_cast<float *>(smem + (size_t)4 * QL * 64 * sizeof(u32x4));
    float *wave_top = red + 4 * NT * 16 * 17;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = blockIdx.x % (p.ndir * p.nwg);
    // Workgroup b runs on XCD b % 8.  `xcd_split` (two directions in the launch): direction 0 on
    // XCDs 0 - 3, direction 1 on XCDs 4 - 7 - an exchange block is then pulled across the fabric
    // by four L2s instead of eight, and an XCD's L2 holds one direction's blocks instead of two.
    // Two batch tiles in the launch (each its own group of workgroups): every (direction, tile)
    // on its own PAIR of XCDs - two L2s per exchange block.
    const bool split = p.xcd_split && p.ndir == 2;
    const bool pairs = PRNN_XCD_TILE_PAIRS && split && (int)gridDim.x == 2 * p.ndir * p.nwg &&
                       p.nwg % 2 == 0;
    const int chain = p.chain0 + (pairs ? ((int)blockIdx.x >> 1) & 1
                                        : (int)blockIdx.x / (p.ndir * p.nwg));
    const int row0 = chain * 16;
    const int dir = p.dir0 + (split ? (wg & 7) >> 2 : wg / p.nwg);
    const int slice = pairs ? ((int)blockIdx.x >> 3) * 2 + ((int)blockIdx.x & 1)
                            : split ? (wg >> 3) * 4 + (wg & 3) : wg % p.nwg;
    const int group_size = p.nwg / PRNN_GROUPS, grp = slice / group_size;
    const int H = p.H, B = p.B, T = p.T, BS = p.BS;
    const int u0 = slice * UPB;

    // ---- stage this workgroup's slice of R as scaled fp16 pieces, in fragment order (once) -----
    // the 8 floats of fragment (chunk c, tile nt) of this lane
    auto wload = [&](int c, int nt, float (&v)[8]) {
        const int col = nt * 16 + (lane & 15);
        if (GRU && col / UPB >= GR) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
            return;
        }
        const float *wrow = p.w + ((size_t)dir * GR * H + (col / UPB) * H + u0 + (col % UPB)) * H +
                            wave * (H / 4) + 32 * c + 8 * (lane >> 4);
        const float4 lo = ldg4(wrow), hi = ldg4(wrow + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    };
    float w_scale;
    {
        float m = 0.f;
        for (int c = 0; c < KC; ++c)
            for (int nt = 0; nt < NT; ++nt) {
                float v[8];
                wload(c, nt, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(v[e]));
            }
        m = wave_max(m);
        if (lane == 0) wave_top[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wave_top[0], wave_top[1]), fmaxf(wave_top[2], wave_top[3]));
        const unsigned bits = __float_as_uint(m);
        const int e = (int)((bits >> 23) & 0xFF) - 127;
        const int se = bits == 0u ? 0 : min(max(14 - e, -60), 60);
        w_scale = __uint_as_float((unsigned)(se + 127) << 23);
    }
    const float out_scale = 1.0f / (w_scale * PRNN_F16_H_SCALE);      // exact: powers of two
    u32x4 wreg[REGW > 0 ? REGW : 1];
    {
        // pieces (first, second) of fragment (c, nt): slots (c * NT + nt) * 2 + {0, 1}
        auto pieces = [&](int c, int nt, u32x4 &first, u32x4 &second) {
            float v[8];
            wload(c, nt, v);
            unsigned q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = f16_pieces(v[e] * w_scale);
            first = (u32x4){(q[0] & 0xFFFFu) | (q[1] << 16), (q[2] & 0xFFFFu) | (q[3] << 16),
                            (q[4] & 0xFFFFu) | (q[5] << 16), (q[6] & 0xFFFFu) | (q[7] << 16)};
            second = (u32x4){(q[0] >> 16) | (q[1] & 0xFFFF0000u), (q[2] >> 16) | (q[3] & 0xFFFF0000u),
                             (q[4] >> 16) | (q[5] & 0xFFFF0000u), (q[6] >> 16) | (q[7] & 0xFFFF0000u)};
        };
        for (int pr = 0; pr < QL / 2; ++pr) {
            u32x4 first, second;
            pieces(pr / NT, pr % NT, first, second);
            frag[(wave * QL + 2 * pr) * 64 + lane] = first;
            frag[(wave * QL + 2 * pr + 1) * 64 + lane] = second;
        }
#pragma unroll
        for (int pr = 0; pr < REGW / 2; ++pr) {
            pieces((QL / 2 + pr) / NT, (QL / 2 + pr) % NT, wreg[2 * pr], wreg[2 * pr + 1]);
        }
    }
    __syncthreads();

    // exchange buffer: [step][dir][32-unit chunk][piece][k group of 8 units][b][8 halves] behind
    // the all-zero block (the size of prnn_fwd_kernel's)
    const size_t x_base = (size_t)2 * B * GR * H;
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.xchg, 0, (int)((x_base + (size_t)T * 2 * B * H) * sizeof(float)), 0x00020000);
    const size_t x_step = (size_t)2 * B * H;
    const int rot = REGW == 0 ? (slice % KC) : 0;

    // ---- the item of this thread: row tid / UPB of the tile, unit tid % UPB -------------------
    const bool has_item = tid < 16 * UPB;
    const int ib = tid / UPB, iu = tid % UPB;
    const int brow = row0 + ib, unit = u0 + iu;
    const int steps = has_item && brow < B ? row_steps(p.seq_len, brow, T) : 0;
    float c_state = 0.f;
    if (p.s_lo > 0 && steps > 0) c_state = p.carry[((size_t)dir * B + brow) * H + unit];
    const int arow = row0 + (lane & 15);
    const int a_steps = arow < B ? row_steps(p.seq_len, arow, T) : 0;
    float xb[GR], bq = 0.f;
#pragma unroll
    for (int g = 0; g < GR; ++g)
        xb[g] = p.bias && has_item ? p.bias[(size_t)dir * GR * H + (size_t)g * H + unit] : 0.f;
    if (GRU && has_item) bq = p.b_hh[(size_t)dir * 3 * H + 2 * H + unit];

    unsigned long long pt[5] = {0, 0, 0, 0, 0};
    const bool prof = p.prof && tid == 0;
    for (int s = p.s_lo; s < p.s_hi; ++s) {
        unsigned long long c0 = prof ? wall_clock64() : 0;
        float xw[GR];
        int it_t = -1;
        if (s < steps) {
            it_t = row_time(dir, s, steps);
            const float *x = p.xw + (((size_t)it_t * BS + brow) * 2 + dir) * GR * H + unit;
#pragma unroll
            for (int g = 0; g < GR; ++g) xw[g] = x[(size_t)g * H] + xb[g];
        }

        // three accumulators per tile: h1 w1, h1 w2, h2 w1 - independent chains for the matrix
        // pipe, and the small terms are summed apart from the big one
        f32x4 acc[3][NT];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[q][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

        if (s > 0) {
            if (s > p.s_lo) {
                dir_wait<1>(p.sync, nullptr, dir, chain, group_size, (unsigned)(s - 1 - p.s_lo),
                            tid);
                if (s == p.s_hi - 1 && tid == 0) counters_done(p.sync, dir, chain, p.nwg);
            }
            if (prof) { unsigned long long c = wall_clock64(); pt[0] += c - c0; c0 = c; }
            const bool ok = s < a_steps;
            const unsigned aoff = (unsigned)(((ok ? x_base + (size_t)(s - 1) * x_step : 0) +
                                              (size_t)dir * B * H +
                                              (size_t)(wave * QW) * B * 16 +
                                              (size_t)(lane >> 4) * B * 4 +
                                              (size_t)(ok ? arow : 0) * 4) * sizeof(float));
            u32x4 a[KC][2];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int cc = (c + rot) % KC;
                a[c][0] = load16u(x_rsrc, aoff + (unsigned)((2 * cc) * B * 64));
                a[c][1] = load16u(x_rsrc, aoff + (unsigned)((2 * cc + 1) * B * 64));
            }
            __builtin_amdgcn_sched_barrier(0);      // every exchange load above the first MFMA
            auto bfrag = [&](int c, int nt, int piece) -> u32x4 {
                if constexpr (REGW == 0) {
                    return frag[(wave * QL + (((c + rot) % KC) * NT + nt) * 2 + piece) * 64 + lane];
                } else {
                    const int sl = (c * NT + nt) * 2 + piece;
                    return sl < QL ? frag[(wave * QL + sl) * 64 + lane] : wreg[sl - QL];
                }
            };
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                Frag16 h1, h2;
                h1.u = a[c][0];
                h2.u = a[c][1];
                Frag16 w1[NT], w2[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    w1[nt].u = bfrag(c, nt, 0);
                    w2[nt].u = bfrag(c, nt, 1);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1.h, w1[nt].h, acc[0][nt],
                                                                        0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1.h, w2[nt].h, acc[1][nt],
                                                                        0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[2][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h2.h, w1[nt].h, acc[2][nt],
                                                                        0, 0, 0);
            }
        }
        if (prof) {
            asm volatile("" ::"v"(acc[0][0][0]));
            unsigned long long c = wall_clock64(); pt[1] += c - c0; c0 = c;
        }
        // cross-wave reduction of the K split (the scales leave here)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                red[((wave * NT + nt) * 16 + 4 * (lane >> 4) + r) * 17 + (lane & 15)] =
                    (acc[0][nt][r] + (acc[1][nt][r] + acc[2][nt][r])) * out_scale;
        __syncthreads();
        if (prof) { unsigned long long c = wall_clock64(); pt[4] += c - c0; }

        float hv = 0.f, rsv[5];
        if (it_t >= 0) {
            float rec[GR];
#pragma unroll
            for (int g = 0; g < GR; ++g) {
                const int c = g * UPB + iu;
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    sum += red[((w * NT + (c >> 4)) * 16 + ib) * 17 + (c & 15)];
                rec[g] = sum;
            }
            if constexpr (!GRU) {
                const float gi = sigmoidf_(xw[0] + rec[0]);
                const float gf = sigmoidf_(xw[1] + rec[1]);
                const float gg = tanhf_(xw[2] + rec[2]);
                const float go = sigmoidf_(xw[3] + rec[3]);
                const float c = gf * c_state + gi * gg;
                c_state = c;
                hv = go * tanhf_(c);
                rsv[0] = gi; rsv[1] = gf; rsv[2] = gg; rsv[3] = go; rsv[4] = c;
            } else {
                const float gr_ = sigmoidf_(xw[0] + rec[0]);
                const float gz = sigmoidf_(xw[1] + rec[1]);
                const float q = rec[2] + bq;
                const float gn = tanhf_(xw[2] + gr_ * q);
                hv = (1.f - gz) * gn + gz * c_state;
                c_state = hv;
                rsv[0] = gr_; rsv[1] = gz; rsv[2] = gn; rsv[3] = q;
            }
        }
        // publish h as its two fp16 pieces: the lanes of 8 consecutive units gather into two
        // 16-byte sc1 stores (a granule of first pieces, one of second pieces)
        u32x4 first, second;
        gather8_pieces(f16_pieces(hv * PRNN_F16_H_SCALE), first, second);
        if (it_t >= 0 && (tid & 7) == 0) {
            const unsigned off =
                (unsigned)((x_base + (size_t)s * x_step + (size_t)dir * B * H +
                            (size_t)(unit >> 5) * B * 32 + (size_t)((unit & 31) >> 3) * B * 4 +
                            (size_t)brow * 4) * sizeof(float));
            __builtin_amdgcn_raw_buffer_store_b128(first, x_rsrc, (int)off, 0, 16);
            __builtin_amdgcn_raw_buffer_store_b128(second, x_rsrc,
                                                   (int)(off + (unsigned)(B * 16 * sizeof(float))),
                                                   0, 16);
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[2] += c - c0; c0 = c; }
        if (s + 1 < p.s_hi) {
            unsigned unused = 0;
            dir_arrive<1>(p.sync, nullptr, dir, chain, grp, tid, unused);
        }
        // y and the reserve for the backward pass: nobody inside this launch reads them
        if (p.y16 && it_t >= 0 && (tid & 7) == 0) {
            // ... and the pieces of y in the layout of ctcasr_split_f16 (blocks: first, first,
            // second; scale 2^15): the NEXT layer's input projection / dense4 / this layer's
            // recurrent weight gradient read them - no split pass over y
            u32x4 *dst = reinterpret_cast<u32x4 *>(
                p.y16 + (((size_t)it_t * BS + brow) * 3) * 2 * H + dir * H + unit);
            dst[0] = first;
            dst[(size_t)2 * H / 8] = first;
            dst[(size_t)4 * H / 8] = second;
        }
        if (it_t >= 0) {
            p.y[((size_t)it_t * BS + brow) * 2 * H + dir * H + unit] = hv;
            float *gr = p.gates + (((size_t)it_t * BS + brow) * 2 + dir) * 4 * H + unit;
            gr[0] = rsv[0]; gr[H] = rsv[1]; gr[2 * H] = rsv[2]; gr[3 * H] = rsv[3];
            if constexpr (!GRU)
                p.cells[(((size_t)it_t * BS + brow) * 2 + dir) * H + unit] = rsv[4];
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[3] += c - c0; c0 = c; }
    }
    if (p.s_hi < T && has_item && brow < B)
        p.carry[((size_t)dir * B + brow) * H + unit] = c_state;
    if (prof) {
        for (int i = 0; i < 4; ++i) {
            if (blockIdx.x == 0) p.sync->prof[chain * 8 + i] = pt[i];
            if (blockIdx.x < 256 && chain == 0) p.sync->prof_all[blockIdx.x][i] = pt[i];
        }
        if (blockIdx.x == 0) p.sync->prof[chain * 8 + 4] = pt[4];
    }
}

// ---------------------------------------------------------------------------------------------
// backward.  Each workgroup owns UPB hidden units (output columns of dh_rec = dgates x R); the K
// dimension is G*H (all gates of all units), split over the 4 waves: QW chunks each.
//   UPB = 8, REGW = 0  : 128 workgroups per direction = the whole chip; the slice (128 KB) is in
//                        LDS as [4*QW][32] float4 - lanes with (lane & 15) >= 8 re-read the first
//                        8 columns, the duplicated MFMA columns are ignored.
//   UPB = 16, REGW = 32: 64 workgroups per direction = HALF the chip, full MFMA tiles; the 256 KB
//                        slice is split between LDS (the first QW-REGW chunks of every wave) and
//                        REGW float4 registers per lane.  Same time per step, but 128 CUs stay
//                        free for the weight-gradient GEMMs of the layer above.
//   UPB = 32, REGW = 32: the plain RNN (G = 1, H = 2048) on half the chip: two N tiles per
//                        workgroup sharing every A chunk (twice the MFMAs per workgroup of the
//                        128-workgroup variant: 6.7 vs 5.7 us per step, 128 CUs free).
// Reduction scratch [4][MT*16][17] follows the fragments.
// ---------------------------------------------------------------------------------------------
template <int CELL, int QW, int MT, int LB, int UPB, int REGW, int CHAINS = 1>
__global__ void __launch_bounds__(PRNN_THREADS * CHAINS) prnn_bwd_kernel(PArgs p) {
    static_assert(CHAINS == 1 || MT == 1, "two chains: one batch tile each");
    constexpr bool GRU = CELL == CTCASR_CELL_GRU;
    constexpr int G = CELL == CTCASR_CELL_LSTM ? 4 : (GRU ? 3 : 1);
    constexpr bool HALF_TILE = UPB == 8;
    // UPB = 32: TWO N tiles per workgroup.  The B-fragment slots of a wave then alternate
    // (tile 0, chunk c), (tile 1, chunk c): QW counts slots, every A chunk feeds a pair of them,
    // and the two alternating accumulators ARE the two tiles (no final sum).
    constexpr bool TWO_TILES = UPB == 32;
    constexpr int NT = TWO_TILES ? 2 : 1;
    constexpr int SLOTS = HALF_TILE ? 32 : 64;      // float4 slots per chunk in LDS
    constexpr int QL = QW - REGW;                   // slots per wave kept in LDS
    constexpr int ITEMS = (16 * MT * UPB + PRNN_THREADS - 1) / PRNN_THREADS;
    constexpr int NB = QW / LB;          // load batches per wave (LB slots in flight each)
    constexpr int QA = QW / NT;          // 16-float A chunks per wave
    constexpr int LA = LB / NT;          // A chunks per load batch
    constexpr int CPG = QA / G;          // 16-float chunks per gate within a wave's unit range
    // (register-resident HALF tiles - H = 2048 - spend a register on every lane although lanes
    // l and l + 8 hold the same value: 8 units x 8192 x 4 B = 256 KB per workgroup is 128 KB of
    // LDS + 256 registers per lane, which a one-wave-per-SIMD kernel can afford)
    static_assert(!TWO_TILES || (G == 1 && REGW > 0), "two tiles: plain RNN, static slot map");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    resident_signal(p.sync, p.ticket);
    if (launch_poisoned(p.sync)) return;
    float4 *frag = reinterpret_cast<float4 *>(smem);
    constexpr int RED_FLOATS = 4 * NT * MT * 16 * 17;
    // chain = batch tile with its own barrier (see ChainSync); `tid` / `wave` count within it
    // (readfirstlane: wave-uniform, so that branches on it are scalar branches - s_setprio is a
    // scalar instruction and ignores the exec mask of a predicated block)
    // CHAINS = 1 with a grid of 2 x (2 * nwg) workgroups: the two tiles run as separate groups of
    // workgroups (each tile on its own CUs, nothing shared but the launch)
    const int chain =
        CHAINS > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / PRNN_THREADS)
                   : p.chain0 + (int)blockIdx.x / (p.ndir * p.nwg);
    const int row0 = chain * 16;
    const int lchain = CHAINS > 1 ? chain : 0;      // chain index WITHIN the workgroup (LDS carve)
    float *red = reinterpret_cast<float *>(smem + (size_t)4 * QL * SLOTS * sizeof(float4)) +
                 lchain * RED_FLOATS;
    ChainSync *cs = reinterpret_cast<ChainSync *>(
                        smem + (size_t)4 * QL * SLOTS * sizeof(float4) +
                        (size_t)CHAINS * RED_FLOATS * sizeof(float)) + lchain;
    unsigned bar_epoch = 0, arrivals = 0;
    // Two chains: a static priority for chain 0 (left alone they start in lockstep).  Round 3
    // tried explicit MFMA turns here as well (an LDS lock, one holder at a time, around
    // the loads + MFMA loop): 11.8 us per step against 11.0 without at B = 32 (GRU 10.3 / 9.7,
    // RNN-2048 11.45 / 11.40) - with the matrix pipe to itself a chain's loads + MFMA phase still
    // takes 5.8 us: this kernel is bound by the A-operand loads in flight (two batches of 16 KB
    // per wave at ~2 us of latency), not by the two chains sharing the pipe.
    if constexpr (CHAINS > 1) {
        if (chain == 0) __builtin_amdgcn_s_setprio(PRNN_CHAIN0_PRIO);
    }

    const int tid = threadIdx.x % PRNN_THREADS, lane = tid & 63, wave = tid >> 6;
    // PRNN_XCD_AWARE (off): workgroup b runs on XCD b % 8 in practice, so direction 0 could take
    // XCDs 0-3 and direction 1 XCDs 4-7 - every line of the exchange buffer an XCD pulls in from
    // the Infinity Cache is then used by twice as many workgroups of that XCD.  Measured: no
    // difference at B = 16 or 32, forward or backward (4.5 / 7.2 / 6.1 / 11.3 us per step either
    // way), so the plain mapping stays.
    const int wg = blockIdx.x % (p.ndir * p.nwg);
#if PRNN_XCD_AWARE
    const int xcd = wg & 7, rank = wg >> 3;
    const int dir = p.dir0 + (xcd >> 2), slice = rank * 4 + (xcd & 3);    // (ndir = 2 only)
    // arrival counters: two per XCD of the direction
    const int group_size = p.nwg / PRNN_GROUPS, grp = (xcd & 3) * 2 + (rank & 1);
#else
    const int dir = p.dir0 + wg / p.nwg, slice = wg % p.nwg;
    const int group_size = p.nwg / PRNN_GROUPS, grp = slice / group_size;
#endif
    const int H = p.H, B = p.B, T = p.T, GH = G * p.H, BS = p.BS;
    const int u0 = slice * UPB;
    const int kq = 4 * (lane >> 4);
    // fragment slot: lanes l and l+8 share one in the half-tile layout
    const int half = HALF_TILE ? (lane >> 4) * 8 + (lane & 7) : lane;

    float4 wreg[REGW > 0 ? REGW : 1];
    if (!HALF_TILE || (lane & 15) < 8 || REGW > 0) {
        // slot i of this wave: A chunk i / NT of tile i % NT
        const float *wrow = p.w + ((size_t)dir * H + u0 + (lane & (UPB / NT - 1))) * GH +
                            wave * (H / 4) + kq;
        auto slot = [&](int i) -> float4 {
            const int c = i / NT;
            return ldg4(wrow + (size_t)(i % NT) * 16 * GH + (c / CPG) * H + (c % CPG) * 16);
        };
        // (two chains share the LDS part: each stages every other slot; the register part is
        // per wave, so both chains load it)
        for (int i = lchain; i < QL; i += CHAINS) frag[(wave * QL + i) * SLOTS + half] = slot(i);
#pragma unroll
        for (int i = 0; i < REGW; ++i) wreg[i] = slot(QL + i);
    }
    if (CHAINS > 1 && tid == 0) *cs = ChainSync{0u, 0u, 0u, 0u};
    __syncthreads();

    // exchange buffer [step][dir][16-float chunk of n = g*H + unit][k group][b][4] (see forward)
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.xchg, 0, (int)((size_t)(T + 1) * 2 * B * GH * sizeof(float)), 0x00020000);
    const size_t x_step = (size_t)2 * B * GH;      // = the all-zero block in front of the steps
    const size_t x_base = x_step;
    // de-synchronise the workgroups' walk over the chunks (LDS-only variant; register-resident
    // fragments need a static chunk -> register map)
    const int rot = REGW == 0 ? (slice % QW) : 0;
    float dc_state[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        dc_state[it] = 0.f;
        if constexpr (CELL == CTCASR_CELL_LSTM || GRU) {
            // continuing a pass that an earlier launch started: pick up its cell-state gradient
            // (LSTM) / the dh * z term of the step above (GRU)
            const int item = tid + it * PRNN_THREADS;
            if (p.s_hi < T && item < 16 * MT * UPB && row0 + item / UPB < B)
                dc_state[it] = p.carry[((size_t)dir * B + row0 + item / UPB) * H + u0 + item % UPB];
        }
    }
    int a_steps[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = row0 + mt * 16 + (lane & 15);
        a_steps[mt] = row < B ? row_steps(p.seq_len, row, T) : 0;
    }

    // bias gradients: an item's unit is the same in every step, so its share of the column sums
    // of dxw (GRU: + of drec's candidate gate) over this launch's steps stays in registers
    constexpr int GS = GRU ? 2 * G : G;
    float dbs[ITEMS][GS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it)
#pragma unroll
        for (int g = 0; g < GS; ++g) dbs[it][g] = 0.f;

    unsigned long long pt[4] = {0, 0, 0, 0};
    const bool prof = p.prof && blockIdx.x == 0 && threadIdx.x == 0;
    for (int s = p.s_hi - 1; s >= p.s_lo; --s) {
        unsigned long long c0 = prof ? wall_clock64() : 0;
        // everything the cell derivative needs except dh_rec: prefetched before the barrier
        float dyv[ITEMS], gv[ITEMS][4], cv[ITEMS], cpv[ITEMS], hv[ITEMS];
        int it_t[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int item = tid + it * PRNN_THREADS;
            it_t[it] = -1;
            if (item < 16 * MT * UPB) {
                const int b = row0 + item / UPB, u = item % UPB;
                if (b < B) {
                    const int steps = row_steps(p.seq_len, b, T);
                    if (s < steps) {
                        const int t = row_time(dir, s, steps);
                        const int unit = u0 + u;
                        it_t[it] = t;
                        dyv[it] = p.dy[((size_t)t * BS + b) * 2 * H + dir * H + unit];
                        if constexpr (CELL == CTCASR_CELL_LSTM) {
                            const float *gr = p.gates + (((size_t)t * BS + b) * 2 + dir) * 4 * H + unit;
                            gv[it][0] = gr[0]; gv[it][1] = gr[H];
                            gv[it][2] = gr[2 * H]; gv[it][3] = gr[3 * H];
                            cv[it] = p.cells[(((size_t)t * BS + b) * 2 + dir) * H + unit];
                            cpv[it] = 0.f;
                            if (s > 0) {
                                const int tp = row_time(dir, s - 1, steps);
                                cpv[it] = p.cells[(((size_t)tp * BS + b) * 2 + dir) * H + unit];
                            }
                        } else if constexpr (GRU) {
                            // r, z, n, q = R_n h + b_Rn of this step; h of the step before
                            const float *gr = p.gates + (((size_t)t * BS + b) * 2 + dir) * 4 * H + unit;
                            gv[it][0] = gr[0]; gv[it][1] = gr[H];
                            gv[it][2] = gr[2 * H]; gv[it][3] = gr[3 * H];
                            hv[it] = 0.f;
                            if (s > 0) {
                                const int tp = row_time(dir, s - 1, steps);
                                hv[it] = p.y[((size_t)tp * BS + b) * 2 * H + dir * H + unit];
                            }
                        } else {
                            hv[it] = p.y[((size_t)t * BS + b) * 2 * H + dir * H + unit];
                        }
                    }
                }
            }
        }

        f32x4 acc[MT], acc2[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            acc2[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }

        if (s < T - 1) {
            // dgates of step s+1 from every workgroup of this direction (the first step of a
            // continued pass reads what the previous launch left: nothing to wait for)
            if (s < p.s_hi - 1) {
                dir_wait<CHAINS>(p.sync, cs, dir, chain, group_size, (unsigned)(p.s_hi - 2 - s),
                                 tid);
                if (s == p.s_lo && tid == 0) counters_done(p.sync, dir, chain, p.nwg);
            }
            if (prof) { unsigned long long c = wall_clock64(); pt[0] += c - c0; c0 = c; }
            unsigned aoff[MT];
            bool ok[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = row0 + mt * 16 + (lane & 15);
                ok[mt] = s + 1 < a_steps[mt];     // otherwise: the all-zero block
                aoff[mt] = (unsigned)(((ok[mt] ? x_base + (size_t)(s + 1) * x_step : 0) +
                                       (size_t)dir * B * GH +
                                       (size_t)(wave * (H / 64)) * B * 16 +
                                       (size_t)(lane >> 4) * B * 4 +
                                       (size_t)(ok[mt] ? row : 0) * 4) * sizeof(float));
            }
            // chunk i of this wave = gate i / CPG, 16-float unit chunk i % CPG; loads of batch
            // nb+1 are in flight while batch nb feeds the MFMAs.
            // (Every variant delivers the A operand at ~50 GB/s per CU - 256 KB in 5.2 us at
            // B = 16, 512 KB in 11.3 at B = 32 - whatever the batch size.  Two probes of why, both
            // negative: the register-resident kernels in four unrolled variants that start the
            // walk over the block a quarter apart, selected per workgroup so that the workgroups
            // of one XCD do not ask for the same lines at the same time: 7.2 -> 7.7 / 11.4 ->
            // 12.7 us per step - walking in step is what makes the XCD's L2 merge the misses;
            // and an L2 warm-up right after the barrier, every workgroup of an XCD touching its
            // own eighth of the block, one line per thread: 7.2 -> 7.6 / 11.3 -> 11.8.)
            float4 a[2][MT][LA];
            auto issue = [&](int nb, float4 (&dst)[MT][LA]) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < LA; ++i) {
                        const int c = (nb * LA + i + rot) % QA;
                        // chunk index in n-space: gate * (H / 16) + unit chunk
                        const unsigned off = (unsigned)(((size_t)(c / CPG) * (H / 16) + (c % CPG)) *
                                                        B * 16 * sizeof(float));
#if PRNN_PROBE_HALF_LOADS     // timing probe only (wrong results): half of the A bytes
                        if (i & 1) dst[mt][i] = dst[mt][i - 1];
                        else
#endif
                        dst[mt][i] = load16_sc1(x_rsrc, aoff[mt] + off);
                    }
            };
            issue(0, a[0]);
            // B fragments (LDS / registers) run one PAIR of chunks ahead of the MFMAs that use
            // them, across load batches too: a ds_read_b128 issued right before its consumers
            // costs about as much as the pair's 8 MFMAs.  The scheduling barriers pin that
            // order - hipcc otherwise sinks each read next to its first use.
            auto bfrag = [&](int c) -> float4 {      // c: chunk index, compile-time after unrolling
                if constexpr (REGW == 0) {
                    return frag[(wave * QL + ((c + rot) % QW)) * SLOTS + half];
                } else {
                    return c < QL ? frag[(wave * QL + c) * SLOTS + half] : wreg[c - QL];
                }
            };
            float4 cb0 = bfrag(0), cb1 = bfrag(1);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if (nb + 1 < NB) issue(nb + 1, a[(nb + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);   // loads stay above this batch's MFMAs
#pragma unroll
                for (int i = 0; i < LB; i += 2) {
                    const int c = nb * LB + i;
                    float4 nb0 = cb0, nb1 = cb1;
                    if (c + 2 < QW) { nb0 = bfrag(c + 2); nb1 = bfrag(c + 3); }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        if constexpr (TWO_TILES)      // one A chunk, the pair of tiles
                            mma4x2(acc[mt], acc2[mt], a[nb & 1][mt][i / 2], cb0,
                                   a[nb & 1][mt][i / 2], cb1);
                        else
                            mma4x2(acc[mt], acc2[mt], a[nb & 1][mt][i], cb0,
                                   a[nb & 1][mt][i + 1], cb1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    cb0 = nb0; cb1 = nb1;
                }
            }
            if constexpr (!TWO_TILES) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] += acc2[mt];
            }
        }
        if (prof) {
            asm volatile("" ::"v"(acc[0][0]));
            unsigned long long c = wall_clock64(); pt[1] += c - c0; c0 = c;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                red[((wave * NT) * MT * 16 + mt * 16 + 4 * (lane >> 4) + r) * 17 + (lane & 15)] =
                    acc[mt][r];
                if constexpr (TWO_TILES)
                    red[((wave * NT + 1) * MT * 16 + mt * 16 + 4 * (lane >> 4) + r) * 17 +
                        (lane & 15)] = acc2[mt][r];
            }
        if constexpr (CHAINS == 1) __syncthreads();
        else chain_barrier(cs, bar_epoch, lane);

#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            // dg: what is published for the recurrence (GRU: drec, the candidate gate scaled by
            // r); dxn: the GRU's dxw entry of the candidate gate (not scaled)
            float dg[G], dxn = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) dg[g] = 0.f;
            const int item = tid + it * PRNN_THREADS;
            const int b = item / UPB, u = item % UPB;          // row within the tile
            if (it_t[it] >= 0) {
                float dh = dyv[it];
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    dh += red[((w * NT + (u >> 4)) * MT * 16 + b) * 17 + (u & 15)];
                if constexpr (CELL == CTCASR_CELL_LSTM) {
                    const float gi = gv[it][0], gf = gv[it][1], gg = gv[it][2], go = gv[it][3];
                    const float tc = tanhf_(cv[it]);
                    const float dc = dc_state[it] + dh * go * (1.f - tc * tc);
                    dg[0] = dc * gg * gi * (1.f - gi);
                    dg[1] = dc * cpv[it] * gf * (1.f - gf);
                    dg[2] = dc * gi * (1.f - gg * gg);
                    dg[3] = dh * tc * go * (1.f - go);
                    dc_state[it] = dc * gf;
                } else if constexpr (GRU) {
                    const float gr_ = gv[it][0], gz = gv[it][1], gn = gv[it][2], q = gv[it][3];
                    const float dht = dh + dc_state[it];          // + dh_{s+1} * z_{s+1}
                    dxn = dht * (1.f - gz) * (1.f - gn * gn);
                    dg[1] = dht * (hv[it] - gn) * gz * (1.f - gz);
                    dg[0] = dxn * q * gr_ * (1.f - gr_);
                    dg[2] = dxn * gr_;
                    dc_state[it] = dht * gz;
                } else {
                    const float h = hv[it];
                    dg[0] = CELL == CTCASR_CELL_RNN_RELU ? (h > 0.f ? dh : 0.f)
                                                         : dh * (1.f - h * h);
                }
            }
            // publish dgates: 4 consecutive units per 16-byte sc1 store, one store per gate
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float d1 = __shfl_down(dg[g], 1, 64), d2 = __shfl_down(dg[g], 2, 64),
                            d3 = __shfl_down(dg[g], 3, 64);
                if (it_t[it] >= 0 && (tid & 3) == 0) {
                    const int n = g * H + u0 + u;
                    store16_sc1(x_rsrc,
                                (unsigned)((x_base + (size_t)s * x_step + (size_t)dir * B * GH +
                                            (size_t)(n >> 4) * B * 16 +
                                            (size_t)((n & 15) >> 2) * B * 4 +
                                            (size_t)(row0 + b) * 4) *
                                           sizeof(float)),
                                dg[g], d1, d2, d3);
                }
            }
            if (it_t[it] >= 0) {      // dxw in its GEMM layout: read after the launch only
                float *dx = p.dxw + (((size_t)it_t[it] * BS + row0 + b) * 2 + dir) * GH + u0 + u;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    dx[(size_t)g * H] = GRU && g == 2 ? dxn : dg[g];
                    dbs[it][g] += GRU && g == 2 ? dxn : dg[g];
                    if constexpr (GRU) dbs[it][G + g] += dg[g];
                }
                if constexpr (GRU) {  // drec: dW_hh and db_hh are GEMMs / column sums of it
                    float *dr = p.drec + (((size_t)it_t[it] * BS + row0 + b) * 2 + dir) * GH + u0 + u;
#pragma unroll
                    for (int g = 0; g < G; ++g) dr[(size_t)g * H] = dg[g];
                }
            }
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[2] += c - c0; c0 = c; }
        if (s > p.s_lo) dir_arrive<CHAINS>(p.sync, cs, dir, chain, grp, tid, arrivals);
        if (prof) { unsigned long long c = wall_clock64(); pt[3] += c - c0; c0 = c; }
    }
    if constexpr (CELL == CTCASR_CELL_LSTM || GRU) {
        if (p.s_lo > 0) {
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                const int item = tid + it * PRNN_THREADS;
                if (item < 16 * MT * UPB && row0 + item / UPB < B)
                    p.carry[((size_t)dir * B + row0 + item / UPB) * H + u0 + item % UPB] =
                        dc_state[it];
            }
        }
    }
    if (p.dbias) {
        // sum the items' shares over the rows of the tile(s) through LDS (the reduction scratch
        // is free now), then one atomic per (unit, gate slot): the other batch tile / block of
        // rows / launch of the pass adds to the same word
        if constexpr (CHAINS == 1) __syncthreads();
        else chain_barrier(cs, bar_epoch, lane);
#pragma unroll
        for (int g = 0; g < GS; ++g) {
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                const int item = tid + it * PRNN_THREADS;
                if (item < 16 * MT * UPB) red[item] = dbs[it][g];
            }
            if constexpr (CHAINS == 1) __syncthreads();
            else chain_barrier(cs, bar_epoch, lane);
            if (tid < UPB) {
                float sum = 0.f;
                for (int r = 0; r < 16 * MT; ++r) sum += red[r * UPB + tid];
                atomicAdd(p.dbias + (size_t)(g / G) * 2 * GH + ((size_t)dir * G + g % G) * H + u0 +
                              tid, sum);
            }
            if constexpr (CHAINS == 1) __syncthreads();
            else chain_barrier(cs, bar_epoch, lane);
        }
    }
    if (prof)
        for (int i = 0; i < 4; ++i) p.sync->prof[4 + i] = pt[i];
}

// ---------------------------------------------------------------------------------------------
// backward on the fp16 matrix pipe (round 4; LSTM, H = 1024, `flags` bit CTCASR_RNN_F16).
//
// prnn_bwd_kernel delivers its A operand - the dgates of ALL 4H gate columns, 256 KB per 16-row
// tile and step - at ~50 GB/s per CU: with 128 registers of weights, fp32 fragments and two chains
// per workgroup only 4 - 16 KB per wave are in flight against ~1 us of latency, and 3.4 us of fp32
// MFMA issue per tile hide behind nothing else.  Here:
//   * dgates x R on v_mfma_f32_16x16x32_f16, two fp16 pieces per operand, three products, fp32
//     accumulation - 96 MFMAs of ~16 cycles per wave, tile and step instead of 256 of 32.
//     R is bounded (per workgroup: the slice's largest magnitude, found while staging, like
//     prnn_fwd16_kernel).  dgates are NOT - a step holds 1e-13 .. 1e-3 - but a sum over K only
//     needs a common scale per ROW AND K BLOCK when the blocks are accumulated apart: every
//     producer (16 units x 4 gates = 64 columns) scales each of its 16 rows by the power of two
//     that puts THAT row's largest of its 64 values into [2^13, 2^14), publishes the two fp16
//     pieces in the 4 bytes per element the fp32 exchange carried, plus 16 inverse scales; the
//     consumer multiplies a producer's 64 columns into a fresh accumulator (6 MFMAs) and adds
//     accumulator x inverse scale to its fp32 total.  22 significand bits relative to a
//     (producer, row) maximum that is never above the row's: finer than one scale per row.
//   * ONE chain of 4 waves (512 registers each) for one or two 16-row tiles (MT): the weights'
//     register half is held once, both tiles share every B fragment, and up to 64 KB per wave of
//     A granules are in flight (a ring of D producers x MT tiles x 4 chunks, refilled as it is
//     consumed) - the step is wait + the time the CU's load path needs for the bytes.
// Exchange, in the bytes of prnn_bwd_kernel's: [step][dir][producer P][gate pair m][piece]
// [k group][b][8 halves] - k group q of (P, m) = units 8 (q & 1) .. + 7 of gate 2 m + (q >> 1) -
// so a lane's 16-byte load is the A-fragment register quadruple of a K = 32 MFMA; behind the
// steps' blocks the inverse scales [step][dir][producer][32 rows].  B-fragment slot
// (P * 2 + m) * 2 + piece, the first QL of a wave in LDS.
// Also accumulates, besides the bias gradients, the per-column maxima of |dxw| over the launch's
// steps (`colmax`, bit patterns, atomicMax): what ctcasr_colmax_scale would find in a pass over
// the finished rows of dxw.
// ---------------------------------------------------------------------------------------------
// maximum over the 16 lanes of a DPP row (quad swaps, then the mirrored half and row)
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, __uint_as_float(dpp_u32<0xB1>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(dpp_u32<0x4E>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(dpp_u32<0x141>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(dpp_u32<0x140>(__float_as_uint(v))));
    return v;
}
// The LSTM cell derivative of the fp16-pipe backward kernels, every operation rounded on its own
// (no contraction, whatever the optimiser makes of the code around it - packed math for two items
// in one kernel, scalar math for one item in the other): prnn_bwd16_kernel and prnn_bwd16s_kernel
// then agree bit for bit, which is how the staggered kernel's exchange is tested.
__device__ __forceinline__ float tanh_pinned(float x) {
#pragma clang fp contract(off)
    const float ax = fabsf(x);
    const float e = __expf(-2.0f * ax);
    const float big = (1.0f - e) * __frcp_rn(1.0f + e);
    const float x2 = ax * ax;
    const float small =
        ax * __fmaf_rn(x2, __fmaf_rn(x2, __fmaf_rn(-x2, 0.053968254f, 0.13333334f), -0.33333334f), 1.0f);
    return copysignf(ax < 0.05f ? small : big, x);
}
__device__ __forceinline__ void lstm_cell_bwd_pinned(float dh, float &dc_state, float gi, float gf,
                                                     float gg, float go, float cv, float cpv,
                                                     float (&dg)[4]) {
#pragma clang fp contract(off)
    const float tc = tanh_pinned(cv);
    const float dc = dc_state + ((dh * go) * (1.f - tc * tc));
    dg[0] = ((dc * gg) * gi) * (1.f - gi);
    dg[1] = ((dc * cpv) * gf) * (1.f - gf);
    dg[2] = (dc * gi) * (1.f - gg * gg);
    dg[3] = ((dh * tc) * go) * (1.f - go);
    dc_state = dc * gf;
}
#define PRNN_B16_H 1024
#define PRNN_B16_NWG 64                 // workgroups per direction = consumers = producers
#define PRNN_B16_SCALE_ROWS 32          // rows per producer in the inverse-scale blocks
#ifndef PRNN_B16_D1
#define PRNN_B16_D1 14                  // ring depth, one tile on 4 waves
#endif
#ifndef PRNN_B16_NW2
#define PRNN_B16_NW2 4                  // waves for two tiles behind one barrier (4 or 8)
#endif
#ifndef PRNN_B16_D2
#define PRNN_B16_D2 5                   // ring depth, two tiles
#endif
__host__ __device__ inline size_t prnn_b16_scale_bytes(int T) {
    return (size_t)(T + 1) * 2 * (PRNN_B16_H / 16) * PRNN_B16_SCALE_ROWS * sizeof(float);
}

// MT batch tiles of 16 rows behind one barrier, NW waves (the K axis - 64 producers - is split
// over them), a ring of D producers' A granules in flight per wave.
// Range of the gradients (this kernel, prnn_bwd16s / 16w and prnn_relu16_kernel alike): the
// scale of a (producer, row) is the power of two 2^(13 - exponent of its maximum), clamped to +-100
// binades, 1 for an all-zero row - so a maximum between roughly 2^-100 and 2^100 is published with
// fp32-grade pieces, and dxw(2^k dy) = 2^k dxw(dy) bit for bit while every maximum stays inside.
// Below it the second fp16 piece goes subnormal (precision falls off, nothing breaks); above 2^115
// the first piece overflows to inf.  The maximum is reduced with fmaxf, which skips a NaN: a NaN
// keeps the scale of its finite neighbours, stays NaN in both pieces, and the consumer's MFMA
// spreads it over that batch row only (rows are the M axis; scales, pieces and sums are per row).
// An inf makes the scale 2^-100: its pieces are inf and NaN, the row's other values of that
// producer vanish - the row turns non-finite, no other row is touched.
//   MT = 1, NW = 4: 512 registers per wave, D = 10 (40 KB per wave in flight)
//   MT = 2, NW = 8: two waves per SIMD hide each other's LDS / VALU latencies, nothing is held
//                   twice (a wave's 8 producers: 16 B-fragment slots in LDS, 16 in 64 registers),
//                   one item per thread
template <int MT, int NW, int D>
__global__ void __launch_bounds__(64 * NW) prnn_bwd16_kernel(PArgs p) {
    constexpr int H = PRNN_B16_H, GH = 4 * H;
    constexpr int NTH = 64 * NW;            // threads
    constexpr int NPW = H / 16 / NW;        // producers per wave (the K split)
    constexpr int QS = NPW * 4;             // B-fragment slots per wave: (producer, half, piece)
    constexpr int QL = QS / 2, REGW = QS - QL;
    constexpr int RED_FLOATS = NW * MT * 16 * 17;
    constexpr int ITEMS = (MT * 256 + NTH - 1) / NTH;
    constexpr int DD = D < NPW ? D : NPW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    resident_signal(p.sync, p.ticket);
    if (launch_poisoned(p.sync)) return;
    u32x4 *frag = reinterpret_cast<u32x4 *>(smem);
    float *red = reinterpret_cast<float *>(smem + (size_t)NW * QL * 64 * sizeof(u32x4));
    constexpr int IVL = 4 * NPW;            // float4 slots of a wave's inverse scales per tile
    float4 *invs = reinterpret_cast<float4 *>(red + RED_FLOATS);      // [NW waves][MT][IVL]
    float *wave_top = reinterpret_cast<float *>(invs + NW * MT * IVL);

    const int chain = p.chain0 + (int)blockIdx.x / (p.ndir * p.nwg);
    const int row0 = chain * 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (uniform: scalar offsets)
    const int wg = blockIdx.x % (p.ndir * p.nwg);
    const bool split = p.xcd_split && p.ndir == 2;      // (see prnn_fwd16_kernel)
    const int dir = p.dir0 + (split ? (wg & 7) >> 2 : wg / p.nwg);
    const int slice = split ? (wg >> 3) * 4 + (wg & 3) : wg % p.nwg;
    const int group_size = p.nwg / PRNN_GROUPS, grp = slice / group_size;
    const int B = p.B, T = p.T, BS = p.BS;
    const int u0 = slice * 16;

    // ---- this workgroup's 16 columns of R^T as scaled fp16 pieces, in fragment order -----------
    // K chunk (producer P, half m) = units 8 m .. 8 m + 7 of P, all four gates: lane l of a
    // fragment (k group q = l >> 4) holds element e = 4 (unit & 1) + gate of units 8 m + 2 q,
    // 8 m + 2 q + 1 - the 8 values two neighbouring producer threads have in registers
    float w_scale;
    {
        // largest magnitude of the slice (any order: whole rows of w_hh_t, 16-byte loads)
        float m = 0.f;
        const float *wrow = p.w + ((size_t)dir * H + u0 + (tid & 15)) * GH;
        for (int n = (tid >> 4) * 4; n < GH; n += NTH / 16 * 4) {
            const float4 v = ldg4(wrow + n);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
        m = wave_max(m);
        if (lane == 0) wave_top[wave] = m;
        __syncthreads();
        m = wave_top[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, wave_top[w]);
        const unsigned bits = __float_as_uint(m);
        const int e = (int)((bits >> 23) & 0xFF) - 127;
        const int se = bits == 0u ? 0 : min(max(14 - e, -60), 60);
        w_scale = __uint_as_float((unsigned)(se + 127) << 23);
    }
    const float out_scale = 1.0f / w_scale;
    u32x4 wreg[REGW];
    {
        auto pieces = [&](int pm, u32x4 &first, u32x4 &second) {
            const float *wcol = p.w + ((size_t)dir * H + u0 + (lane & 15)) * GH +
                                16 * (wave * NPW + (pm >> 1)) + 8 * (pm & 1) + 2 * (lane >> 4);
            unsigned q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                q[e] = f16_pieces(wcol[(size_t)(e & 3) * H + (e >> 2)] * w_scale);
            first = (u32x4){(q[0] & 0xFFFFu) | (q[1] << 16), (q[2] & 0xFFFFu) | (q[3] << 16),
                            (q[4] & 0xFFFFu) | (q[5] << 16), (q[6] & 0xFFFFu) | (q[7] << 16)};
            second = (u32x4){(q[0] >> 16) | (q[1] & 0xFFFF0000u), (q[2] >> 16) | (q[3] & 0xFFFF0000u),
                             (q[4] >> 16) | (q[5] & 0xFFFF0000u), (q[6] >> 16) | (q[7] & 0xFFFF0000u)};
        };
        for (int pm = 0; pm < QL / 2; ++pm) {
            u32x4 first, second;
            pieces(pm, first, second);
            frag[(wave * QL + 2 * pm) * 64 + lane] = first;
            frag[(wave * QL + 2 * pm + 1) * 64 + lane] = second;
        }
#pragma unroll
        for (int pm = 0; pm < REGW / 2; ++pm) pieces(QL / 2 + pm, wreg[2 * pm], wreg[2 * pm + 1]);
    }
    __syncthreads();

    // exchange: [step][dir][producer][half][piece][k group][b][16 B] behind an all-zero block;
    // inverse scales [step][dir][producer][32 rows] (zero-filled once: rows nobody writes read 0)
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.xchg, 0, (int)((size_t)(T + 1) * 2 * B * GH * sizeof(float)), 0x00020000);
    const size_t x_step = (size_t)2 * B * GH;
    const size_t x_base = x_step;
    const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.rs, 0, (int)prnn_b16_scale_bytes(T), 0x00020000);
    constexpr unsigned S_STEP = 2u * (H / 16) * PRNN_B16_SCALE_ROWS * sizeof(float);
    // the per-item tensors through buffer descriptors: scalar base + one 32-bit offset per lane
    // (64-bit per-lane pointers cost two registers each and their arithmetic)
    const int rnum = 0x7FFFFFFF;
    const __amdgpu_buffer_rsrc_t dy_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.dy), 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t g_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.gates, 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.cells, 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t dx_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.dxw, 0, rnum, 0x00020000);
    auto ldf = [](__amdgpu_buffer_rsrc_t r, unsigned off) -> float {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
    };

    // ---- items: item = tid + it * NTH -> tile item >> 8, row (item >> 4) & 15, unit item & 15 ---
    const int iu = tid & 15, unit = u0 + iu;
    int steps[ITEMS], brow[ITEMS];
    float dc_state[ITEMS], dbs[ITEMS][4], cmx[ITEMS][4];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int item = tid + it * NTH;
        brow[it] = row0 + (item >> 4);
        const bool has = item < MT * 256 && brow[it] < B;
        steps[it] = has ? row_steps(p.seq_len, brow[it], T) : 0;
        dc_state[it] = 0.f;
        if (p.s_hi < T && has) dc_state[it] = p.carry[((size_t)dir * B + brow[it]) * H + unit];
#pragma unroll
        for (int g = 0; g < 4; ++g) dbs[it][g] = cmx[it][g] = 0.f;
    }
    int a_steps[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int arow = row0 + t * 16 + (lane & 15);
        a_steps[t] = arow < B ? row_steps(p.seq_len, arow, T) : 0;
    }

    unsigned long long pt[4] = {0, 0, 0, 0};
    const bool prof = p.prof && blockIdx.x == 0 && threadIdx.x == 0;
    for (int s = p.s_hi - 1; s >= p.s_lo; --s) {
        unsigned long long c0 = prof ? wall_clock64() : 0;
        // everything the cell derivative needs except dh_rec: requested before the barrier
        float dyv[ITEMS], gi[ITEMS], gf[ITEMS], gg[ITEMS], go[ITEMS], cv[ITEMS], cpv[ITEMS];
        int it_t[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            it_t[it] = -1;
            dyv[it] = gi[it] = gf[it] = gg[it] = go[it] = cv[it] = cpv[it] = 0.f;
            if (s < steps[it]) {
                const int t = row_time(dir, s, steps[it]);
                it_t[it] = t;
                // element index of (t, row, dir, unit) in a [T, BS, 2, H] tensor
                const unsigned e0 = (unsigned)(((t * BS + brow[it]) * 2 + dir) * H + unit);
                dyv[it] = ldf(dy_rsrc, e0 * 4u);
                gi[it] = ldf(g_rsrc, (e0 * 4u - 3u * unit) * 4u);
                gf[it] = ldf(g_rsrc, (e0 * 4u - 3u * unit + H) * 4u);
                gg[it] = ldf(g_rsrc, (e0 * 4u - 3u * unit + 2 * H) * 4u);
                go[it] = ldf(g_rsrc, (e0 * 4u - 3u * unit + 3 * H) * 4u);
                cv[it] = ldf(c_rsrc, e0 * 4u);
                if (s > 0)
                    cpv[it] = ldf(c_rsrc, (unsigned)(((row_time(dir, s - 1, steps[it]) * BS +
                                                       brow[it]) * 2 + dir) * H + unit) * 4u);
            }
        }

        f32x4 total[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) total[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

        if (s < T - 1) {
            if (s < p.s_hi - 1) {
                dir_wait<1>(p.sync, nullptr, dir, chain, group_size, (unsigned)(p.s_hi - 2 - s),
                            tid);
                if (s == p.s_lo && tid == 0) counters_done(p.sync, dir, chain, p.nwg);
            }
            if (prof) { unsigned long long c = wall_clock64(); pt[0] += c - c0; c0 = c; }
            // inverse scales of the wave's producers (1 KB per tile covers 16 of them), lane-linear
            float4 iv[MT];
            unsigned aoff[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                iv[t] = load16_sc1(s_rsrc, (unsigned)(s + 1) * S_STEP +
                                               (unsigned)(((dir * (H / 16) + wave * NPW + (lane >> 2)) *
                                                           PRNN_B16_SCALE_ROWS + row0 + t * 16 +
                                                           4 * (lane & 3)) * sizeof(float)));
                const int row = row0 + t * 16 + (lane & 15);
                const bool ok = s + 1 < a_steps[t];       // otherwise: the all-zero block
                aoff[t] = (unsigned)(((ok ? x_base + (size_t)(s + 1) * x_step : 0) +
                                      (size_t)dir * B * GH + (size_t)(lane >> 4) * B * 4 +
                                      (size_t)(ok ? row : 0) * 4) * sizeof(float));
            }
            u32x4 a[DD][MT][4];
            auto issue = [&](int P, u32x4 (&dst)[MT][4]) {
#pragma unroll
                for (int t = 0; t < MT; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g)       // g = half * 2 + piece
                        dst[t][g] = load16u(x_rsrc, aoff[t],
                                            (unsigned)(((wave * NPW + P) * 4 + g) * B * 16 *
                                                       sizeof(float)));
            };
#pragma unroll
            for (int P = 0; P < DD; ++P) issue(P, a[P]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < MT; ++t)
                if (lane < IVL) invs[(wave * MT + t) * IVL + lane] = iv[t];
            auto bfrag = [&](int sl) -> u32x4 {      // compile-time slot after unrolling
                return sl < QL ? frag[(wave * QL + sl) * 64 + lane] : wreg[sl - QL];
            };
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int P = 0; P < NPW; ++P) {
                u32x4 (&ap)[MT][4] = a[P % DD];
                // the six products of a producer's 64 columns: ONE fresh accumulator per tile when
                // two tiles alternate on the matrix pipe (a dependent MFMA is two issues away),
                // two - first-piece products / the two small terms - for a single tile
                constexpr int NA = MT == 1 ? 2 : 1;
                f32x4 acc[MT][NA];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    Frag16 w1, w2;
                    w1.u = bfrag((P * 2 + m) * 2);
                    w2.u = bfrag((P * 2 + m) * 2 + 1);
                    Frag16 d1[MT], d2[MT];
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        d1[t].u = ap[t][2 * m];
                        d2[t].u = ap[t][2 * m + 1];
                    }
#pragma unroll
                    for (int t = 0; t < MT; ++t)
                        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            d1[t].h, w1.h, m == 0 ? zero : acc[t][0], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < MT; ++t)
                        acc[t][NA - 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            d1[t].h, w2.h, (m == 0 && NA == 2) ? zero : acc[t][NA - 1], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < MT; ++t)
                        acc[t][NA - 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            d2[t].h, w1.h, acc[t][NA - 1], 0, 0, 0);
                }
                if (P + DD < NPW) issue(P + DD, a[P % DD]);
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const float4 ivp = invs[(wave * MT + t) * IVL + 4 * P + (lane >> 4)];
                    f32x4 sum = acc[t][0];
                    if constexpr (NA == 2) sum += acc[t][1];
                    total[t][0] += sum[0] * ivp.x;
                    total[t][1] += sum[1] * ivp.y;
                    total[t][2] += sum[2] * ivp.z;
                    total[t][3] += sum[3] * ivp.w;
                }
                // (one producer at a time: left alone the scheduler hoists the LDS reads of many
                // producers above the MFMAs of the first and runs out of registers)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (prof) {
            asm volatile("" ::"v"(total[0][0]));
            unsigned long long c = wall_clock64(); pt[1] += c - c0; c0 = c;
        }
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                red[((wave * MT + t) * 16 + 4 * (lane >> 4) + r) * 17 + (lane & 15)] =
                    total[t][r] * out_scale;
        __syncthreads();

#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int item = tid + it * NTH;
            const int tile = item >> 8, ib = (item >> 4) & 15;
            float dg[4] = {0.f, 0.f, 0.f, 0.f};
            if (it_t[it] >= 0) {
                float dh = dyv[it];
#pragma unroll
                for (int w = 0; w < NW; ++w) dh += red[((w * MT + tile) * 16 + ib) * 17 + iu];
                lstm_cell_bwd_pinned(dh, dc_state[it], gi[it], gf[it], gg[it], go[it], cv[it],
                                     cpv[it], dg);
            }
            if (ITEMS * NTH > MT * 256 && item >= MT * 256) continue;     // (wave-uniform)
            // the row's scale over this workgroup's 64 values; two fp16 pieces of every value
            float mx = fmaxf(fmaxf(fabsf(dg[0]), fabsf(dg[1])), fmaxf(fabsf(dg[2]), fabsf(dg[3])));
            mx = row16_max(mx);
            const unsigned mbits = __float_as_uint(mx);
            const int me = (int)((mbits >> 23) & 0xFF) - 127;
            const int mse = mbits == 0u ? 0 : min(max(13 - me, -100), 100);
            const float rscale = __uint_as_float((unsigned)(mse + 127) << 23);
            const float rinv = __uint_as_float((unsigned)(127 - mse) << 23);
            // this thread's 4 gates and its neighbour unit's: one granule of first pieces (stored
            // by the even lane), one of second pieces (by the odd lane)
            unsigned q[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) q[g] = f16_pieces(dg[g] * rscale);
            // mine: the piece this lane stores (even: first, odd: second) of my own 4 gates;
            // theirs: the piece the NEIGHBOUR stores, handed over by a lane swap
            const bool odd = (tid & 1) != 0;
            const unsigned f01 = (q[0] & 0xFFFFu) | (q[1] << 16), f23 = (q[2] & 0xFFFFu) | (q[3] << 16);
            const unsigned s01 = (q[0] >> 16) | (q[1] & 0xFFFF0000u),
                           s23 = (q[2] >> 16) | (q[3] & 0xFFFF0000u);
            const unsigned give01 = odd ? f01 : s01, give23 = odd ? f23 : s23;
            const unsigned got01 = dpp_u32<0xB1>(give01), got23 = dpp_u32<0xB1>(give23);   // lane ^ 1
            // element order of a granule: e = 4 (unit & 1) + gate
            const u32x4 v = odd ? (u32x4){got01, got23, s01, s23} : (u32x4){f01, f23, got01, got23};
            if (it_t[it] >= 0) {
                // block (producer, half = unit >> 3, piece), k group (unit >> 1) & 3
                const unsigned off = (unsigned)(
                    (x_base + (size_t)s * x_step + (size_t)dir * B * GH +
                     (size_t)((slice * 2 + (iu >> 3)) * 2 + (odd ? 1 : 0)) * B * 16 +
                     (size_t)((iu >> 1) & 3) * B * 4 + (size_t)brow[it] * 4) * sizeof(float));
                __builtin_amdgcn_raw_buffer_store_b128(v, x_rsrc, (int)off, 0, 16);
            }
            // the four rows of this wave: one 16-byte store of their inverse scales
            const float r0 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 0));
            const float r1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 16));
            const float r2 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 32));
            const float r3 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 48));
            if (lane == 0)
                store16_sc1(s_rsrc,
                            (unsigned)s * S_STEP +
                                (unsigned)(((dir * (H / 16) + slice) * PRNN_B16_SCALE_ROWS + row0 +
                                            (item >> 4)) * sizeof(float)),
                            r0, r1, r2, r3);
            if (it_t[it] >= 0) {      // dxw in its GEMM layout: read after the launch only
                const unsigned dx0 = (unsigned)(((it_t[it] * BS + brow[it]) * 2 + dir) * GH + unit) * 4u;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg[g]), dx_rsrc,
                                                          (int)(dx0 + (unsigned)g * H * 4u), 0, 0);
                    dbs[it][g] += dg[g];
                    cmx[it][g] = fmaxf(cmx[it][g], fabsf(dg[g]));
                }
            }
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[2] += c - c0; c0 = c; }
        if (s > p.s_lo) {
            unsigned unused = 0;
            dir_arrive<1>(p.sync, nullptr, dir, chain, grp, tid, unused);
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[3] += c - c0; c0 = c; }
    }
    if (p.s_lo > 0) {
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int item = tid + it * NTH;
            if (item < MT * 256 && brow[it] < B)
                p.carry[((size_t)dir * B + brow[it]) * H + unit] = dc_state[it];
        }
    }
    if (p.dbias || p.colmax) {
        // sums / maxima over the rows of the tile(s) through LDS, then one atomic per column: the
        // other batch tile / block of rows / launch of the pass meets it at the same word
        float *sums = red, *tops = reinterpret_cast<float *>(frag);     // (the weights are done with)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            __syncthreads();
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                const int item = tid + it * NTH;
                if (item < MT * 256) {
                    sums[item] = dbs[it][g];
                    tops[item] = cmx[it][g];
                }
            }
            __syncthreads();
            if (tid < 16) {
                float sum = 0.f, top = 0.f;
                for (int r = 0; r < 16 * MT; ++r) {
                    sum += sums[r * 16 + tid];
                    top = fmaxf(top, tops[r * 16 + tid]);
                }
                if (p.dbias) atomicAdd(p.dbias + ((size_t)dir * 4 + g) * H + u0 + tid, sum);
                if (p.colmax)
                    atomicMax(p.colmax + ((size_t)dir * 4 + g) * H + u0 + tid, __float_as_uint(top));
            }
        }
    }
    if (prof)
        for (int i = 0; i < 4; ++i) p.sync->prof[4 + i] = pt[i];
}

// ---------------------------------------------------------------------------------------------
// prnn_bwd16s_kernel (round 5): the same recurrence for batches of 17..32 rows on half of the
// chip with the two 16-row tiles STAGGERED by half a step instead of behind one barrier.
//
// prnn_bwd16_kernel<2, 4, 5> pays per step: barrier round trip (1.2 us), first byte of freshly
// published cross-XCD data (~1.5 us), 512 KB through the CU's load path, gate math + publish (1.0),
// store drain (0.5) - one after the other, 8.3 us.  The tiles are independent recurrences, so one
// tile's exchange round trip (publish -> drain -> arrive -> everybody's arrival visible -> first
// byte) can run under the other tile's 256 KB of loads.  One instruction stream per wave (4 waves,
// 512 registers: the weights' register half is held once), software-pipelined by hand:
//
//   phase (s, X):  main loop over the wave's 16 producers of tile X (their A granules were
//                  requested during the phase before), pairs of producers alternate on the matrix
//                  pipe; as ring slots come free they are refilled with tile X's remaining
//                  producers, then - from pair JW on - with the FIRST producers of the next phase
//                  (tile X ^ 1: the same step for X = 0, the next step for X = 1);
//                  reduce + cell derivative + publish of (s, X) while those loads are in flight.
//                  (Measured: JW = the last pair - all of the next phase's first half requested at
//                  once, just before the publish part - beats every earlier point: a poll that is
//                  looked at before the arrivals are visible stalls the whole stream.)
//   arrival of (s, X): vmcnt counts loads and stores in ONE in-order queue on gfx950, so the
//                  publish stores cannot be waited for alone - a 4-byte marker load is issued right
//                  behind them and the arrival is posted where the next phase's main loop first
//                  waits for that marker (pair JA): by then the stores in front of it are complete,
//                  and nothing younger had to drain.  Every wave counts itself in on an LDS word,
//                  the fourth posts the workgroup's arrival (no workgroup barrier).
//   wait for (s', X'): every wave polls for itself, asynchronously - the counter loads are issued
//                  at pair JP and looked at at pair JW; only a wave that finds them short spins.
//
// Each tile has its own arrival counters (SyncWords.group_cnt[dir][tile]).  Arithmetic, exchange
// layout, scales, column maxima: prnn_bwd16_kernel's, and the per-tile order of every sum is that of
// <2, 4, 5> - results are bit-identical to it (tests/test_gpu_kernels.py).
// ---------------------------------------------------------------------------------------------
#ifndef PRNN_B16S_D
#define PRNN_B16S_D 8                   // ring slots = producers of a tile in flight per wave
#endif
#ifndef PRNN_B16S_JW
#define PRNN_B16S_JW 7                  // pair at which the next phase's loads may start (>= (16 - D) / 2)
#endif
#ifndef PRNN_B16S_JP
#define PRNN_B16S_JP 5                  // pair at which the poll loads for them are issued
#endif
#ifndef PRNN_B16S_XCD_EXCL
#define PRNN_B16S_XCD_EXCL 0            // probe: the launch on XCDs 0 - 3 only (see the kernel)
#endif
#ifndef PRNN_B16S_JA
#define PRNN_B16S_JA 1                  // pair at which the phase before posts its arrival
#endif
template <int DD, int JW, int JP, int JA, bool PROF = false>
__global__ void __launch_bounds__(PRNN_THREADS) prnn_bwd16s_kernel(PArgs p) {
    constexpr int H = PRNN_B16_H, GH = 4 * H;
    constexpr int NW = 4, NTH = 256, NPW = 16, QS = NPW * 4, QL = QS / 2, REGW = QS - QL;
    constexpr int RED_FLOATS = NW * 16 * 17, IVL = 4 * NPW;
    static_assert(DD % 2 == 0 && DD <= NPW && (NPW % DD == 0 || JW == NPW / 2 - 1),
                  "ring slots: even; not a divisor of 16 only when the next phase is requested at the end");
    static_assert(2 * JW >= NPW - DD && JW < NPW / 2 && JP <= JW && JA <= JP, "pipeline points");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    resident_signal(p.sync, p.ticket);
    if (launch_poisoned(p.sync)) return;
    u32x4 *frag = reinterpret_cast<u32x4 *>(smem);
    float *red = reinterpret_cast<float *>(smem + (size_t)NW * QL * 64 * sizeof(u32x4));   // [2 tiles]
    float4 *invs = reinterpret_cast<float4 *>(red + 2 * RED_FLOATS);       // [2 tiles][NW][IVL]
    float *wave_top = reinterpret_cast<float *>(invs + 2 * NW * IVL);
    unsigned *arrived = reinterpret_cast<unsigned *>(wave_top + 4);        // [2 tiles]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#if PRNN_B16S_XCD_EXCL
    // PROBE (timing of a placement): the launch has twice the workgroups; those that land on XCDs
    // 4 - 7 leave at once, the others fill XCDs 0 - 3 - direction 0 on XCDs 0, 1, direction 1 on 2, 3
    if (((int)blockIdx.x & 7) >= 4) return;
    const int dir = p.dir0 + (((int)blockIdx.x & 7) >> 1);
    const int slice = ((int)blockIdx.x >> 3) * 2 + ((int)blockIdx.x & 1);
#else
    const int wg = blockIdx.x % (p.ndir * p.nwg);
    const bool split = p.xcd_split && p.ndir == 2;
    const int dir = p.dir0 + (split ? (wg & 7) >> 2 : wg / p.nwg);
    const int slice = split ? (wg >> 3) * 4 + (wg & 3) : wg % p.nwg;
#endif
    const int group_size = p.nwg / PRNN_GROUPS, grp = slice / group_size;
    const int B = p.B, T = p.T, BS = p.BS;
    const int u0 = slice * 16;
    if (tid < 2) arrived[tid] = 0u;

    // ---- this workgroup's 16 columns of R^T as scaled fp16 pieces (prnn_bwd16_kernel's layout) --
    float w_scale;
    {
        float m = 0.f;
        const float *wrow = p.w + ((size_t)dir * H + u0 + (tid & 15)) * GH;
        for (int n = (tid >> 4) * 4; n < GH; n += NTH / 16 * 4) {
            const float4 v = ldg4(wrow + n);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
        m = wave_max(m);
        if (lane == 0) wave_top[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wave_top[0], wave_top[1]), fmaxf(wave_top[2], wave_top[3]));
        const unsigned bits = __float_as_uint(m);
        const int e = (int)((bits >> 23) & 0xFF) - 127;
        const int se = bits == 0u ? 0 : min(max(14 - e, -60), 60);
        w_scale = __uint_as_float((unsigned)(se + 127) << 23);
    }
    const float out_scale = 1.0f / w_scale;
    u32x4 wreg[REGW];
    {
        auto pieces = [&](int pm, u32x4 &first, u32x4 &second) {
            const float *wcol = p.w + ((size_t)dir * H + u0 + (lane & 15)) * GH +
                                16 * (wave * NPW + (pm >> 1)) + 8 * (pm & 1) + 2 * (lane >> 4);
            unsigned q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                q[e] = f16_pieces(wcol[(size_t)(e & 3) * H + (e >> 2)] * w_scale);
            first = (u32x4){(q[0] & 0xFFFFu) | (q[1] << 16), (q[2] & 0xFFFFu) | (q[3] << 16),
                            (q[4] & 0xFFFFu) | (q[5] << 16), (q[6] & 0xFFFFu) | (q[7] << 16)};
            second = (u32x4){(q[0] >> 16) | (q[1] & 0xFFFF0000u), (q[2] >> 16) | (q[3] & 0xFFFF0000u),
                             (q[4] >> 16) | (q[5] & 0xFFFF0000u), (q[6] >> 16) | (q[7] & 0xFFFF0000u)};
        };
        for (int pm = 0; pm < QL / 2; ++pm) {
            u32x4 first, second;
            pieces(pm, first, second);
            frag[(wave * QL + 2 * pm) * 64 + lane] = first;
            frag[(wave * QL + 2 * pm + 1) * 64 + lane] = second;
        }
#pragma unroll
        for (int pm = 0; pm < REGW / 2; ++pm) pieces(QL / 2 + pm, wreg[2 * pm], wreg[2 * pm + 1]);
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.xchg, 0, (int)((size_t)(T + 1) * 2 * B * GH * sizeof(float)), 0x00020000);
    const size_t x_step = (size_t)2 * B * GH;
    const size_t x_base = x_step;
    const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.rs, 0, (int)prnn_b16_scale_bytes(T), 0x00020000);
    constexpr unsigned S_STEP = 2u * (H / 16) * PRNN_B16_SCALE_ROWS * sizeof(float);
    const int rnum = 0x7FFFFFFF;
    const __amdgpu_buffer_rsrc_t dy_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.dy), 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t g_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.gates, 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.cells, 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t dx_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.dxw, 0, rnum, 0x00020000);
    auto ldf = [](__amdgpu_buffer_rsrc_t r, unsigned off) -> float {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
    };

    // ---- one item per thread and tile: row x * 16 + (tid >> 4), unit tid & 15.  No per-row lengths
    // (cuDNN semantics: the caller takes prnn_bwd16_kernel for those), so the time of step s is
    // wave-uniform and every per-item address is a scalar part + a per-lane constant ---------------
    const int iu = tid & 15, unit = u0 + iu;
    float dc_state[2], dbs[2][4], cmx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int brow = x * 16 + (tid >> 4);
        dc_state[x] = 0.f;
        if (p.s_hi < T && brow < B) dc_state[x] = p.carry[((size_t)dir * B + brow) * H + unit];
#pragma unroll
        for (int g = 0; g < 4; ++g) dbs[x][g] = 0.f;
    }
    // element index of (row, dir, unit) in a [BS, 2, H] slab; the [T] part goes into the scalar offset
    auto item_elem = [&](int x) -> unsigned {
        return (unsigned)(((x * 16 + (tid >> 4)) * 2 + dir) * H + unit);
    };
    auto ldf2 = [](__amdgpu_buffer_rsrc_t r, unsigned lane_off, unsigned uni_off) -> float {
        return __uint_as_float(
            __builtin_amdgcn_raw_buffer_load_b32(r, (int)lane_off, (int)uni_off, 0));
    };

    // what the cell derivative of (step, tile) needs besides dh_rec, requested half a phase ahead
    // (behind the first loads of the tile's A operand).  Unconditional - rows past the batch read
    // the batch's last row - so that the vector-memory queue has no data-dependent entries and
    // every wait below is a counted one.
    float c_dy[2], c_gi[2], c_gf[2], c_gg[2], c_go[2], c_cv[2], c_cp[2];
    auto cell_prefetch = [&](int s, int x) {
        int tq = tid;
        asm volatile("" : "+v"(tq));
        s = max(s, 0);                    // (behind the launch's last phase: any valid address)
        const unsigned t = (unsigned)(dir == 0 ? s : T - 1 - s);
        const unsigned tp = s > 0 ? (unsigned)(dir == 0 ? s - 1 : T - s) : t;
        const unsigned unit = (unsigned)(u0 + (tq & 15));
        const unsigned e = (unsigned)((min(x * 16 + (tq >> 4), B - 1) * 2 + dir) * H) + unit;
        const unsigned slab = t * (unsigned)BS * 2u * H * 4u;               // bytes of [BS, 2, H] rows
        c_dy[x] = ldf2(dy_rsrc, e * 4u, slab);
        const unsigned ge = (e * 4u - 3u * unit) * 4u;
        c_gi[x] = ldf2(g_rsrc, ge, slab * 4u);
        c_gf[x] = ldf2(g_rsrc, ge + H * 4u, slab * 4u);
        c_gg[x] = ldf2(g_rsrc, ge + 2 * H * 4u, slab * 4u);
        c_go[x] = ldf2(g_rsrc, ge + 3 * H * 4u, slab * 4u);
        c_cv[x] = ldf2(c_rsrc, e * 4u, slab);
        c_cp[x] = ldf2(c_rsrc, e * 4u, tp * (unsigned)BS * 2u * H * 4u);
        if (s == 0) c_cp[x] = 0.f;        // (no cell state before the first step)
    };

    // A operand of (step s, tile x): block of step s + 1 (the all-zero block for s = T - 1, where
    // nothing has been published) - a scalar; rows past the batch read the batch's last row (their
    // results are never used); inverse scales
    unsigned ablock[2];                   // scalar: byte offset of (step, dir) in the exchange buffer
    float4 iv_next;
    auto lane_aoff = [&](int x) -> unsigned {
        const int row = min(x * 16 + (lane & 15), B - 1);
        return (unsigned)(((size_t)(lane >> 4) * B * 4 + (size_t)row * 4) * sizeof(float));
    };
    auto tile_addresses = [&](int s, int x) {
        ablock[x] = (unsigned)(((s + 1 < T ? x_base + (size_t)(s + 1) * x_step : 0) +
                                (size_t)dir * B * GH) * sizeof(float));
        // (L1 / L2 bypassed: a producer's 32 inverse scales - BOTH tiles' - share one 128-byte line,
        // and the other tile's half is written after this tile's half has been read: see the
        // dispatch in prnn_bwd)
        iv_next = load16_sc1<16>(s_rsrc, (unsigned)(s + 1) * S_STEP +
                                         (unsigned)(((dir * (H / 16) + wave * NPW + (lane >> 2)) *
                                                     PRNN_B16_SCALE_ROWS + x * 16 + 4 * (lane & 3)) *
                                                    sizeof(float)));
    };
    u32x4 a[DD][4];                       // ring: producer P of the tile in flight sits in slot P % DD
    // (the 64 wave-uniform offsets are products with the runtime batch: made opaque per use, or
    // the optimiser hoists them all and spills scalar registers - see prnn_bwd16w_kernel)
    const unsigned wave_off = (unsigned)(wave * NPW * 4) * (unsigned)B * 64u;
    auto issue = [&](int x, int P) {
        unsigned bstride = (unsigned)B * 64u;
        asm volatile("" : "+s"(bstride));
        const unsigned lo = lane_aoff(x);
#pragma unroll
        for (int g = 0; g < 4; ++g)       // g = half * 2 + piece
            a[P % DD][g] = load16u(x_rsrc, lo, ablock[x] + wave_off + (unsigned)(P * 4 + g) * bstride);
    };
    auto poll = [&](int x) -> unsigned {  // lanes 0 .. 7: the arrival counter of group `lane`
        unsigned v = 0xFFFFFFFFu;
        if (lane < PRNN_GROUPS)
            v = __hip_atomic_load(&p.sync->group_cnt[dir][x][lane][0], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
        return v;
    };
    auto bfrag = [&](int sl) -> u32x4 {   // compile-time slot after unrolling
        return sl < QL ? frag[(wave * QL + sl) * 64 + lane] : wreg[sl - QL];
    };

    // phase timers (CTCASR_RNN_PROF: a second instantiation - the timed stream needs registers the
    // plain one does not have to spare): wave 0 of workgroup 0, wave-uniform -> scalar registers.
    // [0] waiting for the marker (publish stores of the phase before), [1] waiting for the polled
    // counters (+ spinning), [2] the rest of the main loops, [3] reduce + cell derivative + publish
    unsigned long long pt[4] = {0, 0, 0, 0}, spins_total = 0;
    const bool profw = PROF && p.prof && blockIdx.x == 0 && wave == 0;
    unsigned marker = 0u;                 // the load behind a phase's publish stores

    // one phase: `xc` = tile (compile-time), s = its step.  prev_arrives: the phase before
    // published something that others wait for; has_next / next_waits: see above
    auto phase = [&](auto xc, int s, bool prev_arrives, bool has_next, bool next_waits) {
        constexpr int X = decltype(xc)::value, XN = X ^ 1;
        const int sn = X == 0 ? s : s - 1;                  // the next phase's step
        f32x4 total = {0.f, 0.f, 0.f, 0.f};
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        unsigned pv = 0xFFFFFFFFu;
        unsigned long long c0 = 0, waited = 0;
        if constexpr (PROF) c0 = profw ? wall_clock64() : 0;
#pragma unroll
        for (int j = 0; j < NPW / 2; ++j) {
            if (j == JA && prev_arrives) {
                // the marker is back -> the publish stores issued in front of it are complete
                unsigned long long w0 = 0;
                if constexpr (PROF) w0 = profw ? wall_clock64() : 0;
                asm volatile("" ::"v"(marker) : "memory");
                if constexpr (PROF) {
                    if (profw) { const unsigned long long d = wall_clock64() - w0; pt[0] += d; waited += d; }
                }
                if (lane == 0) {
                    const unsigned before = __hip_atomic_fetch_add(
                        &arrived[XN], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if ((before & 3u) == 3u)
                        __hip_atomic_fetch_add(&p.sync->group_cnt[dir][XN][grp][0], 1u,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (j == JP && has_next && next_waits) pv = poll(XN);
            const int P0 = 2 * j, P1 = 2 * j + 1;
            f32x4 acc0, acc1;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                Frag16 w10, w20, w11, w21, d10, d20, d11, d21;
                w10.u = bfrag((P0 * 2 + m) * 2);
                w20.u = bfrag((P0 * 2 + m) * 2 + 1);
                w11.u = bfrag((P1 * 2 + m) * 2);
                w21.u = bfrag((P1 * 2 + m) * 2 + 1);
                d10.u = a[P0 % DD][2 * m];
                d20.u = a[P0 % DD][2 * m + 1];
                d11.u = a[P1 % DD][2 * m];
                d21.u = a[P1 % DD][2 * m + 1];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d10.h, w10.h, m == 0 ? zero : acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d11.h, w11.h, m == 0 ? zero : acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d10.h, w20.h, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d11.h, w21.h, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d20.h, w10.h, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d21.h, w11.h, acc1, 0, 0, 0);
            }
            // refill the two slots: the tile's own remaining producers ...
            if (P0 + DD < NPW) issue(X, P0 + DD);
            if (P1 + DD < NPW) issue(X, P1 + DD);
            // ... then the next phase's first ones, as soon as everybody has published them
            // (unconditional - after the launch's last phase they read blocks nobody needs: the
            // instruction stream stays straight-line)
            if (j >= JW) {
                if (j == JW) {
                    // the counters polled at pair JP: looked at in straight-line code (a counted
                    // vmcnt - the ring stays in flight); only a wave that finds them short spins
                    const unsigned target = (unsigned)group_size * (unsigned)(p.s_hi - 1 - sn);
                    unsigned long long w1 = 0;
                    if constexpr (PROF) {
                        w1 = profw ? wall_clock64() : 0;
                        asm volatile("" ::"v"(pv) : "memory");
                        if (profw) { const unsigned long long d = wall_clock64() - w1; pt[1] += d; waited += d; }
                        w1 = profw ? wall_clock64() : 0;
                    }
                    if (__builtin_expect(has_next && next_waits && !__all(pv >= target), 0)) {
                        unsigned spins = 0;
                        for (;;) {
                            __builtin_amdgcn_s_sleep(PRNN_POLL_SLEEP);
                            const unsigned again = poll(XN);
                            if constexpr (PROF) spins_total += 1;
                            if (__all(again >= target)) break;
                            if (++spins > PRNN_SPIN_LIMIT ||
                                ((spins & 1023u) == 0 &&
                                 __hip_atomic_load(&p.sync->error, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT))) {
                                if (lane == 0)
                                    __hip_atomic_store(&p.sync->error, 1u, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
                                break;
                            }
                        }
                        if constexpr (PROF) {
                            if (profw) { const unsigned long long d = wall_clock64() - w1; pt[1] += d; waited += d; }
                        }
                    }
                    tile_addresses(sn, XN);
#pragma unroll
                    for (int q = 0; q <= P1 + DD - NPW; ++q) issue(XN, q);
                    cell_prefetch(sn, XN);
                } else {
                    issue(XN, P0 + DD - NPW);
                    issue(XN, P1 + DD - NPW);
                }
            }
            {
                const float4 iv0 = invs[(X * NW + wave) * IVL + 4 * P0 + (lane >> 4)];
                const float4 iv1 = invs[(X * NW + wave) * IVL + 4 * P1 + (lane >> 4)];
                total[0] += acc0[0] * iv0.x;
                total[1] += acc0[1] * iv0.y;
                total[2] += acc0[2] * iv0.z;
                total[3] += acc0[3] * iv0.w;
                total[0] += acc1[0] * iv1.x;
                total[1] += acc1[1] * iv1.y;
                total[2] += acc1[2] * iv1.z;
                total[3] += acc1[3] * iv1.w;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- reduce over the waves' K shares, cell derivative, publish ---------------------------
        if constexpr (PROF) {
            asm volatile("" ::"v"(total[0]));
            if (profw) { const unsigned long long c = wall_clock64(); pt[2] += c - c0 - waited; c0 = c; }
        }
        // (per-lane address constants of this part are recomputed from an opaque copy of the thread
        // index every phase: hoisted out of the step loop they are spilled, and a scratch reload is
        // a vector-memory load - waiting for it drains the ring)
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int lq = tq & 63, iu = tq & 15, unit = u0 + iu;
        float *redx = red + X * RED_FLOATS;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            redx[(wave * 16 + 4 * (lq >> 4) + r) * 17 + (lq & 15)] = total[r] * out_scale;
        __syncthreads();
        {
            const int ib = tq >> 4;
            const bool has = X * 16 + ib < B;
            float dg[4] = {0.f, 0.f, 0.f, 0.f};
            if (has) {
                float dh = c_dy[X];
#pragma unroll
                for (int w = 0; w < NW; ++w) dh += redx[(w * 16 + ib) * 17 + iu];
                lstm_cell_bwd_pinned(dh, dc_state[X], c_gi[X], c_gf[X], c_gg[X], c_go[X], c_cv[X],
                                     c_cp[X], dg);
            }
            float mx = fmaxf(fmaxf(fabsf(dg[0]), fabsf(dg[1])), fmaxf(fabsf(dg[2]), fabsf(dg[3])));
            mx = row16_max(mx);
            const unsigned mbits = __float_as_uint(mx);
            const int me = (int)((mbits >> 23) & 0xFF) - 127;
            const int mse = mbits == 0u ? 0 : min(max(13 - me, -100), 100);
            const float rscale = __uint_as_float((unsigned)(mse + 127) << 23);
            const float rinv = __uint_as_float((unsigned)(127 - mse) << 23);
            unsigned q[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) q[g] = f16_pieces(dg[g] * rscale);
            const bool odd = (tq & 1) != 0;
            const unsigned f01 = (q[0] & 0xFFFFu) | (q[1] << 16), f23 = (q[2] & 0xFFFFu) | (q[3] << 16);
            const unsigned s01 = (q[0] >> 16) | (q[1] & 0xFFFF0000u),
                           s23 = (q[2] >> 16) | (q[3] & 0xFFFF0000u);
            const unsigned give01 = odd ? f01 : s01, give23 = odd ? f23 : s23;
            const unsigned got01 = dpp_u32<0xB1>(give01), got23 = dpp_u32<0xB1>(give23);
            const u32x4 v = odd ? (u32x4){got01, got23, s01, s23} : (u32x4){f01, f23, got01, got23};
            if (has) {
                // block (producer, half = unit >> 3, piece), k group (unit >> 1) & 3
                const unsigned lo = (unsigned)(
                    ((size_t)((slice * 2 + (iu >> 3)) * 2 + (odd ? 1 : 0)) * B * 16 +
                     (size_t)((iu >> 1) & 3) * B * 4 + (size_t)(X * 16 + ib) * 4) * sizeof(float));
                const unsigned uo = (unsigned)((x_base + (size_t)s * x_step + (size_t)dir * B * GH) *
                                               sizeof(float));
                __builtin_amdgcn_raw_buffer_store_b128(v, x_rsrc, (int)lo, (int)uo, 16);
            }
            const float r0 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 0));
            const float r1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 16));
            const float r2 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 32));
            const float r3 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 48));
            if (lq == 0)
                store16_sc1(s_rsrc,
                            (unsigned)s * S_STEP +
                                (unsigned)(((dir * (H / 16) + slice) * PRNN_B16_SCALE_ROWS + X * 16 +
                                            ib) * sizeof(float)),
                            r0, r1, r2, r3);
            if (has) {      // dxw in its GEMM layout: read after the launch only
                const unsigned t = (unsigned)(dir == 0 ? s : T - 1 - s);
                const unsigned lo = (unsigned)(((X * 16 + ib) * 2 + dir) * GH + unit) * 4u;
                const unsigned uo = t * (unsigned)BS * 2u * GH * 4u;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg[g]), dx_rsrc,
                                                          (int)(lo + (unsigned)g * H * 4u), (int)uo, 0);
                    dbs[X][g] += dg[g];
                    cmx[g] = fmaxf(cmx[g], fabsf(dg[g]));
                }
            }
        }
        // the marker behind the stores (any address that is always valid: the all-zero block)
        asm volatile("" ::: "memory");
        marker = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(x_rsrc, 0, 0, 0);
        // the next phase's inverse scales -> this wave's LDS rows (requested at pair JW)
        invs[(XN * NW + wave) * IVL + lane] = iv_next;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (PROF) {
            if (profw) pt[3] += wall_clock64() - c0;
        }
    };

    // ---- prologue: the first phase's operands (no wait: what it reads was published by the launch
    // before, or it is the all-zero block) ---------------------------------------------------------
    {
        const int s = p.s_hi - 1;
        tile_addresses(s, 0);
#pragma unroll
        for (int q = 0; q < DD; ++q) issue(0, q);
        cell_prefetch(s, 0);
        invs[(0 * NW + wave) * IVL + lane] = iv_next;
    }
    for (int s = p.s_hi - 1; s >= p.s_lo; --s) {
        // (s, 0): the phase before, (s + 1, 1), arrives if it exists; next = (s, 1), which waits
        // for arrivals unless this is the launch's first step
        phase(std::integral_constant<int, 0>{}, s, s < p.s_hi - 1, true, s < p.s_hi - 1);
        // (s, 1): the phase before, (s, 0), arrives unless this is the launch's last step;
        // next = (s - 1, 0)
        phase(std::integral_constant<int, 1>{}, s, s > p.s_lo, s > p.s_lo, true);
    }
    __syncthreads();        // every wave is through its last poll
    if (tid == 0 && p.s_hi - p.s_lo >= 2) {
        counters_done(p.sync, dir, 0, p.nwg);
        counters_done(p.sync, dir, 1, p.nwg);
    }
    if constexpr (PROF) {
        if (profw && lane == 0) {
            for (int i = 0; i < 4; ++i) p.sync->prof[4 + i] = pt[i];
            p.sync->prof[8] = spins_total;
        }
    }
    if (p.s_lo > 0) {
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const int brow = x * 16 + (tid >> 4);
            if (brow < B) p.carry[((size_t)dir * B + brow) * H + unit] = dc_state[x];
        }
    }
    if (p.dbias || p.colmax) {
        float *sums = red, *tops = reinterpret_cast<float *>(frag);     // (the weights are done with)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            __syncthreads();
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                sums[tid + x * NTH] = dbs[x][g];
                tops[tid + x * NTH] = cmx[g];
            }
            __syncthreads();
            if (tid < 16) {
                float sum = 0.f, top = 0.f;
                for (int r = 0; r < 32; ++r) {
                    sum += sums[r * 16 + tid];
                    top = fmaxf(top, tops[r * 16 + tid]);
                }
                if (p.dbias) atomicAdd(p.dbias + ((size_t)dir * 4 + g) * H + u0 + tid, sum);
                if (p.colmax)
                    atomicMax(p.colmax + ((size_t)dir * 4 + g) * H + u0 + tid, __float_as_uint(top));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same backward recurrence on the fp16 matrix pipe for the LSTM at H = 2048 (round 5; the
// reference's best published models are 4 - 5 x BiLSTM-2048, testruns.md): ONE direction per launch
// on 256 workgroups of 8 units - 8 x 8192 weights as two fp16 pieces = 256 KB per workgroup, half
// in LDS (unpadded: a fragment's lanes l and l + 8 read the same 16 bytes), half in 256 registers
// per lane.  A producer = one workgroup = 8 units x 4 gates = 32 gate columns = ONE K = 32 MFMA
// step: its 16 rows are scaled by the power of two that puts the row's largest of those 32
// values into [2^13, 2^14).  Exchange [step][dir][producer P][piece][k group q][b][8 halves],
// k group q = units 2 q, 2 q + 1 of P, element e = 4 (unit & 1) + gate; inverse scales
// [step][dir][producer][32 rows].  Only 8 of an MFMA tile's 16 output columns are real (the other
// 8 repeat them and are never read).  One 16-row tile per launch (B <= 32: the tiles, like the
// directions, run one after the other).
#define PRNN_W16_H 2048
#ifndef PRNN_W16_D
#define PRNN_W16_D 12                  // ring depth: producers whose A granules are in flight
#endif
#ifndef PRNN_W16_KS
#define PRNN_W16_KS 2                  // CTCASR_RNN_KPAIR: workgroups that share a K axis (2 or 4)
#endif
#ifndef PRNN_W16_KD
#define PRNN_W16_KD 12                 // ... and their ring depth (64 / KS producers per wave)
#endif
__host__ __device__ inline size_t prnn_w16_scale_bytes(int T) {
    return (size_t)(T + 1) * 2 * (PRNN_W16_H / 8) * PRNN_B16_SCALE_ROWS * sizeof(float);
}
// K split: the words of a direction that last from launch to launch.  Every hand-off word carries
// the parity of its slot's write count in its lowest significand bit; the count at the start of a
// launch is kept here (advanced by the launch's last workgroup to leave), so a slot's current
// content never looks like the next one.
struct KPairWords {
    unsigned total;         // hand-offs every slot has seen before this launch (parity = tag base)
    unsigned pad0[15];
    unsigned done;          // workgroups of the launch that have left
    unsigned pad1[47];
};
// one KPairWords per direction, then [dir][workgroup][sending member 0 .. 3][128 words]
__host__ __device__ inline size_t prnn_w16_kp_bytes() {
    return 2 * sizeof(KPairWords) + (size_t)2 * (PRNN_W16_H / 8) * 4 * 128 * sizeof(unsigned);
}
// KS > 1 (round 6, CTCASR_RNN_KPAIR): the K axis split over KS workgroups of one XCD (2: pairs,
// 4: quads).  The workgroups that differ only in bits 3.. of their slice share 8 KS hidden units =
// KS / 2 FULL N tiles (the plain form multiplies half-empty tiles): each holds one K part
// (256 / KS producers) of the weights of all those units (the same 256 KB: 64 KB per wave, half in
// LDS, half in 128 registers), reads only that part's blocks - 512 / KS KB instead of 512 KB per
// direction-step, through L2s that were at half of their aggregate peak -, issues half of the
// MFMAs, and hands every partner the partial sums of that partner's 8 units: 16 x 8 fp32 words,
// each tagged in its lowest significand bit with the parity of the slot's write count
// (KPairWords of the direction; the receiver clears the bit again).  This kernel has ONE barrier
// per step and nothing in flight at the hand-off, so the receiver polls with L2-bypassing vector
// loads.  Publishes what the plain form publishes; the K sums differ in their order (to rounding).
template <int D, int KS = 1>
__global__ void __launch_bounds__(PRNN_THREADS) prnn_bwd16w_kernel(PArgs p) {
    constexpr int H = PRNN_W16_H, GH = 4 * H, NW = 4, NTH = PRNN_THREADS;
    constexpr int NP = H / 8;               // producers per direction = workgroups
    constexpr bool KP = KS > 1;
    constexpr int NT = KP ? KS / 2 : 1;     // N tiles of 16 units (plain form: one, half empty)
    constexpr int NPW = NP / NW / KS;       // producers per wave: 64 / KS
    constexpr int QS = NPW * 2 * NT;        // B-fragment slots per wave: (producer, piece, N tile)
    // plain form: 64 slots in LDS (512 B each: 8 real columns), 64 in registers; K split: 32 full
    // slots of 1 KB in LDS, 32 in registers
    constexpr int QL = QS / 2, REGW = QS - QL, SLOT = KP ? 64 : 32;
    static_assert(KS == 1 || KS == 2 || KS == 4, "K split");
    constexpr int RED_FLOATS = NW * 16 * 17;
    constexpr int IVL = NPW * 4;            // float4 slots of a wave's inverse scales
    extern __shared__ __attribute__((aligned(16))) char smem[];
    resident_signal(p.sync, p.ticket);
    if (launch_poisoned(p.sync)) return;
    u32x4 *frag = reinterpret_cast<u32x4 *>(smem);          // [wave][QL][32 granules]
    float *red = reinterpret_cast<float *>(smem + (size_t)NW * QL * SLOT * sizeof(u32x4));
    float4 *invs = reinterpret_cast<float4 *>(red + NT * RED_FLOATS);   // [wave][IVL]
    float *wave_top = reinterpret_cast<float *>(invs + NW * IVL);

    const int chain = p.chain0 + (int)blockIdx.x / (p.ndir * p.nwg);
    const int row0 = chain * 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x % (p.ndir * p.nwg);
    const int dir = p.dir0 + wg / p.nwg, slice = wg % p.nwg;
    const int group_size = p.nwg / PRNN_GROUPS, grp = slice / group_size;
    const int B = p.B, T = p.T, BS = p.BS;
    const int u0 = slice * 8;
    // K split: the KS workgroups that differ in bits 3.. of their slice (one XCD: workgroup b runs
    // on XCD b % 8); member j's 8 units are columns 8 j .. 8 j + 7 of the N tiles; this workgroup
    // is member kh and multiplies K part kh: producers (256 / KS) kh ...
    const int kh = KP ? (slice >> 3) & (KS - 1) : 0;
    auto member = [&](int j) -> int { return (slice & ~(8 * (KS - 1))) | (8 * j); };
    const int pb = (NP / KS) * kh + wave * NPW;             // this wave's first producer
    auto tile_unit = [&](int c) -> int { return KP ? member(c >> 3) * 8 + (c & 7) : u0 + (c & 7); };
    KPairWords *kpw = nullptr;
    unsigned kp_base = 0;
    if constexpr (KP) {
        kpw = reinterpret_cast<KPairWords *>(p.kp) + dir;
        kp_base = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(
            &kpw->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }

    // ---- this workgroup's 8 columns of R^T as scaled fp16 pieces -------------------------------
    float w_scale;
    {
        float m = 0.f;
        if constexpr (KP) {
            // 16 NT rows of R^T, the K part's H / KS columns of every gate
            for (int n = 0; n < NT; ++n) {
                const float *wrow = p.w + ((size_t)dir * H + tile_unit(n * 16 + (tid & 15))) * GH +
                                    (H / KS) * kh;
                for (int g = 0; g < 4; ++g)
                    for (int x = (tid >> 4) * 4; x < H / KS; x += NTH / 16 * 4) {
                        const float4 v = ldg4(wrow + (size_t)g * H + x);
                        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))),
                                  fmaxf(fabsf(v.z), fabsf(v.w)));
                    }
            }
        } else {
            const float *wrow = p.w + ((size_t)dir * H + u0 + (tid & 7)) * GH;
            for (int n = (tid >> 3) * 4; n < GH; n += NTH / 8 * 4) {
                const float4 v = ldg4(wrow + n);
                m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            }
        }
        m = wave_max(m);
        if (lane == 0) wave_top[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wave_top[0], wave_top[1]), fmaxf(wave_top[2], wave_top[3]));
        const unsigned bits = __float_as_uint(m);
        const int e = (int)((bits >> 23) & 0xFF) - 127;
        const int se = bits == 0u ? 0 : min(max(14 - e, -60), 60);
        w_scale = __uint_as_float((unsigned)(se + 127) << 23);
    }
    const float out_scale = 1.0f / w_scale;
    u32x4 wreg[REGW];
    {
        // fragment of producer P (of this wave), N tile n: lane (k group q = lane >> 4, column
        // lane & 15 [& 7])
        auto pieces = [&](int pw, int n, u32x4 &first, u32x4 &second) {
            const float *wcol = p.w + ((size_t)dir * H + tile_unit(n * 16 + (lane & 15))) * GH +
                                8 * (pb + pw) + 2 * (lane >> 4);
            unsigned q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                q[e] = f16_pieces(wcol[(size_t)(e & 3) * H + (e >> 2)] * w_scale);
            first = (u32x4){(q[0] & 0xFFFFu) | (q[1] << 16), (q[2] & 0xFFFFu) | (q[3] << 16),
                            (q[4] & 0xFFFFu) | (q[5] << 16), (q[6] & 0xFFFFu) | (q[7] << 16)};
            second = (u32x4){(q[0] >> 16) | (q[1] & 0xFFFF0000u), (q[2] >> 16) | (q[3] & 0xFFFF0000u),
                             (q[4] >> 16) | (q[5] & 0xFFFF0000u), (q[6] >> 16) | (q[7] & 0xFFFF0000u)};
        };
        // slot = (producer 2 + piece) NT + n
        for (int pw = 0; pw < QL / 2 / NT; ++pw)
            for (int n = 0; n < NT; ++n) {
                u32x4 first, second;
                pieces(pw, n, first, second);
                if constexpr (KP) {
                    frag[(wave * QL + (2 * pw) * NT + n) * 64 + lane] = first;
                    frag[(wave * QL + (2 * pw + 1) * NT + n) * 64 + lane] = second;
                } else if ((lane & 15) < 8) {
                    const int cell16 = (lane >> 4) * 8 + (lane & 7);
                    frag[(wave * QL + 2 * pw) * 32 + cell16] = first;
                    frag[(wave * QL + 2 * pw + 1) * 32 + cell16] = second;
                }
            }
#pragma unroll
        for (int pw = 0; pw < REGW / 2 / NT; ++pw)
#pragma unroll
            for (int n = 0; n < NT; ++n)
                pieces(QL / 2 / NT + pw, n, wreg[(2 * pw) * NT + n], wreg[(2 * pw + 1) * NT + n]);
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.xchg, 0, (int)((size_t)(T + 1) * 2 * B * GH * sizeof(float)), 0x00020000);
    const size_t x_step = (size_t)2 * B * GH;
    const size_t x_base = x_step;
    const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.rs, 0, (int)prnn_w16_scale_bytes(T), 0x00020000);
    constexpr unsigned S_STEP = 2u * NP * PRNN_B16_SCALE_ROWS * sizeof(float);
    const int rnum = 0x7FFFFFFF;
    const __amdgpu_buffer_rsrc_t dy_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.dy), 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t g_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.gates, 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.cells, 0, rnum, 0x00020000);
    const __amdgpu_buffer_rsrc_t dx_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.dxw, 0, rnum, 0x00020000);
    // K split: the hand-off slots behind the two directions' KPairWords:
    // [dir][slice][sending member 0 .. 3][128 words]
    const __amdgpu_buffer_rsrc_t kp_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        KP ? p.kp + 2 * sizeof(KPairWords) / sizeof(unsigned) : nullptr, 0,
        KP ? (int)(2 * NP * 4 * 128 * sizeof(unsigned)) : 0, 0x00020000);
    auto ldf = [](__amdgpu_buffer_rsrc_t r, unsigned off) -> float {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
    };

    // ---- the item of this thread (threads 0 .. 127): row tid >> 3 of the tile, unit tid & 7 -----
    const bool has_item = tid < 128;
    const int ib = (tid >> 3) & 15, iu = tid & 7, unit = u0 + iu;
    const int brow = row0 + ib;
    const int steps = has_item && brow < B ? row_steps(p.seq_len, brow, T) : 0;
    float dc_state = 0.f, dbs[4] = {0.f, 0.f, 0.f, 0.f}, cmx[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.s_hi < T && steps > 0) dc_state = p.carry[((size_t)dir * B + brow) * H + unit];
    const int arow = row0 + (lane & 15);
    const int a_steps = arow < B ? row_steps(p.seq_len, arow, T) : 0;

    unsigned long long pt[4] = {0, 0, 0, 0};
    const bool prof = p.prof && threadIdx.x == 0;       // (every workgroup: prof_all)
    for (int s = p.s_hi - 1; s >= p.s_lo; --s) {
        unsigned long long c0 = prof ? wall_clock64() : 0;
        float dyv = 0.f, gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, cv = 0.f, cpv = 0.f;
        int it_t = -1;
        // what the cell derivative needs besides dh_rec: requested before the barrier (behind the
        // first ring loads instead - the barrier's polls wait for everything in front of them in
        // the in-order queue - measured slower: profiles/r06_rnn_bwd_k_split_2048.md)
        auto cell_prefetch = [&]() {
            if (s < steps) {
                const int t = row_time(dir, s, steps);
                it_t = t;
                const unsigned e0 = (unsigned)(((t * BS + brow) * 2 + dir) * H + unit);
                dyv = ldf(dy_rsrc, e0 * 4u);
                gi = ldf(g_rsrc, (e0 * 4u - 3u * unit) * 4u);
                gf = ldf(g_rsrc, (e0 * 4u - 3u * unit + H) * 4u);
                gg = ldf(g_rsrc, (e0 * 4u - 3u * unit + 2 * H) * 4u);
                go = ldf(g_rsrc, (e0 * 4u - 3u * unit + 3 * H) * 4u);
                cv = ldf(c_rsrc, e0 * 4u);
                if (s > 0)
                    cpv = ldf(c_rsrc, (unsigned)(((row_time(dir, s - 1, steps) * BS + brow) * 2 +
                                                  dir) * H + unit) * 4u);
            }
        };
        cell_prefetch();
        f32x4 total[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) total[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (s < T - 1) {
            if (s < p.s_hi - 1) {
                dir_wait<1>(p.sync, nullptr, dir, chain, group_size, (unsigned)(p.s_hi - 2 - s),
                            tid);
                if (s == p.s_lo && tid == 0) counters_done(p.sync, dir, chain, p.nwg);
            }
            if (prof) { unsigned long long c = wall_clock64(); pt[0] += c - c0; c0 = c; }
            // inverse scales of the wave's 64 (32) producers x 16 rows: four (two) 1 KB loads
            float4 iv[NPW / 16];
#pragma unroll
            for (int j = 0; j < NPW / 16; ++j)
                iv[j] = load16_sc1(s_rsrc, (unsigned)(s + 1) * S_STEP +
                                               (unsigned)(((dir * NP + pb + 16 * j + (lane >> 2)) *
                                                           PRNN_B16_SCALE_ROWS + row0 + 4 * (lane & 3)) *
                                                          sizeof(float)));
            const bool ok = s + 1 < a_steps;        // otherwise: the all-zero block
            const unsigned aoff = (unsigned)(((ok ? x_base + (size_t)(s + 1) * x_step : 0) +
                                              (size_t)dir * B * GH + (size_t)(lane >> 4) * B * 4 +
                                              (size_t)(ok ? arow : 0) * 4) * sizeof(float));
            u32x4 a[D][2];
            // (the 128 wave-uniform offsets of a step are products with the runtime batch: opaque
            // to the optimiser here, or it computes them all ahead of the step loop and spills
            // a hundred scalar registers)
            unsigned gstride = (unsigned)(B * 16 * sizeof(float));
            asm volatile("" : "+s"(gstride));
            const unsigned wbase = (unsigned)(pb * 2) * gstride;
            auto issue = [&](int P, u32x4 (&dst)[2]) {
#pragma unroll
                for (int pc = 0; pc < 2; ++pc)
                    dst[pc] = load16u(x_rsrc, aoff, wbase + (unsigned)(P * 2 + pc) * gstride);
            };
#pragma unroll
            for (int P = 0; P < D; ++P) issue(P, a[P]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NPW / 16; ++j) invs[wave * IVL + 64 * j + lane] = iv[j];
            auto bfrag = [&](int sl) -> u32x4 {      // compile-time slot after unrolling
                if constexpr (KP)
                    return sl < QL ? frag[(wave * QL + sl) * 64 + lane] : wreg[sl - QL];
                return sl < QL ? frag[(wave * QL + sl) * 32 + (lane >> 4) * 8 + (lane & 7)]
                               : wreg[sl - QL];
            };
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int P = 0; P < NPW; ++P) {
                Frag16 w1[NT], w2[NT], d1, d2;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    w1[n].u = bfrag((2 * P) * NT + n);
                    w2[n].u = bfrag((2 * P + 1) * NT + n);
                }
                d1.u = a[P % D][0];
                d2.u = a[P % D][1];
                f32x4 acc0[NT], acc1[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc0[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(d1.h, w1[n].h, zero, 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc1[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(d1.h, w2[n].h, zero, 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc1[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(d2.h, w1[n].h, acc1[n], 0, 0, 0);
                if (P + D < NPW) issue(P + D, a[P % D]);
                const float4 ivp = invs[wave * IVL + 4 * P + (lane >> 4)];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const f32x4 sum = acc0[n] + acc1[n];
                    total[n][0] += sum[0] * ivp.x;
                    total[n][1] += sum[1] * ivp.y;
                    total[n][2] += sum[2] * ivp.z;
                    total[n][3] += sum[3] * ivp.w;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (prof) {
            asm volatile("" ::"v"(total[0][0]));
            unsigned long long c = wall_clock64(); pt[1] += c - c0; c0 = c;
        }
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                red[n * RED_FLOATS + (wave * 16 + 4 * (lane >> 4) + r) * 17 + (lane & 15)] =
                    total[n][r] * out_scale;
        __syncthreads();

        // K split: sum of the waves' shares of member j's 8 columns, for row ib and unit iu
        auto member_sum = [&](int j) -> float {
            const float *r = red + (j >> 1) * RED_FLOATS + ib * 17 + (j & 1) * 8 + iu;
            float v = r[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) v += r[w * 16 * 17];
            return v;
        };
        float others = 0.f;                 // K split: the partners' K parts of this item's sum
        if constexpr (KP) {
            const unsigned tag = (kp_base + (unsigned)(p.s_hi - s)) & 1u;
            if (!has_item) {
                // threads 128 .. 255: row (tid >> 3) & 15, unit tid & 7 of every partner -> word
                // tid - 128 of the partner's slot for this sender
#pragma unroll
                for (int j = 0; j < KS; ++j) {
                    if (j == kh) continue;
                    __builtin_amdgcn_raw_buffer_store_b32(
                        (__float_as_uint(member_sum(j)) & ~1u) | tag, kp_rsrc, (int)((tid - 128) * 4),
                        (int)((((dir * NP + member(j)) * 4 + kh) * 128) * 4),
                        16);
                }
            } else {
                unsigned rv[KS], spins = 0;
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < KS; ++j) {
                        rv[j] = tag;
                        if (j != kh)
                            rv[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(
                                kp_rsrc, (int)(tid * 4), (int)((((dir * NP + slice) * 4 + j) * 128) * 4),
                                16);
                    }
#pragma unroll
                    for (int j = 0; j < KS; ++j) ok = ok && (rv[j] & 1u) == tag;
                    if (__all(ok)) break;
                    if (++spins > PRNN_SPIN_LIMIT ||
                        ((spins & 1023u) == 0 &&
                         __hip_atomic_load(&p.sync->error, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT))) {
                        if (lane == 0)
                            __hip_atomic_store(&p.sync->error, 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
#pragma unroll
                for (int j = 0; j < KS; ++j)
                    if (j != kh) others += __uint_as_float(rv[j] & ~1u);
            }
        }
        if (has_item) {
            float dg[4] = {0.f, 0.f, 0.f, 0.f};
            if (it_t >= 0) {
                float dh = dyv;
                if constexpr (KP) {
                    dh += member_sum(kh) + others;
                } else {
#pragma unroll
                    for (int w = 0; w < NW; ++w) dh += red[(w * 16 + ib) * 17 + iu];
                }
                const float tc = tanhf_(cv);
                const float dc = dc_state + dh * go * (1.f - tc * tc);
                dg[0] = dc * gg * gi * (1.f - gi);
                dg[1] = dc * cpv * gf * (1.f - gf);
                dg[2] = dc * gi * (1.f - gg * gg);
                dg[3] = dh * tc * go * (1.f - go);
                dc_state = dc * gf;
            }
            // the row's scale over this workgroup's 32 values (8 lanes of a DPP row)
            float mx = fmaxf(fmaxf(fabsf(dg[0]), fabsf(dg[1])), fmaxf(fabsf(dg[2]), fabsf(dg[3])));
            mx = fmaxf(mx, __uint_as_float(dpp_u32<0xB1>(__float_as_uint(mx))));
            mx = fmaxf(mx, __uint_as_float(dpp_u32<0x4E>(__float_as_uint(mx))));
            mx = fmaxf(mx, __uint_as_float(dpp_u32<0x141>(__float_as_uint(mx))));
            const unsigned mbits = __float_as_uint(mx);
            const int me = (int)((mbits >> 23) & 0xFF) - 127;
            const int mse = mbits == 0u ? 0 : min(max(13 - me, -100), 100);
            const float rscale = __uint_as_float((unsigned)(mse + 127) << 23);
            const float rinv = __uint_as_float((unsigned)(127 - mse) << 23);
            unsigned q[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) q[g] = f16_pieces(dg[g] * rscale);
            const bool odd = (tid & 1) != 0;
            const unsigned f01 = (q[0] & 0xFFFFu) | (q[1] << 16), f23 = (q[2] & 0xFFFFu) | (q[3] << 16);
            const unsigned s01 = (q[0] >> 16) | (q[1] & 0xFFFF0000u),
                           s23 = (q[2] >> 16) | (q[3] & 0xFFFF0000u);
            const unsigned give01 = odd ? f01 : s01, give23 = odd ? f23 : s23;
            const unsigned got01 = dpp_u32<0xB1>(give01), got23 = dpp_u32<0xB1>(give23);   // lane ^ 1
            const u32x4 v = odd ? (u32x4){got01, got23, s01, s23} : (u32x4){f01, f23, got01, got23};
            if (it_t >= 0) {
                const unsigned off = (unsigned)(
                    (x_base + (size_t)s * x_step + (size_t)dir * B * GH +
                     (size_t)(slice * 2 + (odd ? 1 : 0)) * B * 16 +
                     (size_t)((iu >> 1) & 3) * B * 4 + (size_t)brow * 4) * sizeof(float));
                __builtin_amdgcn_raw_buffer_store_b128(v, x_rsrc, (int)off, 0, 16);
            }
            // the eight rows of this wave: two 16-byte stores of their inverse scales
            float rr[8];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                rr[k] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(rinv), 8 * k));
            if (lane == 0) {
                const unsigned so = (unsigned)s * S_STEP +
                                    (unsigned)(((dir * NP + slice) * PRNN_B16_SCALE_ROWS + row0 +
                                                (tid >> 3)) * sizeof(float));
                store16_sc1(s_rsrc, so, rr[0], rr[1], rr[2], rr[3]);
                store16_sc1(s_rsrc, so + 16u, rr[4], rr[5], rr[6], rr[7]);
            }
            if (it_t >= 0) {
                const unsigned dx0 = (unsigned)(((it_t * BS + brow) * 2 + dir) * GH + unit) * 4u;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg[g]), dx_rsrc,
                                                          (int)(dx0 + (unsigned)g * H * 4u), 0, 0);
                    dbs[g] += dg[g];
                    cmx[g] = fmaxf(cmx[g], fabsf(dg[g]));
                }
            }
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[2] += c - c0; c0 = c; }
        if (s > p.s_lo) {
            unsigned unused = 0;
            dir_arrive<1>(p.sync, nullptr, dir, chain, grp, tid, unused);
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[3] += c - c0; c0 = c; }
    }
    if (prof)
        for (int i = 0; i < 4; ++i) {
            if (blockIdx.x == 0) p.sync->prof[4 + i] = pt[i];
            p.sync->prof_all[blockIdx.x & 255][i] = pt[i];
        }
    if constexpr (KP) {
        // the last workgroup to leave advances the direction's write count (KPairWords)
        __syncthreads();
        if (tid == 0) {
            const unsigned before = __hip_atomic_fetch_add(&kpw->done, 1u, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
            if (before + 1 == (unsigned)p.nwg) {
                __hip_atomic_store(&kpw->total, kp_base + (unsigned)(p.s_hi - p.s_lo),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&kpw->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (p.s_lo > 0 && steps > 0) p.carry[((size_t)dir * B + brow) * H + unit] = dc_state;
    if (p.dbias || p.colmax) {
        float *sums = red, *tops = reinterpret_cast<float *>(frag);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            __syncthreads();
            if (has_item) {
                sums[tid] = dbs[g];
                tops[tid] = cmx[g];
            }
            __syncthreads();
            if (tid < 8) {
                float sum = 0.f, top = 0.f;
                for (int r = 0; r < 16; ++r) {
                    sum += sums[r * 8 + tid];
                    top = fmaxf(top, tops[r * 8 + tid]);
                }
                if (p.dbias) atomicAdd(p.dbias + ((size_t)dir * 4 + g) * H + u0 + tid, sum);
                if (p.colmax)
                    atomicMax(p.colmax + ((size_t)dir * 4 + g) * H + u0 + tid, __float_as_uint(top));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The plain ReLU recurrence at H = 2048 - the reference's DEFAULT model, asr/params.py:43-50 - on the
// fp16 matrix pipe (round 5), forward (BWD = false: h_t = relu(xw_t + b + h_(t-1) W_hh^T)) and
// backward (BWD = true: dpre_t = (dy_t + dpre_(t+1) W_hh) [y_t > 0]) from one kernel: both are "a
// row vector of 2048 values times a 2048 x 2048 matrix, then something elementwise".  Neither h
// (no bound behind a ReLU) nor dpre has a range, so BOTH take the block scaling of the LSTM
// backward kernel (section 4.1e): a producer = one workgroup = 32 units = ONE K = 32 MFMA step
// scales each of its 16 rows by the power of two of the row's largest of those 32 values,
// publishes two fp16 pieces per value [step][dir][producer][piece][k group of 8 units][b][8 halves]
// + 16 inverse scales; the consumer multiplies a producer's block into fresh accumulators and
// adds them times the inverse scale.  64 workgroups per direction (128 CUs: weight-gradient GEMMs
// fit beside it), 32 units = two N tiles each, 32 x 2048 weights as two fp16 pieces = 256 KB = 128
// KB LDS + 128 registers per lane, scaled per workgroup.  One 16-row tile (B <= 16), every row
// running all T steps; everything else takes the fp32 kernels.
#define PRNN_R16_H 2048
__host__ __device__ inline size_t prnn_r16_scale_bytes(int T) {
    return (size_t)(T + 1) * 2 * (PRNN_R16_H / 32) * PRNN_B16_SCALE_ROWS * sizeof(float);
}
template <bool BWD>
__global__ void __launch_bounds__(PRNN_THREADS) prnn_relu16_kernel(PArgs p) {
    constexpr int H = PRNN_R16_H, NW = 4, NTH = PRNN_THREADS;
    constexpr int NP = H / 32;              // producers per direction = workgroups: 64
    constexpr int NPW = NP / NW;            // producers per wave: 16
    constexpr int QS = NPW * 4;             // B-fragment slots per wave: (producer, N tile, piece)
    constexpr int QL = QS / 2, REGW = QS - QL;
    constexpr int RED_FLOATS = NW * 2 * 16 * 17;
    constexpr int IVL = NPW * 4;            // float4 slots of a wave's inverse scales
    extern __shared__ __attribute__((aligned(16))) char smem[];
    resident_signal(p.sync, p.ticket);
    if (launch_poisoned(p.sync)) return;
    u32x4 *frag = reinterpret_cast<u32x4 *>(smem);
    float *red = reinterpret_cast<float *>(smem + (size_t)NW * QL * 64 * sizeof(u32x4));
    float4 *invs = reinterpret_cast<float4 *>(red + RED_FLOATS);
    float *wave_top = reinterpret_cast<float *>(invs + NW * IVL);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x % (p.ndir * p.nwg);
    const int dir = p.dir0 + wg / p.nwg, slice = wg % p.nwg;
    const int chain = 0;
    const int group_size = p.nwg / PRNN_GROUPS, grp = slice / group_size;
    const int B = p.B, T = p.T, BS = p.BS;
    const int u0 = slice * 32;

    // ---- this workgroup's 32 rows of the matrix (forward: w_hh [dir][unit][k]; backward: w_hh_t
    // [dir][unit][k] - the contraction index is the contiguous one either way) as scaled pieces
    float w_scale;
    {
        float m = 0.f;
        const float *wrow = p.w + ((size_t)dir * H + u0 + (tid & 31)) * H;
        for (int n = (tid >> 5) * 4; n < H; n += NTH / 32 * 4) {
            const float4 v = ldg4(wrow + n);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
        m = wave_max(m);
        if (lane == 0) wave_top[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wave_top[0], wave_top[1]), fmaxf(wave_top[2], wave_top[3]));
        const unsigned bits = __float_as_uint(m);
        const int e = (int)((bits >> 23) & 0xFF) - 127;
        const int se = bits == 0u ? 0 : min(max(14 - e, -60), 60);
        w_scale = __uint_as_float((unsigned)(se + 127) << 23);
    }
    const float out_scale = 1.0f / w_scale;
    u32x4 wreg[REGW];
    {
        // slot (producer pw of this wave, N tile nt): lane (k group q = lane >> 4, column lane & 15)
        // holds the 8 contraction indices 32 P + 8 q .. + 7 of unit u0 + 16 nt + column
        auto pieces = [&](int sl2, u32x4 &first, u32x4 &second) {
            const int pw = sl2 >> 1, nt = sl2 & 1;
            const float *wcol = p.w + ((size_t)dir * H + u0 + 16 * nt + (lane & 15)) * H +
                                32 * (wave * NPW + pw) + 8 * (lane >> 4);
            const float4 lo = ldg4(wcol), hi = ldg4(wcol + 4);
            const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            unsigned q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = f16_pieces(v[e] * w_scale);
            first = (u32x4){(q[0] & 0xFFFFu) | (q[1] << 16), (q[2] & 0xFFFFu) | (q[3] << 16),
                            (q[4] & 0xFFFFu) | (q[5] << 16), (q[6] & 0xFFFFu) | (q[7] << 16)};
            second = (u32x4){(q[0] >> 16) | (q[1] & 0xFFFF0000u), (q[2] >> 16) | (q[3] & 0xFFFF0000u),
                             (q[4] >> 16) | (q[5] & 0xFFFF0000u), (q[6] >> 16) | (q[7] & 0xFFFF0000u)};
        };
        for (int sl2 = 0; sl2 < QL / 2; ++sl2) {
            u32x4 first, second;
            pieces(sl2, first, second);
            frag[(wave * QL + 2 * sl2) * 64 + lane] = first;
            frag[(wave * QL + 2 * sl2 + 1) * 64 + lane] = second;
        }
#pragma unroll
        for (int sl2 = 0; sl2 < REGW / 2; ++sl2)
            pieces(QL / 2 + sl2, wreg[2 * sl2], wreg[2 * sl2 + 1]);
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.xchg, 0, (int)((size_t)(T + 1) * 2 * B * H * sizeof(float)), 0x00020000);
    const size_t x_step = (size_t)2 * B * H;
    const size_t x_base = x_step;
    const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.rs, 0, (int)prnn_r16_scale_bytes(T), 0x00020000);
    constexpr unsigned S_STEP = 2u * NP * PRNN_B16_SCALE_ROWS * sizeof(float);

    // ---- the two items of this thread: row (item >> 5), unit item & 31; item = tid + 256 it -----
    const int iu = tid & 31, unit = u0 + iu;
    int brow[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) brow[it] = (tid >> 5) + 8 * it;
    const float bias = (!BWD && p.bias) ? p.bias[(size_t)dir * H + unit] : 0.f;
    const int arow = lane & 15;
    float dbs = 0.f, cmx = 0.f;

    const int s_first = BWD ? p.s_hi - 1 : p.s_lo, s_last = BWD ? p.s_lo : p.s_hi - 1;
    const int s_inc = BWD ? -1 : 1;
    unsigned long long pt[4] = {0, 0, 0, 0};
    const bool prof = p.prof && blockIdx.x == 0 && threadIdx.x == 0;
    for (int s = s_first; BWD ? s >= s_last : s <= s_last; s += s_inc) {
        unsigned long long c0 = prof ? wall_clock64() : 0;
        const int t = row_time(dir, s, T);
        // the step's own inputs, requested before the barrier
        float in0[2], in1[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            in0[it] = in1[it] = 0.f;
            if (brow[it] < B) {
                if constexpr (BWD) {
                    const size_t e = ((size_t)t * BS + brow[it]) * 2 * H + dir * H + unit;
                    in0[it] = p.dy[e];
                    in1[it] = p.y[e];
                } else {
                    in0[it] = p.xw[(((size_t)t * BS + brow[it]) * 2 + dir) * H + unit] + bias;
                }
            }
        }
        f32x4 total[2];
        total[0] = total[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int src = BWD ? s + 1 : s - 1;            // the step whose published block is read
        if (BWD ? s < T - 1 : s > 0) {
            if (s != s_first) {
                dir_wait<1>(p.sync, nullptr, dir, chain, group_size,
                            (unsigned)(BWD ? p.s_hi - 2 - s : s - 1 - p.s_lo), tid);
                if (s == s_last && tid == 0) counters_done(p.sync, dir, chain, p.nwg);
            }
            if (prof) { unsigned long long c = wall_clock64(); pt[0] += c - c0; c0 = c; }
            const float4 iv = load16_sc1(
                s_rsrc, (unsigned)src * S_STEP +
                            (unsigned)(((dir * NP + wave * NPW + (lane >> 2)) * PRNN_B16_SCALE_ROWS +
                                        4 * (lane & 3)) * sizeof(float)));
            const bool ok = arow < B;
            const unsigned aoff = (unsigned)(((ok ? x_base + (size_t)src * x_step : 0) +
                                              (size_t)dir * B * H + (size_t)(lane >> 4) * B * 4 +
                                              (size_t)(ok ? arow : 0) * 4) * sizeof(float));
            unsigned gstride = (unsigned)(B * 16 * sizeof(float));
            asm volatile("" : "+s"(gstride));
            const unsigned wbase = (unsigned)(wave * NPW * 2) * gstride;
            u32x4 a[NPW][2];
#pragma unroll
            for (int P = 0; P < NPW; ++P)
#pragma unroll
                for (int pc = 0; pc < 2; ++pc)
                    a[P][pc] = load16u(x_rsrc, aoff, wbase + (unsigned)(P * 2 + pc) * gstride);
            __builtin_amdgcn_sched_barrier(0);
            if (lane < IVL) invs[wave * IVL + lane] = iv;
            auto bfrag = [&](int sl) -> u32x4 {
                return sl < QL ? frag[(wave * QL + sl) * 64 + lane] : wreg[sl - QL];
            };
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int P = 0; P < NPW; ++P) {
                Frag16 d1, d2;
                d1.u = a[P][0];
                d2.u = a[P][1];
                const float4 ivp = invs[wave * IVL + 4 * P + (lane >> 4)];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    Frag16 w1, w2;
                    w1.u = bfrag((P * 2 + nt) * 2);
                    w2.u = bfrag((P * 2 + nt) * 2 + 1);
                    f32x4 acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d1.h, w1.h, zero, 0, 0, 0);
                    f32x4 acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d1.h, w2.h, zero, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d2.h, w1.h, acc1, 0, 0, 0);
                    const f32x4 sum = acc0 + acc1;
                    total[nt][0] += sum[0] * ivp.x;
                    total[nt][1] += sum[1] * ivp.y;
                    total[nt][2] += sum[2] * ivp.z;
                    total[nt][3] += sum[3] * ivp.w;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (prof) {
            asm volatile("" ::"v"(total[0][0]));
            unsigned long long c = wall_clock64(); pt[1] += c - c0; c0 = c;
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                red[((wave * 2 + nt) * 16 + 4 * (lane >> 4) + r) * 17 + (lane & 15)] =
                    total[nt][r] * out_scale;
        __syncthreads();

#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const bool has = brow[it] < B;
            float acc = in0[it];
#pragma unroll
            for (int w = 0; w < NW; ++w)
                acc += red[((w * 2 + (iu >> 4)) * 16 + brow[it]) * 17 + (iu & 15)];
            float val;                               // what the next step multiplies
            if constexpr (BWD) val = in1[it] > 0.f ? acc : 0.f;
            else val = relu_keep_nan(acc);
            if (!has) val = 0.f;
            // the row's scale over this workgroup's 32 values (two DPP rows of 16 lanes)
            float mx = row16_max(fabsf(val));
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            const unsigned mbits = __float_as_uint(mx);
            const int me = (int)((mbits >> 23) & 0xFF) - 127;
            const int mse = mbits == 0u ? 0 : min(max(13 - me, -100), 100);
            const float rscale = __uint_as_float((unsigned)(mse + 127) << 23);
            const float rinv = __uint_as_float((unsigned)(127 - mse) << 23);
            u32x4 first, second;
            gather8_pieces(f16_pieces(val * rscale), first, second);
            if (has && (tid & 7) == 0) {
                const unsigned off = (unsigned)(
                    (x_base + (size_t)s * x_step + (size_t)dir * B * H + (size_t)slice * B * 32 +
                     (size_t)(iu >> 3) * B * 4 + (size_t)brow[it] * 4) * sizeof(float));
                __builtin_amdgcn_raw_buffer_store_b128(first, x_rsrc, (int)off, 0, 16);
                __builtin_amdgcn_raw_buffer_store_b128(
                    second, x_rsrc, (int)(off + (unsigned)(B * 16 * sizeof(float))), 0, 16);
            }
            if (has && (tid & 31) == 0)
                __builtin_amdgcn_raw_buffer_store_b32(
                    __float_as_uint(rinv), s_rsrc,
                    (int)((unsigned)s * S_STEP +
                          (unsigned)(((dir * NP + slice) * PRNN_B16_SCALE_ROWS + brow[it]) *
                                     sizeof(float))), 0, 16);
            if (has) {
                if constexpr (BWD) {
                    p.dxw[(((size_t)t * BS + brow[it]) * 2 + dir) * H + unit] = val;
                    dbs += val;
                    cmx = fmaxf(cmx, fabsf(val));
                } else {
                    p.y[((size_t)t * BS + brow[it]) * 2 * H + dir * H + unit] = val;
                }
            }
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[2] += c - c0; c0 = c; }
        if (s != s_last) {
            unsigned unused = 0;
            dir_arrive<1>(p.sync, nullptr, dir, chain, grp, tid, unused);
        } else {
            __syncthreads();            // (the partial sums in LDS are reused by nobody after this)
        }
        if (prof) { unsigned long long c = wall_clock64(); pt[3] += c - c0; c0 = c; }
    }
    if (prof)
        for (int i = 0; i < 4; ++i) p.sync->prof[(BWD ? 4 : 0) + i] = pt[i];
    if (BWD && (p.dbias || p.colmax)) {
        // sums / maxima over the 8 rows a thread column holds, then one atomic per unit
        float *sums = red, *tops = red + 256;
        __syncthreads();
        sums[tid] = dbs;
        tops[tid] = cmx;
        __syncthreads();
        if (tid < 32) {
            float sum = 0.f, top = 0.f;
            for (int r = 0; r < 8; ++r) {
                sum += sums[r * 32 + tid];
                top = fmaxf(top, tops[r * 32 + tid]);
            }
            if (p.dbias) atomicAdd(p.dbias + (size_t)dir * H + u0 + tid, sum);
            if (p.colmax) atomicMax(p.colmax + (size_t)dir * H + u0 + tid, __float_as_uint(top));
        }
    }
}

int device_cu_count() {
    static int cus = -1;
    if (cus < 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        else
            cus = 0;
    }
    return cus;
}

// Optional HIP-event timing of the persistent launches themselves (option "rnn_kernel_events"):
// an event pair is recorded on the launch stream right around each kernel, so that a benchmark can
// report the kernel's duration as a profiler's kernel trace sees it - without the memsets and the
// host-side gaps a caller-side bracket around ctcasr_rnn_fwd / _bwd would include.
struct TimedLaunch { hipEvent_t start, stop; int backward; };
int g_kernel_events = 0;
std::vector<TimedLaunch> g_timed;

template <typename K>
int launch_persistent(K kernel, const PArgs &p, size_t lds, hipStream_t s, int chains = 1,
                      int tile_groups = 1) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return CTCASR_ERR_LAUNCH;
    // No memsets: the arrival counters are zeroed again by the launch that used them
    // (counters_done), the all-zero block of the exchange buffer is never written, and the
    // time-out word is sticky (ctcasr_rnn_poll_error reads and clears it).  All three rely on the
    // workspace having been zero-filled ONCE before its first use with this (B, H), and on the
    // words that last from launch to launch (barrier words, K-pair hand-off words) sitting at
    // offsets that do not move with T: the workspace's control header (rnn_step.hip).  The
    // all-zero block of row blocks >= 1 does move with T; the library clears it at the start of
    // each pass (ctcasr_rnn_fwd_steps / _bwd_steps).
    TimedLaunch timed = {};
    const bool record = g_kernel_events && g_timed.size() < 65536 &&
                        hipEventCreate(&timed.start) == hipSuccess &&
                        hipEventCreate(&timed.stop) == hipSuccess;
    if (record) (void)hipEventRecord(timed.start, s);
    kernel<<<p.ndir * p.nwg * tile_groups, PRNN_THREADS * chains, lds, s>>>(p);
    if (record) {
        (void)hipEventRecord(timed.stop, s);
        timed.backward = p.dxw != nullptr;
        g_timed.push_back(timed);
    }
    return ctcasr_launch_status();
}

}  // namespace

// Sums and clears the recorded launches: launches[0] / total_ms[0] forward, [1] backward.  Waits
// for the recorded events to complete.
extern "C" int ctcasr_rnn_kernel_events(int *launches, double *total_ms) {
    if (!launches || !total_ms) return CTCASR_ERR_BAD_ARGUMENT;
    launches[0] = launches[1] = 0;
    total_ms[0] = total_ms[1] = 0.0;
    int rc = CTCASR_OK;
    for (TimedLaunch &t : g_timed) {
        float ms = 0.f;
        if (hipEventSynchronize(t.stop) == hipSuccess &&
            hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
            launches[t.backward] += 1;
            total_ms[t.backward] += ms;
        } else {
            rc = CTCASR_ERR_LAUNCH;
        }
        (void)hipEventDestroy(t.start);
        (void)hipEventDestroy(t.stop);
    }
    g_timed.clear();
    return rc;
}

// Whether the LDS-resident kernels cover this shape (LSTM, H = 1024, B <= 32 for now; every
// other shape takes the streaming kernels of rnn_step.hip).
extern "C" int ctcasr_rnn_persistent_supported(int cell, int T, int B, int H) {
    // shapes whose weight slice is 128 KB per CU: LSTM H=1024 (BASELINE configs) and the plain
    // ReLU / tanh RNN at H=2048 (the reference's default model).  B <= 32: two batch tiles keep
    // the reduction scratch next to the weight slice.
    // ... and the LSTM at H = 2048 (the reference's best published models, testruns.md): 67 MB of
    // recurrent weights per direction fit the chip's LDS + registers only one direction at a time,
    // so its two directions run as two launches of 256 workgroups each.
    const bool lstm = cell == CTCASR_CELL_LSTM && (H == 1024 || H == 2048);
    // the GRU rides on the LSTM kernels' four-gate column layout (fourth slot empty)
    const bool gru = cell == CTCASR_CELL_GRU && (H == 1024 || H == 2048);
    const bool rnn = (cell == CTCASR_CELL_RNN_RELU || cell == CTCASR_CELL_RNN_TANH) && H == 2048;
    // batches of 33..64 rows run as two launches over blocks of at most 32 rows
    if (!(lstm || gru || rnn) || B < 1 || B > 2 * PRNN_BLOCK_ROWS || T < 1) return 0;
    // the exchange buffer (of one block of rows) is addressed through a 32-bit buffer descriptor
    const int rows = B < PRNN_BLOCK_ROWS ? B : PRNN_BLOCK_ROWS;
    if ((size_t)(T + 1) * 2 * rows * (lstm ? 4 : (gru ? 3 : 1)) * H * sizeof(float) >= (1ull << 31))
        return 0;
    const char *mode = getenv("CTCASR_RNN_MODE");   // "stream" forces the per-step kernels
    if (mode && mode[0] == 's') return 0;
    return device_cu_count() >= 256 ? 1 : 0;
}

size_t prnn_sync_bytes() { return sizeof(SyncWords); }

// Process-wide switches that change no result: "rnn_kernel_events" (profiling) and
// "wgrad16_spin_limit" (polls before a part of ctcasr_wgrad16_gemm gives up waiting for its turn;
// 0 = the default - for the test of that path).  Which variant of a persistent kernel runs is a
// per-call argument (`flags` of ctcasr_rnn_fwd_steps / _bwd_steps).
void wgrad16_set_spin_limit(long polls);      // (wgrad16.hip)
extern int g_grad_norm_blocks;                // (grad_norm.hip)
extern int g_seq_bn_blocks;                   // (seq_bn.hip)
extern "C" int ctcasr_set_option(const char *name, int value) {
    if (!name) return CTCASR_ERR_BAD_ARGUMENT;
    if (strcmp(name, "rnn_kernel_events") == 0) { g_kernel_events = value ? 1 : 0; return CTCASR_OK; }
    if (strcmp(name, "wgrad16_spin_limit") == 0) { wgrad16_set_spin_limit(value); return CTCASR_OK; }
    if (strcmp(name, "grad_norm_blocks") == 0) {
        if (value < 0 || value > 65536) return CTCASR_ERR_BAD_ARGUMENT;
        g_grad_norm_blocks = value;
        return CTCASR_OK;
    }
    if (strcmp(name, "seq_bn_blocks") == 0) {
        if (value < 0 || value > 65536) return CTCASR_ERR_BAD_ARGUMENT;
        g_seq_bn_blocks = value;
        return CTCASR_OK;
    }
    return CTCASR_ERR_BAD_ARGUMENT;
}

static size_t prnn_step_exchange_bytes(int T, int B, int H, int G) {
    return ctcasr_align_up((size_t)(T + 1) * 2 * B * G * H * sizeof(float), 256);
}
// the per-step blocks, then the inverse scales of the fp16 backward kernels.  Everything here is written by a pass
// before that pass reads it - except the all-zero block in front of the steps (rnn_step.hip) - so
// it may sit at offsets that move with T; the K-pair hand-off words, which last from launch to
// launch, are not part of it (prnn_kp_region_bytes).
size_t prnn_exchange_bytes(int T, int B, int H, int G) {
    return prnn_step_exchange_bytes(T, B, H, G) +
           (G == 4 && H == PRNN_B16_H ? ctcasr_align_up(prnn_b16_scale_bytes(T), 256) : 0) +
           (G == 4 && H == PRNN_W16_H ? ctcasr_align_up(prnn_w16_scale_bytes(T), 256) : 0) +
           (G == 1 && H == PRNN_R16_H ? prnn_r16_scale_bytes(T) : 0);
}

int prnn_fwd(int cell, const float *xw, const float *xw_bias, const float *w_hh,
             const float *b_hh_n, const int32_t *seq_len, int T, int B, int BS, int H, float *y,
             void *y16, float *gates, float *cells, void *sync, void *xchg, float *carry,
             int step_begin, int step_end, int flags, hipStream_t s) {
    // forward default: the whole chip (nothing of the same layer can overlap it)
    const bool fwd_half_chip = (flags & CTCASR_RNN_HALF_CHIP) != 0;
    PArgs p = {};
    p.carry = carry;
    p.xchg = reinterpret_cast<float *>(xchg);
    p.xw = xw; p.w = w_hh; p.seq_len = seq_len; p.y = y; p.gates = gates; p.cells = cells;
    p.y16 = reinterpret_cast<unsigned short *>(y16);
    p.bias = xw_bias; p.b_hh = b_hh_n;
    p.ndir = 2; p.dir0 = 0; p.chain0 = 0;
    p.sync = reinterpret_cast<SyncWords *>(sync);
    p.T = T; p.B = B; p.BS = BS; p.H = H;
    p.s_lo = step_begin; p.s_hi = step_end;
    p.prof = getenv("CTCASR_RNN_PROF") != nullptr;
    p.ticket = ((unsigned)flags >> 8) & 0xFFFFFFu;
    p.xcd_split = (flags & CTCASR_RNN_XCD_SPLIT) != 0;
    const int mt = (B + 15) / 16;
    const bool one_barrier = (flags & CTCASR_RNN_ONE_BARRIER) != 0;
    // fp16 matrix pipe (CTCASR_RNN_F16): the same geometries as the fp32 kernels below - H = 2048
    // one direction per launch on 256 workgroups; H = 1024 on 64 workgroups per direction and
    // batch tile (16 units, weights half in LDS, half in registers) for B > 16 or on half of the
    // chip, else 128 workgroups per direction with the 128 KB slice in LDS
    if ((flags & CTCASR_RNN_F16) && (cell == CTCASR_CELL_LSTM || cell == CTCASR_CELL_GRU) &&
        !(mt == 2 && one_barrier)) {
        const bool lstm = cell == CTCASR_CELL_LSTM;
        if (H == 2048) {
            p.nwg = 256; p.ndir = 1;
            const size_t lds = (size_t)4 * 32 * 64 * 16 + (size_t)4 * 2 * 16 * 17 * 4 + 32;
            for (int tile = 0; tile < mt; ++tile)
                for (int dir = 0; dir < 2; ++dir) {
                    p.chain0 = tile; p.dir0 = dir;
                    const int rc = lstm
                        ? launch_persistent(prnn_fwd16_kernel<CTCASR_CELL_LSTM, 2, 16, 32>, p, lds, s)
                        : launch_persistent(prnn_fwd16_kernel<CTCASR_CELL_GRU, 2, 16, 32>, p, lds, s);
                    if (rc != CTCASR_OK) return rc;
                }
            return CTCASR_OK;
        }
        if (mt == 2 || fwd_half_chip) {
            p.nwg = 64;
            const size_t lds = (size_t)4 * 32 * 64 * 16 + (size_t)4 * 4 * 16 * 17 * 4 + 32;
            return lstm
                ? launch_persistent(prnn_fwd16_kernel<CTCASR_CELL_LSTM, 4, 8, 32>, p, lds, s, 1, mt)
                : launch_persistent(prnn_fwd16_kernel<CTCASR_CELL_GRU, 4, 8, 32>, p, lds, s, 1, mt);
        }
        p.nwg = 128;
        const size_t lds = (size_t)4 * 32 * 64 * 16 + (size_t)4 * 2 * 16 * 17 * 4 + 32;
        return lstm ? launch_persistent(prnn_fwd16_kernel<CTCASR_CELL_LSTM, 2, 8, 0>, p, lds, s)
                    : launch_persistent(prnn_fwd16_kernel<CTCASR_CELL_GRU, 2, 8, 0>, p, lds, s);
    }
    if ((flags & CTCASR_RNN_F16) && cell == CTCASR_CELL_RNN_RELU && H == PRNN_R16_H && mt == 1 &&
        !seq_len) {
        // the reference's default cell on the fp16 pipe: 64 workgroups per direction, 32 units each
        p.nwg = PRNN_R16_H / 32;
        p.rs = reinterpret_cast<float *>(reinterpret_cast<char *>(p.xchg) +
                                         prnn_step_exchange_bytes(T, B, H, 1));
        const size_t lds = (size_t)4 * 32 * 64 * 16 + (size_t)4 * 2 * 16 * 17 * 4 +
                           (size_t)4 * 64 * 16 + 64;
        return launch_persistent(prnn_relu16_kernel<false>, p, lds, s);
    }
    // 128 workgroups per direction, 16 * NT gate columns each, QW = H / 64 K chunks per wave
#define PRNN_FWD(CELL_, NT_, QW_, MT_)                                                        \
    return launch_persistent(prnn_fwd_kernel<CELL_, NT_, QW_, MT_>, p,                         \
                             (size_t)NT_ * 4 * QW_ * 64 * 16 +                                 \
                                 (size_t)4 * NT_ * MT_ * 16 * 17 * 4 + 32, s)
    p.nwg = 128;
    if ((cell == CTCASR_CELL_LSTM || cell == CTCASR_CELL_GRU) && H == 2048) {
        // 8 units = 2 N tiles per workgroup, 256 workgroups = the whole chip for ONE direction:
        // 32 x 2048 x 4 B = 256 KB per workgroup, half in LDS, half in registers.  Directions (and
        // 16-row batch tiles) one after the other, each launch with its own counters.
        p.nwg = 256; p.ndir = 1;
        for (int tile = 0; tile < mt; ++tile)
            for (int dir = 0; dir < 2; ++dir) {
                p.chain0 = tile; p.dir0 = dir;
                const size_t lds = (size_t)4 * 32 * 64 * 16 + (size_t)4 * 2 * 16 * 17 * 4 + 32;
                const int rc = cell == CTCASR_CELL_LSTM
                    ? launch_persistent(prnn_fwd_kernel<CTCASR_CELL_LSTM, 2, 32, 1, 32>, p, lds, s)
                    : launch_persistent(prnn_fwd_kernel<CTCASR_CELL_GRU, 2, 32, 1, 32>, p, lds, s);
                if (rc != CTCASR_OK) return rc;
            }
        return CTCASR_OK;
    }
    if (cell == CTCASR_CELL_GRU) {
        // H = 1024: the LSTM's geometry (8 units per workgroup, 128 per direction; B > 16: one
        // group of 2 x 64 sixteen-unit workgroups per batch tile)
        if (mt == 2 && !one_barrier) {
            p.nwg = 64;
            return launch_persistent(prnn_fwd_kernel<CTCASR_CELL_GRU, 4, 16, 1, 32>, p,
                                     (size_t)4 * 32 * 64 * 16 + (size_t)4 * 4 * 16 * 17 * 4 + 32,
                                     s, 1, mt);
        }
        if (mt == 1) { PRNN_FWD(CTCASR_CELL_GRU, 2, 16, 1); }
        PRNN_FWD(CTCASR_CELL_GRU, 2, 16, 2);
    }
    // LSTM on 64 workgroups per direction: 16 units = 4 N tiles each, 256 KB of weights - half in
    // LDS, half in registers.  Two uses: (1) B <= 16 with CTCASR_RNN_HALF_CHIP (128 CUs stay free
    // for the next layer's input projection); (2) B = 17..32: the two 16-row batch tiles are
    // independent recurrences, so each gets its own half of the chip and its own barrier in ONE
    // launch of 2 x 128 workgroups - 6.0 us per step against 7.3 for the kernel that walks both
    // tiles behind one barrier (and 8.7 for two chains inside every workgroup: the in-order
    // memory queue of a CU makes one chain's bulk loads delay the other's publish / poll; the
    // same two chains on HALF the chip - 64 columns per workgroup, 34 fragment registers, for a
    // pipelined input projection at B = 32 - run 11.3 us per step: publish 4.0, arrive 1.1).
    if (cell == CTCASR_CELL_LSTM && ((fwd_half_chip && mt == 1) || (mt == 2 && !one_barrier))) {
        p.nwg = 64;
        return launch_persistent(prnn_fwd_kernel<CTCASR_CELL_LSTM, 4, 16, 1, 32>, p,
                                 (size_t)4 * 32 * 64 * 16 + (size_t)4 * 4 * 16 * 17 * 4 + 32,
                                 s, 1, mt);
    }
    if (cell == CTCASR_CELL_LSTM) {
        if (mt == 1) { PRNN_FWD(CTCASR_CELL_LSTM, 2, 16, 1); }
        PRNN_FWD(CTCASR_CELL_LSTM, 2, 16, 2);
    }
    if (cell == CTCASR_CELL_RNN_RELU) {
        if (mt == 1) { PRNN_FWD(CTCASR_CELL_RNN_RELU, 1, 32, 1); }
        PRNN_FWD(CTCASR_CELL_RNN_RELU, 1, 32, 2);
    }
    if (mt == 1) { PRNN_FWD(CTCASR_CELL_RNN_TANH, 1, 32, 1); }
    PRNN_FWD(CTCASR_CELL_RNN_TANH, 1, 32, 2);
#undef PRNN_FWD
}

int prnn_bwd(int cell, const float *dy, const float *y, const float *w_hh_t,
             const int32_t *seq_len, int T, int B, int BS, int H, const float *gates,
             const float *cells, float *dxw, float *drec, float *dbias, unsigned *colmax,
             void *sync, void *kp, void *xchg, float *carry, int step_begin, int step_end,
             int flags, hipStream_t s) {
    PArgs p = {};
    p.dbias = dbias;
    p.s_lo = step_begin; p.s_hi = step_end; p.carry = carry;
    p.xchg = reinterpret_cast<float *>(xchg);
    p.w = w_hh_t; p.seq_len = seq_len; p.y = const_cast<float *>(y); p.dy = dy; p.dxw = dxw;
    p.drec = drec;
    p.gates = const_cast<float *>(gates); p.cells = const_cast<float *>(cells);
    p.sync = reinterpret_cast<SyncWords *>(sync);
    // backward default: half of the chip (measured faster than the whole-chip variant even
    // without GEMMs beside it)
    const bool half_chip = (flags & CTCASR_RNN_WHOLE_CHIP) == 0;
    p.T = T; p.B = B; p.BS = BS; p.H = H;
    p.ndir = 2; p.dir0 = 0; p.chain0 = 0;
    p.nwg = cell == CTCASR_CELL_LSTM ? (half_chip ? H / 16 : H / 8) : (half_chip ? H / 32 : H / 16);
    p.prof = getenv("CTCASR_RNN_PROF") != nullptr;
    p.ticket = ((unsigned)flags >> 8) & 0xFFFFFFu;
    p.xcd_split = (flags & CTCASR_RNN_XCD_SPLIT) != 0;
    const int mt = (B + 15) / 16;
    // batches of 17..32 rows = two independent 16-row tiles (see ChainSync):
    //   half of the chip: two chains inside every workgroup (8 waves): LSTM 11.0 us per step
    //     against 12.1 for the kernel that walks both tiles behind one barrier;
    //   whole chip: each tile as its own group of half-chip workgroups (2 x 128 in one launch),
    //     7.1 us per step against 14.0.
    // (The two chains of a workgroup share the CU's in-order vector-memory queue: the bulk
    // exchange loads of one chain sit in front of the other's latency-critical publish stores,
    // arrival atomic and poll loads.  More loads in flight per chain - PRNN_CHAIN_LB 8 with
    // PRNN_CHAIN_REGW 28 to stay spill-free - shorten the load + MFMA phase, 6.8 -> 5.1 us, and
    // lengthen publish + wait by as much, 4.1 -> 6.1 us: 11.8 us per step against 11.3.)
    const bool chains = mt == 2 && !(flags & CTCASR_RNN_ONE_BARRIER);
#define PRNN_BWD(CELL_, QW_, MT_, LB_, UPB_, REGW_, CH_, TG_)                                  \
    return launch_persistent(prnn_bwd_kernel<CELL_, QW_, MT_, LB_, UPB_, REGW_, CH_>, p,        \
                             (size_t)4 * (QW_ - REGW_) * (UPB_ == 8 ? 32 : 64) * 16 +          \
                                 (size_t)CH_ * (4 * (UPB_ == 32 ? 2 : 1) * MT_ * 16 * 17 * 4 + \
                                                16) + 16, s, CH_, TG_)
    if (cell == CTCASR_CELL_GRU && H == 2048) {
        // like the LSTM at H = 2048: 8 units x 6144 x 4 B = 192 KB per workgroup = 128 KB LDS +
        // 128 registers per lane (half tiles), one direction per launch
        p.nwg = 256; p.ndir = 1;
        for (int tile = 0; tile < mt; ++tile)
            for (int dir = 0; dir < 2; ++dir) {
                p.chain0 = tile; p.dir0 = dir;
                const int rc = launch_persistent(
                    prnn_bwd_kernel<CTCASR_CELL_GRU, 96, 1, 8, 8, 32>, p,
                    (size_t)4 * 64 * 32 * 16 + (size_t)4 * 16 * 17 * 4 + 32, s);
                if (rc != CTCASR_OK) return rc;
            }
        return CTCASR_OK;
    }
    if (cell == CTCASR_CELL_GRU) {
        // H = 1024, 16 units x 3072 x 4 B = 192 KB per workgroup (128 KB LDS + 64 registers),
        // 64 workgroups per direction; B > 16: two chains per workgroup (half of the chip) or one
        // group of workgroups per batch tile (whole chip)
        p.nwg = H / 16;
        if (chains && !half_chip) { PRNN_BWD(CTCASR_CELL_GRU, 48, 1, 16, 16, 16, 1, 2); }
        if (mt == 1) { PRNN_BWD(CTCASR_CELL_GRU, 48, 1, 16, 16, 16, 1, 1); }
        if (chains) { PRNN_BWD(CTCASR_CELL_GRU, 48, 1, 8, 16, 16, 2, 1); }
        PRNN_BWD(CTCASR_CELL_GRU, 48, 2, 8, 16, 16, 1, 1);
    }
    if ((flags & CTCASR_RNN_F16) && cell == CTCASR_CELL_RNN_RELU && H == PRNN_R16_H && mt == 1 &&
        !seq_len) {
        p.nwg = PRNN_R16_H / 32;
        p.colmax = colmax;
        p.rs = reinterpret_cast<float *>(reinterpret_cast<char *>(p.xchg) +
                                         prnn_step_exchange_bytes(T, B, H, 1));
        const size_t lds = (size_t)4 * 32 * 64 * 16 + (size_t)4 * 2 * 16 * 17 * 4 +
                           (size_t)4 * 64 * 16 + 64;
        return launch_persistent(prnn_relu16_kernel<true>, p, lds, s);
    }
    if (cell == CTCASR_CELL_LSTM && H == PRNN_W16_H && (flags & CTCASR_RNN_F16)) {
        // fp16 matrix pipe (round 5): the same geometry as the fp32 kernel below - 256 workgroups
        // of 8 units, one direction and one 16-row tile per launch
        p.nwg = 256; p.ndir = 1;
        p.colmax = colmax;
        p.rs = reinterpret_cast<float *>(reinterpret_cast<char *>(p.xchg) +
                                         prnn_step_exchange_bytes(T, B, H, 4));
        const size_t lds = (size_t)4 * 64 * 32 * 16 + (size_t)4 * 16 * 17 * 4 +
                           (size_t)4 * 256 * 16 + 64;
        const bool pairs = (flags & CTCASR_RNN_KPAIR) != 0;
        p.kp = reinterpret_cast<unsigned *>(kp);
        for (int tile = 0; tile < mt; ++tile)
            for (int dir = 0; dir < 2; ++dir) {
                p.chain0 = tile; p.dir0 = dir;
                const int rc = pairs
                    ? launch_persistent(prnn_bwd16w_kernel<PRNN_W16_KD, PRNN_W16_KS>, p, lds, s)
                    : launch_persistent(prnn_bwd16w_kernel<PRNN_W16_D>, p, lds, s);
                if (rc != CTCASR_OK) return rc;
            }
        return CTCASR_OK;
    }
    if (cell == CTCASR_CELL_LSTM && H == 2048) {
        // 8 units per workgroup (half MFMA tiles: 16 units would be 512 KB of weights), 256
        // workgroups = the whole chip for ONE direction; 8 x 8192 x 4 B = 256 KB per workgroup =
        // 128 KB LDS + 256 registers per lane.  Directions / batch tiles one after the other.
        p.nwg = 256; p.ndir = 1;
        for (int tile = 0; tile < mt; ++tile)
            for (int dir = 0; dir < 2; ++dir) {
                p.chain0 = tile; p.dir0 = dir;
                const int rc = launch_persistent(
                    prnn_bwd_kernel<CTCASR_CELL_LSTM, 128, 1, 8, 8, 64>, p,
                    (size_t)4 * 64 * 32 * 16 + (size_t)4 * 16 * 17 * 4 + 32, s);
                if (rc != CTCASR_OK) return rc;
            }
        return CTCASR_OK;
    }
    if (cell == CTCASR_CELL_LSTM && H == PRNN_B16_H && (flags & CTCASR_RNN_F16)) {
        // fp16 matrix pipe: 64 workgroups per direction, ONE chain of 4 waves; B > 16 on half of
        // the chip: both 16-row tiles in every workgroup (one barrier); on the whole chip: each
        // tile as its own group of workgroups
        p.nwg = PRNN_B16_NWG;
        p.colmax = colmax;
        p.rs = reinterpret_cast<float *>(reinterpret_cast<char *>(p.xchg) +
                                         prnn_step_exchange_bytes(T, B, H, 4));
        auto lds = [](int tiles, int waves) {
            return (size_t)128 * 1024 + (size_t)waves * tiles * 16 * 17 * 4 +
                   (size_t)tiles * 256 * 16 + 64;      // (inverse scales: 4 float4 per producer)
        };
        // The staggered kernel publishes tile 1's rows of a step AFTER tile 0's rows of that step
        // have been read: the two must not share a cache line, or the reader's L1 / L2 keeps tile
        // 1's bytes as they were when the line came in for tile 0 (round 6: a K-pair form of this
        // kernel, since removed, read the pass before at B = 17 .. 20; the staggered kernel was
        // never caught, but nothing but the volume of its other loads protects it).  A k group's
        // rows are B x 16 bytes in the exchange buffer: tile 1 starts on a 128-byte line when B is
        // a multiple of 8 - other batches keep the one-barrier kernel.
        // (The inverse scales of a producer share ONE line for both tiles at every B: the
        // staggered kernel reads them past the caches.)
        // CTCASR_RNN_KPAIR has no form at this H and is ignored.
        const bool tiles_apart = B % 8 == 0;
        if (mt == 2 && half_chip && (flags & CTCASR_RNN_STAGGER) && !seq_len && tiles_apart) {
            if (p.prof)
                return launch_persistent(
                    prnn_bwd16s_kernel<PRNN_B16S_D, PRNN_B16S_JW, PRNN_B16S_JP, PRNN_B16S_JA, true>,
                    p, lds(2, 4), s);
            return launch_persistent(
                prnn_bwd16s_kernel<PRNN_B16S_D, PRNN_B16S_JW, PRNN_B16S_JP, PRNN_B16S_JA>, p,
                lds(2, 4), s, 1, PRNN_B16S_XCD_EXCL ? 2 : 1);
        }
        if (mt == 2 && half_chip)
            return launch_persistent(prnn_bwd16_kernel<2, PRNN_B16_NW2, PRNN_B16_D2>, p, lds(2, PRNN_B16_NW2), s, PRNN_B16_NW2 / 4);
        return launch_persistent(prnn_bwd16_kernel<1, 4, PRNN_B16_D1>, p, lds(1, 4), s, 1, mt);
    }
    if (cell == CTCASR_CELL_LSTM) {
        if (chains && !half_chip) {
            p.nwg = H / 16;
            PRNN_BWD(CTCASR_CELL_LSTM, 64, 1, 16, 16, 32, 1, 2);
        }
        if (half_chip) {
            if (mt == 1) { PRNN_BWD(CTCASR_CELL_LSTM, 64, 1, 16, 16, 32, 1, 1); }
            if (chains) { PRNN_BWD(CTCASR_CELL_LSTM, 64, 1, PRNN_CHAIN_LB, 16, PRNN_CHAIN_REGW, 2, 1); }
            PRNN_BWD(CTCASR_CELL_LSTM, 64, 2, 8, 16, 32, 1, 1);
        }
        if (mt == 1) { PRNN_BWD(CTCASR_CELL_LSTM, 64, 1, 32, 8, 0, 1, 1); }
        PRNN_BWD(CTCASR_CELL_LSTM, 64, 2, 16, 8, 0, 1, 1);
    }
    // plain RNN, H = 2048, half of the chip: 32 units (two N tiles) x 2048 x 4 B = 256 KB per
    // workgroup, split between LDS and registers like the LSTM's; 64 workgroups per direction
    if (cell == CTCASR_CELL_RNN_RELU) {
        if (chains && !half_chip) {
            p.nwg = H / 32;
            PRNN_BWD(CTCASR_CELL_RNN_RELU, 64, 1, 16, 32, 32, 1, 2);
        }
        if (half_chip) {
            if (mt == 1) { PRNN_BWD(CTCASR_CELL_RNN_RELU, 64, 1, 16, 32, 32, 1, 1); }
            if (chains) { PRNN_BWD(CTCASR_CELL_RNN_RELU, 64, 1, 8, 32, 32, 2, 1); }
            PRNN_BWD(CTCASR_CELL_RNN_RELU, 64, 2, 8, 32, 32, 1, 1);
        }
        // 16 units x 2048 x 4 B = 128 KB per workgroup, 128 per direction
        if (mt == 1) { PRNN_BWD(CTCASR_CELL_RNN_RELU, 32, 1, 32, 16, 0, 1, 1); }
        PRNN_BWD(CTCASR_CELL_RNN_RELU, 32, 2, 16, 16, 0, 1, 1);
    }
    if (chains && !half_chip) {
        p.nwg = H / 32;
        PRNN_BWD(CTCASR_CELL_RNN_TANH, 64, 1, 16, 32, 32, 1, 2);
    }
    if (half_chip) {
        if (mt == 1) { PRNN_BWD(CTCASR_CELL_RNN_TANH, 64, 1, 16, 32, 32, 1, 1); }
        if (chains) { PRNN_BWD(CTCASR_CELL_RNN_TANH, 64, 1, 8, 32, 32, 2, 1); }
        PRNN_BWD(CTCASR_CELL_RNN_TANH, 64, 2, 8, 32, 32, 1, 1);
    }
    if (mt == 1) { PRNN_BWD(CTCASR_CELL_RNN_TANH, 32, 1, 32, 16, 0, 1, 1); }
    PRNN_BWD(CTCASR_CELL_RNN_TANH, 32, 2, 16, 16, 0, 1, 1);
#undef PRNN_BWD
}

// Where prnn_bwd16_kernel keeps what it publishes, for the block-scaled data-gradient kernel that
// reads it after the pass (csrc/dgrad16.hip): the exchange blocks (the all-zero block first, then
// one per step) and the inverse scales, of a pass over T steps of B <= 32 rows.
// (``exchange``: the exchange region of the pass's row block, rnn_step.hip:
// rnn_workspace_xchg_block0)
int prnn_b16_published(const void *exchange, int T, int B, int H, const char **xchg,
                       const float **scales) {
    if (!exchange || H != PRNN_B16_H || B < 1 || B > PRNN_BLOCK_ROWS || T < 1)
        return CTCASR_ERR_BAD_ARGUMENT;
    const char *x = reinterpret_cast<const char *>(exchange);
    *xchg = x;
    *scales = reinterpret_cast<const float *>(x + prnn_step_exchange_bytes(T, B, H, 4));
    return CTCASR_OK;
}

size_t prnn_error_offset() { return offsetof(SyncWords, error); }

// Bytes of a row block's K-pair hand-off words (KPairWords + the tagged slots; 0 for shapes
// without them).  `total` must last from launch to launch - its parity is the tag base - so they
// sit in the workspace's control header, at an offset that does not move with T (rnn_step.hip);
// after a time-out their write counts are undefined and ctcasr_rnn_poll_error zero-fills them
// with the barrier words.
size_t prnn_kp_region_bytes(int H, int G) {
    if (G == 4 && H == PRNN_W16_H) return prnn_w16_kp_bytes();
    return 0;
}

int prnn_resident_gate(void *sync, unsigned ticket, int max_wait_us, hipStream_t s) {
    resident_gate_kernel<<<1, 1, 0, s>>>(reinterpret_cast<SyncWords *>(sync), ticket & 0xFFFFFFu,
                                         (unsigned long long)max_wait_us * 100ull);
    return ctcasr_launch_status();
}

// Which non-default tuning / probe macros this library was compiled with (include/ctcasr.h).
unsigned dgrad16_build_flags();     // (dgrad16.hip)
extern "C" unsigned ctcasr_build_flags(void) {
    unsigned flags = dgrad16_build_flags();
    if (PRNN_PROBE_HALF_LOADS) flags |= CTCASR_BUILD_PROBE_WRONG_RESULTS;
    if (PRNN_GROUPS != 8 || PRNN_XCD_AWARE != 0 || PRNN_CHAIN_LB != 4 || PRNN_CHAIN_REGW != 32 ||
        PRNN_CHAIN0_PRIO != 1 || PRNN_POLL_SLEEP != 1 ||
        PRNN_XCD_TILE_PAIRS != 1 || PRNN_B16S_D != 8 || PRNN_B16S_JW != 7 || PRNN_B16S_JP != 5 ||
        PRNN_B16S_JA != 1 || PRNN_B16S_XCD_EXCL != 0 || PRNN_W16_D != 12 ||
        PRNN_W16_KD != 12 || PRNN_W16_KS != 2)
        flags |= CTCASR_BUILD_NONDEFAULT_TUNING;
    return flags;
}
