// K10: CTC beam search on the GPU with the semantics of TensorFlow 1.12's CTCBeamSearchDecoder
// (merge_repeated=False; the top path, or the top_paths best leaves of the final beam with
// NBEST) as called by CTCModel.decode_fn (asr/model.py:292-296).
//
// One workgroup per utterance; the beam (<= 1024 leaves) lives in LDS.  Per frame:
//   1. all threads: normalise the frame, copy new -> old, update every leaf from its own and its
//      parent's old probabilities (TensorFlow's first loop is embarrassingly parallel);
//   2. all threads: a bitonic sort of the leaves by OLD total (descending: TensorFlow's branch
//      order);
//   3. wave 0: TensorFlow's second loop, literally - branches in order, children in symbol order,
//      a bounded set of the W best leaves whose bottom is replaced when a child beats it
//      (`beam_expand`: the set's keys live in registers, the bottom is a wave-wide minimum).
// The serial part is kept because TensorFlow's result is order dependent in one corner: a leaf
// that is pushed out of the heap and then re-proposed (and rejected) by its still-active parent
// before its own turn has its old probabilities wiped and does not expand in this frame.  That
// is tracked with per-leaf eviction / expansion event numbers instead of mutable tree state.
// The prefix tree (parent, label, children table, beam slot per node) lives in HBM so that a
// prefix that leaves the beam and re-enters later is the same node, like TensorFlow's BeamEntry.
// Ties in total are broken towards the older tree node (TensorFlow leaves them to gtl::TopN /
// std::sort); node ages can differ from the CPU oracle's, so exact ties are not a parity case.
// LM = true fuses a language model in where TensorFlow calls its BeamScorer (`BeamLm` below:
// ExpandState / GetStateExpansionScore in both loops, GetStateEndExpansionScore at the end);
// LM = false compiles all of it out and is the search as it was.
// K24: the scorer is a policy, `LM` its number - 0 none, 1 the dense automaton, 2 a word n-gram
// over a lexicon trie (`BeamWordLm`): the same search, the same places where the scorer enters; only
// where an edge's score and state come from differs.
// K26: 3 is the word n-gram with look-ahead - the trie node's table entry `la` is charged on
// entering the node and settled at the space; the states, the contexts and the memo are K24's.
#include "common.h"

#define BEAM_THREADS 256
#define BEAM_MAX_WIDTH 1024
#define BEAM_SLOTS (2 * BEAM_MAX_WIDTH)   // live leaves + leaves evicted but still due to expand
#define BEAM_MAX_CLASSES 64

namespace {

__device__ __forceinline__ float lse2f(float a, float b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    return hi + log1pf(expf(lo - hi));
}
__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ int gload(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void gstore(int *p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct BeamLds {
    // per slot
    int node[BEAM_SLOTS], label[BEAM_SLOTS], parent[BEAM_SLOTS], pslot[BEAM_SLOTS];
    float o_total[BEAM_SLOTS], o_blank[BEAM_SLOTS];
    float n_total[BEAM_SLOTS], n_blank[BEAM_SLOTS], n_label[BEAM_SLOTS];
    unsigned long long kids_in_beam[BEAM_SLOTS];   // bit c: child c of this leaf is in the heap
    short alive[BEAM_SLOTS], was_alive[BEAM_SLOTS], expanded[BEAM_SLOTS];
    int bidx[BEAM_SLOTS], evict_time[BEAM_SLOTS];
    // per beam position
    int heap[BEAM_MAX_WIDTH], branches[BEAM_MAX_WIDTH];
    unsigned long long sort_a[BEAM_MAX_WIDTH];
    int freelist[BEAM_SLOTS];
    float x[BEAM_MAX_CLASSES];
    int misc[8];   // 0 nheap, 1 node count, 2 nfree
};
// ... with a language model: the automaton state of each leaf and the expansion score of the edge
// that leads to it, both constants of the leaf's tree node.  They trail the plain layout, so the
// search without a model addresses LDS exactly as before; 160 032 of the CU's 163 840 bytes.
struct BeamLdsLm : BeamLds {
    int lm_state[BEAM_SLOTS];
    float lm_e[BEAM_SLOTS];
};
template <int LM> struct BeamLdsOf { typedef BeamLdsLm type; };   // LM 1, 2, 3
template <> struct BeamLdsOf<0> { typedef BeamLds type; };

// The scorer of the fused search: a deterministic weighted automaton over label ids, TensorFlow's
// BeamScorer with an integer state.  Entering label c in state s costs score[s * C + c] (the
// expansion score, -inf: no such edge) and leads to next[s * C + c]; a hypothesis that ends in s
// gets final[s] (NULL: nothing).  States read from `next` are clamped into [0, S), so the tables
// are never indexed outside themselves, whatever they hold.
struct BeamLm {
    const int *next;
    const float *score;
    const float *final;
    int states;
};

// K24, the implicit scorer: the automaton is the composition of a lexicon trie with the contexts of
// a back-off word n-gram, far too large to tabulate.  A leaf's state is the pair (trie node,
// context).  The trie node is `lm_state` of the leaf's slot; the context is a constant of the
// leaf's tree node and lives in the workspace (`pool_ctx`), next to the memo of the node's space
// edge (`pool_sp_ctx` < 0: not computed yet; `pool_sp_score`: its float bits) - LDS has no room
// for a second int per slot.  The three pool pointers are part of the struct so that the kernel's
// arguments are those of the dense scorer's kernel; the host fills them in from the workspace.
// Every index read from a table is clamped into its array.
struct BeamWordLm {
    const int *trie_next;            // [nodes, C]  -1: no edge; node 0 the root, 1 the OOV sink
    const int *trie_word;            // [nodes]     word id that ends here, or -1
    const long long *ctx_begin;      // [contexts + 1]
    const int *succ_word;            // [succ]      ascending inside a context's range
    const double *succ_lp;           // [succ]
    const int *succ_ctx;             // [succ]
    const double *ctx_backoff;       // [contexts]
    const int *ctx_parent;           // [contexts]
    long long succ;
    int nodes, contexts, order, space;
    double bonus, oov;               // oov -inf: closed vocabulary
    long long *stats;                // NULL or [B, 2]: branches expanded, space edges looked up
    int *pool_ctx, *pool_sp_ctx, *pool_sp_score;
};
// K26: the same tables plus the look-ahead table of the trie.  A leaf's `la` is a function of its
// trie node, which is `lm_state` of its slot: nothing per slot or per tree node is added.  No index
// is derived from `la`.
struct BeamWordLmLa : BeamWordLm {
    const double *la;                // [nodes]
};
template <int LM> struct BeamLmOf { typedef BeamLm type; };
template <> struct BeamLmOf<2> { typedef BeamWordLm type; };
template <> struct BeamLmOf<3> { typedef BeamWordLmLa type; };

// the scorer as one utterance sees it: the word model's pools start at the utterance's first node
__device__ __forceinline__ const BeamLm &lm_of_row(const BeamLm &lm, size_t) { return lm; }
__device__ __forceinline__ BeamWordLm lm_of_row(BeamWordLm lm, size_t first) {
    lm.pool_ctx += first;
    lm.pool_sp_ctx += first;
    lm.pool_sp_score += first;
    return lm;
}
__device__ __forceinline__ BeamWordLmLa lm_of_row(BeamWordLmLa lm, size_t first) {
    lm.pool_ctx += first;
    lm.pool_sp_ctx += first;
    lm.pool_sp_score += first;
    return lm;
}

#define WORDLM_MAX_ORDER 5
#define WORDLM_MAX_PROBES 11     // 64-way narrowing of a range below 2^63 to <= 64 entries

// Wd(h, w), by a whole wave (all 64 lanes active, every argument wave-uniform): search h's
// successor range for w; found: acc += succ_lp, done; else acc += ctx_backoff[h], h = ctx_parent[h],
// again - at most `order` searches, each of at most WORDLM_MAX_PROBES + 1 probes (64 pivots per
// probe: one coalesced-ish load per step instead of six dependent ones of a one-lane bisection).
// Tables that would run longer give -inf (and context 0).  The adds are in fp64, in that order.
__device__ double wordlm_wd(const BeamWordLm &m, int h, int w, int lane, int &next_ctx) {
    double acc = 0.0;
    next_ctx = 0;
    h = min(max(h, 0), m.contexts - 1);
    for (int it = 0; it < m.order; ++it) {
        long long lo = min(max(m.ctx_begin[h], 0ll), m.succ);
        long long hi = min(max(m.ctx_begin[h + 1], lo), m.succ);
        for (int probe = 0; probe < WORDLM_MAX_PROBES && hi - lo > 64; ++probe) {
            const long long step = (hi - lo + 63) / 64;
            const long long p = lo + lane * step;
            const int k = __popcll(__ballot(p < hi && m.succ_word[p] <= w));
            if (k == 0) { hi = lo; break; }        // w is below the range's first word
            const long long first = lo + (k - 1) * step;     // the last pivot <= w
            hi = min(first + step, hi);
            lo = first;
        }
        if (hi - lo > 64) return -INFINITY;
        const long long p = lo + lane;
        const unsigned long long hit = __ballot(p < hi && m.succ_word[p] == w);
        if (hit) {
            const long long at = lo + (__ffsll((long long)hit) - 1);
            acc += m.succ_lp[at];
            next_ctx = min(max(m.succ_ctx[at], 0), m.contexts - 1);
            return acc;
        }
        acc += m.ctx_backoff[h];
        h = min(max(m.ctx_parent[h], 0), m.contexts - 1);
    }
    return -INFINITY;
}

// The score of the word that trie node n closes in context h, without the bonus, and the context
// after it: Wd(h, w) for a vocabulary word; with OOV on Wd(h, <unk>) in the sink and Wd(h, <unk>) +
// oov anywhere else; -inf where nothing closes (the root: a leading or doubled space).  `walks`
// counts the back-off walks actually run (for `stats`).
__device__ double wordlm_close(const BeamWordLm &m, int n, int h, int lane, int &ctx, int &walks) {
    ctx = 0;
    if (n == 0) return -INFINITY;
    const int w = n == 1 ? -1 : m.trie_word[n];
    if (w >= 0) { ++walks; return wordlm_wd(m, h, w, lane, ctx); }
    if (!(m.oov > -INFINITY)) return -INFINITY;
    ++walks;
    const double d = wordlm_wd(m, h, 0, lane, ctx);
    return n == 1 ? d : d + m.oov;
}

// The end score of a hypothesis in (n, h): at the root Wd(h, </s>); where n closes a word that
// word's score (no bonus) + Wd(ctx', </s>); else -inf.  fp64, rounded once.
__device__ float wordlm_end(const BeamWordLm &m, int n, int h, int lane) {
    int ctx, walks = 0;
    if (n == 0) return (float)wordlm_wd(m, h, 1, lane, ctx);
    const double d = wordlm_close(m, n, h, lane, ctx, walks);
    if (!(d > -INFINITY)) return -INFINITY;
    int unused;
    return (float)(d + wordlm_wd(m, ctx, 1, lane, unused));
}

// K26: what the word that n closes costs in full - K24's, but the sink's word carries oov too (the
// edge into the sink charged la[1] - la[n] instead of it) -, and the end score that settles la[n].
__device__ double wordlm_close_la(const BeamWordLmLa &m, int n, int h, int lane, int &ctx,
                                  int &walks) {
    const double d = wordlm_close(m, n, h, lane, ctx, walks);
    return n == 1 ? d + m.oov : d;
}
__device__ float wordlm_end_la(const BeamWordLmLa &m, int n, int h, int lane) {
    int ctx, walks = 0;
    if (n == 0) return (float)wordlm_wd(m, h, 1, lane, ctx);
    const double d = wordlm_close_la(m, n, h, lane, ctx, walks);
    if (!(d > -INFINITY)) return -INFINITY;
    int unused;
    return (float)((d - m.la[n]) + wordlm_wd(m, ctx, 1, lane, unused));
}

// a ranks below b in the heap order (lower total; equal totals: the younger node)
__device__ __forceinline__ bool worse(const BeamLds &L, int a, int b) {
    if (L.n_total[a] != L.n_total[b]) return L.n_total[a] < L.n_total[b];
    return L.node[a] > L.node[b];
}

// heap-order key of a slot: ascending = worse first (lower total; equal totals: the younger node)
__device__ __forceinline__ unsigned long long heap_key(float total, int node, int slot) {
    const unsigned nd = min((unsigned)node, 0x1fffffu);
    return ((unsigned long long)order_key(total) << 32) | ((0x1fffffu - nd) << 11) | (unsigned)slot;
}
__device__ __forceinline__ float key_total(unsigned long long key) {
    const unsigned k = (unsigned)(key >> 32);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// wave-wide minimum of a u32 by DPP: four shifts within the rows of 16 lanes, then the row
// broadcasts (lane 63 ends up with the minimum of all 64 lanes); a few VALU instructions instead
// of six LDS-crossbar shuffles
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#define BEAM_DPP_MIN(ctrl, row_mask)                                                          \
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, row_mask, 0xf, false))
    BEAM_DPP_MIN(0x111, 0xf);    // row_shr:1
    BEAM_DPP_MIN(0x112, 0xf);    // row_shr:2
    BEAM_DPP_MIN(0x114, 0xf);    // row_shr:4
    BEAM_DPP_MIN(0x118, 0xf);    // row_shr:8   -> lane 15 of every row holds the row's minimum
    BEAM_DPP_MIN(0x142, 0xa);    // row_bcast:15 into rows 1 and 3
    BEAM_DPP_MIN(0x143, 0xc);    // row_bcast:31 into rows 2 and 3
#undef BEAM_DPP_MIN
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        const unsigned lo = __shfl_xor((unsigned)v, off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// ascending bitonic sort of n 64-bit keys (n padded to pow2 with ~0ull), all threads
// (NBEST: a copy per kind of kernel, for the reason given at `beam_expand`)
template <bool NBEST>
__device__ void bitonic_sort(unsigned long long *keys, int n_pow2, int tid) {
    for (int k = 2; k <= n_pow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n_pow2; i += BEAM_THREADS) {
                const int partner = i ^ j;
                if (partner > i) {
                    const unsigned long long a = keys[i], b = keys[partner];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[partner] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// TensorFlow's second loop for one frame, run by ONE wave: branches in order, children in symbol
// order, a bounded set of the W best leaves whose worst member is replaced when a child beats it.
// TensorFlow keeps that set in a min-heap; only its bottom is ever looked at, so here the set is
// unordered - position p = k * 64 + lane of L.heap[] belongs to `lane`, which keeps the member's
// heap key and what an eviction needs to know about it (parent slot, label, "was in the beam
// when the frame began") in registers k - and the bottom is a wave-wide minimum of the keys,
// recomputed after every insertion.  One wave runs a long dependent instruction stream here, so
// the insertion path avoids LDS round trips: values cross lanes with v_readlane (the lane index
// is a ballot result), the read-modify-writes of the children masks are LDS atomics without
// return, an evicted transient hands its slot straight to the child that pushed it out, the next
// free slot and the next branch's children row (tree nodes, global memory) are fetched one
// step ahead.  A serial sift through an LDS heap cost ~2 us per insertion; this ~0.4.
// LM: lane c also holds the model's edge (branch, c) - its score and the state it leads to, one
// coalesced row load each per branch, fetched one branch ahead like the children row - and a
// child's value is x[c] + (prev + score): TensorFlow's GetStateExpansionScore.  An edge of -inf
// is no candidate and creates no node.
// LM == 2: lane c holds the trie's edge (branch's node, c) instead - one coalesced row load -, the
// space's lane the memo of the branch's tree node; the context and the memo come from the
// workspace one branch ahead too.  The memo is filled by the whole wave on the node's first
// expansion (`wordlm_close`: a chain of dependent loads, run once per tree node, not per frame).
// LM == 3: as LM == 2, but the non-space lanes' scores are (la[target] - la[node]) + bonus, finished
// in the prefetch, and the memo holds the space edge less la[node] (`wordlm_close_la`).
// NBEST changes nothing here: it gives the n-best kernels copies of their own, so that the
// inliner sees the top-1 kernels' callees exactly as it did before there were four kernels.
template <int PER, int LM, bool NBEST>
__device__ void beam_expand(typename BeamLdsOf<LM>::type &L, int lane, int W, int C, int blank,
                            int nslots, int nheap0, int *pool_parent, int *pool_label,
                            int *pool_children, int nodes_per_utt,
                            const typename BeamLmOf<LM>::type &lm) {
    int nheap = nheap0, nfree = 0, nodes = L.misc[1];
    for (int base = 0; base < nslots; base += 64) {      // free slots, ordered
        const bool is_free = base + lane < nslots && !L.alive[base + lane];
        const unsigned long long m = __ballot(is_free);
        if (is_free)
            L.freelist[nfree + __popcll(m & ((1ull << lane) - 1ull))] = base + lane;
        nfree += __popcll(m);
    }
    unsigned long long hk[PER];
    unsigned hm[PER];        // parent slot (0xfff: none) | label << 12 | was_alive << 18
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int pos = k * 64 + lane;
        hk[k] = ~0ull;
        hm[k] = 0;
        if (pos < nheap) {
            const int s = L.heap[pos];
            hk[k] = heap_key(L.n_total[s], L.node[s], s);
            hm[k] = ((unsigned)L.pslot[s] & 0xfffu) | (((unsigned)L.label[s] & 0x3fu) << 12) |
                    ((unsigned)(L.was_alive[s] != 0) << 18);
        }
    }
    // the worst leaf of the beam: key, owning lane (valid when nheap > 0)
    unsigned long long bkey = ~0ull;
    int owner = 0;
    auto find_bottom = [&]() {
        unsigned long long m = hk[0];
#pragma unroll
        for (int k = 1; k < PER; ++k) m = hk[k] < m ? hk[k] : m;
        // the total's 32 bits decide almost always; exact ties go the long way
        const unsigned hi = (unsigned)(m >> 32), best = wave_min_u32(hi);
        unsigned long long tied = __ballot(hi == best);
        if (tied & (tied - 1)) {
            bkey = wave_min_u64(m);
            tied = __ballot(m == bkey);
        }
        owner = __ffsll((long long)tied) - 1;
        bkey = ((unsigned long long)best << 32) |
               (unsigned)__builtin_amdgcn_readlane((int)(unsigned)m, owner);
    };
    find_bottom();
    float btot = key_total(bkey);
    int free_top = nfree > 0 ? L.freelist[nfree - 1] : -1;      // next free slot, read ahead

    // the children rows (tree nodes of a branch's children) are read one branch ahead: the
    // global-memory round trip would otherwise sit in front of every branch's first insertion
    int kid_next = -1;
    if (nheap0 > 0 && lane < C)
        kid_next = gload(&pool_children[(size_t)L.node[L.branches[0]] * C + lane]);
    // the model's rows of a branch's state, likewise (the blank's column is never read)
    float lms_next = -INFINITY;
    int lmn_next = 0;
    // LM >= 2: the branch's trie node, context and space-edge memo (context < 0: not computed)
    int wn_next = 0, wh_next = 0, wsc_next = 0, wss_next = 0;
    double wla_next = 0.0;      // LM == 3: la[the branch's trie node]
    int n_expanded = 0, n_lookups = 0;
    auto lm_fetch = [&](int slot) {
        if constexpr (LM == 1) {
            if (lane < C && lane != blank) {
                const size_t at = (size_t)L.lm_state[slot] * C + lane;
                lms_next = lm.score[at];
                lmn_next = min(max(lm.next[at], 0), lm.states - 1);
            }
        }
        if constexpr (LM == 2) {
            const int node = L.node[slot];
            wn_next = L.lm_state[slot];
            wh_next = gload(&lm.pool_ctx[node]);
            wsc_next = gload(&lm.pool_sp_ctx[node]);
            wss_next = gload(&lm.pool_sp_score[node]);
            lmn_next = -1;
            if (lane < C && lane != blank && lane != lm.space && wn_next != 1)
                lmn_next = min(max(lm.trie_next[(size_t)wn_next * C + lane], -1), lm.nodes - 1);
        }
        if constexpr (LM == 3) {
            // K26: the non-space lanes' edges are finished here, one branch ahead - state and
            // score -, so that the gather of la[target] is not in front of the branch's first
            // insertion.  la[wn] is one address for the wave (a scalar load).
            const int node = L.node[slot];
            wn_next = __builtin_amdgcn_readfirstlane(min(max(L.lm_state[slot], 0), lm.nodes - 1));
            wh_next = gload(&lm.pool_ctx[node]);
            wsc_next = gload(&lm.pool_sp_ctx[node]);
            wss_next = gload(&lm.pool_sp_score[node]);
            wla_next = lm.la[wn_next];
            lmn_next = 1;
            lms_next = -INFINITY;
            if (lane < C && lane != blank && lane != lm.space) {
                if (wn_next == 1) {
                    lms_next = (float)lm.bonus;
                } else {
                    const int m = min(max(lm.trie_next[(size_t)wn_next * C + lane], -1),
                                      lm.nodes - 1);
                    lmn_next = m >= 0 ? m : 1;
                    if (m >= 0 || lm.oov > -INFINITY)
                        lms_next = (float)((lm.la[lmn_next] - wla_next) + lm.bonus);
                }
            }
        }
    };
    if constexpr (LM != 0) {
        if (nheap0 > 0) lm_fetch(L.branches[0]);
    }
    for (int j = 0; j < nheap0; ++j) {
        const int s = L.branches[j];
        const float ot = L.o_total[s];
        const int kidv = kid_next;           // tree nodes of this branch's children (-1: none yet)
        if (j + 1 < nheap0 && lane < C)
            kid_next = gload(&pool_children[(size_t)L.node[L.branches[j + 1]] * C + lane]);
        float lms = lms_next;                // the model's edges out of this branch's state
        int lmn = lmn_next;
        const int wn = wn_next, wh = wh_next;
        int wsc = wsc_next, wss = wss_next;
        const double wla = wla_next;
        if constexpr (LM != 0) {
            if (j + 1 < nheap0) lm_fetch(L.branches[j + 1]);
        }
        // branches come in descending old total and the bottom only rises: once a branch cannot
        // beat the bottom of a full beam, no later one can
        if (nheap == W && !(ot > btot)) break;
        if (!L.alive[s]) {
            // pushed out earlier in this frame: wiped if its parent re-proposed it since
            const int ps = L.pslot[s];
            if (ps >= 0 && L.expanded[ps] && L.evict_time[s] < L.bidx[ps] * 64 + L.label[s])
                continue;
        }
        if (!(ot > -INFINITY)) continue;
        if (lane == 0) L.expanded[s] = 1;
        if constexpr (LM == 2) {
            ++n_expanded;
            if (wsc < 0) {      // the node's first expansion: its space edge, once and for all
                const double d = wordlm_close(lm, wn, wh, lane, wsc, n_lookups);
                wss = __float_as_int((float)(d + lm.bonus));
                if (lane == 0) {
                    gstore(&lm.pool_sp_score[L.node[s]], wss);
                    gstore(&lm.pool_sp_ctx[L.node[s]], wsc);
                }
            }
            if (lane == lm.space) {
                lms = __int_as_float(wss);
                lmn = 0;
            } else if (lane < C && lane != blank) {
                if (wn == 1 || lmn >= 0) {
                    lms = (float)lm.bonus;
                    lmn = wn == 1 ? 1 : lmn;
                } else {
                    lms = lm.oov > -INFINITY ? (float)(lm.oov + lm.bonus) : -INFINITY;
                    lmn = 1;
                }
            }
        }
        if constexpr (LM == 3) {
            ++n_expanded;
            if (wsc < 0) {      // as above; the memo holds the space edge of this rule
                const double d = wordlm_close_la(lm, wn, wh, lane, wsc, n_lookups);
                wss = __float_as_int((float)((d - wla) + lm.bonus));
                if (lane == 0) {
                    gstore(&lm.pool_sp_score[L.node[s]], wss);
                    gstore(&lm.pool_sp_ctx[L.node[s]], wsc);
                }
            }
            if (lane == lm.space) {
                lms = __int_as_float(wss);
                lmn = 0;
            }
        }
        const int slabel = L.label[s];
        const unsigned long long active = L.kids_in_beam[s];
        float v = -INFINITY;
        if (lane < C && lane != blank && !((active >> lane) & 1ull)) {
            if constexpr (LM != 0) v = L.x[lane] + ((lane == slabel ? L.o_blank[s] : ot) + lms);
            else v = L.x[lane] + (lane == slabel ? L.o_blank[s] : ot);
        }
        // children that could enter right now; the bottom only rises while we insert
        unsigned long long cand = __ballot(v > -INFINITY && (nheap < W || v > btot));
        if (!cand) continue;
        const int pnode = L.node[s];
        while (cand) {
            const int c = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const float vc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), c));
            if (!(nheap < W || vc > btot)) continue;
            if (nodes + 1 >= nodes_per_utt) {     // tree pool exhausted
                if (lane == 0) L.misc[3] = 1;
                cand = 0ull;
                continue;
            }
            const bool full = nheap == W;
            int ns = -1;
            if (full) {
                // the bottom leaves the beam; a transient (a child that entered in this frame)
                // hands its slot straight to the child that pushes it out
                unsigned meta = 0;
#pragma unroll
                for (int k = 0; k < PER; ++k) meta = hk[k] == bkey ? hm[k] : meta;
                meta = (unsigned)__builtin_amdgcn_readlane((int)meta, owner);
                const int ev = (int)(bkey & 0x7ffu);
                if (lane == 0) {
                    L.alive[ev] = 0;
                    L.evict_time[ev] = j * 64 + c;
                    if ((meta & 0xfffu) != 0xfffu)
                        atomicAnd(&L.kids_in_beam[meta & 0xfffu], ~(1ull << ((meta >> 12) & 0x3fu)));
                }
                if (!((meta >> 18) & 1u)) ns = ev;
            }
            if (ns < 0) {
                ns = free_top;
                --nfree;
                free_top = nfree > 0 ? L.freelist[nfree - 1] : -1;
            }
            // node of child (s, c): reuse or create
            int kid = __builtin_amdgcn_readlane(kidv, c);
            if (kid < 0) {
                kid = nodes++;
                if (lane == 0) {
                    gstore(&pool_children[(size_t)pnode * C + c], kid);
                    gstore(&pool_parent[kid], pnode);
                    gstore(&pool_label[kid], c);
                }
                if (lane < C) gstore(&pool_children[(size_t)kid * C + lane], -1);
                if constexpr (LM >= 2) {
                    // the child's context, and a memo that says "not computed": a workspace that
                    // another launch left behind never serves a stale entry
                    if (lane == 0) {
                        gstore(&lm.pool_ctx[kid], c == lm.space ? wsc : wh);
                        gstore(&lm.pool_sp_ctx[kid], -1);
                    }
                }
            }
            if (lane == 0) {
                L.node[ns] = kid; L.label[ns] = c; L.parent[ns] = pnode; L.pslot[ns] = s;
                L.n_total[ns] = vc; L.n_label[ns] = vc; L.n_blank[ns] = -INFINITY;
                L.alive[ns] = 1; L.was_alive[ns] = 0; L.expanded[ns] = 0;
                L.kids_in_beam[ns] = 0ull;
                atomicOr(&L.kids_in_beam[s], 1ull << c);
            }
            if constexpr (LM != 0) {
                const int st = __builtin_amdgcn_readlane(lmn, c);
                const int e = __builtin_amdgcn_readlane(__float_as_int(lms), c);
                if (lane == 0) { L.lm_state[ns] = st; L.lm_e[ns] = __int_as_float(e); }
            }
            const unsigned long long nk = heap_key(vc, kid, ns);
            const unsigned nm = ((unsigned)s & 0xfffu) | ((unsigned)c << 12);
            if (full) {
#pragma unroll
                for (int k = 0; k < PER; ++k)
                    if (hk[k] == bkey) { hk[k] = nk; hm[k] = nm; L.heap[k * 64 + lane] = ns; }
            } else {
                if (lane == (nheap & 63)) {
#pragma unroll
                    for (int k = 0; k < PER; ++k)
                        if (k == (nheap >> 6)) { hk[k] = nk; hm[k] = nm; }
                    L.heap[nheap] = ns;
                }
                ++nheap;
            }
            find_bottom();
            btot = key_total(bkey);
        }
    }
    if (lane == 0) { L.misc[0] = nheap; L.misc[1] = nodes; }
    if constexpr (LM >= 2) {
        if (lane == 0) { L.misc[4] += n_expanded; L.misc[5] += n_lookups; }
    }
}

// LM = false is the search without a model: every use of `lm` is compiled out.
// NBEST = true returns the `top_paths` best leaves of the final beam instead of one (out
// [B, top_paths, T], out_len / logp [B, top_paths], n_paths [B]); the search loop is the same, and
// NBEST = false reads neither `top_paths` nor `n_paths` and is the kernel as it was.
template <int LM, bool NBEST>
__global__ void __launch_bounds__(BEAM_THREADS)
beam_decode_kernel(const float *__restrict__ logits, const int *__restrict__ seq_len, int T, int B,
                   int C, int blank, int W, int norm_mode, int *__restrict__ out,
                   int *__restrict__ out_len, float *__restrict__ logp, int *pool_parent,
                   int *pool_label, int *pool_slot, int *pool_children, int nodes_per_utt,
                   typename BeamLmOf<LM>::type lm_all, int top_paths, int *__restrict__ n_paths) {
    typedef typename BeamLdsOf<LM>::type Lds;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Lds &L = *reinterpret_cast<Lds *>(smem);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int len = seq_len[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    pool_parent += (size_t)b * nodes_per_utt;
    pool_label += (size_t)b * nodes_per_utt;
    pool_slot += (size_t)b * nodes_per_utt;
    pool_children += (size_t)b * nodes_per_utt * C;
    const auto &lm = lm_of_row(lm_all, (size_t)b * nodes_per_utt);
    const int nslots = 2 * W;

    for (int s = tid; s < nslots; s += BEAM_THREADS) { L.alive[s] = 0; L.was_alive[s] = 0; }
    for (int c = tid; c < C; c += BEAM_THREADS) gstore(&pool_children[c], -1);
    if constexpr (NBEST) {
        for (int i = tid; i < top_paths * T; i += BEAM_THREADS)
            out[(size_t)b * top_paths * T + i] = 0;
    } else {
        for (int i = tid; i < T; i += BEAM_THREADS) out[(size_t)b * T + i] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        L.node[0] = 0; L.label[0] = -1; L.parent[0] = -1; L.alive[0] = 1;
        L.n_total[0] = 0.f; L.n_blank[0] = 0.f; L.n_label[0] = -INFINITY;
        if constexpr (LM != 0) { L.lm_state[0] = 0; L.lm_e[0] = 0.f; }
        if constexpr (LM >= 2) {
            gstore(&lm.pool_ctx[0], 0); gstore(&lm.pool_sp_ctx[0], -1);
            L.misc[4] = 0; L.misc[5] = 0;
        }
        gstore(&pool_parent[0], -1); gstore(&pool_label[0], -1); gstore(&pool_slot[0], 0);
        L.heap[0] = 0;
        L.misc[0] = 1; L.misc[1] = 1; L.misc[3] = 0;
    }
    __syncthreads();

    for (int t = 0; t < len; ++t) {
        const int nheap0 = L.misc[0];
        // ---- 1. frame, old <- new, parent slots, children-in-beam masks -------------------------
        if (tid < 64) {
            const float *row = logits + ((size_t)t * B + b) * C;
            const float v = tid < C ? row[tid] : -INFINITY;
            const float mx = wave_max(v);
            float off = mx;
            if (norm_mode == 1) off = mx + logf(wave_sum(tid < C ? expf(v - mx) : 0.f));
            if (tid < C) L.x[tid] = v - off;
        }
        for (int s = tid; s < nslots; s += BEAM_THREADS) {
            L.kids_in_beam[s] = 0ull;
            L.was_alive[s] = L.alive[s];
            L.expanded[s] = 0;
            L.evict_time[s] = 0x7fffffff;
        }
        __syncthreads();
        for (int i = tid; i < nheap0; i += BEAM_THREADS) {
            const int s = L.heap[i];
            L.o_total[s] = L.n_total[s];
            L.o_blank[s] = L.n_blank[s];
            int ps = -1;
            if (L.parent[s] >= 0) ps = gload(&pool_slot[L.parent[s]]);
            L.pslot[s] = ps;
            if (ps >= 0) atomicOr(&L.kids_in_beam[ps], 1ull << L.label[s]);
        }
        __syncthreads();
        // ---- update the leaves (TensorFlow's first loop) ------------------------------------------
        for (int i = tid; i < nheap0; i += BEAM_THREADS) {
            const int s = L.heap[i];
            float nl = L.n_label[s];
            const int lab = L.label[s];
            if (lab >= 0) {
                const int ps = L.pslot[s];
                if constexpr (LM != 0) {
                    if (ps >= 0)
                        nl = lse2f(nl, (lab == L.label[ps] ? L.o_blank[ps] : L.o_total[ps]) +
                                           L.lm_e[s]);
                } else {
                    if (ps >= 0) nl = lse2f(nl, lab == L.label[ps] ? L.o_blank[ps] : L.o_total[ps]);
                }
                nl += L.x[lab];
            }
            const float nb = L.o_total[s] + L.x[blank];
            L.n_label[s] = nl;
            L.n_blank[s] = nb;
            L.n_total[s] = lse2f(nb, nl);
        }
        __syncthreads();
        // ---- 2. branch order (old total desc, older node first) -------------------------------
        int n_pow2 = 1;
        while (n_pow2 < nheap0) n_pow2 <<= 1;
        for (int i = tid; i < n_pow2; i += BEAM_THREADS) {
            if (i < nheap0) {
                const int s = L.heap[i];
                const unsigned nd = min((unsigned)L.node[s], 0x1fffffu);
                // descending old total == ascending ~key; ties: older (smaller id) node first
                L.sort_a[i] = ((unsigned long long)(~order_key(L.o_total[s])) << 32) |
                              (nd << 11) | (unsigned)s;
            } else {
                L.sort_a[i] = ~0ull;
            }
        }
        __syncthreads();
        bitonic_sort<NBEST>(L.sort_a, n_pow2, tid);
        for (int i = tid; i < nheap0; i += BEAM_THREADS) {
            const int sa = (int)(L.sort_a[i] & 0x7ffu);
            L.branches[i] = sa;
            L.bidx[sa] = i;
        }
        __syncthreads();

        // ---- 3. TensorFlow's second loop, serial over branches, on wave 0 ------------------------
        if (tid < 64) {
            const int per = (W + 63) / 64;
            if (per <= 1)
                beam_expand<1, LM, NBEST>(L, lane, W, C, blank, nslots, nheap0, pool_parent,
                                          pool_label, pool_children, nodes_per_utt, lm);
            else if (per <= 4)
                beam_expand<4, LM, NBEST>(L, lane, W, C, blank, nslots, nheap0, pool_parent,
                                          pool_label, pool_children, nodes_per_utt, lm);
            else
                beam_expand<16, LM, NBEST>(L, lane, W, C, blank, nslots, nheap0, pool_parent,
                                           pool_label, pool_children, nodes_per_utt, lm);
        }
        __syncthreads();
        // ---- beam slots of the tree nodes for the next frame -----------------------------------
        for (int s = tid; s < nslots; s += BEAM_THREADS) {
            if (L.alive[s]) gstore(&pool_slot[L.node[s]], s);
            else if (L.was_alive[s]) gstore(&pool_slot[L.node[s]], -1);
        }
        __syncthreads();
    }

    // ---- best leaf and its label path --------------------------------------------------------------
    if constexpr (LM >= 2) {
        // the end scores of the (at most W) final leaves, one wave per leaf, all waves at work
        const int nheap = L.misc[0];
        for (int i = tid >> 6; i < nheap; i += BEAM_THREADS / 64) {
            const int s = L.heap[i];
            float e;
            if constexpr (LM == 3)
                e = wordlm_end_la(lm, min(max(L.lm_state[s], 0), lm.nodes - 1),
                                  gload(&lm.pool_ctx[L.node[s]]), lane);
            else
                e = wordlm_end(lm, L.lm_state[s], gload(&lm.pool_ctx[L.node[s]]), lane);
            if (lane == 0) L.n_total[s] += e;
        }
        if (lm.stats && tid == 0) {
            lm.stats[2 * b] = L.misc[4];
            lm.stats[2 * b + 1] = L.misc[5];
        }
        __syncthreads();
    }
    if constexpr (LM == 1) {
        // TensorFlow's TopPaths: the end score of each leaf's state joins its total first
        if (lm.final) {
            const int nheap = L.misc[0];
            for (int i = tid; i < nheap; i += BEAM_THREADS)
                L.n_total[L.heap[i]] += lm.final[L.lm_state[L.heap[i]]];
            __syncthreads();
        }
    }
    if constexpr (NBEST) {
        // the final leaves in the order of the branch sort - total descending, equal totals: the
        // older node first, so rank 0 is the leaf `worse` picks below - then one thread per rank
        // walks its leaf's parent chain
        const int nheap = L.misc[0];
        int n_pow2 = 1;
        while (n_pow2 < nheap) n_pow2 <<= 1;
        for (int i = tid; i < n_pow2; i += BEAM_THREADS) {
            if (i < nheap) {
                const int s = L.heap[i];
                const unsigned nd = min((unsigned)L.node[s], 0x1fffffu);
                // + 0.f: -0 and +0 are one total, as they are to `worse`
                L.sort_a[i] = ((unsigned long long)(~order_key(L.n_total[s] + 0.f)) << 32) |
                              (nd << 11) | (unsigned)s;
            } else {
                L.sort_a[i] = ~0ull;
            }
        }
        __syncthreads();
        bitonic_sort<NBEST>(L.sort_a, n_pow2, tid);
        const bool overflow = L.misc[3] != 0;     // the prefix-tree pool ran out: the row is void
        const int found = min(top_paths, nheap);
        if (tid == 0) n_paths[b] = overflow ? -1 : found;
        for (int r = tid; r < top_paths; r += BEAM_THREADS) {
            const size_t at = (size_t)b * top_paths + r;
            if (r >= found) {
                out_len[at] = overflow ? -1 : 0;
                logp[at] = -INFINITY;
                continue;
            }
            const int s = (int)(L.sort_a[r] & 0x7ffu);
            int n = 0;
            for (int node = L.node[s]; gload(&pool_parent[node]) >= 0;
                 node = gload(&pool_parent[node]))
                ++n;
            n = min(n, T);      // a label needs a frame: never more than T, whatever the pool holds
            out_len[at] = overflow ? -1 : n;
            logp[at] = L.n_total[s];
            int k = n;
            for (int node = L.node[s]; k > 0 && gload(&pool_parent[node]) >= 0;
                 node = gload(&pool_parent[node]))
                out[at * T + --k] = gload(&pool_label[node]);
        }
    } else if (tid == 0) {
        const int nheap = L.misc[0];
        int best = L.heap[0];
        for (int i = 1; i < nheap; ++i)
            if (worse(L, best, L.heap[i])) best = L.heap[i];
        int n = 0;
        for (int node = L.node[best]; gload(&pool_parent[node]) >= 0; node = gload(&pool_parent[node]))
            ++n;
        out_len[b] = L.misc[3] ? -1 : n;      // -1: the prefix-tree pool overflowed
        if (logp) logp[b] = L.n_total[best];
        int k = n;
        for (int node = L.node[best]; gload(&pool_parent[node]) >= 0; node = gload(&pool_parent[node]))
            out[(size_t)b * T + --k] = gload(&pool_label[node]);
    }
}

// Tree nodes per utterance.  Every insertion of a child that has no node yet creates one, and
// a frame can insert up to W * (C - 1) children (each branch proposes all its symbols, each
// pushing the previous bottom out): T * W * (C - 1) + 1 is the true bound - 14 M nodes of 128 B
// at width 1024, T' = 500.  Measured on noise logits, the worst case for churn, a frame inserts
// 0.8-1.5 W children; the pool holds 4 W per frame plus 64 K (never more than the true bound, so
// small searches cannot exhaust it, and at most 2^21, the id field of the sort key).  Running
// out is reported (out_len = -1 -> CtcAsrError), never silent.
size_t nodes_per_utt(int T, int W, int C) {
    size_t n = (size_t)4 * W * T + 65536;
    const size_t bound = (size_t)T * W * (C > 1 ? C - 1 : 1) + 2;
    n = n < bound ? n : bound;
    return n < (1u << 21) ? n : (1u << 21);
}

}  // namespace

extern "C" size_t ctcasr_ctc_beam_workspace_bytes(int T, int B, int C, int beam_width) {
    if (T <= 0 || B <= 0 || C <= 0 || beam_width <= 0) return 0;
    return (size_t)B * nodes_per_utt(T, beam_width, C) * (3 + (size_t)C) * sizeof(int) + 256;
}

namespace {

// ... and with a word model three more ints per tree node: its context and its space-edge memo
size_t wordlm_workspace_bytes(int T, int B, int C, int beam_width) {
    if (T <= 0 || B <= 0 || C <= 0 || beam_width <= 0) return 0;
    return (size_t)B * nodes_per_utt(T, beam_width, C) * (6 + (size_t)C) * sizeof(int) + 256;
}

// the caller's tables as the kernels take them; false: an argument error
bool wordlm_tables(const ctcasr_wordlm_t *lm, BeamWordLm *m) {
    if (!lm || !lm->succ_word || !lm->succ_lp || !lm->succ_ctx || !lm->ctx_begin ||
        !lm->ctx_backoff || !lm->ctx_parent || lm->num_ctx < 1 || lm->num_succ < 0 ||
        lm->order < 1 || lm->order > WORDLM_MAX_ORDER)
        return false;
    *m = BeamWordLm{};
    m->trie_next = lm->trie_next;
    m->trie_word = lm->trie_word;
    m->ctx_begin = reinterpret_cast<const long long *>(lm->ctx_begin);
    m->succ_word = lm->succ_word;
    m->succ_lp = lm->succ_lp;
    m->succ_ctx = lm->succ_ctx;
    m->ctx_backoff = lm->ctx_backoff;
    m->ctx_parent = lm->ctx_parent;
    m->succ = lm->num_succ;
    m->nodes = lm->num_nodes;
    m->contexts = lm->num_ctx;
    m->order = lm->order;
    m->space = lm->space;
    m->bonus = lm->bonus;
    m->oov = lm->oov_score;
    m->stats = reinterpret_cast<long long *>(lm->stats);
    return true;
}

// what the search needs of the tables beyond what a lookup needs
bool wordlm_search_arguments(const BeamWordLm &m, int C, int blank) {
    return m.trie_next && m.trie_word && m.nodes >= 2 && m.space >= 0 && m.space < C &&
           m.space != blank && m.bonus == m.bonus && m.bonus - m.bonus == 0.0 && m.oov == m.oov &&
           m.oov != INFINITY;
}

// The model of one search as its entry point was given it: which kind it is, and that kind's
// tables, unchecked.
struct BeamModel {
    enum Kind { NONE, DENSE, WORD, WORD_LOOKAHEAD } kind;
    BeamLm dense;                   // DENSE
    const ctcasr_wordlm_t *word;    // WORD, WORD_LOOKAHEAD
    const double *lookahead;        // WORD_LOOKAHEAD: [nodes]
};

// arguments, limits, workspace layout and launch of all entry points (nbest false: the top-1
// entry points, whose `logp` may be NULL and which have neither `top_paths` nor `n_paths`)
int beam_launch(const float *logits, const int32_t *seq_len, int T, int B, int C, int blank,
                int beam_width, int norm_mode, const BeamModel &model, bool nbest, int top_paths,
                int32_t *out, int32_t *out_len, float *logp, int32_t *n_paths, void *workspace,
                size_t workspace_bytes, ctcasr_stream_t stream) {
    const bool dense = model.kind == BeamModel::DENSE;
    const bool word = model.kind == BeamModel::WORD || model.kind == BeamModel::WORD_LOOKAHEAD;
    if (nbest && (!logp || !n_paths || top_paths < 1 || top_paths > beam_width))
        return CTCASR_ERR_BAD_ARGUMENT;
    BeamWordLmLa wlm = {};
    if (word && (!wordlm_tables(model.word, &wlm) || !wordlm_search_arguments(wlm, C, blank)))
        return CTCASR_ERR_BAD_ARGUMENT;
    if (model.kind == BeamModel::WORD_LOOKAHEAD && !model.lookahead)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (!logits || !seq_len || !out || !out_len || T <= 0 || B <= 0 || C <= 1 || blank < 0 ||
        blank >= C || beam_width <= 0 || norm_mode < 0 || norm_mode > 1)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (dense && (!model.dense.next || !model.dense.score || model.dense.states < 1))
        return CTCASR_ERR_BAD_ARGUMENT;
    if (beam_width > BEAM_MAX_WIDTH || C > BEAM_MAX_CLASSES) return CTCASR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < (word ? wordlm_workspace_bytes(T, B, C, beam_width)
                                              : ctcasr_ctc_beam_workspace_bytes(T, B, C, beam_width)))
        return CTCASR_ERR_WORKSPACE;
    const size_t n = nodes_per_utt(T, beam_width, C);
    int *pool_parent = reinterpret_cast<int *>(workspace);
    int *pool_label = pool_parent + (size_t)B * n;
    int *pool_slot = pool_label + (size_t)B * n;
    int *pool_children = pool_slot + (size_t)B * n;
    const size_t lds = dense || word ? sizeof(BeamLdsLm) : sizeof(BeamLds);
    // the word model's three pools trail the plain search's four
    wlm.la = model.lookahead;
    wlm.pool_ctx = pool_children + (size_t)B * n * C;
    wlm.pool_sp_ctx = wlm.pool_ctx + (size_t)B * n;
    wlm.pool_sp_score = wlm.pool_sp_ctx + (size_t)B * n;
#define BEAM_LAUNCH(LM, NBEST, MODEL)                                                                \
    do {                                                                                        \
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_decode_kernel<LM, NBEST>), \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=        \
            hipSuccess)                                                                         \
            return CTCASR_ERR_LAUNCH;                                                           \
        beam_decode_kernel<LM, NBEST><<<B, BEAM_THREADS, lds, (hipStream_t)stream>>>(           \
            logits, seq_len, T, B, C, blank, beam_width, norm_mode, out, out_len, logp,         \
            pool_parent, pool_label, pool_slot, pool_children, (int)n, MODEL, top_paths,        \
            n_paths);                                                                           \
    } while (0)
    if (model.kind == BeamModel::WORD_LOOKAHEAD) BEAM_LAUNCH(3, true, wlm);
    else if (word) BEAM_LAUNCH(2, true, static_cast<const BeamWordLm &>(wlm));
    else if (dense && nbest) BEAM_LAUNCH(1, true, model.dense);
    else if (dense) BEAM_LAUNCH(1, false, model.dense);
    else if (nbest) BEAM_LAUNCH(0, true, BeamLm{});
    else BEAM_LAUNCH(0, false, BeamLm{});
#undef BEAM_LAUNCH
    return ctcasr_launch_status();
}

}  // namespace

extern "C" int ctcasr_ctc_beam_decode(const float *logits, const int32_t *seq_len, int T, int B,
                                      int C, int blank, int beam_width, int norm_mode,
                                      int32_t *out, int32_t *out_len, float *logp, void *workspace,
                                      size_t workspace_bytes, ctcasr_stream_t stream) {
    return beam_launch(logits, seq_len, T, B, C, blank, beam_width, norm_mode, BeamModel{}, false,
                       0, out, out_len, logp, nullptr, workspace, workspace_bytes, stream);
}

// A leaf's state and edge score are constants of its tree node, and the branch's rows give them
// again whenever the node re-enters the beam: the prefix tree itself carries nothing of the model,
// and the fused search needs the plain search's pool.
extern "C" size_t ctcasr_ctc_beam_lm_workspace_bytes(int T, int B, int C, int beam_width) {
    return ctcasr_ctc_beam_workspace_bytes(T, B, C, beam_width);
}

extern "C" int ctcasr_ctc_beam_decode_lm(const float *logits, const int32_t *seq_len, int T, int B,
                                         int C, int blank, int beam_width, int norm_mode,
                                         const int32_t *lm_next, const float *lm_score,
                                         const float *lm_final, int lm_states, int32_t *out,
                                         int32_t *out_len, float *logp, void *workspace,
                                         size_t workspace_bytes, ctcasr_stream_t stream) {
    const BeamModel model = {BeamModel::DENSE, {lm_next, lm_score, lm_final, lm_states}};
    return beam_launch(logits, seq_len, T, B, C, blank, beam_width, norm_mode, model, false, 0,
                       out, out_len, logp, nullptr, workspace, workspace_bytes, stream);
}

// The n-best list is read off the final beam: the search and its prefix tree are the plain ones.
extern "C" size_t ctcasr_ctc_beam_nbest_workspace_bytes(int T, int B, int C, int beam_width) {
    return ctcasr_ctc_beam_workspace_bytes(T, B, C, beam_width);
}

extern "C" int ctcasr_ctc_beam_decode_nbest(const float *logits, const int32_t *seq_len, int T,
                                            int B, int C, int blank, int beam_width, int norm_mode,
                                            int top_paths, const int32_t *lm_next,
                                            const float *lm_score, const float *lm_final,
                                            int lm_states, int32_t *out, int32_t *out_len,
                                            float *logp, int32_t *n_paths, void *workspace,
                                            size_t workspace_bytes, ctcasr_stream_t stream) {
    const BeamModel model = {lm_next ? BeamModel::DENSE : BeamModel::NONE,
                             {lm_next, lm_score, lm_final, lm_states}};
    return beam_launch(logits, seq_len, T, B, C, blank, beam_width, norm_mode, model, true,
                       top_paths, out, out_len, logp, n_paths, workspace, workspace_bytes, stream);
}

// ---- K24: word n-gram over a lexicon trie, fused into the search ----------------------------------
namespace {

// one wave per pair, the device function of the search
__global__ void __launch_bounds__(BEAM_THREADS)
wordlm_lookup_kernel(BeamWordLm m, const int *__restrict__ ctx, const int *__restrict__ word, int n,
                     float *__restrict__ score, int *__restrict__ next_ctx) {
    const int lane = threadIdx.x & 63;
    const int waves = BEAM_THREADS / 64;
    for (long long i = (long long)blockIdx.x * waves + (threadIdx.x >> 6); i < n;
         i += (long long)gridDim.x * waves) {
        int nc;
        const double d = wordlm_wd(m, ctx[i], word[i], lane, nc);
        if (lane == 0) {
            score[i] = (float)d;
            next_ctx[i] = nc;
        }
    }
}

}  // namespace

extern "C" size_t ctcasr_ctc_beam_wordlm_workspace_bytes(int T, int B, int C, int beam_width) {
    return wordlm_workspace_bytes(T, B, C, beam_width);
}

extern "C" int ctcasr_ctc_beam_decode_wordlm(const float *logits, const int32_t *seq_len, int T,
                                             int B, int C, int blank, int beam_width,
                                             int norm_mode, int top_paths,
                                             const ctcasr_wordlm_t *lm, int32_t *out,
                                             int32_t *out_len, float *logp, int32_t *n_paths,
                                             void *workspace, size_t workspace_bytes,
                                             ctcasr_stream_t stream) {
    const BeamModel model = {BeamModel::WORD, {}, lm};
    return beam_launch(logits, seq_len, T, B, C, blank, beam_width, norm_mode, model, true,
                       top_paths, out, out_len, logp, n_paths, workspace, workspace_bytes, stream);
}

// K26: the same search with look-ahead scores inside a word; the table only steers pruning
extern "C" int ctcasr_ctc_beam_decode_wordlm_lookahead(
    const float *logits, const int32_t *seq_len, int T, int B, int C, int blank, int beam_width,
    int norm_mode, int top_paths, const ctcasr_wordlm_t *lm, const double *trie_lookahead,
    int32_t *out, int32_t *out_len, float *logp, int32_t *n_paths, void *workspace,
    size_t workspace_bytes, ctcasr_stream_t stream) {
    const BeamModel model = {BeamModel::WORD_LOOKAHEAD, {}, lm, trie_lookahead};
    return beam_launch(logits, seq_len, T, B, C, blank, beam_width, norm_mode, model, true,
                       top_paths, out, out_len, logp, n_paths, workspace, workspace_bytes, stream);
}

extern "C" int ctcasr_wordlm_lookup(const ctcasr_wordlm_t *lm, const int32_t *ctx,
                                    const int32_t *word, int n, float *score, int32_t *next_ctx,
                                    ctcasr_stream_t stream) {
    BeamWordLm m;
    if (!wordlm_tables(lm, &m) || !ctx || !word || !score || !next_ctx || n < 0)
        return CTCASR_ERR_BAD_ARGUMENT;
    if (n == 0) return CTCASR_OK;
    const int waves = BEAM_THREADS / 64;
    const int grid = (int)std::min<long long>(((long long)n + waves - 1) / waves, 1 << 16);
    wordlm_lookup_kernel<<<grid, BEAM_THREADS, 0, (hipStream_t)stream>>>(m, ctx, word, n, score,
                                                                          next_ctx);
    return ctcasr_launch_status();
}
