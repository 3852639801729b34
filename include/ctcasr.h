/* ctcasr.h — C ABI of the MI355X-native CTC acoustic-model hot path (libctcasr.so).
 *
 * The reference (mdangschat/ctc-asr) has no FFI of its own: its hot path is a chain of
 * TensorFlow / cuDNN / python_speech_features calls made from Python.  Each entry point below
 * replaces one of those call sites (cited per function; paths relative to the reference root)
 * and is what a binding for that call site would bind.  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions (all functions):
 *   - plain C types only; every pointer is a DEVICE pointer (HBM) owned by the caller unless the
 *     parameter name ends in `_host`; tensors are contiguous, row-major, float32 unless noted;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously on it and the
 *     function returns without synchronising; nothing is allocated behind the caller's back —
 *     scratch memory is sized by the matching *_workspace_bytes() query and passed in;
 *   - return value: CTCASR_OK (0) or a negative CTCASR_ERR_* code for an argument / launch
 *     error; functions never throw and never abort.  Per-utterance data errors (an infeasible
 *     CTC alignment) are reported through a device-side `status` array, mirroring the point at
 *     which TensorFlow raises InvalidArgumentError.
 *   - time-major activations: [T, B, *]; direction index 0 = forward, 1 = backward.
 */
#ifndef CTCASR_H_
#define CTCASR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTCASR_ABI_VERSION 8

enum {
    CTCASR_OK = 0,
    CTCASR_ERR_BAD_ARGUMENT = -1,   /* null pointer, non-positive size, unknown enum           */
    CTCASR_ERR_UNSUPPORTED = -2,    /* valid request outside what the kernels cover            */
    CTCASR_ERR_WORKSPACE = -3,      /* workspace pointer null or too small                     */
    CTCASR_ERR_LAUNCH = -4,         /* hipGetLastError() reported a launch failure             */
    CTCASR_ERR_TIMEOUT = -5         /* a bounded in-kernel wait gave up (persistent RNN kernel) */
};

/* RNN cell types; names follow FLAGS.rnn_cell (asr/params.py:47-50, asr/model.py:194-199). */
enum {
    CTCASR_CELL_RNN_RELU = 0,
    CTCASR_CELL_RNN_TANH = 1,
    CTCASR_CELL_LSTM = 2,
    CTCASR_CELL_GRU = 3
};

typedef void *ctcasr_stream_t;

int ctcasr_abi_version(void);
/* Bit mask of the non-default compile-time macros this library was built with.  A/B and probe
 * builds of the recurrence kernels (tools/build_alt.sh) come out of the same sources as the
 * product; a loader must refuse a library whose CTCASR_BUILD_PROBE_WRONG_RESULTS bit is set
 * (a timing probe that skips part of the arithmetic ON PURPOSE) unless it was asked for one -
 * ctc_asr_amd/hip.py does (CTCASR_ALLOW_PROBE_BUILD=1 to override).  0 = the product build. */
#define CTCASR_BUILD_PROBE_WRONG_RESULTS 1u   /* e.g. -DPRNN_PROBE_HALF_LOADS=1               */
#define CTCASR_BUILD_NONDEFAULT_TUNING   2u   /* PRNN_GROUPS / _XCD_AWARE / _CHAIN_* / ...     */
unsigned ctcasr_build_flags(void);
/* Process-wide PROFILING switch (no option changes what a call computes or which kernel variant
 * it runs - that is the per-call `flags` argument of ctcasr_rnn_fwd_steps / _bwd_steps):
 * "rnn_kernel_events" (0/1, default 0): record a HIP event pair on the launch stream around every
 * persistent recurrence kernel; ctcasr_rnn_kernel_events() waits for them, returns launch counts
 * and summed durations ([0] forward, [1] backward) and clears the record (benchmarking). */
int ctcasr_set_option(const char *name, int value);
int ctcasr_rnn_kernel_events(int launches[2], double total_ms[2]);
const char *ctcasr_error_string(int code);

/* ---- K8: (log-)softmax over the class axis ------------------------------------------------
 * Replaces the softmax inside tf.nn.ctc_loss / ctc_beam_search_decoder (asr/model.py:259,292).
 * x, y: [rows, C] with C <= 64.  bwd: dx = dy - exp(y) * sum_c(dy). */
int ctcasr_log_softmax_fwd(const float *x, float *y, int rows, int C, ctcasr_stream_t stream);
int ctcasr_log_softmax_bwd(const float *y, const float *dy, float *dx, int rows, int C,
                           ctcasr_stream_t stream);

/* ---- K9: CTC loss + gradient, log-softmax fused ---------------------------------------------
 * Replaces tf.nn.ctc_loss(labels, inputs=logits, sequence_length, time_major=True,
 * ctc_merge_repeated=True, preprocess_collapse_repeated=False) and its gradient
 * (asr/model.py:259-264; the reduce_mean of :267 is applied through `grad_scale` = 1/B).
 *   logits        [T, B, C] raw activations; blank = C - 1 for the reference (pass it anyway)
 *   labels        int32, concatenated label ids of all B utterances (ids in [0, C) \ {blank})
 *   label_offsets int32 [B + 1], labels of utterance b are labels[label_offsets[b] .. [b+1])
 *   seq_len       int32 [B], frames of utterance b that count (<= T)
 *   loss          [B]   -ln p(label_b | x_b); +inf when status[b] != 0
 *   grad_logits   [T, B, C] d(sum_b grad_scale * loss_b) / d logits; rows t >= seq_len[b] are 0
 *   status        int32 [B]: 0 ok; 1 "not enough time for target transition sequence"
 *                 (TensorFlow raises here); 2 label id out of range / seq_len > T, or the row
 *                 is longer than max_label_len / has a negative length
 * Workspace: ctcasr_ctc_loss_workspace_bytes(T, B, C, max_label_len). */
size_t ctcasr_ctc_loss_workspace_bytes(int T, int B, int C, int max_label_len);
int ctcasr_ctc_loss_fwd_bwd(const float *logits, const int32_t *labels,
                            const int32_t *label_offsets, const int32_t *seq_len, int T, int B,
                            int C, int blank, int max_label_len, float grad_scale, float *loss,
                            float *grad_logits, int32_t *status, void *workspace,
                            size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K10: decoding --------------------------------------------------------------------------
 * Greedy: argmax per frame (first maximum), merge repeats, drop blank — ctc_greedy_decoder
 * semantics (named in asr/model.py:290,298 and required by BASELINE.json).
 *   out [B, T] int32 (row padded with 0), out_len [B]. */
int ctcasr_ctc_greedy_decode(const float *logits, const int32_t *seq_len, int T, int B, int C,
                             int blank, int32_t *out, int32_t *out_len, ctcasr_stream_t stream);

/* Beam search: tf.nn.ctc_beam_search_decoder(inputs=logits, sequence_length,
 * beam_width, top_paths=1, merge_repeated=False) (asr/model.py:292-296).
 *   norm_mode 0: per-frame max subtraction (TensorFlow 1.12); 1: full log-softmax (TF >= 1.14)
 *   out [B, T] int32, out_len [B], logp [B] (log-probability of the top path; may be NULL)
 * Workspace: ctcasr_ctc_beam_workspace_bytes(T, B, C, beam_width). */
size_t ctcasr_ctc_beam_workspace_bytes(int T, int B, int C, int beam_width);
int ctcasr_ctc_beam_decode(const float *logits, const int32_t *seq_len, int T, int B, int C,
                           int blank, int beam_width, int norm_mode, int32_t *out,
                           int32_t *out_len, float *logp, void *workspace,
                           size_t workspace_bytes, ctcasr_stream_t stream);

/* Beam search with a language model fused in (no counterpart in the reference).  The model is a
 * deterministic weighted automaton over label ids - TensorFlow's BeamScorer with an integer
 * state; a back-off n-gram of any order and a word list both compile to it:
 *   lm_next   int32 [lm_states, C]: the state after label c in state s; state 0 is the start
 *   lm_score  float [lm_states, C]: the expansion score of that edge, weight and insertion bonus
 *             already folded in; -inf forbids the edge (it is never a candidate and creates no
 *             tree node).  +inf and NaN are the caller's to refuse.
 *   lm_final  float [lm_states] or NULL: the end score of a hypothesis that ends in s
 * The blank's column of both tables is never read.  Entries of lm_next are clamped into
 * [0, lm_states): the tables are never indexed outside themselves, whatever they hold.
 * The scorer enters where TensorFlow calls it.  A leaf's edge score e = lm_score[state(parent),
 * label] and its state are constants of its tree node (root: state 0, e = 0).  Per frame, a leaf
 * whose parent is in the beam gets new.label = lse(new.label, prev + e) before + x[label]; a
 * proposed child is worth x[c] + (prev + lm_score[state(branch), c]), added in that order in
 * fp32 (prev: the parent's old blank for a repeated label, else its old total).  At the end
 * lm_final[state] joins every leaf's total before the best is chosen, and logp is that fused
 * total.  With lm_states = 1, all scores 0 and no lm_final the result is bit for bit that of
 * ctcasr_ctc_beam_decode.
 * Tie rule, as in the plain search: the leaf with the lowest total leaves the beam first and,
 * among equal totals, the youngest tree node; the best leaf among equal totals is the oldest.
 * Arguments, limits, outputs (out_len -1: pool exhausted) and status codes are those of
 * ctcasr_ctc_beam_decode; lm_states < 1 or a NULL lm_next / lm_score is
 * CTCASR_ERR_BAD_ARGUMENT.  Workspace: ctcasr_ctc_beam_lm_workspace_bytes(T, B, C, beam_width)
 * (the prefix tree carries nothing of the model: the size of the plain search's). */
size_t ctcasr_ctc_beam_lm_workspace_bytes(int T, int B, int C, int beam_width);
int ctcasr_ctc_beam_decode_lm(const float *logits, const int32_t *seq_len, int T, int B, int C,
                              int blank, int beam_width, int norm_mode, const int32_t *lm_next,
                              const float *lm_score, const float *lm_final, int lm_states,
                              int32_t *out, int32_t *out_len, float *logp, void *workspace,
                              size_t workspace_bytes, ctcasr_stream_t stream);

/* N-best lists from both searches: tf.nn.ctc_beam_search_decoder's top_paths (the reference
 * passes 1).  One entry point; lm_next == NULL is the plain search, otherwise the four lm_*
 * arguments are those of ctcasr_ctc_beam_decode_lm.  The search is the same search: only what is
 * read off the final beam differs.  Arguments, limits and status codes are those of
 * ctcasr_ctc_beam_decode_lm, plus top_paths N with 1 <= N <= beam_width (else
 * CTCASR_ERR_BAD_ARGUMENT); logp and n_paths may not be NULL.
 *   out      int32 [B, N, T]: the label path of rank k of utterance b, zero-padded
 *   out_len  int32 [B, N]
 *   logp     float [B, N]: the beam's total of that leaf (with a model: the fused total, lm_final
 *            included).  Under norm_mode 0 it is no log-probability, and under either mode it
 *            sums only the alignments that survived pruning: ctcasr_ctc_score gives the exact one.
 *   n_paths  int32 [B] = min(N, leaves in the final beam)
 * Order (pinned): total descending; among equal totals the older tree node first (-0 and +0 are
 * equal).  It is the order of the search's branch sort, and rank 0 is the leaf that
 * ctcasr_ctc_beam_decode / _lm return: out[b][0], out_len[b][0], logp[b][0] are theirs bit for
 * bit.  No two ranks of a row hold the same path (a path is one tree node).
 * Ranks k >= n_paths[b]: out_len 0, logp -inf, out 0.  A row whose prefix-tree pool ran out has
 * n_paths = -1 and every out_len of the row -1 (its out / logp are not to be used).  Every
 * output element is written.  Workspace: ctcasr_ctc_beam_nbest_workspace_bytes(T, B, C,
 * beam_width), the size of the plain search's.
 * Left out on purpose: merge_repeated, lattice output. */
size_t ctcasr_ctc_beam_nbest_workspace_bytes(int T, int B, int C, int beam_width);
int ctcasr_ctc_beam_decode_nbest(const float *logits, const int32_t *seq_len, int T, int B, int C,
                                 int blank, int beam_width, int norm_mode, int top_paths,
                                 const int32_t *lm_next, const float *lm_score,
                                 const float *lm_final, int lm_states, int32_t *out,
                                 int32_t *out_len, float *logp, int32_t *n_paths, void *workspace,
                                 size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K14: CTC scoring ---------------------------------------------------------------------------
 * Forward-only CTC log-likelihood of H label sequences against B utterances (no counterpart in
 * the reference): the exact ln p(y | x) of every hypothesis of an n-best list, for posteriors
 * and second-pass rescoring.  One wavefront per hypothesis, the lattice in registers; nothing
 * but one float per hypothesis is written.
 *   logits, seq_len  as ctcasr_ctc_loss_fwd_bwd takes them; blank is any id in [0, C)
 *   labels         int32, the concatenated label ids of all H hypotheses
 *   label_offsets  int32 [H + 1]
 *   utt            int32 [H]: the utterance of hypothesis h, in [0, B); any order, and an
 *                  utterance may have no hypothesis at all
 *   score          [H]  ln p(labels_h | x_utt[h]) = -loss of ctcasr_ctc_loss_fwd_bwd; an empty
 *                  label is legal (the sum of the blank's log-softmax over the frames; 0 for
 *                  seq_len 0)
 *   status         int32 [H]: 0 ok; 1 seq_len < L + adjacent repeats; 2 a label id out of range
 *                  or the blank, utt[h] outside [0, B), seq_len > T or < 0, or a row longer than
 *                  max_label_len (or of negative length).  Non-zero: score -inf.
 * A non-finite logit in the first seq_len frames of the utterance makes the score NaN, as it
 * makes the loss; frames beyond seq_len are never read.  A hypothesis' score does not depend on
 * the others of the call or on their order, bit for bit.  Every output element is written.
 * 2 * max_label_len + 1 <= 1152, C <= 64 (else CTCASR_ERR_UNSUPPORTED).  Workspace:
 * ctcasr_ctc_score_workspace_bytes(T, B, C, H, max_label_len) (the log-softmax table). */
size_t ctcasr_ctc_score_workspace_bytes(int T, int B, int C, int H, int max_label_len);
int ctcasr_ctc_score(const float *logits, const int32_t *seq_len, int T, int B, int C, int blank,
                     const int32_t *labels, const int32_t *label_offsets, const int32_t *utt,
                     int H, int max_label_len, float *score, int32_t *status, void *workspace,
                     size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K23: expected-risk gradient over n-best lists (MWER training) ------------------------------
 * The gradient, with respect to the logits, of the expected error count over an n-best list (no
 * counterpart in the reference): the training signal that ctcasr_ctc_beam_decode_nbest, K14 and
 * K13 lack between them.  CTC forward AND backward lattices of B * N hypotheses, folded into one
 * gradient with per-hypothesis weights computed on the device.  (An added entry point, as K19 -
 * K22: CTCASR_ABI_VERSION stays.)
 *   logits, seq_len  as ctcasr_ctc_score takes them; blank is any id in [0, C)
 *   labels         int32, the concatenated label ids of all B * N rows
 *   label_offsets  int32 [B * N + 1]; row b * N + i is hypothesis i (rank i) of utterance b
 *   n_hyps         int32 [B]: rows i >= n_hyps[b] of utterance b are unused - nothing of them is
 *                  read, neither their offsets' labels nor their risk.  A negative value counts as
 *                  0 (the n-best search's n_paths = -1), one above N as N.
 *   risk           float [B * N]: W_i, an error count (any finite value)
 *   scale, accumulate  see grad
 *
 * PINNED: the arithmetic (tests/mwer_reference.py restates it).  Per utterance b the VALID
 * hypotheses are its used rows of status 0, in rank order, with s_i = score and W_i = risk:
 *   - score[h] is bit for bit what ctcasr_ctc_score returns for the same row: the table of
 *     ctcasr_log_softmax_fwd, lse3's operand order, fp64 state, fp32 exp / log of the
 *     differences, for every states-per-lane count;
 *   - in fp64, from the fp32 scores widened to double: P_i = exp(s_i - max s) / sum_j exp(s_j -
 *     max s) (sums in ascending rank; if every valid score is -inf they share the mass equally),
 *     R_b = sum_i P_i W_i, c_i = P_i (W_i - R_b), so sum_i c_i = 0;
 *   - occ_i[t, k] = the sum over the extended states u of y_i with l'[u] = k of exp(alpha_i(t, u) +
 *     beta_i(t, u) - s_i) (K9's occupancy; 0 throughout when s_i = -inf).  As d s_i / d logit[t, k]
 *     = occ_i[t, k] - softmax[t, k] and the c_i sum to zero, the softmax terms cancel:
 *         grad[t, b, k] = scale * sum_i c_i occ_i[t, k]       for t < seq_len[b],
 *     the sum over i in ascending rank in fp64, times (double)scale, rounded to fp32 once;
 *     every such row sums to zero over k up to rounding;
 *   - accumulate != 0: grad[t, b, k] = (float)((double)grad_in[t, b, k] + that fp64 value);
 *   - rows t >= seq_len[b] (a seq_len outside [0, T]: every row) are +0.0, or with accumulate
 *     keep grad_in bit for bit;
 *   - an utterance with fewer than two valid hypotheses has the fp64 value +0.0 in every row
 *     below seq_len; R_b is then the one valid risk, or 0 with none.
 * No float atomics: an utterance's outputs do not depend on the other utterances of the call, and
 * two runs give equal bits.
 *   grad           [T, B, C], see above
 *   expected_risk  float [B]: R_b
 *   score          float [B * N]; -inf for a non-zero status other than 3
 *   posterior      float [B * N]: P_i; 0 for a row that is not valid
 *   status         int32 [B * N]: K14's codes - 0 ok; 1 seq_len < L + adjacent repeats; 2 a label
 *                  id out of range or the blank, seq_len > T or < 0, a row longer than
 *                  max_label_len or of negative length - and, where K14 returns status 0 with a
 *                  NaN score, K11's 3: a non-finite logit in the first seq_len frames.  score (the
 *                  same NaN bits as K14's) and posterior of such a row, expected_risk of its
 *                  utterance and every gradient element of the utterance with t < seq_len are then
 *                  NaN.  An unused row has status -1, score -inf, posterior 0.
 * Every output element is written (grad with accumulate: as pinned above).  Frames at or beyond
 * seq_len are never read.  C <= 64, 2 * max_label_len + 1 <= 1152, B <= 65535 (else
 * CTCASR_ERR_UNSUPPORTED); N < 1, C < 2, a blank outside [0, C), a negative size or a null pointer:
 * CTCASR_ERR_BAD_ARGUMENT, before the device is touched.  Workspace:
 * ctcasr_ctc_mwer_workspace_bytes(T, B, C, N, max_label_len) (0 for arguments the call would
 * refuse): the table, both fp64 lattices of every row ([T] frames of 64 * ceil-to-{1,2,3,6,18}
 * ((2 * max_label_len + 1) / 64) states), two fp64 per row and one word per utterance; its
 * contents on entry do not matter.
 * Left out on purpose: a language model term in s_i, the reference appended to the list, risks
 * computed inside the call. */
size_t ctcasr_ctc_mwer_workspace_bytes(int T, int B, int C, int N, int max_label_len);
int ctcasr_ctc_mwer(const float *logits, const int32_t *seq_len, int T, int B, int C, int blank,
                    const int32_t *labels, const int32_t *label_offsets, const int32_t *n_hyps,
                    const float *risk, int N, int max_label_len, float scale, int accumulate,
                    float *grad, float *expected_risk, float *score, float *posterior,
                    int32_t *status, void *workspace, size_t workspace_bytes,
                    ctcasr_stream_t stream);

/* ---- K24: word n-gram language model fused into the beam search ---------------------------------
 * The search of K10 under a word-level model (no counterpart in the reference).  The decode-time
 * automaton of a word n-gram is the composition of a lexicon trie with the n-gram's contexts - far
 * too many states for the dense tables of ctcasr_ctc_beam_decode_lm -, so it stays implicit: a
 * leaf's state is the pair (n, h) of a trie node and a context, the start state (0, 0), and a
 * word's score is looked up with back-off when a hypothesis closes the word.  (Added entry points,
 * as K19 - K23: CTCASR_ABI_VERSION stays.)
 *
 * Tables (device pointers; ctcasr_wordlm_t), C the classes of the logits:
 *   trie_next   int32  [num_nodes, C]  -1: no edge.  Node 0 is the root, node 1 the out-of-
 *                                      vocabulary sink (its row is never read).
 *   trie_word   int32  [num_nodes]     the word id that ends at this node, or -1
 *   ctx_begin   int64  [num_ctx + 1]   start of each context's successor range
 *   succ_word   int32  [num_succ]      ascending inside a range; context 0 lists every word id
 *   succ_lp     double [num_succ]      log-probability of the successor (weight folded in)
 *   succ_ctx    int32  [num_succ]      the context after (h, w)
 *   ctx_backoff double [num_ctx]       ln bo(h) (weight folded in)
 *   ctx_parent  int32  [num_ctx]       h less its oldest word
 * Word id 0 is <unk>, 1 is </s>.  order is 1 .. 5; space is the label that ends a word; bonus is
 * added per label; oov_score is -inf (closed vocabulary) or finite ("OOV on").
 *
 * PINNED (tests/word_lm_reference.py restates it).  Wd(h, w), in fp64: acc = 0; search h's
 * successor range for w; found: acc += succ_lp, the next context is succ_ctx, stop; otherwise
 * acc += ctx_backoff[h], h = ctx_parent[h], search again.  The adds happen in exactly that order.
 * At most `order` searches, each bounded; tables that would run longer give -inf (and context 0).
 * No loop on the device is open-ended, whatever the tables hold, and every index read from a
 * table is clamped into its array.  Each score below is computed in fp64 and rounded once to
 * fp32.  The edge for label c out of (n, h); the blank's column is never read:
 *   c not the space:  n == 1                       -> (1, h)     bonus
 *                     m = trie_next[n, c] >= 0     -> (m, h)     bonus
 *                     no trie edge, OOV on         -> (1, h)     oov_score + bonus
 *                     no trie edge, OOV off        -> none       -inf
 *   c the space:      n == 0                       -> none       -inf  (leading / doubled space)
 *                     w = trie_word[n] >= 0        -> (0, ctx')  Wd(h, w) + bonus
 *                     n == 1 (OOV on)              -> (0, ctx')  Wd(h, 0) + bonus
 *                     other n, OOV on              -> (0, ctx')  (Wd(h, 0) + oov_score) + bonus
 *                     other n, OOV off             -> none       -inf
 * The end of a hypothesis in (n, h), without a bonus: n == 0: Wd(h, 1); n closes a word or an OOV
 * by the rules above: (that word's score without the bonus) + Wd(ctx', 1); otherwise -inf.
 * The search's own arithmetic is that of ctcasr_ctc_beam_decode_lm / _nbest, which read these
 * values where they read lm_score / lm_next / lm_final: on the dense automaton over the reachable
 * (n, h) pairs of a small model those entry points return the same bits.
 *
 * ctcasr_ctc_beam_decode_wordlm: the outputs, their order, n_paths = -1 on pool exhaustion and the
 * refusals of ctcasr_ctc_beam_decode_nbest; top_paths = 1 is the top-1 decode.  A NULL table, order
 * outside 1 .. 5, num_nodes < 2, num_ctx < 1, a space outside [0, C) or equal to the blank, a
 * non-finite bonus, a NaN or +inf oov_score: CTCASR_ERR_BAD_ARGUMENT.  stats is NULL or int64
 * [B, 2]: branches expanded and word lookups performed for space edges, per utterance.
 * The trie node of a leaf lives with the beam; its context, and the space edge of its tree node
 * (score and next context, computed once, on the node's first expansion), live in the workspace,
 * initialised where the node is created: ctcasr_ctc_beam_wordlm_workspace_bytes(T, B, C,
 * beam_width), three ints per tree node more than the plain search's.  Its contents on entry do
 * not matter.
 *
 * ctcasr_wordlm_lookup: score[i] = fp32(Wd(ctx[i], word[i])) and next_ctx[i] for n pairs, by the
 * device function the search uses (trie_*, space, bonus, oov_score and stats are not read; ctx[i]
 * is clamped into [0, num_ctx)).  n == 0 returns CTCASR_OK and launches nothing.
 * Left out on purpose: hashed or quantised storage, orders above 5, lattice output.  (Look-ahead
 * scores inside a word: K26, below the declarations.) */
typedef struct ctcasr_wordlm {
    const int32_t *trie_next;
    const int32_t *trie_word;
    const int64_t *ctx_begin;
    const int32_t *succ_word;
    const double *succ_lp;
    const int32_t *succ_ctx;
    const double *ctx_backoff;
    const int32_t *ctx_parent;
    int64_t num_succ;
    int32_t num_nodes, num_ctx, order, space;
    double bonus, oov_score;
    int64_t *stats;
} ctcasr_wordlm_t;
size_t ctcasr_ctc_beam_wordlm_workspace_bytes(int T, int B, int C, int beam_width);
int ctcasr_ctc_beam_decode_wordlm(const float *logits, const int32_t *seq_len, int T, int B, int C,
                                  int blank, int beam_width, int norm_mode, int top_paths,
                                  const ctcasr_wordlm_t *lm, int32_t *out, int32_t *out_len,
                                  float *logp, int32_t *n_paths, void *workspace,
                                  size_t workspace_bytes, ctcasr_stream_t stream);
int ctcasr_wordlm_lookup(const ctcasr_wordlm_t *lm, const int32_t *ctx, const int32_t *word, int n,
                         float *score, int32_t *next_ctx, ctcasr_stream_t stream);

/* ---- K26: look-ahead scores inside a word ------------------------------------------------------
 * K24 pays a word's score when the hypothesis closes the word, so between two spaces the beam is
 * pruned on acoustics alone.  With look-ahead ("smearing") entering a trie node charges the best
 * score a word below that node can still get, and the space settles the difference.  (An added
 * entry point, as K19 - K24: CTCASR_ABI_VERSION stays; ctcasr_wordlm_t keeps its layout.)
 *
 * One table joins K24's: trie_lookahead, double [num_nodes], `la` below.  Everything K24 pins
 * stands - Wd, the contexts, the memo, the outputs; only the scores of the edges and of the end
 * change.  PINNED (tests/word_lm_lookahead_reference.py restates it).  Each score is one fp64
 * expression, in exactly the order written, rounded once to fp32.  The edge for label c out of
 * (n, h):
 *   c not the space:  n == 1                       -> (1, h)     bonus
 *                     m = trie_next[n, c] >= 0     -> (m, h)     (la[m] - la[n]) + bonus
 *                     no trie edge, OOV on         -> (1, h)     (la[1] - la[n]) + bonus
 *                     no trie edge, OOV off        -> none       -inf
 *   c the space, d what the word costs in full:
 *                     n == 0                       -> none       -inf
 *                     w = trie_word[n] >= 0        d = Wd(h, w)
 *                     n == 1 (OOV on)              d = Wd(h, 0) + oov_score
 *                     other n, OOV on              d = Wd(h, 0) + oov_score
 *                     other n, OOV off             -> none       -inf
 *                     otherwise                    -> (0, ctx')  (d - la[n]) + bonus
 * The end of a hypothesis in (n, h): n == 0: Wd(h, 1); otherwise (d - la[n]) + Wd(ctx', 1), or -inf
 * where nothing closes.  Note the sink: K24 charges oov_score on the edge into node 1 and Wd(h, 0)
 * at its space; here the edge into the sink charges la[1] - la[n] and the space settles against
 * the full Wd(h, 0) + oov_score.
 * The sums telescope: along any label row the scores from a root state to the next root state, or
 * to the end, add up to K24's (to rounding), for every table of finite values.  The table steers
 * pruning and never what a complete hypothesis is worth, so any finite table is accepted; the
 * caller answers for its entries being finite.  No index is derived from the table, and every
 * index read from a table stays clamped.  (The project's table, lm.WordLmScorer.lookahead_table:
 * la[n] = the best unigram score succ_lp[w], context 0, of a word at or below n - with OOV on
 * never below oov_score + succ_lp[0], which is la[1] -, 0 where nothing is finite, and la[0] = 0:
 * nothing is paid ahead at the root, so the state after a space is the start state.)
 *
 * ctcasr_ctc_beam_decode_wordlm_lookahead: the arguments, outputs, refusals and stats of
 * ctcasr_ctc_beam_decode_wordlm; a NULL trie_lookahead: CTCASR_ERR_BAD_ARGUMENT.  The workspace is
 * K24's, ctcasr_ctc_beam_wordlm_workspace_bytes; its contents on entry do not matter, and one that
 * a launch of either entry point left behind serves the other (the memo of a tree node is
 * initialised where the node is created).
 * Left out on purpose: look-ahead from higher-order contexts (this is the unigram bound when the
 * project's table is used), look-ahead for the dense automaton of ctcasr_ctc_beam_decode_lm. */
int ctcasr_ctc_beam_decode_wordlm_lookahead(const float *logits, const int32_t *seq_len, int T,
                                            int B, int C, int blank, int beam_width,
                                            int norm_mode, int top_paths,
                                            const ctcasr_wordlm_t *lm,
                                            const double *trie_lookahead, int32_t *out,
                                            int32_t *out_len, float *logp, int32_t *n_paths,
                                            void *workspace, size_t workspace_bytes,
                                            ctcasr_stream_t stream);

/* ---- K11: CTC forced alignment ----------------------------------------------------------------
 * The Viterbi (max-sum) form of K9's alpha recursion: the single best alignment of each
 * utterance's label to its frames (no counterpart in the reference).  Inputs and status codes
 * are those of ctcasr_ctc_loss_fwd_bwd; blank is any id in [0, C).  Per utterance, with L labels
 * and S = 2L + 1 extended states, the lattice runs in fp64 and ends in S - 1 or (L > 0) S - 2.
 * Tie rule: predecessors are compared with strict > in the order s, s - 1, s - 2, and S - 1 wins
 * over S - 2 at the end, so equal scores keep the smaller move; results are bit-reproducible.
 *   path       int32 [B, T]: the state s in [0, S) of the best path at frame t < seq_len[b]
 *              (even s: blank, odd s: label position (s - 1) / 2); -1 for t >= seq_len[b]
 *   score      [B]   log-probability of the best path (0 for seq_len 0 and L = 0)
 *   frame_logp [B, T] log-softmax of the class the path emits at frame t, 0 for t >= seq_len[b];
 *              may be NULL
 *   status     int32 [B]: 0 ok; 1 seq_len < L + adjacent repeats (no alignment exists); 2 label
 *              id out of range / the blank, seq_len > T or < 0, or the row is longer than
 *              max_label_len; 3 a non-finite logit in the first seq_len frames.  Non-zero: score
 *              -inf (NaN for 3), path -1 and frame_logp 0 for the whole row.
 * Every output is fully written.  2 * max_label_len + 1 <= 1152, C <= 64 (else
 * CTCASR_ERR_UNSUPPORTED).  Workspace: ctcasr_ctc_align_workspace_bytes(T, B, C,
 * max_label_len). */
size_t ctcasr_ctc_align_workspace_bytes(int T, int B, int C, int max_label_len);
int ctcasr_ctc_align(const float *logits, const int32_t *labels, const int32_t *label_offsets,
                     const int32_t *seq_len, int T, int B, int C, int blank, int max_label_len,
                     int32_t *path, float *score, float *frame_logp, int32_t *status,
                     void *workspace, size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K21: CTC forced alignment of one long sequence -------------------------------------------
 * K11's alignment without K11's ceiling (2L + 1 <= 1152): one sequence of T frames against L
 * labels, the lattice tiled in the workspace - CTCASR_ALIGN_LONG_TILE_STATES states by
 * tile_frames frames (0: CTCASR_ALIGN_LONG_TILE_FRAMES; a value above T counts as T) per
 * workgroup, one launch per anti-diagonal of tiles, rows + cols - 1 of them, between a launch
 * that builds the table and one that walks the path back.  No workgroup waits for another: a tile
 * reads only what earlier launches wrote, and the host never synchronises.  logits [T, C] (a
 * time-major [T, 1, C] tensor is the same memory), labels int32 [L].
 *
 * PINNED: the arithmetic is K11's, operation for operation.
 *   - the fp32 log-softmax table per frame: mx = the sequential fmaxf over the row, sum = the
 *     sequential sum of expf(row[c] - mx), lz = mx + logf(sum), table[c] = row[c] - lz;
 *   - the lattice in fp64: delta_0(0) = table_0[blank], delta_0(1) = table_0[l_1], delta_t(s) =
 *     max(...) + (double)table_t[ext[s]]; predecessors compared with strict > in the order s,
 *     s - 1, s - 2, the skip s - 2 taken only into a non-blank state with ext[s] != ext[s - 2];
 *   - at the end S - 1 wins over S - 2 unless S - 2 is strictly better.
 * Max and add do not depend on how the lattice is tiled: path, score and frame_logp are a pure
 * function of the table, bit for bit, for every tile_frames, and equal K11's where K11 serves
 * (its float score is this one rounded).  Tiles through which no path from the start to the end
 * can pass are skipped; that changes no output.
 *   path       int32 [T]: the state of the best path at frame t (as K11)
 *   score      double [1]: the fp64 lattice value of the best path, unrounded (0 for T = 0, L = 0)
 *   frame_logp [T] table value of the class the path emits at frame t; may be NULL
 *   logp       [T, C] receives the table the lattice ran on (written whatever the status); may
 *              be NULL
 *   status     int32 [1]: 0 ok; 1 T < L + adjacent repeats; 2 a label id out of range or the
 *              blank; 3 a non-finite logit.  Non-zero: score -inf (NaN for 3), path -1 and
 *              frame_logp 0 throughout.  Every output is fully written.
 * Limits: C <= 64, T <= 2^22, L <= 2^20, at most 65536 tile rows (else CTCASR_ERR_UNSUPPORTED).
 * T = 0 is served (status 0 for L = 0, else 1) and needs no logits and no path; L = 0 needs no
 * labels.  Any other null pointer, a negative size or tile_frames, C < 2 or a blank outside
 * [0, C): CTCASR_ERR_BAD_ARGUMENT, before the device is touched.  Workspace:
 * ctcasr_ctc_align_long_workspace_bytes(T, C, L, tile_frames) bytes (0 for arguments the call
 * would refuse), 8-byte aligned; its contents on entry do not matter.  It holds the table, 2
 * bits of back-pointer per cell, one fp64 per state and tile row, one fp64 per frame and tile
 * column. */
#define CTCASR_ALIGN_LONG_TILE_STATES 1024
#define CTCASR_ALIGN_LONG_TILE_FRAMES 256
size_t ctcasr_ctc_align_long_workspace_bytes(int64_t T, int C, int64_t L, int tile_frames);
int ctcasr_ctc_align_long(const float *logits, const int32_t *labels, int64_t T, int C, int blank,
                          int64_t L, int tile_frames, int32_t *path, double *score,
                          float *frame_logp, float *logp, int32_t *status, void *workspace,
                          size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K25: CTC forced alignment with wildcard spans ----------------------------------------------
 * K21 for a text that covers only part of the recording.  The signature, the outputs, the status
 * words, the workspace (ctcasr_ctc_align_long_workspace_bytes) and the limits are K21's; the one
 * difference is that a label may be CTCASR_ALIGN_WILDCARD: "something is said here that the text
 * does not hold", any number of frames >= 1, at the price the greedy path pays for those frames.
 * A wildcard in front of the first label and one behind the last free the ends.  (An added entry
 * point, as K19 - K24: CTCASR_ABI_VERSION stays.)
 *
 * PINNED: the wildcard is one more class.
 *   - its log-probability at frame t is fill[t] = the fmaxf over table_t[0 .. C-1], fp32, of the
 *     table K21 builds (what the greedy path emits at t);
 *   - in the lattice it is an ordinary label state: at an odd s, a blank on either side, at least
 *     one frame; it differs from every label, so the skip s - 2 into it and out of it is allowed;
 *   - everything else is K21's, operation for operation: delta = max(...) + (double)emission in
 *     fp64, strict > in the order s, s - 1, s - 2, S - 1 over S - 2 at the end, 2-bit
 *     back-pointers, the same tiles and the same rule for skipping them.
 * Reference semantics: append to the table a column C that holds fill and give the wildcard the
 * id C; the result is K21's on that table of C + 1 classes (tests/align_partial_reference.py).
 * The limit C <= 64 counts real classes: the column exists in no buffer, logp stays [T, C].
 *   path       as K21; a wildcard sits at an odd state like any label
 *   frame_logp fill[t] on a frame the path spends in a wildcard
 *   score      the fp64 sum along the path, wildcard frames included
 *   status     2 also for a label that is neither the wildcard nor a valid non-blank class, and
 *              for two wildcards side by side; 1 T < L + adjacent repeats, where a wildcard
 *              counts as a label and never as a repeat; 3 as K21.  The order 2, 1, 3 and the
 *              outputs of a sequence without a path are K21's.
 * Without a wildcard among the labels every output equals ctcasr_ctc_align_long's, bit for bit,
 * for every tile_frames.  ctcasr_ctc_align_long itself keeps refusing -1 with status 2.
 * Left out on purpose: a wildcard that may take no frame, optional words, a price per wildcard
 * frame. */
#define CTCASR_ALIGN_WILDCARD (-1)
int ctcasr_ctc_align_partial(const float *logits, const int32_t *labels, int64_t T, int C,
                             int blank, int64_t L, int tile_frames, int32_t *path, double *score,
                             float *frame_logp, float *logp, int32_t *status, void *workspace,
                             size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K22: CTC phrase spotting -------------------------------------------------------------------
 * Is this phrase said in here, and where?  (No counterpart in the reference.)  P phrases, each
 * stored once, scored against the logits directly: pair h runs phrase pair_phrase[h] over
 * utterance pair_utt[h] on a Viterbi lattice with a free start and a free end, and the hits -
 * non-overlapping spans whose score reaches the phrase's threshold - are picked on the device.
 * One wavefront per pair, the lattice in registers (K14's shape).  (An added entry point, as
 * K19 - K21: CTCASR_ABI_VERSION stays.)
 *   logits, seq_len  as ctcasr_ctc_score takes them; blank is any id in [0, C)
 *   labels         int32, the concatenated label ids of the P phrases
 *   label_offsets  int32 [P + 1]
 *   min_score      double [P]: the threshold of phrase p (<= 0 to be of use; NaN: no hit ever)
 *   pair_utt, pair_phrase  int32 [H]: any order, any subset, any repetition
 *
 * PINNED: the arithmetic (tests/search_reference.py restates it).
 *   - table = the output of ctcasr_log_softmax_fwd on the logits, bit for bit.
 *   - fill[t, b] = the fmaxf over table[t, b, 0 .. C-1], fp32: what the greedy path emits.  A row
 *     of the table that is NaN (a NaN or +inf logit, or a row of -inf, makes one) has fill NaN.
 *   - a phrase of L >= 1 labels has S = 2L - 1 states, no blank in front and none behind: even
 *     u is label lab[u / 2], odd u is the blank.
 *   - cost_t(u) = (double)table[t, b, ext(u)] - (double)fill[t, b], never positive.
 *   - the lattice: fp64, max-sum, over frames 0 <= t < seq_len[b]; state u carries a value
 *     d_t(u) and the frame s_t(u) at which its path entered state 0.  Candidates in this order,
 *     a later one replacing the best so far only when strictly greater, starting from -inf:
 *       1. stay   d_{t-1}(u);
 *       2. step   d_{t-1}(u - 1), u >= 1;
 *       3. skip   d_{t-1}(u - 2), even u >= 2 with lab[u/2] != lab[u/2 - 1];
 *       4. entry  u == 0 only: the value 0.0 with start t.
 *     The first three do not exist at t = 0.  d_t(u) = best + cost_t(u); whenever that is -inf
 *     the start is -1.
 *   - end_score[h, t] = d_t(S - 1), end_start[h, t] = s_t(S - 1); -inf and -1 for t >= seq_len.
 *     end_score[t] is the log of (best path through the phrase that ends at t) over (the greedy
 *     path on the same frames): 0 exactly when the two coincide.
 *   - best_score / best_span = the first t, by strict >, that reaches the largest end_score,
 *     with its start: (start, t).  -inf and (-1, -1) when nothing is finite.
 *   - hits: one pass in ascending t with pending = none, flushed_end = -1.  Frame t is a
 *     candidate (score, start, t) when end_score[t] > -inf and end_score[t] >= min_score[phrase].
 *     The first rule that applies handles it:
 *       1. start <= flushed_end: dropped;
 *       2. no pending: it becomes pending;
 *       3. start <= pending.end: it replaces pending when score > pending.score, or when score
 *          == pending.score and start == pending.start (the same occurrence, its last label held
 *          longer); otherwise it is dropped;
 *       4. otherwise pending is flushed - appended, flushed_end = pending.end - and the
 *          candidate becomes pending.
 *     After the last frame pending is flushed.
 *   hits       int32 [H, max_hits, 2]: (start, end) frames, both inclusive, of the first max_hits
 *              flushed hits; pairwise disjoint, ascending.  NULL iff max_hits == 0
 *   hit_score  double [H, max_hits].  NULL iff max_hits == 0
 *   n_hits     int32 [H]: every flushed hit counts, stored or not.  Rows of hits / hit_score at
 *              or beyond min(n_hits, max_hits) hold (-1, -1) and -inf
 *   best_score double [H], best_span int32 [H, 2]
 *   end_score  double [H, T], end_start int32 [H, T]: each may be NULL
 *   status     int32 [H]: 0 ok; 1 seq_len < L + adjacent repeats (no span exists: the outputs
 *              hold the no-hit values above); 2 a label id out of range or the blank, L == 0,
 *              L > max_label_len or a negative row, pair_utt or pair_phrase out of range,
 *              seq_len > T or < 0; 3 fill is NaN in some frame t < seq_len of the utterance.
 *              2 and 3: n_hits 0, span (-1, -1), hit rows empty, best_score and end_score[0 .. T)
 *              -inf for 2 and NaN for 3, end_start -1.
 * Frames at or beyond seq_len are never read by a pair.  A pair's outputs do not depend on the
 * other pairs of the call or on their order, bit for bit.  Every output element is written.
 * C <= 64, 2 * max_label_len - 1 <= 1151, max_hits <= 1024 (else CTCASR_ERR_UNSUPPORTED).  A
 * negative size, C < 2, a blank outside [0, C), a null required pointer, hits / hit_score null
 * while max_hits > 0: CTCASR_ERR_BAD_ARGUMENT, before the device is touched.  H == 0 returns
 * CTCASR_OK and launches nothing.  Workspace: ctcasr_ctc_search_workspace_bytes(T, B, C) (the
 * table and fill); a short one gives CTCASR_ERR_WORKSPACE; its contents on entry do not matter. */
size_t ctcasr_ctc_search_workspace_bytes(int T, int B, int C);
int ctcasr_ctc_search(const float *logits, const int32_t *seq_len, int T, int B, int C, int blank,
                      const int32_t *labels, const int32_t *label_offsets, int P, int max_label_len,
                      const double *min_score, const int32_t *pair_utt, const int32_t *pair_phrase,
                      int H, int max_hits, int32_t *hits, double *hit_score, int32_t *n_hits,
                      double *best_score, int32_t *best_span, double *end_score,
                      int32_t *end_start, int32_t *status, void *workspace, size_t workspace_bytes,
                      ctcasr_stream_t stream);

/* ---- K13: edit distance ------------------------------------------------------------------------
 * Replaces tf.edit_distance(decoded, labels) (asr/model.py:338) and the Levenshtein distance of
 * asr/util/metrics.py:110-141, for a whole batch in one launch, and adds the error breakdown.
 * Pair b compares hyp[hyp_offsets[b] .. + hyp_len[b]) with ref[ref_offsets[b] .. + ref_len[b]);
 * symbols are arbitrary int32 (label ids, word ids).  Offsets plus lengths serve the decoders'
 * dense out [B, T] / out_len (hyp_offsets[b] = b * T) and the CTC loss's packed labels alike;
 * rows may overlap and hyp may be ref.  Unit costs.
 *   distance       int32 [B]: the Levenshtein distance
 *   substitutions  int32 [B] (S), deletions (D: reference symbols left unmatched), insertions
 *                  (I: hypothesis symbols inserted); each of the three may be NULL
 *   status         int32 [B]: 0 ok; 2 a length that is negative (the beam search's out_len = -1
 *                  included) or above its max_*_len - the four outputs of that pair are -1
 * Tie rule: the counts are those of the alignment with the fewest substitutions among all
 * alignments of minimum distance - the lexicographic minimum of (distance, S), which does not
 * depend on the order in which alignments are visited.  distance = S + D + I and
 * D - I = ref_len - hyp_len, so (distance, S) fixes all four; results are bit-reproducible.
 * A length of 0 on either side is valid (distance = the other length, all D or all I).  Every
 * output is fully written.  max_hyp_len, max_ref_len <= 32767 (else CTCASR_ERR_UNSUPPORTED);
 * B < 1 is CTCASR_ERR_BAD_ARGUMENT.  Workspace: ctcasr_edit_distance_workspace_bytes(B,
 * max_hyp_len, max_ref_len) - 0 while the kernel's carry columns fit in LDS, and `workspace`
 * may then be NULL. */
size_t ctcasr_edit_distance_workspace_bytes(int B, int max_hyp_len, int max_ref_len);
int ctcasr_edit_distance(const int32_t *hyp, const int32_t *hyp_offsets, const int32_t *hyp_len,
                         const int32_t *ref, const int32_t *ref_offsets, const int32_t *ref_len,
                         int B, int max_hyp_len, int max_ref_len, int32_t *distance,
                         int32_t *substitutions, int32_t *deletions, int32_t *insertions,
                         int32_t *status, void *workspace, size_t workspace_bytes,
                         ctcasr_stream_t stream);

/* ---- K4/K5: recurrence of one bidirectional RNN layer ----------------------------------------
 * Replaces the time loop of tfc.cudnn_rnn.Cudnn{LSTM,GRU,RNNRelu,RNNTanh}(direction=
 * 'bidirectional') (asr/model.py:194-215) and of stack_bidirectional_dynamic_rnn over
 * BasicRNNCell (asr/model.py:171-183).  The input projection W x + b_W (+ b_R where it commutes)
 * is a plain GEMM done by the caller; this entry point runs h_t = cell(xw_t, h_{t-1}).
 *   cell     CTCASR_CELL_*; G = gates per unit (LSTM 4: i,f,g,o; GRU 3: r,z,n; RNN 1)
 *   xw       [T, B, 2, G*H] pre-computed input projections, both directions
 *   xw_bias  [2, G*H] or NULL: added to xw inside the kernel (b_W, + b_R where it commutes) - the
 *            caller's GEMM then needs no bias epilogue; NULL when xw already includes the bias
 *   w_hh     [2, G*H, H] recurrent weights (cuDNN / torch layout, gate-major rows)
 *   b_hh_n   GRU only (NULL otherwise): the recurrent bias b_hh [2, 3H]; its candidate-gate third
 *            is applied inside r * (R_n h + b_Rn), the r / z thirds must be folded into xw
 *   seq_len  int32 [B] or NULL.  NULL = cuDNN semantics (all T steps for every row; the backward
 *            direction starts at t = T-1).  Non-NULL = dynamic_rnn semantics (steps
 *            t >= seq_len[b] emit zeros and keep the state; backward direction reversed per row).
 *   y        [T, B, 2H]  = [h_fw || h_bw]
 *   reserve  activations kept for the backward pass, ctcasr_rnn_reserve_bytes()
 *   workspace ctcasr_rnn_workspace_bytes() (state ping-pong, grid-barrier words, exchange
 *            buffer).  ZERO-FILL IT ONCE before its first use with a given (B, H): the launches
 *            themselves issue no memset - the arrival counters are reset by the kernel that used
 *            them, the all-zero block of the exchange buffer is never written, and the time-out
 *            word is sticky until ctcasr_rnn_poll_error reads it.  A workspace sized for T serves
 *            every T' <= T: the words that last from launch to launch sit at offsets that do not
 *            depend on T (B = 33 .. 64: the all-zero block of the second row block does move, and
 *            the first launch of a pass clears it).
 * bwd: dy [T,B,2H] -> dxw [T,B,2,G*H] (gradient w.r.t. xw, which is also what the weight
 * gradients are GEMMs of), w_hh_t = w_hh transposed to [2, H, G*H] (caller keeps it current;
 * ctcasr_transpose_batched does it).  GRU: the recurrent path differs from dxw in the candidate
 * gate (scaled by r); that tensor, drec [T,B,2,3H], is left in `reserve` at
 * ctcasr_rnn_gru_drec_offset(): dW_hh is a GEMM of it.
 *   dbias    (optional) bias gradients, ACCUMULATED into (caller zeroes them before a pass):
 *            [2, G*H] column sums of dxw over (t, b) = db_ih, then - GRU only - [2, 3H] column sums
 *            of drec = db_hh (for the other cells db_hh = db_ih).  Complete once the launch that
 *            covers step 0 has run (the persistent kernels add each launch's share, the
 *            streaming path sums the whole pass at its end).  Summation order is not fixed
 *            (atomics), like ctcasr_colsum_accumulate's. */
size_t ctcasr_rnn_gru_drec_offset(int T, int B, int H);
size_t ctcasr_rnn_reserve_bytes(int cell, int T, int B, int H);
size_t ctcasr_rnn_workspace_bytes(int cell, int T, int B, int H);
int ctcasr_rnn_fwd(int cell, const float *xw, const float *xw_bias, const float *w_hh,
                   const float *b_hh_n, const int32_t *seq_len, int T, int B, int H, float *y,
                   void *reserve, void *workspace, size_t workspace_bytes, ctcasr_stream_t stream);
/* Steps [step_begin, step_end) of the forward recurrence only; ctcasr_rnn_fwd == (0, T).  A pass may
 * be cut into launches covering 0..T in ascending order on the same workspace and reserve: after
 * a launch, y of the steps it covered is final (time s of the forward direction, time
 * seq_len-1-s of the backward direction), so the next layer's input projection of those steps
 * can run on another stream while the next launch continues the recurrence.
 *
 * `flags` (CTCASR_RNN_*) picks the variant of the persistent kernel for THIS call - there is no
 * process-wide state, so calls from different threads / streams do not interact:
 *   CTCASR_RNN_DEFAULT     forward: all 256 CUs; backward: 128 CUs
 *   CTCASR_RNN_HALF_CHIP   128 CUs (64 workgroups per direction, weights split between LDS and
 *                          registers), so that GEMMs on another stream can run beside it
 *   CTCASR_RNN_WHOLE_CHIP  all 256 CUs
 * Batches of 17..32 rows are two independent 16-row tiles: on the whole chip each tile runs as
 * its own group of half-chip workgroups, on half of the chip as a second chain of 4 waves inside
 * every workgroup - each tile with its own barrier, results identical to one tile at a time.
 * Shapes without the requested variant, and the streaming kernels, ignore it. */
#define CTCASR_RNN_DEFAULT 0
#define CTCASR_RNN_HALF_CHIP 1
#define CTCASR_RNN_WHOLE_CHIP 2
/* batches of 17..32 rows: the round-1 kernels (both 16-row tiles behind ONE barrier per step)
 * instead of the default two independent chains per workgroup - for A/B measurements */
#define CTCASR_RNN_ONE_BARRIER 4
/* (value 8: the reduce-scatter backward form of ABI v3 - v7, removed in ABI v8.  The bit is unknown
 * now: a call that carries it returns CTCASR_ERR_BAD_ARGUMENT.) */
/* forward, LSTM / GRU on the persistent kernels (ABI v5): the recurrent product h W_hh^T on the
 * fp16 matrix pipe - h (|h| <= 1) and the workgroup's slice of W_hh (scaled by a power of two found
 * inside the kernel from the slice's largest magnitude, so no weight can overflow) as TWO fp16
 * pieces each, three piece products, fp32 accumulation: fp32-grade (22 significand bits, the
 * dropped term <= 2^-22 of a product), not bit-equal to the fp32-MFMA kernel.  Every launch of one
 * pass (step ranges) must carry the same value of this bit: the exchange buffer then holds h as
 * its two pieces.  The backward kernels and everything else are unaffected (y, the reserve and
 * the carry stay fp32).  Other cells / shapes / CTCASR_RNN_ONE_BARRIER ignore the bit. */
#define CTCASR_RNN_F16 16
/* fp16-pipe kernels, both directions in one launch: direction 0's workgroups on XCDs 0 - 3,
 * direction 1's on XCDs 4 - 7 (workgroup b runs on XCD b % 8) - every exchange block crosses the
 * fabric into four L2s instead of eight.  Same results bit for bit (ABI v5). */
#define CTCASR_RNN_XCD_SPLIT 32
/* backward, LSTM with H = 1024 on the fp16 pipe, 24 or 32 rows (17..32 and a multiple of 8: tile 1's
 * rows then start on a cache line of their own in the exchange buffer; ABI v7 - other batches keep
 * the one-barrier kernel) on half of the chip: the two 16-row tiles staggered by half a step (prnn_bwd16s_kernel: each tile with its own arrival counters, one
 * tile's exchange round trip under the other tile's loads) instead of both behind one barrier.
 * Same results bit for bit; every launch of a pass may choose freely.  Calls with per-row lengths
 * and other shapes ignore it.  (ABI v6) */
#define CTCASR_RNN_STAGGER 64
/* backward, LSTM with H = 2048 on the fp16 pipe: the K-pair form (prnn_bwd16w_kernel with a K
 * split, ABI v7) - pairs of workgroups on one XCD share 16 hidden units, each holds one K half of
 * their weights, reads only that half of the published dgates and hands its partner the partial
 * sums of the partner's units through L2.  Publishes exactly what the plain form publishes; results
 * agree with it to rounding (the order of the K sums differs; the hand-off carries a tag in the
 * lowest significand bit of each partial sum), step ranges bit-identical to one launch.  Every
 * launch of a pass may choose freely.  Other shapes ignore it (ABI v8: H = 1024 too, whose K-pair
 * form of the staggered kernel was removed). */
#define CTCASR_RNN_KPAIR 128
/* Residency ticket (bits 8..31 of `flags`, 0 = none): a persistent launch that carries one posts
 * it in the workspace once ALL of its workgroups are running; ctcasr_rnn_resident_gate() makes
 * another stream wait for exactly that (bounded).  Use: work for the CUs a half-chip launch
 * leaves free is enqueued behind such a gate, so that it cannot occupy the chip first and make
 * the persistent kernel wait for CUs.  Tickets are caller-chosen launch numbers in 1..2^24-1,
 * increasing per workspace, compared modulo 2^24.  (ABI v3; replaces ctcasr_stream_delay.) */
#define CTCASR_RNN_TICKET(ticket) ((int)(((unsigned)(ticket) & 0xFFFFFFu) << 8))
int ctcasr_rnn_fwd_steps(int cell, const float *xw, const float *xw_bias, const float *w_hh,
                         const float *b_hh_n, const int32_t *seq_len, int T, int B, int H,
                         float *y, void *y_pieces, void *reserve, void *workspace,
                         size_t workspace_bytes, int step_begin, int step_end, int flags,
                         ctcasr_stream_t stream);
/* ABI v5.  `y_pieces` (optional; only where ctcasr_rnn_fwd_f16_supported and seq_len == NULL, else
 * CTCASR_ERR_UNSUPPORTED): fp16 [T, B, 3, 2H] - the two fp16 pieces of y * 2^15 in the block
 * layout of ctcasr_split_f16(order 0, 0, 1), written by the fp16-pipe forward kernel itself (it
 * has them in registers: they are what it publishes to the other workgroups): the operand of the
 * next layer's forward projection / dense4 and of this layer's recurrent weight gradient, without
 * a split pass over y. */
int ctcasr_rnn_fwd_f16_supported(int cell, int T, int B, int H, int flags);
/* 1 when the LDS-resident single-launch kernels cover (cell, T, B, H) on this device, else the
 * per-step streaming kernels run.  CTCASR_RNN_MODE=stream in the environment forces the latter. */
int ctcasr_rnn_persistent_supported(int cell, int T, int B, int H);
/* Synchronises the stream and returns CTCASR_ERR_TIMEOUT if ANY persistent launch that used
 * `workspace` since the previous poll abandoned a grid barrier (the results of that pass are then
 * invalid), else CTCASR_OK.  The time-out word is sticky across launches, layers and passes and
 * is cleared by this call (after a time-out the barrier words and - ABI v7 - the write counts of
 * the K-split kernels' hand-off slots are zero-filled with it). */
int ctcasr_rnn_poll_error(void *workspace, size_t workspace_bytes, int cell, int T, int B,
                          int H, ctcasr_stream_t stream);
/* Enqueues a one-lane gate kernel on `stream` that returns as soon as the persistent launch that
 * carries CTCASR_RNN_TICKET(ticket) on this workspace has every workgroup running (or a later
 * ticket has been posted), and after `max_wait_us` (<= 100 ms) at the latest.  No-op for shapes
 * that take the streaming kernels and for `max_wait_us` = 0.
 * The predicate, exactly: with `seen` the ticket posted last on the workspace (0 in a zero-filled
 * one), the gate opens iff  seen != 0 && ((seen - ticket) & 0xFFFFFF) < 0x800000.
 *  - Staleness window: "posted at or after mine" reaches 2^23 - 1 tickets back.  A gate for a
 *    ticket 2^23 or more ahead of `seen` - a workspace whose last post lies more than 2^23 of the
 *    caller's tickets back - opens at once.  That costs the head start, never a result.
 *  - A launch that finds the time-out word set (ctcasr_rnn_poll_error) leaves at once, but it
 *    still posts its ticket first: a poisoned launch does not hold the work behind its gate for
 *    the whole bound.
 *  - A poll after a time-out zero-fills the barrier words, the posted ticket among them: the
 *    workspace has then posted nothing, and gates for earlier tickets wait again.
 * CTCASR_ERR_BAD_ARGUMENT for a ticket outside 1..2^24-1 or a bound outside 0..100000 us,
 * CTCASR_ERR_WORKSPACE for a workspace smaller than ctcasr_rnn_workspace_bytes(); neither
 * enqueues anything. */
int ctcasr_rnn_resident_gate(void *workspace, size_t workspace_bytes, int cell, int T, int B,
                             int H, unsigned ticket, int max_wait_us, ctcasr_stream_t stream);
int ctcasr_rnn_bwd(int cell, const float *dy, const float *y, const float *w_hh_t,
                   const float *b_hh_n, const int32_t *seq_len, int T, int B, int H,
                   const void *reserve, float *dxw, float *dbias, void *workspace,
                   size_t workspace_bytes, ctcasr_stream_t stream);
/* Steps [step_begin, step_end) of the backward recurrence only (it walks the steps downwards;
 * step s is time s of the forward direction and time seq_len-1-s of the backward direction).
 * ctcasr_rnn_bwd == (0, T).  A pass may be cut into launches covering T..0 in descending order
 * on the same workspace, e.g. (T/2, T) then (0, T/2): after a launch, dxw of the steps it
 * covered is final, so their share of the weight-gradient GEMMs can run on another stream while
 * the next launch continues the recurrence. */
int ctcasr_rnn_bwd_steps(int cell, const float *dy, const float *y, const float *w_hh_t,
                         const float *b_hh_n, const int32_t *seq_len, int T, int B, int H,
                         const void *reserve, float *dxw, float *dbias, uint32_t *colmax,
                         void *workspace, size_t workspace_bytes, int step_begin, int step_end,
                         int flags, ctcasr_stream_t stream);
/* ABI v5.  CTCASR_RNN_F16 in a BACKWARD call's flags (LSTM, H = 1024 on the persistent kernels;
 * ctcasr_rnn_bwd_f16_supported says whether a call qualifies, every other call ignores the bit):
 * dgates x W_hh on the fp16 matrix pipe - each producer workgroup scales every row of its 64 gate
 * columns by its own power of two and publishes two fp16 pieces, the consumer accumulates every
 * producer's block apart and adds it, unscaled, to an fp32 total; W_hh as in the forward kernel.
 * fp32-grade (22 significand bits per (row, 64-column block)), not bit-equal to the fp32 kernel.
 * `colmax` (optional, only with that kernel - else CTCASR_ERR_UNSUPPORTED): u32[2 * 4H], zeroed
 * by the caller; the kernel raises (atomicMax) word [dir][g H + unit] to the bit pattern of the
 * largest |dxw| of that column over the steps of the call - what ctcasr_colmax_scale's pass over
 * the finished rows of dxw would find (same values, no pass). */
int ctcasr_rnn_bwd_f16_supported(int cell, int T, int B, int H, int flags);
/* ABI v6: whether a recurrence call with these flags runs an fp16-pipe kernel at all (`backward`:
 * the backward pass; `ragged`: the call passes per-row lengths).  Differs from the two functions
 * above for the ReLU cell at H = 2048 (B <= 16, no lengths: round 5), whose forward kernel writes
 * no y_pieces. */
int ctcasr_rnn_f16_recurrence(int cell, int T, int B, int H, int flags, int backward, int ragged);

/* ---- fused dense / conv epilogues (tf.layers.dense + ReLU + tf.minimum(., relu_cutoff) +
 * tf.layers.dropout: asr/util/tf_contrib.py:50-61,122-135, asr/model.py:219-225) --------------
 * fwd (in place): y[r, c] = dropout(min(max(y[r, c] + bias[c], 0), cutoff)); inverted dropout
 *   with keep = 1 - rate, counter-based RNG keyed by (seed, element index); rate 0 = no dropout.
 *   `cutoff` <= 0 disables the activation entirely (plain bias add: the logits layer).
 * bwd: dz = dy * [0 < y < cutoff/keep] / keep * [y != 0] from the stored *output* y (no mask
 *   tensor is kept); dbias[c] += sum_r dz[r, c] when dbias != NULL (caller zeroes it).
 *   `cols` is the fastest dimension; for conv activations in NHWC pass rows = B*T*F, cols = C. */
int ctcasr_bias_act_fwd(float *y, const float *bias, int64_t rows, int cols, float cutoff,
                        float dropout_rate, uint64_t seed, ctcasr_stream_t stream);
int ctcasr_bias_act_bwd(const float *y, const float *dy, float *dz, float *dbias, int64_t rows,
                        int cols, float cutoff, float dropout_rate, ctcasr_stream_t stream);
/* Inverted dropout without activation (cuDNN's inter-layer RNN dropout, DropoutWrapper of the
 * BasicRNNCell path: asr/model.py:203, asr/util/tf_contrib.py:190-194): out = in * mask / keep,
 * mask regenerated from (seed, element index) - call it on the gradient with the same seed for
 * the backward pass.  in == out is allowed. */
int ctcasr_dropout(const float *in, float *out, int64_t n, float dropout_rate, uint64_t seed,
                   ctcasr_stream_t stream);
/* dbias[c] += sum_r dz[r, c] on its own (layers without activation). */
int ctcasr_colsum_accumulate(const float *dz, float *dbias, int64_t rows, int cols,
                             ctcasr_stream_t stream);

/* ---- the 11 x 21, stride (1, 2) convolutions over 32 input channels of the DS2 stack (layers 2
 * and 3 of conv_layers, asr/util/tf_contrib.py:64-146; TensorFlow SAME padding): forward pass and
 * data gradient and kernel gradient as implicit GEMMs on the fp32 MFMA units, NHWC, any number of frames, no padded
 * intermediates.  Covered (ctcasr_conv_s12_supported): freq_in = 40, cout = 32 and freq_in = 20,
 * cout = 96.
 *   fwd:       x  [B, T, freq_in, 32]       -> y  [B, T, freq_in/2, cout] = conv(x) + bias|NULL
 *   bwd_data:  dz [B, T, freq_in/2, cout]   -> dx [B, T, freq_in, 32]
 *   wrw:       dz, x                        -> dw [cout, 32, 11, 21]
 * `packed`: fragment-ordered copies of the kernel w [cout, 32, 11, 21] made by
 * ctcasr_conv_s12_pack_weights, 2 * 11*21*32*cout floats (backward order, then forward order). */
int ctcasr_conv_s12_supported(int freq_in, int cout);
int ctcasr_conv_s12_pack_weights(const float *w, float *packed, int cout, ctcasr_stream_t stream);
/* relu_cutoff > 0: the epilogue also applies min(max(., 0), relu_cutoff) (the ReLU + tf.minimum of
 * conv_layers; 0 = convolution + bias only).  y_time_major / dz_time_major != 0: that tensor is
 * laid out [T, B, F, C] instead of [B, T, F, C] - the last layer of the stack hands its output
 * to the recurrent stack (and takes its gradient back) without a transpose. */
/* ABI v5: the forward pass with its products on the fp16 matrix pipe (csrc/conv16.hip): input and
 * weights as two fp16 pieces each, three piece products per tap, fp32 accumulation - for inputs
 * with a known bound (behind the clipped ReLU of the previous layer): bound * x_scale < 65504,
 * x_scale a power of two.  The weights are packed per step by ctcasr_conv_s12_pack_weights16 into
 * `packed16` (ctcasr_conv_s12_pack16_bytes(cout) bytes: the bit pattern of max |w|, found on the
 * device, then the pieces in fragment order under the scale derived from it). */
size_t ctcasr_conv_s12_pack16_bytes(int cout);
int ctcasr_conv_s12_pack_weights16(const float *w, void *packed16, int cout,
                                   ctcasr_stream_t stream);
int ctcasr_conv_s12_fwd16(const float *x, float x_scale, const void *packed16, const float *bias,
                          float *y, int B, int T, int freq_in, int cout, float relu_cutoff,
                          int y_time_major, ctcasr_stream_t stream);
/* ... and the data gradient (arguments of ctcasr_conv_s12_bwd_data): dz has no bound, so every dz
 * frame of a workgroup's patch (all taps of one kt read one frame) gets its own power-of-two
 * scale while it is staged; the weights' pieces are the backward-order half of `packed16`. */
int ctcasr_conv_s12_bwd_data16(const float *dz, const void *packed16, float *dx, int B, int T,
                               int freq_in, int cout, int dz_time_major, const float *act,
                               float relu_cutoff, ctcasr_stream_t stream);
/* ... and the kernel gradient (arguments of ctcasr_conv_s12_wrw plus x_scale as in
 * ctcasr_conv_s12_fwd16): the summation runs over (b, t, fo), so x * x_scale and the masked dz -
 * scaled per OUTPUT CHANNEL by the power of two that the channel's largest magnitude asks for,
 * found on the device - are first written to `workspace` as fp16 pieces with 8 utterances
 * innermost (the one axis no tap shifts), then one launch multiplies (asr/util/tf_contrib.py:64-146
 * under tf.gradients). */
size_t ctcasr_conv_s12_wrw16_workspace_bytes(int B, int T, int freq_in, int cout);
int ctcasr_conv_s12_wrw16(const float *dz, const float *x, float x_scale, float *dw, int B, int T,
                          int freq_in, int cout, int dz_time_major, const float *act,
                          float relu_cutoff, float *dbias, void *workspace,
                          size_t workspace_bytes, ctcasr_stream_t stream);
int ctcasr_conv_s12_fwd(const float *x, const float *packed, const float *bias, float *y, int B,
                        int T, int freq_in, int cout, float relu_cutoff, int y_time_major,
                        ctcasr_stream_t stream);
/* Backward of the fused epilogue (round 3): `act` != NULL is the layer's stored OUTPUT (same
 * layout as dz) and `dz` the gradient w.r.t. that output - the kernels apply the mask
 * [0 < act < relu_cutoff] while they stage dz, so no elementwise pass runs in front of them; the
 * wrw kernels then also ADD the bias gradient (column sums of the masked dz over b, t, f) to
 * dbias[cout] when it is non-NULL (caller zeroes it; atomics: summation order not fixed).
 * `act` NULL: dz is the pre-activation gradient already (relu_cutoff ignored). */
int ctcasr_conv_s12_bwd_data(const float *dz, const float *packed, float *dx, int B, int T,
                             int freq_in, int cout, int dz_time_major, const float *act,
                             float relu_cutoff, ctcasr_stream_t stream);
/*   wrw: dz [B, T, freq_in/2, cout], x [B, T, freq_in, 32] -> dw [cout, 32, 11, 21] (overwritten):
 *        the kernel gradient, split over (b, t) tiles with a deterministic two-stage reduction;
 *        workspace: per-split partial sums, ctcasr_conv_s12_wrw_workspace_bytes(B, T, freq_in, cout) */
size_t ctcasr_conv_s12_wrw_workspace_bytes(int B, int T, int freq_in, int cout);
int ctcasr_conv_s12_wrw(const float *dz, const float *x, float *dw, int B, int T, int freq_in,
                        int cout, int dz_time_major, const float *act, float relu_cutoff,
                        float *dbias, void *workspace, size_t workspace_bytes,
                        ctcasr_stream_t stream);

/* ---- the first DS2 convolution: 1 -> 32 channels, 11 x 41 taps, stride (2, 2), SAME padding ----
 *   fwd: x [B, T, 80] -> y [B, ceil(T/2), 40, 32] (NHWC) = conv(x) + bias|NULL; w [32, 1, 11, 41] */
int ctcasr_conv0_fwd(const float *x, const float *w, const float *bias, float *y, int B, int T,
                     float relu_cutoff, ctcasr_stream_t stream);
/*   wrw: dz [B, ceil(T/2), 40, 32] (NHWC), x [B, T, 80] -> dw [32, 1, 11, 41] (overwritten);
 *        workspace: per-workgroup partial sums, ctcasr_conv0_wrw_workspace_bytes(B, T) */
size_t ctcasr_conv0_wrw_workspace_bytes(int B, int T);
int ctcasr_conv0_wrw(const float *dz, const float *x, float *dw, int B, int T, const float *act,
                     float relu_cutoff, float *dbias, void *workspace, size_t workspace_bytes,
                     ctcasr_stream_t stream);

/* ... the same two on the fp16 matrix pipe (round 4; csrc/conv16.hip).  fwd16: the weights as
 * fp16 pieces in fragment order (`packed16`: ctcasr_conv0_pack16_bytes() bytes, re-packed every
 * step, scale found on the device); the features have no bound, every workgroup scales its own
 * input patch by the power of two its largest magnitude asks for.  wrw16: dz scaled per output
 * channel, x by the tensor's largest magnitude, both written to `workspace` as fp16 pieces with
 * 8 utterances innermost (see ctcasr_conv_s12_wrw16). */
size_t ctcasr_conv0_pack16_bytes(void);
int ctcasr_conv0_pack_weights16(const float *w, void *packed16, ctcasr_stream_t stream);
int ctcasr_conv0_fwd16(const float *x, const void *packed16, const float *bias, float *y, int B,
                       int T, float relu_cutoff, ctcasr_stream_t stream);
size_t ctcasr_conv0_wrw16_workspace_bytes(int B, int T);
int ctcasr_conv0_wrw16(const float *dz, const float *x, float *dw, int B, int T, const float *act,
                       float relu_cutoff, float *dbias, void *workspace, size_t workspace_bytes,
                       ctcasr_stream_t stream);

/* out[n][c][r] = in[n][r][c] for n < batch (weight re-layouts, e.g. w_hh -> w_hh_t). */
int ctcasr_transpose_batched(const float *in, float *out, int batch, int rows, int cols,
                             ctcasr_stream_t stream);

/* ---- fp32 operands of the dense / input-projection GEMMs, split for the bf16 matrix pipe ---------
 * The GEMMs of asr/model.py:166-171 (dense), :203-214 (cuDNN RNN input projections) and their
 * gradients are fp32 x fp32 -> fp32.  gfx950 has no xf32 and its fp32 MFMA runs at 1/16 of the bf16
 * rate, so the host side may feed the library GEMM three-piece bfloat16 splits instead:
 *   x = x1 + x2 + x3,  x1 = rne_bf16(x), x2 = rne_bf16(x - x1), x3 = rne_bf16(x - x1 - x2)
 * (both differences are exact in fp32; 24 mantissa bits in all) and sum the six products of order
 * <= 2 (x1w1; x1w2 + x2w1; x1w3 + x2w2 + x3w1) with fp32 accumulation - every term down to 2^-24
 * relative, i.e. what an fp32 FMA chain keeps.
 *   x     f32 [rows, cols], row stride ld_x elements (cols % 8 == 0, ld_x % 4 == 0, 16-byte aligned)
 *   order host int[blocks], piece index (0, 1, 2) held by each block, blocks <= 6
 *   out   bf16, element (r, b, c) at r * ld_out + b * block_stride + c (both strides in elements,
 *         multiples of 8, 16-byte aligned base).  ld_out = blocks * cols, block_stride = cols is the
 *         K-concatenated form [rows, blocks, cols]: order {0,1,2,0,1,0} against a second operand
 *         split with {2,1,0,1,0,0} makes ONE bf16 GEMM over K = 6 * cols the whole product;
 *         ld_out = cols, block_stride = rows * cols stacks the blocks along the rows instead (for an
 *         operand whose K axis is its row axis); wider strides write a column range of a bigger
 *         matrix. */
#define CTCASR_SPLIT_MAX_BLOCKS 6
int ctcasr_split_bf16(const float *x, int64_t rows, int cols, int64_t ld_x, const int *order,
                      int blocks, void *out, int64_t ld_out, int64_t block_stride,
                      ctcasr_stream_t stream);

/* Forward projections of BOUNDED operands (activations behind a clipped ReLU, |h| <= 1 of an LSTM /
 * GRU / tanh cell, weights) also go in TWO fp16 pieces of x * scale - h1 = rne_f16(x scale),
 * h2 = rne_f16(x scale - h1), 11 + 11 mantissa bits - and three products h1 k1 + h1 k2 + h2 k1
 * (dropped: h2 k2 <= 2^-22): measured error = the fp32 GEMM's, at half the bf16 form's cost.
 *   scale  a power of two with |x| * scale < 65504 for every element (the caller knows the bound);
 *   order  host int[blocks] of 0 (h1) / 1 (h2); out / ld_out / block_stride as above, fp16.
 * The product of two such operands carries scale_x * scale_w: fold 1 / that into the GEMM's alpha. */
int ctcasr_split_f16(const float *x, int64_t rows, int cols, int64_t ld_x, float scale,
                     const int *order, int blocks, void *out, int64_t ld_out,
                     int64_t block_stride, ctcasr_stream_t stream);

/* Operands WITHOUT a bound (the gradients dxw: 1e-13 .. 1e-2 inside one matrix) take the same
 * two-piece form with a power-of-two scale per column or per row - along whichever axis is NOT the
 * product's K axis, so that the scale factors out of the sum: per column of dxw (per gate unit)
 * for the weight gradients dW = dxw^T x, per row (per frame) for the data gradient dx = dxw W.
 * The largest magnitude of a column / row lands in [2^13, 2^14); smaller elements keep 22 bits down
 * to 2^-18 of it, never less than 2^-40 of it in absolute terms - measured on the operands of real
 * training steps the weight gradients come out with the fp32 GEMM's error (1.03e-6 vs 1.07e-6 rms
 * relative, profiles/r03_gemm_bf16_split.md).
 *   ctcasr_colmax_scale   scale[c] = 2^(13 - exponent(max_r |x[r][c]|)) (1 for an all-zero column)
 *                         and inv_scale[c] = 1 / scale[c]; workspace: 4 * cols bytes
 *   ctcasr_split_f16_cols two fp16 pieces of x[r][c] * col_scale[c] * scale (layout as above)
 *   ctcasr_split_f16_rows the same with the scale of each ROW found on the fly (one workgroup per
 *                         row, cols <= 16384); inv_scale[r] = 1 / scale of row r
 *   ctcasr_rescale_rows   out[r][c] (+)= t[r][c] * row_factor[r] * alpha: takes the scales back out
 *                         of a product (cols % 4 == 0, 16-byte aligned) */
int ctcasr_colmax_scale(const float *x, int64_t rows, int cols, int64_t ld_x, void *workspace,
                        float *scale, float *inv_scale, ctcasr_stream_t stream);
/* (ABI v5) the same scales from column maxima already known: max_bits u32[cols] = bit patterns of
 * max_r |x[r][c]| as ctcasr_rnn_bwd_steps(..., colmax, ...) leaves them */
int ctcasr_colscale_from_max(const uint32_t *max_bits, int cols, float *scale, float *inv_scale,
                             ctcasr_stream_t stream);
int ctcasr_split_f16_cols(const float *x, int64_t rows, int cols, int64_t ld_x,
                          const float *col_scale, float scale, const int *order, int blocks,
                          void *out, int64_t ld_out, int64_t block_stride, ctcasr_stream_t stream);
int ctcasr_split_f16_rows(const float *x, int64_t rows, int cols, int64_t ld_x, const int *order,
                          int blocks, void *out, int64_t ld_out, int64_t block_stride,
                          float *inv_scale, ctcasr_stream_t stream);
int ctcasr_rescale_rows(const float *t, int64_t ld_t, const float *row_factor, float alpha,
                        float *out, int64_t ld_out, int64_t rows, int cols, int accumulate,
                        ctcasr_stream_t stream);

/* The same product with the split done in registers by an own kernel (csrc/split_gemm.hip): no
 * split pass, no K-concatenated copies, no inter-workgroup waits.
 *   C[M, N] (+)= A[M, K] . B[N, K]^T    all fp32, row-major with leading dimensions lda / ldb / ldc
 *   (elements); K % 16 == 0, lda % 4 == ldb % 4 == 0, A and B 16-byte aligned; accumulate != 0 adds
 *   to C.  Result: the six bf16 piece products of order <= 2 in fp32 accumulation, as above. */
int ctcasr_gemm_split_nt(const float *a, int64_t lda, const float *b, int64_t ldb, float *c,
                         int64_t ldc, int m, int n, int k, int accumulate, ctcasr_stream_t stream);
/*   C[M, N] (+)= A[K, M]^T . B[K, N]   (K = the ROW axis of both operands: the weight gradients
 *   dW = dxw^T x of asr/model.py:203-214's layers); any K, no alignment requirement. */
int ctcasr_gemm_split_tn(const float *a, int64_t lda, const float *b, int64_t ldb, float *c,
                         int64_t ldc, int m, int n, int k, int accumulate, ctcasr_stream_t stream);

/* ABI v6: the data gradient of a recurrent layer's input projection straight from what the fp16
 * backward recurrence published (csrc/dgrad16.hip) - the gradient of the cuDNN input projection,
 * asr/model.py:194-215, which TensorFlow computes as one cuBLAS GEMM over dxw:
 *   dx[T * B, n] (+)= dxw[T * B, 2 * 4H] . W_ih[2 * 4H, n]
 * where dxw is NOT read as fp32: a pass of ctcasr_rnn_bwd_steps with CTCASR_RNN_F16 (LSTM,
 * H = 1024, B <= 32, every row running all T steps) has left each step's dgates in the workspace's
 * exchange buffer as two fp16 pieces per value, scaled per (row, 64 gate columns) by a power of two,
 * in MFMA operand order, with the inverse scales beside them; the kernel multiplies those into the
 * packed fp16 pieces of W_ih with one fresh accumulator per 32-column stage that enters the fp32
 * total times the row's inverse scale (22 significand bits relative to a (row, 64-column block)
 * maximum; piece product h2 w2 dropped).  No library GEMM, no inter-workgroup waits.
 *   workspace   the recurrence workspace the backward pass ran in (same T, B as that pass);
 *               valid until the next persistent launch in that workspace
 *   packed      ctcasr_dgrad16_packed_bytes(n) bytes from ctcasr_dgrad16_pack_weights(W_ih [2 * 4H,
 *               n] with leading dimension ld_w, scale): fp16 pieces of W_ih * scale (saturating at
 *               +-60000: the caller keeps |w| * scale in range; infinities saturate too, a NaN
 *               is KEPT in both pieces and makes its column of dx NaN), K order and fragment
 *               order of the exchange buffer
 *   [t_lo, t_hi)    the time steps (rows t * B .. ) to produce;  [dir_lo, dir_hi) the directions
 *               whose gate columns enter the sum (0..2: both) - a finished direction / step range
 *               can be multiplied while the other is still running, the rest added later
 *               (accumulate != 0)
 * ctcasr_dgrad16_supported says whether (cell, T, B, H) qualifies.
 * ctcasr_dgrad16_published_offsets: byte offsets inside the recurrence workspace of the exchange
 * blocks (block 0 all-zero, block 1 + s = step s: [dir][producer][half][piece][k group][b][8 halves],
 * step s = time s of direction 0 and time T - 1 - s of direction 1) and of the inverse scales
 * ([step][dir][producer][32 rows] floats) of a pass over (T, B) - the layout contract between the
 * recurrence kernel and this one, exposed for tests and for other consumers of the pieces. */
size_t ctcasr_dgrad16_packed_bytes(int n);
int ctcasr_dgrad16_published_offsets(int T, int B, int hidden, size_t *exchange,
                                     size_t *inverse_scales);
int ctcasr_dgrad16_pack_weights(const float *w_ih, int64_t ld_w, int hidden, int n, float scale,
                                void *packed, ctcasr_stream_t stream);
int ctcasr_dgrad16_supported(int cell, int T, int B, int hidden);
int ctcasr_dgrad16_blockscaled(void *workspace, int T, int B, int hidden, const void *packed,
                               float scale, int n, float *dx, int64_t ld_dx, int t_lo, int t_hi,
                               int dir_lo, int dir_hi, int accumulate, ctcasr_stream_t stream);

/* ABI v6: the weight gradients of a recurrent layer's two matrices for one direction and step range
 * as one own kernel (csrc/wgrad16.hip; TensorFlow: cuDNN's RNN backward-weights, asr/model.py:194-215):
 *   dW_x[m, nx] += D^T X,  dW_y[m, ny] += D^T Y      (sums over the ROWS of D / X / Y)
 * from operands packed transposed - K = the row axis - as fp16 pieces in MFMA fragment order:
 * ctcasr_wgrad16_pack writes rows [row0, row0 + 32 * stages) of x [rows_total, cols] (leading
 * dimension ld_x; rows outside [0, rows_total) read as zeros - a negative / positive row0 shifts
 * an operand by time steps), each column times col_scale[c] (NULL: 1) times scale, saturating at
 * +-60000 (infinities too; a NaN is KEPT in both pieces, so that it reaches dW and the gradient
 * guard drops the step), into ctcasr_wgrad16_packed_bytes(stages, cols) bytes - every byte of
 * them is written: columns up to the next multiple of 16 as zeros.  ctcasr_wgrad16_gemm multiplies
 * `stages` stages of the packed D (m columns, inverse column scales inv_scale[m]) into stages
 * [x_stage0, x_stage0 + stages) of the packed X (nx columns, fixed scale x_scale) and - optional -
 * of the packed Y, and ACCUMULATES into dW_x / dW_y (row-major, leading dimensions ld_*): two fp16
 * pieces per operand, three products, fp32 accumulation, no library GEMM.  Tiles of 256 x 256
 * outputs; `parts` >= 1 cuts every tile's row sum into that many workgroups (for launches whose
 * tiles alone do not fill the chip), which add to dW in part order through the words of `sync`
 * (ctcasr_wgrad16_sync_ints(m, nx, ny) int32, ZERO before the first launch that uses them; every
 * launch leaves them zero; parts < 4096).  A tile's word is 0 while no launch adds to the tile:
 * part 0 takes it by compare-and-swap, part q > 0 adds when it reads this launch's number << 12 | q,
 * the last part hands it back as 0, so launches of different streams that share the words take
 * turns at a tile.  The launch number is drawn when ctcasr_wgrad16_gemm is CALLED: two launches
 * that carry the same number must not be in flight together - a call with parts > 1 captured
 * into a graph may be replayed one after the other, not on two streams at once.  ABI v7: a part that gives up
 * waiting (bounded; ctcasr_set_option("wgrad16_spin_limit", polls) shortens the bound for tests)
 * sets word 0 and leaves WITHOUT adding and without passing the turn on; while word 0 is set
 * every launch on these words returns at once.  The caller folds word 0 into the optimizer's skip
 * flag (ctcasr_step_guard's wgrad_word), raises, and zeroes the words before the next launch.
 * sync may be NULL for parts == 1. */
size_t ctcasr_wgrad16_packed_bytes(int stages, int cols);
size_t ctcasr_wgrad16_sync_ints(int m, int nx, int ny);
int ctcasr_wgrad16_pack(const float *x, int64_t ld_x, int64_t rows_total, int cols, int64_t row0,
                        int stages, const float *col_scale, float scale, void *packed,
                        ctcasr_stream_t stream);
int ctcasr_wgrad16_gemm(const void *d_packed, int m, int stages, const float *inv_scale,
                        const void *x_packed, int x_stage0, int nx, float x_scale, float *dw_x,
                        int64_t ld_x, const void *y_packed, int y_stage0, int ny, float y_scale,
                        float *dw_y, int64_t ld_y, int parts, int32_t *sync, ctcasr_stream_t stream);

/* ---- K12: TensorFlow-form Adam over a flat parameter arena ------------------------------------
 * Replaces tf.train.AdamOptimizer(lr, beta1, beta2, epsilon).minimize (asr/model.py:80-83):
 *   lr_t = lr * sqrt(1 - beta2^step) / (1 - beta1^step);  m, v updated in place;
 *   param -= lr_t * m / (sqrt(v) + epsilon)     (epsilon OUTSIDE the bias correction).
 * `step` counts from 1.  grad is scaled by grad_scale first (1/world_size after a summed
 * all-reduce). */
int ctcasr_adam_step(float *param, const float *grad, float *m, float *v, int64_t n, float lr,
                     float beta1, float beta2, float epsilon, int64_t step, float grad_scale,
                     const int32_t *skip, ctcasr_stream_t stream);
/* ABI v5: `skip` (optional device word): the launch leaves param, m and v untouched when it is
 * non-zero - a step whose gradients are known to be invalid never reaches the parameters, without
 * the host having to look first.  ctcasr_step_guard fills it:
 *   skip[0] = any ctc_status[b] != 0 (tf.nn.ctc_loss would have raised, asr/model.py:259)
 *             | any per_utterance_loss[b] not finite | any persistent-recurrence time-out word
 *             (device pointers to the sticky words of up to two row blocks of the workspace,
 *             ctcasr_rnn_timeout_word_offset; either may be NULL)
 *             | *wgrad_word (ABI v7; may be NULL: word 0 of ctcasr_wgrad16_gemm's `sync`, raised
 *             by a part of a weight-gradient tile that gave up waiting for its turn - it and
 *             every later part then leave without adding);
 *   skip[1] = the time-out words or-ed together, bit 30 for the weight-gradient word (the host
 *             can poll this copy asynchronously - ctcasr_rnn_poll_error synchronises). */
int ctcasr_step_guard(const int32_t *ctc_status, const float *per_utterance_loss, int batch,
                      const uint32_t *timeout_word0, const uint32_t *timeout_word1,
                      const int32_t *wgrad_word, int32_t *skip, ctcasr_stream_t stream);
/* The same launch with a factor that is still on the device (ctcasr_grad_norm's clip_factor):
 *   gr = grad[i] * (grad_scale * *grad_factor),   the inner product formed once in fp32.
 * grad_factor == NULL is a factor of 1 - ctcasr_adam_step is this call with NULL - and a factor of
 * exactly 1.0f gives that call's results bit for bit.  `skip` still wins over any factor. */
int ctcasr_adam_step_clipped(float *param, const float *grad, float *m, float *v, int64_t n,
                             float lr, float beta1, float beta2, float epsilon, int64_t step,
                             float grad_scale, const int32_t *skip, const float *grad_factor,
                             ctcasr_stream_t stream);
/* ... and with the exponential moving average of the parameters in the same launch: param,
 * m and v come out as ctcasr_adam_step_clipped leaves them for the same arguments, bit for bit
 * (the same expressions in the same order), and
 *   ema[i] = ema[i] + ema_alpha * (param_new[i] - ema[i])        in fp32,
 * TensorFlow's assign_sub(ema, (1 - decay) * (ema - param)): param_new is the fp32 value this
 * launch has just formed, read from its registers; the subtraction, the product and the sum each
 * round once (or the last two as one fused multiply-add - either way within 3 * 2^-24 *
 * (|param_new| + |ema|) of the exact result).  ema_alpha = 1 - decay_t, formed by the host in
 * float64 and rounded once; 0 leaves a finite average as it is.  A NaN or inf parameter reaches
 * the average.  skip[0] != 0 leaves all four arrays untouched.  ema: fp32 [n], 16-byte aligned,
 * NULL is CTCASR_ERR_BAD_ARGUMENT (callers without an average call the entries above), and so is
 * an ema_alpha outside [0, 1] or NaN.  36 B of traffic per parameter instead of 28. */
int ctcasr_adam_step_ema(float *param, const float *grad, float *m, float *v, float *ema,
                         int64_t n, float lr, float beta1, float beta2, float epsilon,
                         int64_t step, float grad_scale, const int32_t *skip,
                         const float *grad_factor, float ema_alpha, ctcasr_stream_t stream);

/* ---- K14: gradient norms per segment, global norm, clip factor, guard -------------------------
 * No counterpart in the reference (it does not clip).  One read of grad; nothing leaves the
 * device, so the optimizer can be enqueued behind it without the host knowing a norm.
 *   grad         fp32 [n], 16-byte aligned (the flat gradient arena)
 *   seg_offsets  DEVICE int64 [segments + 1], ascending, [0] = 0, [segments] = n, every interior
 *                offset a multiple of 4 (the arena starts every tensor on 16 bytes; its layer
 *                slices are the segments).  Empty segments are allowed.  A table that breaks these
 *                rules never makes the kernels read outside grad[0, n): they clamp every entry
 *                into [0, n], make the table ascending and round every entry but the last down to
 *                a multiple of 4 - the norms of such a table mean nothing.
 *   norms        fp32 [segments + 1]: norms[s] = f32(grad_scale * sqrt(sum of x^2 over segment s)),
 *                norms[segments] = the same over all segments, the global norm.
 *   clip_factor  fp32 [1]: max_norm / global (ONE IEEE fp32 division of the two fp32 values) when
 *                max_norm > 0 and global > max_norm; 0.0f when the global norm as fp32 is NaN or
 *                +-inf (whatever max_norm is); exactly 1.0f otherwise.
 *   skip         optional: the words of ctcasr_step_guard.  skip[0] = 1 when the global norm as
 *                fp32 is not finite; otherwise left as it is (never cleared).  skip[1] untouched.
 *   workspace    ctcasr_grad_norm_workspace_bytes(n, segments) bytes, 8-byte aligned (chunk sums;
 *                nothing is allocated behind the caller).
 * Arithmetic (pinned, like the tie rules of the decoders): every square is formed and added in
 * fp64 - (double)x * (double)x is exact.  The order is fixed by the layout alone: each segment is
 * cut, FROM ITS OWN START, into chunks of CTCASR_GRAD_NORM_CHUNK floats.  In a chunk, with
 * q = index of a group of four floats, lane t = q % 256 adds the squares of its groups in
 * ascending q, x y z w inside a group, starting from +0 (elements past the end of a short chunk
 * count as +0); lanes 64w .. 64w + 63 are added by butterfly (v += v[lane ^ 32], ^ 16, ... ^ 1),
 * the four w as ((w0 + w1) + w2) + w3.  A segment's chunk sums: lane l = chunk % 64 adds its
 * chunks in ascending order, the 64 lanes by the same butterfly.  The global sum adds the segment
 * sums in index order starting from +0.  Each norm: sqrt in fp64, times (double)grad_scale, ONE
 * rounding to fp32.  No float atomics.  Hence: results are bit-reproducible, independent of the
 * grid size, and norms[s] depends on the values and the length of segment s only - not on where
 * the segment sits in grad, on `segments`, or on its neighbours.
 * Errors: null grad (n > 0) / seg_offsets / norms / clip_factor, n < 0, segments < 1, grad not
 * 16-byte aligned: CTCASR_ERR_BAD_ARGUMENT; segments > CTCASR_GRAD_NORM_MAX_SEGMENTS:
 * CTCASR_ERR_UNSUPPORTED; workspace null, short or misaligned: CTCASR_ERR_WORKSPACE.
 * ctcasr_set_option("grad_norm_blocks", k), 0 <= k <= 65536, sets the workgroup count of the
 * reading launch (0: the default) - a tuning knob that changes no result. */
#define CTCASR_GRAD_NORM_CHUNK 8192
#define CTCASR_GRAD_NORM_MAX_SEGMENTS 64
size_t ctcasr_grad_norm_workspace_bytes(int64_t n, int segments);
int ctcasr_grad_norm(const float *grad, int64_t n, const int64_t *seg_offsets, int segments,
                     float grad_scale, float max_norm, float *norms, float *clip_factor,
                     int32_t *skip, void *workspace, size_t workspace_bytes,
                     ctcasr_stream_t stream);
/* byte offset inside the recurrence workspace of the sticky time-out word of row block `block`
 * (0 .. (B - 1) / 32), or (size_t)-1 when (cell, T, B, H) runs the streaming kernels / there is
 * no such block */
size_t ctcasr_rnn_timeout_word_offset(int cell, int T, int B, int H, int block);
/* DIAGNOSTIC (ABI v5): `workgroups` (1..256) workgroups of 256 threads that hold their CUs for
 * `busy_us` (<= 100 ms) and touch no memory - the CU footprint of a collective's ring kernels, for
 * measuring on ONE GPU what such kernels cost beside the persistent recurrences (NCCL / RCCL
 * refuse two ranks on one device).  Not used by the training path. */
int ctcasr_occupy_cus(int workgroups, int busy_us, ctcasr_stream_t stream);
/* DIAGNOSTIC (ABI v6): the same footprint WITH a ring all-reduce's memory traffic - the workgroups
 * stream 2 x payload_bytes of a[i] += b[i] (16-byte elements, read twice and written once: 6 x
 * payload_bytes over L2 / fabric / HBM) through the scratch pair a, b (scratch_floats each, 16-byte
 * aligned), paced over busy_us: what a reduce-scatter + all-gather of the payload does to the
 * memory system beside the persistent recurrences and the library GEMMs.  Not used by training. */
int ctcasr_collective_traffic(int workgroups, int busy_us, float *a, const float *b,
                              int64_t scratch_floats, int64_t payload_bytes,
                              ctcasr_stream_t stream);
/* max_bits[0] = max(max_bits[0], bit pattern of max |x[i]|) (atomicMax; the caller zeroes it):
 * range guard of operands that go to the fp16 matrix pipe under a FIXED scale (the input
 * projections' weights, split_gemm.py) */
int ctcasr_absmax(const float *x, int64_t n, uint32_t *max_bits, ctcasr_stream_t stream);

/* ---- K1: feature extraction ----------------------------------------------------------------
 * Replaces python_speech_features.logfbank / mfcc / delta + the post-processing of load_sample
 * (asr/input_functions.py:156-335) for a batch of utterances.
 *   pcm            int16 [B, max_samples] raw PCM (NOT rescaled), rows zero padded
 *   num_samples    int32 [B] valid samples per row.  The reference refuses fewer than 401; the
 *                  kernels serve 1..max_samples (n <= 400 is psf's one zero-padded frame).  A row
 *                  outside [1, max_samples] reads none of its PCM and gets out_len 0 and all-zero
 *                  output rows, like ctcasr_features_num_frames(n < 1) = 0.
 *   feature_type   0 = 'mel' (80 log-mel), 1 = 'mfcc' (40 cepstra + 40 deltas)
 *   normalization  0 = 'none', 1 = 'local', 2 = 'local_scalar'
 *   tables         device block of ctcasr_features_tables_bytes(), filled once by
 *                  ctcasr_features_init_tables(tables, sampling_rate, stream) (synchronous).
 *                  The frame length 400 and step 160 are 25 ms / 10 ms at 16 kHz only, so any
 *                  sampling_rate other than 16000 is CTCASR_ERR_BAD_ARGUMENT.
 *   out            float32 [B, out_frames, 80], rows beyond an utterance's length are 0
 *   out_len        int32 [B] frames per utterance (after the optional every-2nd-frame drop)
 * 'local' / 'local_scalar' divide by the population std with no epsilon, like the reference: a
 * column (matrix) that is constant over the kept frames comes out all NaN.
 * ctcasr_features_num_frames(n) = 1 + ceil((n - 400) / 160) is the frame count of n samples. */
int ctcasr_features_num_frames(int num_samples);
size_t ctcasr_features_tables_bytes(void);
int ctcasr_features_init_tables(void *tables, int sampling_rate, ctcasr_stream_t stream);
size_t ctcasr_features_workspace_bytes(int B, int max_samples);
int ctcasr_features(const int16_t *pcm, const int32_t *num_samples, int B, int max_samples,
                    int feature_type, int normalization, int drop_every_second_frame,
                    const void *tables, float *out, int out_frames, int32_t *out_len,
                    void *workspace, size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K15: augmentation of training batches ----------------------------------------------------
 * No counterpart in the reference (it does not augment).  Two kernels around ctcasr_features:
 * speed perturbation of the PCM before it, SpecAugment masks on the features after it.  Left out
 * on purpose: time warping and any mask fill other than zero.  (Additive noise: K16.)
 *
 * Counter generator (integers only, so that a host reference reproduces every draw):
 *   r24(seed, idx)      = the top 24 bits (z >> 40) of the splitmix64 finaliser over
 *                         z = seed + 0x9E3779B97F4A7C15 * (idx + 1), the generator of the dropout
 *                         masks (bias_act_fwd / dropout)
 *   below(seed, idx, n) = (r24(seed, idx) * n) >> 24 in 64 bits, 1 <= n <= 2^24: uniform over
 *                         [0, n), never n.  (A larger n is still well defined; not every value
 *                         is reached.)
 *
 * ctcasr_spec_augment: in place on the output of ctcasr_features (after normalisation and the
 * frame drop).
 *   features   float32 [B, out_frames, 80]
 *   lengths    int32 [B] frames per row; L = lengths[b] clamped into [0, out_frames]
 *   Row b, frequency mask i < n_freq: w  = below(seed, 64 b + 2 i,     min(freq_width, 80) + 1),
 *                                     f0 = below(seed, 64 b + 2 i + 1, 80 - w + 1):
 *                                     columns [f0, f0 + w) of frames [0, L).
 *   Row b, time mask i < n_time:      cap = min(time_width, L * time_permille / 1000) (integer
 *                                     division),
 *                                     w  = below(seed, 64 b + 32 + 2 i,     cap + 1),
 *                                     t0 = below(seed, 64 b + 32 + 2 i + 1, L - w + 1):
 *                                     all 80 columns of frames [t0, t0 + w).
 *   A row with L == 0 gets no masks.  Masks may overlap.
 *   Every masked cell is STORED +0.0f whatever it held (a NaN included: a store, not a multiply);
 *   no other cell is stored to and no cell is read, so cells outside the masks and frames at or
 *   beyond L keep their bits, and the traffic is the masked area.  Zero is the per-column mean
 *   under 'local' normalisation; under 'none' and 'local_scalar' zero is written all the same.
 *   intervals  optional int32 [B, n_freq + n_time, 2]: (start, width) of every mask, the
 *              frequency masks first; all zero for a row with L == 0.  May be NULL.
 *   out_frames == 0 is served: every L is 0, nothing is stored to the features (which may then be
 *   NULL, as the address of an empty buffer is) and `intervals` is written all zero.
 * Errors (CTCASR_ERR_BAD_ARGUMENT, before any launch): null lengths, null features with
 * out_frames > 0, B < 1, out_frames < 0, n_freq or n_time outside
 * [0, CTCASR_SPEC_AUGMENT_MAX_MASKS], a negative width, time_permille outside [0, 1000];
 * out_frames >= 2^24: CTCASR_ERR_UNSUPPORTED.
 * n_freq == n_time == 0 launches nothing.
 *
 * ctcasr_speed_perturb: band-limited resampling of each row by its own factor; percent[b] = P
 * plays row b P / 100 times as fast (P in [50, 200]).
 *   pcm, num_samples   int16 [B, max_in], int32 [B]     percent   int32 [B]      (all device)
 *   out, out_samples   int16 [B, max_out], int32 [B]
 *   n_out = max(1, n * 100 / P) (integer division, 64-bit product, at most INT32_MAX) =
 *   ctcasr_resample_num_samples(n, P), pure host arithmetic, 0 for n < 1 or P outside [50, 200].
 *   Output sample j sits at input position t = j * P / 100: integer part t0 = (j * P) / 100 and
 *   phase p = (j * P) % 100 in 64-bit integers (no float position that drifts over a long row).
 *   y[j] = sum over input samples k in [0, n) of x[k] * h(t - k), x = 0 outside, with
 *     c = 95 / max(P, 100)                        (= 0.95 * min(1, 100 / P): the cut-off)
 *     h(d) = c * sinc(c d) * 0.5 * (1 + cos(pi c d / 12)) for |c d| < 12, else 0;
 *     sinc(u) = sin(pi u) / (pi u), sinc(0) = 1   (a Hann-windowed sinc of 12 zero crossings a side)
 *   Taps: k = t0 + m for m in [-R, R + 1], R = 12 * max(P, 100) / 95 (integer division): 26 taps up
 *   to P = 100, 52 at P = 200.  The weight of (p, m) is h(p / 100 - m) evaluated in fp64 and
 *   rounded once to fp32; a row has at most 100 distinct phases.  The sum is fp32, starting from
 *   +0, one fused multiply-add per tap in ascending k; the result is rounded to nearest even and
 *   saturated to [-32768, 32767].
 *   A row with P == 100 is a bit copy.  A row whose n is outside [1, max_in] or whose P is outside
 *   [50, 200] reads none of its PCM and gets count 0 and an all-zero row, as in ctcasr_features.
 *   Columns [n_out, max_out) are zero.  A row whose n_out exceeds max_out is cut to max_out and
 *   out_samples reports max_out (the host cannot check this without a synchronisation; size
 *   max_out with ctcasr_resample_num_samples).
 * Errors (CTCASR_ERR_BAD_ARGUMENT): a null pointer, B < 1, max_in < 1, max_out < 1; max_in or
 * max_out above 2^30: CTCASR_ERR_UNSUPPORTED. */
#define CTCASR_SPEC_AUGMENT_MAX_MASKS 16
int ctcasr_spec_augment(float *features, const int32_t *lengths, int B, int out_frames,
                        uint64_t seed, int n_freq, int freq_width, int n_time, int time_width,
                        int time_permille, int32_t *intervals, ctcasr_stream_t stream);
int ctcasr_resample_num_samples(int num_samples, int percent);
int ctcasr_speed_perturb(const int16_t *pcm, const int32_t *num_samples, const int32_t *percent,
                         int B, int max_in, int16_t *out, int max_out, int32_t *out_samples,
                         ctcasr_stream_t stream);

/* ---- K16: additive noise at a drawn SNR -----------------------------------------------------
 * No counterpart in the reference.  Mixes a run of a noise clip into every drawn row of a batch
 * of PCM, before ctcasr_features (and after ctcasr_speed_perturb where that is on), scaled so
 * that the row's speech-to-noise power ratio is the drawn number of dB.
 *   pcm, out      int16 [B, max_samples]; out == pcm (in place) is allowed, any other overlap is not
 *   num_samples   int32 [B]; n = num_samples[b]
 *   bank          int16: all noise clips back to back
 *   clip_offsets  DEVICE int64 [num_clips + 1], clip k = bank[clip_offsets[k] : clip_offsets[k + 1]]
 *                 of length len_k.  Only 1 <= len_k <= 2^24 is served (below() then reaches every
 *                 offset); a row that draws any other clip is copied.  The table is trusted to
 *                 stay inside the bank.
 * Draws of row b, all from the generator of K15:
 *   hit = below(seed, 8 b, 1000) < prob_permille        k   = below(seed, 8 b + 1, num_clips)
 *   o   = below(seed, 8 b + 2, len_k)                   snr = snr_lo_db + below(seed, 8 b + 3,
 *                                                                   snr_hi_db - snr_lo_db + 1)
 * Noise under sample i < n: v[i] = clip_k[(o + i) mod len_k] - a clip shorter than the row wraps
 * as often as needed.
 * Powers: Ps = sum of x[i]^2, Pn = sum of v[i]^2 over i < n, in 64-bit integers: exact (n <= 2^30,
 * a square <= 2^30), so independent of grid shape and arrival order (integer atomics, one per
 * workgroup and sum; no float atomics).
 * Gain: g = f32(sqrt(Ps / Pn) * 10^(-snr / 20)) evaluated in fp64; pinned to within one fp32 ulp
 * (relative 2^-23) of that value, NOT to a particular rounding of the device's fp64 sqrt / pow.
 * Every workgroup of a row computes it from the same two sums, so it is one value per row.
 * Mix: y[i] = clamp(rint(x[i] + g * v[i]), -32768, 32767) in fp32 by one fused multiply-add,
 * rounded to nearest even.
 * Everything that is not mixed is a bit copy (and is not stored at all when out == pcm): rows
 * with hit false; rows whose n is outside [1, max_samples] (all max_samples columns);  rows with
 * Ps == 0 or Pn == 0; rows whose clip has a length outside [1, 2^24]; in every row the columns at
 * or beyond n.
 * Optional outputs (each may be NULL):
 *   draws   int32 [B, 4] = (status, k, o, snr).  status 1 = mixed; 0 = not drawn or a bad row, the
 *           other three are then 0; 2 = drawn, but speech or noise is silent or the clip's length
 *           is not served (o = 0 then): copied.
 *   powers  int64 [B, 2] = (Ps, Pn); both 0 where status is 0 and where the clip is not served.
 *   gain    fp32 [B]; 0 where the row is not mixed.
 *   workspace  ctcasr_noise_mix_workspace_bytes(B) bytes, 8-byte aligned (the two sums per row).
 * Two launches behind a memset of the workspace: the sums, then the mix.  A workgroup serves
 * CTCASR_NOISE_MIX_CHUNK samples of one row, cut into groups of 8 by the address of the stored
 * stream: whole groups below n whose noise does not cross the clip's end move as 16-byte
 * accesses, all others sample by sample.
 * Errors, before any launch: null pcm / num_samples / bank / clip_offsets / out, B < 1,
 * max_samples < 1, num_clips < 1, snr_lo_db > snr_hi_db, either outside
 * [CTCASR_NOISE_MIX_MIN_SNR_DB, CTCASR_NOISE_MIX_MAX_SNR_DB], prob_permille outside [0, 1000]:
 * CTCASR_ERR_BAD_ARGUMENT; max_samples > 2^30 or num_clips > 2^24: CTCASR_ERR_UNSUPPORTED;
 * workspace null, short or misaligned: CTCASR_ERR_WORKSPACE.
 * prob_permille == 0 launches no kernel: a device-to-device copy when out != pcm, and the optional
 * outputs are zeroed by memsets. */
#define CTCASR_NOISE_MIX_CHUNK 8192
#define CTCASR_NOISE_MIX_MIN_SNR_DB (-20)
#define CTCASR_NOISE_MIX_MAX_SNR_DB 60
size_t ctcasr_noise_mix_workspace_bytes(int B);
int ctcasr_noise_mix(const int16_t *pcm, const int32_t *num_samples, int B, int max_samples,
                     const int16_t *bank, const int64_t *clip_offsets, int num_clips,
                     uint64_t seed, int snr_lo_db, int snr_hi_db, int prob_permille,
                     int16_t *out, int32_t *draws, int64_t *powers, float *gain,
                     void *workspace, size_t workspace_bytes, ctcasr_stream_t stream);

/* ---- K17: reverberation with a drawn room impulse response ----------------------------------
 * No counterpart in the reference.  Convolves every drawn row of a batch of PCM with one response
 * of a bank, after ctcasr_speed_perturb and before ctcasr_noise_mix.  The output has the input's
 * length: rir_delay puts the direct path of the room on the sample it came from, and the tail
 * beyond n is cut, so num_samples, labels and timestamps do not move.
 *   pcm, out      int16 [B, max_samples]; out must NOT be pcm (a sample is read by its neighbours)
 *   num_samples   int32 [B]; n = num_samples[b]
 *   taps          int16: all responses back to back, 16-byte aligned
 *   rir_offsets   DEVICE int64 [num_rirs + 1]; response r = taps[rir_offsets[r] : rir_offsets[r + 1]],
 *                 K_r taps.  Trusted to stay inside `taps`.
 *   rir_delay     DEVICE int32 [num_rirs]: the tap that holds the direct path
 *   rir_scale     DEVICE fp32 [num_rirs]
 * Draws of row b, from the generator of K15:
 *   hit = below(seed, 8 b, 1000) < prob_permille        r = below(seed, 8 b + 1, num_rirs)
 * Status of row b:
 *   0  hit false, or n outside [1, max_samples]                                   (r reported 0)
 *   2  drew a response that is not served: K_r outside [CTCASR_REVERB_TAP_ALIGN,
 *      CTCASR_REVERB_MAX_TAPS], K_r or rir_offsets[r] not a multiple of CTCASR_REVERB_TAP_ALIGN
 *      (or a negative offset), rir_delay[r] outside [0, K_r)
 *   1  reverberated: for i < n, with h = taps + rir_offsets[r], K = K_r, d = rir_delay[r],
 *        acc    = sum over k < K of h[k] * x[i + d - k],  x = 0 outside [0, n),
 *                 as a 32-bit two's-complement integer (the sum mod 2^32: exact, so it depends on
 *                 no grid, tile or order of summation; a bank with sum |h[k]| <= 65535 per
 *                 response - ctc_asr_amd/reverb.py makes one - never wraps: |acc| <= 32768 * 65535)
 *        out[i] = clamp(rintf((float)acc * rir_scale[r]), -32768, 32767)
 *                 one int-to-fp32 conversion (round to nearest even), one fp32 multiply, rintf.
 * Everything else is a bit copy of pcm: rows of status 0 and 2 (all max_samples columns), and in
 * every row the columns at or beyond n.
 *   draws   optional int32 [B, 2] = (status, r); may be NULL.
 * One launch; a workgroup serves CTCASR_REVERB_CHUNK output samples of one row and walks the taps
 * CTCASR_REVERB_TAP_BLOCK at a time (a remainder 8 at a time).
 * Errors, before any launch: a null pcm / num_samples / taps / rir_offsets / rir_delay / rir_scale
 * / out, out == pcm, B < 1, max_samples < 1, num_rirs < 1, prob_permille outside [0, 1000]:
 * CTCASR_ERR_BAD_ARGUMENT; max_samples > 2^30, num_rirs > 2^24 or more than INT_MAX workgroups:
 * CTCASR_ERR_UNSUPPORTED.
 * prob_permille == 0 launches no kernel: a device-to-device copy, and draws zeroed by a memset. */
#define CTCASR_REVERB_CHUNK 2048
#define CTCASR_REVERB_TAP_BLOCK 32
#define CTCASR_REVERB_TAP_ALIGN 8
#define CTCASR_REVERB_MAX_TAPS 8192
int ctcasr_reverb(const int16_t *pcm, const int32_t *num_samples, int B, int max_samples,
                  const int16_t *taps, const int64_t *rir_offsets, const int32_t *rir_delay,
                  const float *rir_scale, int num_rirs, uint64_t seed, int prob_permille,
                  int16_t *out, int32_t *draws, ctcasr_stream_t stream);

/* ---- K18: speech segmentation of a long recording --------------------------------------------
 * No counterpart in the reference (it transcribes one utterance).  The device side of
 * ctc_asr_amd/vad.py and ctc_asr_amd/transcribe.py: one pass over the PCM of a whole recording,
 * and the gather that turns the pieces the host chose into a batch for ctcasr_features.
 *
 * ctcasr_vad_energy: energy and level histogram per hop of CTCASR_VAD_HOP = 160 samples (the
 * feature step).  F = ceil(n / 160) hops.
 *   pcm      int16 [n], any 2-byte aligned address (a slice of a tensor).  A 16-byte aligned base
 *            is read 16 bytes per lane; any other base through aligned loads and shifts, with
 *            the same results.  Only read.
 *   energy   int64 [F]: energy[f] = sum of x * x over samples [160 f, min(160 f + 160, n)), exact;
 *            at most 160 * 2^30.  The last hop may be partial.
 *   hist     uint32 [CTCASR_VAD_LEVELS]: zeroed by the call on the stream, then hist[level(e)]
 *            counts the hops of energy e.  Integer atomics: no grid, order or run changes it.
 * level(e), a quarter-octave scale in integers: with b the bit length of e (0 for e = 0),
 *   level(e) = e                                   for b <= 2
 *            = 4 (b - 2) + ((e >> (b - 3)) & 3)    otherwise;
 * monotone, 145 at the largest energy, one level at most a factor 1.25 in energy.  Its lower edge:
 *   level_floor(L) = L                                   for L < 4
 *                  = (4 + (L & 3)) << ((L >> 2) - 1)     otherwise.
 * A workgroup serves CTCASR_VAD_CHUNK samples (256 hops).
 * Errors, before any launch: a null pointer or n < 1: CTCASR_ERR_BAD_ARGUMENT; n > 2^31 - 1:
 * CTCASR_ERR_UNSUPPORTED.
 *
 * ctcasr_gather_segments: row b of out = pcm[seg_start[b] : seg_start[b] + len), zeros behind it.
 *   pcm          int16 [n], any 2-byte aligned address.  Only read.
 *   seg_start    DEVICE int64 [B], in samples; any value (multiples of 8 from an aligned base keep
 *                the reads at one 16-byte load per lane)
 *   seg_len      DEVICE int32 [B]
 *   out          int16 [B, max_samples], the input layout of ctcasr_features; every column written
 *   num_samples  int32 [B]: len, that is seg_len[b] clipped so that the range stays inside [0, n)
 *                and len <= max_samples.  A row with seg_start[b] < 0, seg_start[b] >= n or
 *                seg_len[b] < 1 is all zero with count 0.
 * Rows may repeat and come in any order.  One launch.
 * Errors, before any launch: a null pointer, B < 1 or max_samples < 1: CTCASR_ERR_BAD_ARGUMENT;
 * max_samples > 2^30 or more than INT_MAX workgroups: CTCASR_ERR_UNSUPPORTED. */
#define CTCASR_VAD_HOP 160
#define CTCASR_VAD_LEVELS 160
#define CTCASR_VAD_CHUNK 40960
int ctcasr_vad_energy(const int16_t *pcm, int64_t n, int64_t *energy, uint32_t *hist,
                      ctcasr_stream_t stream);
int ctcasr_gather_segments(const int16_t *pcm, int64_t n, const int64_t *seg_start,
                           const int32_t *seg_len, int B, int max_samples, int16_t *out,
                           int32_t *num_samples, ctcasr_stream_t stream);

/* ---- K19: sampling-rate conversion and channel downmix ---------------------------------------
 * No counterpart in the reference (its corpus is 16 kHz mono int16).  One recording of interleaved
 * PCM in the layout of its file - any of four sample formats, 1..8 channels, rate_in - becomes
 * int16 mono at rate_out.  The filter is that of ctcasr_speed_perturb at the ratio of the two
 * rates; that kernel's rule is the special case L = 100, M = P.  (These entry points were added
 * without a change of CTCASR_ABI_VERSION: they break no caller.)
 *
 * Plan (ctcasr_resample_plan, pure host arithmetic):
 *   g = gcd(rate_in, rate_out), M = rate_in / g, L = rate_out / g, S = max(M, L)
 *   c = 95 L / (100 S) in fp64                    (0.95 * min(1, L / M): the cut-off)
 *   R = (1200 S) / (95 L) (integer division), taps = 2 R + 2
 *   Rates within [4000, 192000] are served (else CTCASR_ERR_BAD_ARGUMENT), and of those the pairs
 *   with L * taps <= CTCASR_RESAMPLE_MAX_TABLE (else CTCASR_ERR_UNSUPPORTED): to 16 000 Hz,
 *     rate_in   8000  11025  12000  22050  24000  32000  44100  48000  88200  96000  192000
 *     M            1    441      3    441      3      2    441      3    441      6      12
 *     L            2    640      4    320      2      1    160      1     80      1       1
 *     R           12     12     12     17     18     25     34     37     69     75     151
 *     taps        26     26     26     36     38     52     70     76    140    152     304
 *   16 001 -> 16 000 would need 416 000 weights and is not served.  A pair whose table and the
 *   input span of 256 outputs do not fit a workgroup's LDS together is not served either (none of
 *   the rates above; 192 000 -> 4000 still is).
 * Count (ctcasr_resample_out_samples, pure host arithmetic):
 *   n_out = max(1, n * L / M) (integer division in 64 bits); 0 for n < 1, n > 2^31 - 1 or a pair
 *   that is not served.
 * Weights (ctcasr_resample_table): table float [L][taps] in DEVICE memory, 16-byte aligned,
 *   ctcasr_resample_table_bytes(rate_in, rate_out) bytes (L * taps floats rounded up to 16 bytes,
 *   the pad zero; 0 for a pair that is not served).  Entry (p, i) = h(p / L - (i - R)) with h and
 *   sinc exactly as in the ctcasr_speed_perturb block above (K15) and the c of the plan, evaluated
 *   in fp64 and rounded once to fp32, in a launch of its own: once per pair of rates.  The
 *   resampling kernel never evaluates a sine.
 * Frame value s[k], k in [0, n): the fp32 sum over the frame's channels, in ascending channel
 *   order (the first channel's value, then one fp32 addition per further channel), of
 *     CTCASR_PCM_S16  int16                (float)x
 *     CTCASR_PCM_U8   uint8                (float)((x - 128) * 256)
 *     CTCASR_PCM_S32  int32                (float)x * 0x1p-16f    (24-bit files, left-justified
 *                                                                   in 32 bits, are this format)
 *     CTCASR_PCM_F32  float32              x * 32768.0f
 *   and s[k] = 0 outside [0, n).  `in` holds n frames of `channels` samples, interleaved, at any
 *   address aligned to one sample (a slice of a tensor); it is read through aligned 16-byte loads
 *   whatever its alignment and frame size (6 bytes for three int16 channels), with the same
 *   results.  Only read.
 * Output j in [0, n_out): pos = j * M in 64 bits, t0 = pos / L, p = pos % L;
 *   acc = +0.0f; for i = 0 .. taps - 1: acc = fmaf(s[t0 - R + i], table[p][i], acc);
 *   out[j] = sat16(rintf(acc * gain)), gain = (float)(1.0 / channels), sat16 the clamp to
 *   [-32768, 32767], rintf to nearest even.
 *   M == L (rate_in == rate_out): no filter, out[j] = sat16(rintf(s[j] * gain)); mono int16 input
 *   comes back bit for bit.  (`table` is not read then, but may not be NULL.)
 *   Only out[0 .. n_out) is written.  n_out must be ctcasr_resample_out_samples(n, rate_in,
 *   rate_out), else CTCASR_ERR_BAD_ARGUMENT.
 * status int32 [1], device: cleared by a memset on the stream, then bit 0 is raised (an integer
 *   atomic OR) when a CTCASR_PCM_F32 sample of a frame in [0, n) is not finite.  Outputs whose
 *   taps touch such a frame are unspecified; all others are what they would be without it.
 * One launch behind the memset.  A workgroup owns ctcasr_resample_chunk(rate_in, rate_out)
 * consecutive outputs (2048, 1024, 512 or 256, the most that fit LDS with the table; 0 for a pair
 * that is not served): it copies the table into LDS, downmixes its span of input once into an
 * fp32 tile in LDS and runs the taps from there.  Every output is computed by the same operations
 * in the same order wherever it falls: the result does not depend on the grid.  No float atomics.
 * ctcasr_resample_chunk is INFORMATIVE, not a contract: the run per workgroup is a tuning detail
 * that may change with the kernel, no caller needs it to size anything, and no result depends on
 * it.  It is exported so that tests can put recordings across the seams of the kernel as built.
 * Errors, before any launch: a null pointer, a format outside 0..3, channels outside 1..8, n < 1,
 * a rate outside [4000, 192000], `in` / `table` / `out` / `status` not aligned to 1 sample / 16 /
 * 2 / 4 bytes, a wrong n_out: CTCASR_ERR_BAD_ARGUMENT; a pair that is not served or n > 2^31 - 1:
 * CTCASR_ERR_UNSUPPORTED. */
#define CTCASR_RESAMPLE_MAX_TABLE 16640      /* 640 x 26: the table of 11 025 -> 16 000 */
#define CTCASR_PCM_S16 0
#define CTCASR_PCM_U8 1
#define CTCASR_PCM_S32 2
#define CTCASR_PCM_F32 3
int ctcasr_resample_plan(int rate_in, int rate_out, int *M, int *L, int *radius, int *taps);
int ctcasr_resample_chunk(int rate_in, int rate_out);
int64_t ctcasr_resample_out_samples(int64_t n, int rate_in, int rate_out);
size_t ctcasr_resample_table_bytes(int rate_in, int rate_out);
int ctcasr_resample_table(int rate_in, int rate_out, float *table, ctcasr_stream_t stream);
int ctcasr_resample(const void *in, int format, int channels, int64_t n, int rate_in, int rate_out,
                    const float *table, int16_t *out, int64_t n_out, int32_t *status,
                    ctcasr_stream_t stream);

/* ---- K20: sequence-wise batch normalisation between the recurrent layers ----------------------
 * No counterpart in the reference (its stack has no normalisation).  The input of a recurrent
 * layer is normalised per channel over every counted frame of the batch.  (Additions only, as for
 * K19: CTCASR_ABI_VERSION stays.)
 *   x        fp32 [T, B, C], time-major, contiguous, 16-byte aligned, C % 4 == 0.  Only read.
 *   lengths  int32 [B] or NULL.  Row r = t * B + b is COUNTED when lengths is NULL or
 *            t < clamp(lengths[b], 0, T); N = the number of counted rows.
 *   gamma, beta, mean, rstd, running_mean, running_var, dgamma, dbeta: fp32 [C], 4-byte aligned.
 *   y, dx    fp32 [T, B, C], 16-byte aligned, tensors of their own (x is the previous layer's
 *            output, whose backward pass still reads it).
 *   workspace  ctcasr_seq_bn_workspace_bytes(T * B, C) bytes, 8-byte aligned: the chunk sums and
 *            two floats per channel.  Nothing is allocated behind the caller.
 * ctcasr_seq_bn_fwd (training), three launches:
 *   S1 = sum of x, S2 = sum of x^2 per channel over the counted rows, in fp64 ((double)x * (double)x
 *   is exact).  Order (pinned): the rows are cut BY ROW NUMBER into chunks of CTCASR_SEQ_BN_ROWS
 *   consecutive rows - the cut does not move with lengths; inside a chunk a channel's values are
 *   added in ascending row order starting from +0 (S2 by one fp64 fma per value), uncounted rows
 *   are left out; the chunk sums are added in ascending chunk order starting from +0.  No float
 *   atomics, no cross-lane step: results are bit-reproducible and do not depend on the grid
 *   (ctcasr_set_option("seq_bn_blocks", k), 0 <= k <= 65536, sets the workgroup count of the
 *   streaming launches of all three entry points; 0: the default).
 *   mean64 = S1 / N, var64 = S2 / N - mean64 * mean64 (two roundings: product, difference), a
 *   negative var64 is 0 (a NaN stays), rstd64 = 1 / sqrt(var64 + eps).
 *   mean = (float)mean64, rstd = (float)rstd64 are written for the backward pass.
 *   Counted rows: y = fmaf(x - mean, a, beta), a = gamma * rstd (one fp32 product).  Uncounted
 *   rows: y = +0.0 whatever x holds there (x is not read).
 *   Running statistics: running = (float)(decay * (double)running + (1 - decay) * batch64) with
 *   batch64 = mean64 / var64 (the population variance), written by the launch that finishes the
 *   sums.  A channel whose mean64 or var64 is not finite leaves both of its running values alone.
 *   N == 0: y is all zeros, mean = rstd = 0, the running values are untouched.
 * ctcasr_seq_bn_infer, one launch: the same y with mean = running_mean and
 *   rstd = (float)(1 / sqrt((double)running_var + eps)).  Writes no statistics, takes no workspace.
 * ctcasr_seq_bn_bwd, three launches: xhat = (x - mean) * rstd in fp32 (two roundings);
 *   s1 = sum of dy, s2 = sum of dy * xhat over the counted rows in fp64 in the order above (the
 *   product of two fp32 values is exact in fp64; one fma per value).  dbeta[c] += (float)s1,
 *   dgamma[c] += (float)s2: ADDED to what is there, one writer per channel.
 *   m1 = (float)(s1 / N), m2 = (float)(s2 / N) (both 0 for N == 0).  Counted rows:
 *   dx = a * ((dy - m1) - xhat * m2), every operation rounded on its own; uncounted rows: +0.0.
 * Errors, before any launch: a null pointer (lengths excepted), T or B < 1, T * B > 2^31 - 1,
 * C < 4 or C % 4 != 0, x / y / dy / dx not 16-byte aligned, decay outside [0, 1] or eps not a
 * positive finite number: CTCASR_ERR_BAD_ARGUMENT; workspace null, short or not 8-byte aligned:
 * CTCASR_ERR_WORKSPACE. */
#define CTCASR_SEQ_BN_ROWS 64
size_t ctcasr_seq_bn_workspace_bytes(int64_t rows, int C);
int ctcasr_seq_bn_fwd(const float *x, const int32_t *lengths, int T, int B, int C,
                      const float *gamma, const float *beta, float *running_mean,
                      float *running_var, double decay, double eps, float *y, float *mean,
                      float *rstd, void *workspace, size_t workspace_bytes,
                      ctcasr_stream_t stream);
int ctcasr_seq_bn_infer(const float *x, const int32_t *lengths, int T, int B, int C,
                        const float *gamma, const float *beta, const float *running_mean,
                        const float *running_var, double eps, float *y, ctcasr_stream_t stream);
int ctcasr_seq_bn_bwd(const float *dy, const float *x, const int32_t *lengths, int T, int B, int C,
                      const float *mean, const float *rstd, const float *gamma, float *dgamma,
                      float *dbeta, float *dx, void *workspace, size_t workspace_bytes,
                      ctcasr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CTCASR_H_ */
