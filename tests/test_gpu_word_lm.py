"""The word n-gram fused into the CTC beam search (csrc/beam.hip `LM == 2`,
`hip.ctc_beam_decode_wordlm`, `hip.wordlm_lookup`, the `--lm_path` drivers with a word model).

The oracle is tests/word_lm_reference.py: n-grams in dicts and, for a small model, the dense
automaton over its reachable (trie node, context) pairs.  The *existing* GPU kernels decode that
automaton, and the new one must return their bits: the search executes the same float32
operations on the same float32 scores.  tests/lm_beam_reference.py decodes it on the CPU at the
bars of test_gpu_beam_lm.py (path and length equal, logp rtol 1e-5 / atol 1e-3; exact ties in a
total are not a parity case: the inputs are continuous random logits).  The lookup is tested at
its seams through `hip.wordlm_lookup`, exactly."""

import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from ctc_asr_amd import lm
from ctc_asr_amd.params import FLAGS
from tests import lm_beam_reference as lref
from tests import word_lm_reference as ref
from tests.beam_helpers import _t, raw_beam

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORMS = ['max', 'log_softmax']
# (classes, blank) -> the space and the letters a, b, c, d, e of the little language
ALPHABETS = {(29, 28): (1, [2, 3, 4, 5, 6]), (6, 5): (4, [0, 1, 2, 3, 3])}
# a one-letter word, words that are prefixes of others ('a' < 'ab' < 'abc')
LEXICON = ['a', 'ab', 'abc', 'ba', 'cab', 'd', 'bad', 'ca', 'dd', 'acbd', 'bb', 'c']


def _spell(text, classes, blank):
    space, letters = ALPHABETS[(classes, blank)]
    return [space if ch == ' ' else letters['abcde'.index(ch)] for ch in text]


@functools.lru_cache(maxsize=None)
def _corpus(classes, blank):
    """40 sentences of 1..5 lexicon words, a Zipf draw; the same text for every order."""
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(40):
        words = [LEXICON[min(int(rng.zipf(1.4)) - 1, len(LEXICON) - 1)]
                 for _ in range(int(rng.integers(1, 6)))]
        rows.append(tuple(_spell(' '.join(words), classes, blank)))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _models(classes, blank, order):
    space = ALPHABETS[(classes, blank)][0]
    rows = _corpus(classes, blank)
    return (lm.build_word_ngram(rows, order, classes, space, blank=blank),
            ref.WordNgram(rows, order, space))


@functools.lru_cache(maxsize=None)
def _dense(classes, blank, order, weight, bonus, oov):
    """(scaled WordLmScorer, dense LmScorer of the reference, backoffs per dense state)."""
    model, restated = _models(classes, blank, order)
    nxt, score, final, _, backoffs = ref.dense_automaton(
        ref.Scorer(restated, weight, bonus, oov), classes, blank)
    return model.scaled(weight, bonus, oov), lm.LmScorer(nxt, score, final), backoffs


def _logits(rng, num_steps, classes, blank, texts, noise=1.0, peak=3.0, blank_bias=2.5):
    """Noise everywhere, and row b leans towards a spelling of ``texts[b]`` (one frame per label,
    blanks between): hypotheses of several words survive, with close competitors."""
    logits = rng.normal(size=(num_steps, len(texts), classes)) * noise
    logits[:, :, blank] += blank_bias
    for b, text in enumerate(texts):
        labels = _spell(text, classes, blank)
        stride = max(num_steps // (len(labels) + 1), 1)
        for i, c in enumerate(labels):
            if i * stride + 1 < num_steps:
                logits[i * stride + 1, b, c] += peak
                logits[i * stride + 1, b, blank] -= blank_bias
    return logits.astype(np.float32)


def _word(hip, logits, seq_len, width, scorer, top_paths=1, blank=None, norm='max', **kwargs):
    got = hip.ctc_beam_decode_wordlm(_t(logits), _t(np.asarray(seq_len), torch.int32), width,
                                     scorer, top_paths, blank=blank, normalization=norm, **kwargs)
    return tuple(t.cpu().numpy() for t in got)


def _dense_nbest(hip, logits, seq_len, width, scorer, top_paths, blank, norm):
    got = hip.ctc_beam_decode_nbest(_t(logits), _t(np.asarray(seq_len), torch.int32), width,
                                    top_paths, scorer=scorer, blank=blank, normalization=norm)
    return tuple(t.cpu().numpy() for t in got)


def _same_bits(a, b):
    return all(x.shape == y.shape and
               np.array_equal(np.ascontiguousarray(x).view(np.int32),
                              np.ascontiguousarray(y).view(np.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------
# 1. The lookup at its seams
# ------------------------------------------------------------------------------------------------
def _lookup(hip, scorer, pairs):
    ctx = _t(np.array([p[0] for p in pairs]), torch.int32)
    word = _t(np.array([p[1] for p in pairs]), torch.int32)
    score, after = hip.wordlm_lookup(scorer, ctx, word)
    return score.cpu().numpy(), after.cpu().numpy()


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_lookup_equals_the_reference_for_every_pair_of_a_small_model(hip, order):
    """Every (context, word) of the model: found at the top order, after 1 .. order - 1
    back-offs, only at context 0; first and last successors; word ids 0 and 1; the lowest and the
    highest context id.  Scaled by a weight, so that the scaled arrays are what is added."""
    model, restated = _models(29, 28, order)
    scaled = model.scaled(0.7, 0.0)
    pairs, want, steps = [], [], set()
    for h in restated.contexts:
        for w in range(restated.events):
            score, after, took = restated.wd(h, w, 0.7)
            pairs.append((restated.context_id[h], w))
            want.append((np.float32(score), restated.context_id[after]))
            steps.add((len(h), took))
    # the cases the seams need are there, by the reference's own count
    assert {took for _, took in steps} == set(range(order))
    assert all((order - 1, took) in steps for took in range(order))
    assert pairs[0][0] == 0 and pairs[-1][0] == model.num_contexts - 1
    score, after = _lookup(hip, scaled, pairs)
    assert np.array_equal(score.view(np.int32),
                          np.array([w[0] for w in want], dtype=np.float32).view(np.int32))
    assert after.tolist() == [w[1] for w in want]
    assert hip.wordlm_lookup(scaled, _t([], torch.int32), _t([], torch.int32))[0].numel() == 0


def _range_tables(rng):
    """Hand-built valid tables: context 0 lists 6000 words; contexts 1 .. 6 hold ranges of 1, 63,
    64, 65, 4097 and 2 successors, parents 0 - every probe count of the 64-way search."""
    words, lengths = 6000, [1, 63, 64, 65, 4097, 2]
    begin, succ_word, succ_ctx = [0, words], [np.arange(words)], [rng.integers(0, 7, size=words)]
    for n in lengths:
        succ_word.append(np.sort(rng.choice(words, size=n, replace=False)))
        succ_ctx.append(rng.integers(0, 7, size=n))
        begin.append(begin[-1] + n)
    succ_word, succ_ctx = np.concatenate(succ_word), np.concatenate(succ_ctx)
    succ_lp = -rng.random(size=len(succ_word)) * 9.0
    backoff = -rng.random(size=7)
    trie_next = np.full((2, 29), -1, dtype=np.int32)
    return lm.WordLmScorer(trie_next, [-1, -1], begin, succ_word, succ_lp, succ_ctx, backoff,
                           np.zeros(7, dtype=np.int32), 2, 1)


def test_lookup_ranges_of_1_63_64_65_and_4097(hip):
    rng = np.random.default_rng(11)
    scorer = _range_tables(rng)
    entries = {}
    for h in range(7):
        for at in range(scorer.ctx_begin[h], scorer.ctx_begin[h + 1]):
            entries[(h, int(scorer.succ_word[at]))] = (float(scorer.succ_lp[at]),
                                                       int(scorer.succ_ctx[at]))
    pairs = []
    for h in range(7):
        low, high = int(scorer.ctx_begin[h]), int(scorer.ctx_begin[h + 1])
        inside = scorer.succ_word[low:high]
        probe = {int(inside[0]), int(inside[-1]), int(inside[len(inside) // 2]), 0, 1, 5999,
                 max(int(inside[0]) - 1, 0), min(int(inside[-1]) + 1, 5999)}
        probe.update(int(w) for w in inside[::61])
        probe.update(int(w) for w in rng.integers(0, 6000, size=40))
        pairs += [(h, w) for w in sorted(probe)]
    want = [ref.wd_tables(entries, scorer.ctx_backoff, scorer.ctx_parent, 2, h, w)
            for h, w in pairs]
    assert any(h > 0 and (h, w) in entries for h, w in pairs)
    assert any(h > 0 and (h, w) not in entries for h, w in pairs)
    score, after = _lookup(hip, scorer, pairs)
    assert np.array_equal(score.view(np.int32),
                          np.array([w[0] for w in want], dtype=np.float32).view(np.int32))
    assert after.tolist() == [w[1] for w in want]


def test_a_parent_chain_longer_than_the_order_gives_minus_inf_and_returns(hip):
    """Tables that validation would refuse (context 0 lists nothing, every parent is the context
    itself), through the raw entry point: -inf after `order` searches, context 0."""
    contexts = 3
    tensors = [_t(np.array([0, 0, 1, 2]), torch.int64),                 # ctx_begin
               _t(np.array([5, 7]), torch.int32),                      # succ_word
               _t(np.array([-1.0, -2.0]), torch.float64),              # succ_lp
               _t(np.array([2, 1]), torch.int32),                      # succ_ctx
               _t(np.array([-0.5, -0.25, -0.125]), torch.float64),     # ctx_backoff
               _t(np.array([0, 1, 2]), torch.int32)]                   # ctx_parent: loops
    for order in (1, 5):
        tables = hip.WordLm(ctx_begin=tensors[0].data_ptr(), succ_word=tensors[1].data_ptr(),
                            succ_lp=tensors[2].data_ptr(), succ_ctx=tensors[3].data_ptr(),
                            ctx_backoff=tensors[4].data_ptr(), ctx_parent=tensors[5].data_ptr(),
                            num_succ=2, num_nodes=0, num_ctx=contexts, order=order, space=0)
        ctx = _t(np.array([0, 1, 2, 1, 2, 99, -4]), torch.int32)
        word = _t(np.array([5, 5, 7, 7, 5, 7, 5]), torch.int32)
        score = torch.full((7,), float('nan'), device=DEV)
        after = torch.full((7,), -7, dtype=torch.int32, device=DEV)
        assert hip.load().ctcasr_wordlm_lookup(
            ctypes.addressof(tables), ctx.data_ptr(), word.data_ptr(), 7, score.data_ptr(),
            after.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        # found at once where the range holds the word (contexts clamp into [0, 3)); else the
        # chain h -> h never ends: -inf
        assert score.cpu().tolist() == [-np.inf, -1.0, -2.0, -np.inf, -np.inf, -2.0, -np.inf]
        assert after.cpu().tolist() == [0, 2, 1, 0, 0, 1, 0]
    bad = hip.WordLm(ctx_begin=tensors[0].data_ptr(), succ_word=tensors[1].data_ptr(),
                     succ_lp=tensors[2].data_ptr(), succ_ctx=tensors[3].data_ptr(),
                     ctx_backoff=tensors[4].data_ptr(), ctx_parent=tensors[5].data_ptr(),
                     num_succ=2, num_nodes=0, num_ctx=contexts, order=6, space=0)
    assert hip.load().ctcasr_wordlm_lookup(ctypes.addressof(bad), ctx.data_ptr(), word.data_ptr(),
                                           7, score.data_ptr(), after.data_ptr(), None) == -1


# ------------------------------------------------------------------------------------------------
# 2. Parity with the dense automaton
# ------------------------------------------------------------------------------------------------
TEXTS = ['ab cab d a', 'dd acbd bb ca', 'c']      # row 1: word pairs the corpus does not hold


def _facts(paths, dense, backoffs, space):
    """(most words in a hypothesis, most back-offs of a space edge on a hypothesis' path), from
    the reference's automaton alone."""
    most_words, most_backoffs = 0, 0
    for path in paths:
        # words: the runs of labels between spaces (a trailing space opens no word)
        state, words = 0, sum(1 for i, c in enumerate(path)
                              if c != space and (i == 0 or path[i - 1] == space))
        for c in path:
            if c == space:
                most_backoffs = max(most_backoffs, backoffs[state] or 0)
            state = int(dense.next[state, c])
        most_words = max(most_words, words)
    return most_words, most_backoffs


@pytest.mark.parametrize('oov', [-np.inf, -4.0])
@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('classes,blank', [(29, 28), (6, 5)])
def test_parity_with_the_dense_automaton(hip, classes, blank, order, oov):
    space = ALPHABETS[(classes, blank)][0]
    rng = np.random.default_rng(100 * classes + order)
    most_words, most_backoffs = 0, 0
    for weight, bonus in ((1.0, 0.0), (0.7, 0.4)):
        scorer, dense, backoffs = _dense(classes, blank, order, weight, bonus, oov)
        for width, num_steps in ((8, 40), (100, 40), (1024, 24)):
            logits = _logits(rng, num_steps, classes, blank, TEXTS, noise=0.6)
            seq_len = np.array([num_steps, num_steps - 7, 1], dtype=np.int32)
            for norm in NORMS:
                # against the existing GPU kernels on the dense automaton: the same bits
                for top_paths in (1, 8):
                    got = _word(hip, logits, seq_len, width, scorer, top_paths, blank, norm)
                    want = _dense_nbest(hip, logits, seq_len, width, dense, top_paths, blank, norm)
                    assert _same_bits(got, want), (weight, width, norm, top_paths)
                top = hip.ctc_beam_decode_lm(_t(logits), _t(seq_len, torch.int32), width, dense,
                                             blank=blank, normalization=norm)
                top = tuple(t.cpu().numpy() for t in top)
                assert _same_bits((got[0][:, 0], got[1][:, 0], got[2][:, 0]), top)
                # the CPU reference is Python, about a second per call at width 100: it decodes
                # width 8 under every setting and width 100 once per configuration, to keep a
                # case within a few seconds; width 1024 is covered GPU against GPU above
                if width > 100 or (width == 100 and (norm != 'max' or bonus)):
                    continue
                # against the CPU reference, at the bars of test_parity_with_the_reference
                one = _word(hip, logits, seq_len, width, scorer, 1, blank, norm)
                paths, logp = lref.beam_search_decode(logits, seq_len, width, dense.next,
                                                      dense.score, dense.final, blank=blank,
                                                      normalization=norm)
                for b in range(3):
                    n = int(one[1][b, 0])
                    assert one[0][b, 0, :n].tolist() == paths[b], (b, width, norm)
                    assert (one[0][b, 0, n:] == 0).all()
                assert np.allclose(one[2][:, 0], logp, rtol=1e-5, atol=1e-3), (one[2], logp)
                words, backed = _facts(paths, dense, backoffs, space)
                most_words, most_backoffs = max(most_words, words), max(most_backoffs, backed)
    assert most_words >= 2, 'no decoded hypothesis of this configuration holds two words'
    if order > 1:
        assert most_backoffs >= 1, 'no scored space edge of this configuration backed off'


# ------------------------------------------------------------------------------------------------
# 3. Memo and workspace
# ------------------------------------------------------------------------------------------------
_raw = functools.partial(raw_beam, top_paths=2)     # the C entry point of the scorer's rule


def test_a_row_in_a_batch_of_64_is_the_row_alone(hip):
    rng = np.random.default_rng(64)
    texts = [' '.join(LEXICON[int(i)] for i in rng.integers(0, len(LEXICON), size=3))
             for _ in range(64)]
    logits = _logits(rng, 40, 29, 28, texts)
    seq_len = rng.integers(0, 41, size=64).astype(np.int32)
    seq_len[[0, 63]] = 40
    scorer = _dense(29, 28, 3, 0.7, 0.4, -4.0)[0]
    for width in (16, 100):
        got = _word(hip, logits, seq_len, width, scorer, 4, 28)
        for b in (0, 17, 40, 63):
            one = _word(hip, logits[:, b:b + 1], seq_len[b:b + 1], width, scorer, 4, 28)
            assert _same_bits(one, tuple(x[b:b + 1] for x in got)), b


def test_scorers_and_lengths_share_one_workspace(hip):
    """Scorer A, then B (another order, OOV on, other contexts on the same bytes), then A again;
    T = 40, then 17, then 40: each as on a fresh workspace, which is filled with 0xff first - a
    context or a memo that a launch reads, it has written."""
    rng = np.random.default_rng(77)
    texts = ['ab cab d a', 'dd acbd bb', 'a a ab abc', 'bad ca c']
    a = _dense(29, 28, 3, 1.0, 0.0, -np.inf)[0]
    b = _dense(29, 28, 2, 0.7, 0.4, -4.0)[0]
    need = hip.ctc_beam_wordlm_workspace_bytes(40, 4, 29, 32)
    shared = torch.full((need,), 0xff, dtype=torch.uint8, device=DEV)
    long_logits, short_logits = _logits(rng, 40, 29, 28, texts), _logits(rng, 17, 29, 28, texts)
    runs = [(a, long_logits, [40, 22, 40, 5]), (b, long_logits, [40, 22, 40, 5]),
            (a, long_logits, [40, 22, 40, 5]), (a, short_logits, [17, 9, 0, 17]),
            (a, long_logits, [40, 22, 40, 5])]
    results = []
    for scorer, logits, seq_len in runs:
        lg, sl = _t(logits), _t(np.array(seq_len), torch.int32)
        status, got = _raw(hip, lg, sl, 32, scorer, shared)
        fresh = torch.zeros((need,), dtype=torch.uint8, device=DEV)
        status_fresh, want = _raw(hip, lg, sl, 32, scorer, fresh)
        assert status == 0 and status_fresh == 0
        assert _same_bits(got, want)
        results.append(got)
    assert _same_bits(results[0], results[2]) and _same_bits(results[0], results[4])
    assert not np.array_equal(results[0][2], results[1][2])
    # too small a workspace, and scorer arguments the entry point refuses: nothing launched
    lg, sl = _t(long_logits), _t(np.array([40, 22, 40, 5]), torch.int32)
    assert _raw(hip, lg, sl, 32, a, shared[:need - 1])[0] == -3
    assert _raw(hip, lg, sl, 32, a, shared, top_paths=33)[0] == -1
    assert _raw(hip, lg, sl, 32, a, shared, blank=1)[0] == -1         # the space is the blank


def test_workspace_function_refuses_what_the_plain_one_refuses(hip):
    lib = hip.load()
    for args in ((0, 4, 29, 8), (30, 0, 29, 8), (30, 4, 0, 8), (30, 4, 29, 0), (-1, 4, 29, 8),
                 (30, 4, 29, -5)):
        assert lib.ctcasr_ctc_beam_workspace_bytes(*args) == 0
        assert lib.ctcasr_ctc_beam_wordlm_workspace_bytes(*args) == 0
    for args in ((30, 4, 29, 8), (500, 16, 29, 1024), (1, 1, 2, 1), (3200, 1, 64, 1024)):
        assert hip.ctc_beam_wordlm_workspace_bytes(*args) > hip.ctc_beam_workspace_bytes(*args) > 0
    scorer = _dense(29, 28, 2, 1.0, 0.0, -np.inf)[0]
    logits, seq_len = _t(np.zeros((6, 5, 29), dtype=np.float32)), _t(np.zeros(5), torch.int32)
    with pytest.raises(hip.CtcAsrError, match='4 lengths for a batch of 5'):
        hip.ctc_beam_decode_wordlm(logits, seq_len[:4], 8, scorer)
    with pytest.raises(hip.CtcAsrError, match='29 classes'):
        hip.ctc_beam_decode_wordlm(logits[:, :, :6].contiguous(), seq_len, 8, scorer)
    for width, top_paths in ((0, 1), (1025, 1), (8, 0), (8, 9)):
        with pytest.raises(hip.CtcAsrError):
            hip.ctc_beam_decode_wordlm(logits, seq_len, width, scorer, top_paths)


# ------------------------------------------------------------------------------------------------
# 4. Behaviour
# ------------------------------------------------------------------------------------------------
def _texts(out, out_len, classes=29, blank=28):
    space, letters = ALPHABETS[(classes, blank)]
    names = {space: ' ', **{c: 'abcde'[i] for i, c in enumerate(letters)}}
    return [''.join(names.get(int(c), '?') for c in out[b, 0, :out_len[b, 0]])
            for b in range(out.shape[0])]


def test_closed_vocabulary_decodes_lexicon_words_only_and_oov_decodes_the_rest(hip):
    rng = np.random.default_rng(5)
    spoken = ['ab cab d a', 'ab ede d', 'dd acbd bb ca', 'eee a', 'bad ca', 'a']
    logits = _logits(rng, 40, 29, 28, spoken, noise=0.3, peak=8.0, blank_bias=4.0)
    seq_len = np.array([40, 40, 33, 40, 12, 40], dtype=np.int32)
    closed = _dense(29, 28, 2, 1.0, 0.0, -np.inf)[0]
    out, out_len, logp, n_paths = _word(hip, logits, seq_len, 32, closed, 4, 28)
    assert np.isfinite(logp[:, 0]).all()
    for b in range(6):
        for k in range(int(n_paths[b])):
            text = _texts(out[b:b + 1, k:k + 1], out_len[b:b + 1, k:k + 1])[0]
            if np.isfinite(logp[b, k]):       # a finished hypothesis: words of the lexicon only
                closed_text = text[:-1] if text.endswith(' ') else text     # (may end at a space)
                assert text == '' or all(w in LEXICON for w in closed_text.split(' ')), text
            assert not text.startswith(' ') and '  ' not in text, text
    texts = _texts(out, out_len)
    assert texts[0] == spoken[0] and 'ede' not in texts[1] and 'eee' not in texts[3]
    # OOV on: the rows that spell a word outside the lexicon decode it
    opened = _dense(29, 28, 2, 1.0, 0.0, -4.0)[0]
    out, out_len, logp, _ = _word(hip, logits, seq_len, 32, opened, 1, 28)
    texts = _texts(out, out_len)
    print('closed / open vocabulary:', texts)
    assert texts[1] == spoken[1] and texts[3] == spoken[3] and texts[0] == spoken[0]


def test_weight_zero_is_the_dense_word_list_constraint_bit_for_bit(hip):
    """Weight 0, bonus 0, OOV off: every score the model adds is 0 or -inf - the lexicon as a
    constraint.  The dense automaton of the same lexicon, written down directly: trie states,
    the space leads back to the root, words end anywhere a word ends or at the root."""
    model, _ = _models(29, 28, 2)
    scorer = model.scaled(0.0, 0.0)
    trie = model.trie_next
    nxt = np.zeros(trie.shape, dtype=np.int32)
    score = np.full(trie.shape, -np.inf, dtype=np.float32)
    score[trie >= 0] = 0.0
    nxt[trie >= 0] = trie[trie >= 0]
    ends = model.trie_word >= 0
    score[ends, 1], nxt[ends, 1] = 0.0, 0
    final = np.where(ends, 0.0, -np.inf).astype(np.float32)
    final[0] = 0.0
    dense = lm.LmScorer(nxt, score, final)
    rng = np.random.default_rng(3)
    logits = _logits(rng, 40, 29, 28, TEXTS)
    seq_len = np.array([40, 33, 1], dtype=np.int32)
    for width in (8, 100):
        for norm in NORMS:
            got = _word(hip, logits, seq_len, width, scorer, 8, 28, norm)
            want = _dense_nbest(hip, logits, seq_len, width, dense, 8, 28, norm)
            assert _same_bits(got, want), (width, norm)


@pytest.mark.parametrize('norm', NORMS)
def test_everything_forbidden_decodes_to_the_empty_string(hip, norm):
    """A lexicon whose letters the logits' classes never reach... here: a trie with no edges and
    OOV off.  Nothing can be emitted; the empty hypothesis ends with Wd(0, </s>)."""
    from oracle import ctc as octc
    scorer = lm.WordLmScorer(np.full((2, 29), -1, dtype=np.int32), [-1, -1], [0, 2], [0, 1],
                             [-2.0, 0.625], [0, 0], [0.0], [0], 1, 1)
    rng = np.random.default_rng(42)
    logits = rng.normal(size=(25, 3, 29)).astype(np.float32) * 2
    seq_len = np.array([25, 0, 9], dtype=np.int32)
    for width in (1, 16):
        out, out_len, logp, n_paths = _word(hip, logits, seq_len, width, scorer, 1, 28, norm)
        assert (out_len == 0).all() and (out == 0).all() and (n_paths == 1).all()
        for b in range(3):
            x = logits[:seq_len[b], b].astype(np.float64)
            x = octc.log_softmax(x) if norm == 'log_softmax' else x - x.max(axis=1, keepdims=True)
            assert float(logp[b, 0]) == pytest.approx(x[:, 28].sum() + 0.625, rel=1e-5, abs=1e-5)
    # ... and where the end is forbidden too, logp is -inf as the dense kernel reports it
    dead = lm.WordLmScorer(np.full((2, 29), -1, dtype=np.int32), [-1, -1], [0, 2], [0, 1],
                           [-2.0, -np.inf], [0, 0], [0.0], [0], 1, 1)
    out, out_len, logp, _ = _word(hip, logits, seq_len, 8, dead, 1, 28, norm)
    assert (out_len == 0).all() and np.isneginf(logp).all()


def test_the_memo_serves_most_space_edges(hip):
    """`stats`: a tree node's space edge is looked up at most once, so the lookups performed stay
    below the branches expanded, and below the tree nodes there can be."""
    rng = np.random.default_rng(9)
    logits = _logits(rng, 40, 29, 28, TEXTS)
    seq_len = np.array([40, 33, 1], dtype=np.int32)
    scorer = _dense(29, 28, 3, 1.0, 0.0, -4.0)[0]
    stats = torch.full((3, 2), -1, dtype=torch.int64, device=DEV)
    _word(hip, logits, seq_len, 32, scorer, 1, 28, stats=stats)
    stats = stats.cpu().numpy()
    print('branches expanded / lookups performed per utterance:', stats.tolist())
    assert (stats[:, 0] > 0).all() and (stats[:, 1] >= 0).all()
    assert (stats[:, 1] <= stats[:, 0]).all() and stats[0, 1] < stats[0, 0]
    # closed vocabulary: a node that closes no word runs no walk, and the root never does
    closed = torch.full((3, 2), -1, dtype=torch.int64, device=DEV)
    _word(hip, logits, seq_len, 32, _dense(29, 28, 3, 1.0, 0.0, -np.inf)[0], 1, 28, stats=closed)
    closed = closed.cpu().numpy()
    assert closed[2].tolist() == [1, 0] and 0 < closed[0, 1] < closed[0, 0]
    assert stats[0, 0] <= 40 * 32 and stats[2, 0] == 1


# ------------------------------------------------------------------------------------------------
# 5. Through the model and the drivers
# ------------------------------------------------------------------------------------------------
@pytest.fixture()
def trained(tmp_path):
    """The synthetic corpus and flags of test_gpu_beam_lm.py's fixture, one epoch trained."""
    from ctc_asr_amd import synth, train
    FLAGS.reset()
    corpus_dir = str(tmp_path / 'corpus')
    rng = np.random.default_rng(5)
    durations = np.round(rng.uniform(0.7, 2.0, size=21), 2)
    for name, seed, count in (('train', 1, 21), ('dev', 2, 9), ('test', 3, 9)):
        synth.write_corpus(corpus_dir, str(tmp_path / (name + '.csv')), durations[:count],
                           seed=seed, chars_per_second=6.0, subdir=name)
    FLAGS.update(corpus_dir=corpus_dir, train_csv=str(tmp_path / 'train.csv'),
                 dev_csv=str(tmp_path / 'dev.csv'), test_csv=str(tmp_path / 'test.csv'),
                 train_dir=str(tmp_path / 'ckpt'), batch_size=4, num_buckets=3,
                 feature_type='mel', feature_normalization='local', used_model='ds2',
                 conv_filters=[4, 4], num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                 rnn_cell='lstm', max_epochs=1, learning_rate=1e-3, beam_width=8,
                 log_frequency=2, random_seed=7, dense_dropout_rate=0.0)
    assert train.main([]) == 0
    yield tmp_path
    FLAGS.reset()


def test_drivers_decode_with_the_word_model_of_lm_path(trained, capsys, monkeypatch):
    from ctc_asr_amd import evaluate, hip, input_functions, predict, storage
    from ctc_asr_amd.model import CTCModel, ModelConfig
    words = str(trained / 'words.npz')
    assert lm.main(['--lm_unit', 'word', '--lm_corpus_csv', FLAGS.train_csv, '--lm_order', '2',
                    '--lm_path', words]) == 0
    FLAGS.update(lm_corpus_csv='', lm_unit='char')
    calls = []
    real = hip.ctc_beam_search

    def counted(logits, seq_len, beam_width, scorer=None, *args, **kwargs):
        if isinstance(scorer, lm.WordLmScorer):         # the searches with the word model
            calls.append(1)
        return real(logits, seq_len, beam_width, scorer, *args, **kwargs)
    monkeypatch.setattr(hip, 'ctc_beam_search', counted)
    capsys.readouterr()
    flags = ['--lm_path', words, '--lm_oov_score=-6']
    assert evaluate.main(['--dev'] + flags) == 0
    out = capsys.readouterr().out
    assert 'word_error_rate' in out and 'mean_edit_distance' in out
    assert calls
    rows = input_functions.read_manifest(FLAGS.test_csv)
    wav = os.path.join(FLAGS.corpus_dir, rows[2]['path'])
    del calls[:]
    assert predict.main(['--input', wav, '--nbest', '4'] + flags) == 0
    out = capsys.readouterr().out
    assert calls and re.search(r"\{'decoded'.*'nbest'.*\}", out, flags=re.S)
    # --rescore_lm_path: the word model re-ranks on the host, lm_logp = sequence_scores
    del calls[:]
    FLAGS.update(lm_path='', nbest=0)
    assert predict.main(['--input', wav, '--nbest', '4', '--rescore_lm_path', words,
                         '--rescore_lm_oov_score=-6']) == 0
    assert not calls and "'nbest'" in capsys.readouterr().out
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=1)
    storage.restore_checkpoint(storage.latest_checkpoint(FLAGS.train_dir), model)
    rescorer = lm.rescorer_from_flags(model.cfg.num_classes)
    assert isinstance(rescorer, lm.WordLmScorer) and rescorer.oov_score == -6.0
    feats, lengths = input_functions.features_from_pcm([input_functions.read_wav(wav)],
                                                       model.device)
    logits, seq_len = model.inference_fn(feats, lengths, training=False)
    listed = model.nbest_fn(logits, seq_len, 4, rescorer=rescorer)[0]
    assert listed['hypotheses']
    for hyp in listed['hypotheses']:
        want = float(rescorer.sequence_scores([hyp['labels']])[0])
        assert hyp['lm_logp'] == want or (np.isneginf(want) and np.isneginf(hyp['lm_logp']))
    # decode_many equals decode_fn batch by batch, through the new entry point
    scorer = lm.load(words, 29).scaled(0.8, 0.2, -6.0)
    rng = np.random.default_rng(91)
    batches = []
    for steps, batch_lengths in ((7, [7, 0, 3]), (40, [40]), (21, [0, 21, 1, 0])):
        noise = rng.normal(size=(steps, len(batch_lengths), 29)).astype(np.float32) * 2
        batches.append((_t(noise), _t(np.array(batch_lengths), torch.int32), None))
    del calls[:]
    joint = model.decode_many(batches, beam_width=8, scorer=scorer)
    assert len(calls) == 1
    for (noise, batch_lengths, _), got in zip(batches, joint):
        one = model.decode_fn(noise, batch_lengths, None, beam_width=8, scorer=scorer)
        assert got[0] == one[0] and list(got[1]) == list(one[1])
    assert len(calls) == 4
    assert model.decode_group_size(500, 16, scorer=scorer) >= 1
