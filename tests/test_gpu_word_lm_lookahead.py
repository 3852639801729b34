"""Look-ahead scores inside a word, fused into the CTC beam search (csrc/beam.hip `LM == 3`,
`ctcasr_ctc_beam_decode_wordlm_lookahead`, `hip.ctc_beam_decode_wordlm` with a scorer that carries
a table, `--lm_lookahead`).

The oracle is tests/word_lm_lookahead_reference.py: K26's edge and end rules over the reference's
dicts, materialised as the dense automaton over the reachable (trie node, context) pairs.  The
*existing* GPU kernels decode that automaton, and the new form must return their bits - the search
executes the same float32 operations on the same float32 scores.  Shapes, logits and bars are
those of tests/test_gpu_word_lm.py."""

import functools
import os
import re

import numpy as np
import pytest
import torch

from ctc_asr_amd import lm
from ctc_asr_amd.params import FLAGS
from tests import lm_beam_reference as lref
from tests import word_lm_lookahead_reference as laref
from tests import word_lm_reference as ref
from tests.test_gpu_word_lm import (ALPHABETS, LEXICON, NORMS, TEXTS, _dense_nbest, _facts, _logits,
                                    _models, _raw, _same_bits, _t, _word, trained)  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@functools.lru_cache(maxsize=None)
def _dense(classes, blank, order, weight, bonus, oov):
    """(scaled WordLmScorer with its table, dense LmScorer of the look-ahead reference, backoffs
    per dense state)."""
    model, restated = _models(classes, blank, order)
    nxt, score, final, _, backoffs = ref.dense_automaton(
        laref.LookaheadScorer(restated, weight, bonus, oov), classes, blank)
    return (model.scaled(weight, bonus, oov, lookahead=True), lm.LmScorer(nxt, score, final),
            backoffs)


# ------------------------------------------------------------------------------------------------
# 1. Parity with the dense automaton
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('oov', [-np.inf, -4.0])
@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('classes,blank', [(29, 28), (6, 5)])
def test_parity_with_the_dense_automaton(hip, classes, blank, order, oov):
    space = ALPHABETS[(classes, blank)][0]
    rng = np.random.default_rng(100 * classes + order)
    most_words, most_backoffs = 0, 0
    for weight, bonus in ((1.0, 0.0), (0.7, 0.4)):
        scorer, dense, backoffs = _dense(classes, blank, order, weight, bonus, oov)
        assert scorer.lookahead is not None and scorer.lookahead[2:].any()
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
                if width != 8:
                    continue
                # against the CPU reference, at the bars of test_gpu_word_lm.py
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


@pytest.mark.parametrize('oov', [-np.inf, -4.0])
def test_weight_zero_returns_the_bits_of_the_plain_launch(hip, oov):
    """Weight 0: the table is 0 (with OOV on: oov_score below the root's children, which the
    edges and the space settle exactly), so every score is K24's."""
    model, _ = _models(29, 28, 2)
    rng = np.random.default_rng(3)
    logits = _logits(rng, 40, 29, 28, TEXTS)
    seq_len = np.array([40, 33, 1], dtype=np.int32)
    for bonus in (0.0, 0.4):
        plain, ahead = model.scaled(0.0, bonus, oov), model.scaled(0.0, bonus, oov, lookahead=True)
        for width in (8, 100):
            for norm in NORMS:
                got = _word(hip, logits, seq_len, width, ahead, 8, 28, norm)
                want = _word(hip, logits, seq_len, width, plain, 8, 28, norm)
                assert _same_bits(got, want), (bonus, width, norm)
                assert np.isfinite(want[2][0, 0])


# ------------------------------------------------------------------------------------------------
# 2. Memo and workspace
# ------------------------------------------------------------------------------------------------
def test_both_rules_share_one_workspace(hip):
    """Plain, look-ahead, plain, look-ahead on the same bytes (filled with 0xff first), the
    look-ahead launches at two lengths: each as on a fresh workspace - the memo of one rule never
    serves the other - and the plain launches equal each other."""
    rng = np.random.default_rng(77)
    texts = ['ab cab d a', 'dd acbd bb', 'a a ab abc', 'bad ca c']
    model, _ = _models(29, 28, 3)
    plain, ahead = model.scaled(0.7, 0.4, -4.0), model.scaled(0.7, 0.4, -4.0, lookahead=True)
    need = hip.ctc_beam_wordlm_workspace_bytes(40, 4, 29, 32)
    shared = torch.full((need,), 0xff, dtype=torch.uint8, device=DEV)
    long_logits, short_logits = _logits(rng, 40, 29, 28, texts), _logits(rng, 17, 29, 28, texts)
    runs = [(plain, long_logits, [40, 22, 40, 5]), (ahead, long_logits, [40, 22, 40, 5]),
            (plain, long_logits, [40, 22, 40, 5]), (ahead, short_logits, [17, 9, 0, 17])]
    results = []
    for scorer, logits, seq_len in runs:
        lg, sl = _t(logits), _t(np.array(seq_len), torch.int32)
        status, got = _raw(hip, lg, sl, 32, scorer, shared)
        fresh = torch.zeros((need,), dtype=torch.uint8, device=DEV)
        status_fresh, want = _raw(hip, lg, sl, 32, scorer, fresh)
        assert status == 0 and status_fresh == 0
        assert _same_bits(got, want)
        results.append(got)
    assert _same_bits(results[0], results[2])
    # the two rules rank the same complete hypotheses, but their beams differ: not the same list
    assert not _same_bits(results[0], results[1])
    # ... and the raw launch is the wrapper's
    assert _same_bits(results[1], _word(hip, long_logits, [40, 22, 40, 5], 32, ahead, 2, 28))


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


def test_stats_count_as_in_the_plain_search(hip):
    """Branches expanded and lookups performed: a tree node's space edge is looked up at most
    once, so the lookups stay far below the expansions, as in
    test_gpu_word_lm.py::test_the_memo_serves_most_space_edges."""
    rng = np.random.default_rng(9)
    logits = _logits(rng, 40, 29, 28, TEXTS)
    seq_len = np.array([40, 33, 1], dtype=np.int32)
    stats = torch.full((3, 2), -1, dtype=torch.int64, device=DEV)
    _word(hip, logits, seq_len, 32, _dense(29, 28, 3, 1.0, 0.0, -4.0)[0], 1, 28, stats=stats)
    stats = stats.cpu().numpy()
    print('branches expanded / lookups performed per utterance:', stats.tolist())
    assert (stats[:, 0] > 0).all() and (stats[:, 1] >= 0).all()
    assert (stats[:, 1] <= stats[:, 0]).all() and stats[0, 1] < stats[0, 0]
    closed = torch.full((3, 2), -1, dtype=torch.int64, device=DEV)
    _word(hip, logits, seq_len, 32, _dense(29, 28, 3, 1.0, 0.0, -np.inf)[0], 1, 28, stats=closed)
    closed = closed.cpu().numpy()
    assert closed[2].tolist() == [1, 0] and 0 < closed[0, 1] < closed[0, 0]
    assert stats[0, 0] <= 40 * 32 and stats[2, 0] == 1


def test_refusals(hip, monkeypatch):
    rng = np.random.default_rng(1)
    logits = _logits(rng, 12, 29, 28, ['ab a', 'c'])
    seq_len = np.array([12, 12], dtype=np.int32)
    scorer = _dense(29, 28, 2, 1.0, 0.0, -np.inf)[0]
    need = hip.ctc_beam_wordlm_workspace_bytes(12, 2, 29, 8)
    workspace = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    lg, sl = _t(logits), _t(seq_len, torch.int32)
    assert _raw(hip, lg, sl, 8, scorer, workspace)[0] == 0
    status, got = _raw(hip, lg, sl, 8, scorer, workspace, table=None)
    assert status == -1                                        # CTCASR_ERR_BAD_ARGUMENT
    assert (got[1] == -7).all() and (got[3] == -7).all()       # nothing was launched
    assert _raw(hip, lg, sl, 8, scorer, workspace[:need - 1])[0] == -3
    assert _raw(hip, lg, sl, 8, scorer, workspace, top_paths=9)[0] == -1
    assert _raw(hip, lg, sl, 8, scorer, workspace, blank=1)[0] == -1      # the space is the blank
    # the wrapper: a table of the wrong length, a NaN, an infinity - before any launch
    launched = []
    real = hip.load()
    monkeypatch.setattr(hip, 'load', lambda: launched.append(1) or real)
    model, _ = _models(29, 28, 2)
    for table in (scorer.lookahead[:-1], np.append(scorer.lookahead, 0.0),
                  np.where(np.arange(scorer.num_nodes) == 3, np.nan, scorer.lookahead),
                  np.where(np.arange(scorer.num_nodes) == 1, -np.inf, scorer.lookahead)):
        bad = model.scaled(1.0, 0.0)
        bad.lookahead = table
        del launched[:]
        with pytest.raises(hip.CtcAsrError, match='look-ahead table'):
            hip.ctc_beam_decode_wordlm(lg, sl, 8, bad)
        assert not launched


# ------------------------------------------------------------------------------------------------
# 3. The effect
# ------------------------------------------------------------------------------------------------
def test_a_narrow_beam_with_look_ahead_agrees_with_the_wide_plain_beam_more_often(hip):
    """The 36 utterances of `laref.effect_batches`.  The device's decodes at widths 4 and 8 are
    the reference's, path by path, for both forms; and against the device's own width-512 plain
    decode the look-ahead decode agrees on strictly more utterances than the plain decode of the
    same width (the reference counts 12 against 6 at width 4, 19 against 10 at width 8)."""
    from tests.test_word_lm_lookahead_host import reference_decoder
    model, _ = _models(laref.EFFECT_CLASSES, laref.EFFECT_BLANK, laref.EFFECT_ORDER)
    scorers = {False: model.scaled(1.0, 0.0), True: model.scaled(1.0, 0.0, lookahead=True)}

    def decode(logits, seq_len, width, ahead):
        out, out_len, _, _ = _word(hip, logits, seq_len, width, scorers[ahead], 1,
                                   laref.EFFECT_BLANK)
        return [out[b, 0, :out_len[b, 0]].tolist() for b in range(out.shape[0])]

    counts, decodes = laref.effect_counts(decode)
    print('utterances of 36 equal to the width-512 plain decode (plain, look-ahead):', counts)
    reference = reference_decoder()
    for seed, (logits, seq_len) in zip(laref.EFFECT_SEEDS, laref.effect_batches()):
        for width in laref.EFFECT_WIDTHS:
            for ahead in (False, True):
                assert decodes[(seed, width, ahead)] == reference(logits, seq_len, width, ahead), \
                    (seed, width, ahead)
    for width in laref.EFFECT_WIDTHS:
        assert counts[width][1] > counts[width][0], (width, counts)


# ------------------------------------------------------------------------------------------------
# 4. Through the drivers
# ------------------------------------------------------------------------------------------------
def test_drivers_decode_with_look_ahead(trained, capsys, monkeypatch):
    from ctc_asr_amd import evaluate, hip, input_functions, predict, storage
    from ctc_asr_amd.model import CTCModel, ModelConfig
    words = str(trained / 'words.npz')
    assert lm.main(['--lm_unit', 'word', '--lm_corpus_csv', FLAGS.train_csv, '--lm_order', '2',
                    '--lm_path', words]) == 0
    FLAGS.update(lm_corpus_csv='', lm_unit='char')
    tables = []
    real = hip.ctc_beam_search

    def counted(logits, seq_len, beam_width, scorer, *args, **kwargs):
        tables.append(scorer.lookahead is not None)
        return real(logits, seq_len, beam_width, scorer, *args, **kwargs)
    monkeypatch.setattr(hip, 'ctc_beam_search', counted)
    rows = input_functions.read_manifest(FLAGS.test_csv)
    wav = os.path.join(FLAGS.corpus_dir, rows[2]['path'])
    flags = ['--lm_path', words, '--lm_oov_score=-6', '--lm_weight', '1.5']
    printed = {}
    for ahead in (False, True):
        extra = ['--lm_lookahead'] if ahead else []
        del tables[:]
        capsys.readouterr()
        assert evaluate.main(['--dev'] + flags + extra) == 0
        out = capsys.readouterr().out
        assert 'word_error_rate' in out and 'mean_edit_distance' in out
        assert tables and all(t == ahead for t in tables)
        del tables[:]
        assert predict.main(['--input', wav] + flags + extra) == 0
        printed[ahead] = capsys.readouterr().out
        assert tables and all(t == ahead for t in tables)
        FLAGS.update(lm_lookahead=False)
    # what predict printed is what the search returns for the scorer of the flags on the same logits
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=1)
    storage.restore_checkpoint(storage.latest_checkpoint(FLAGS.train_dir), model)
    feats, lengths = input_functions.features_from_files([wav], model.device)
    logits, seq_len = model.inference_fn(feats, lengths, training=False)
    for ahead in (False, True):
        scorer = lm.load(words, 29).scaled(1.5, 0.0, -6.0, lookahead=ahead)
        out, out_len, _, _ = hip.ctc_beam_decode_wordlm(logits, seq_len, FLAGS.beam_width, scorer)
        labels = out[0, 0, :int(out_len[0, 0])].cpu().tolist()
        found = re.search(r"'decoded': array\(\[([^\]]*)\]", printed[ahead])
        assert found and [int(v) for v in re.findall(r'\d+', found.group(1))] == labels, \
            (ahead, printed[ahead], labels)
