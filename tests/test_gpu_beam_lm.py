"""The CTC beam search with a language model fused in (csrc/beam.hip `LM = true`,
`hip.ctc_beam_decode_lm`, `CTCModel.decode_fn` / `decode_many(scorer=...)`, the `--lm_path`
drivers).

Four kinds of evidence.  GPU against GPU, exact: with a scorer that scores nothing the fused
kernel returns the bits of the plain one.  Parity with the numpy restatement
(tests/lm_beam_reference.py) under real scorers at the bars of test_gpu_beam_edges.py: path and
length equal, logp rtol 1e-5 / atol 1e-3.  The truth, not through any TensorFlow-style code: an
unpruned search returns the argmax over labellings of ln p_ctc + automaton score, p_ctc from all
C^T paths.  And behaviour: forbidden edges are never taken, a scorer flips a close call, rows
and launches do not leak into each other.  Inputs are continuous random logits: exact ties in a
total are not a parity case (beam.hip's header)."""

import os
import re

import numpy as np
import pytest
import torch

from ctc_asr_amd import lm
from ctc_asr_amd.params import FLAGS
from oracle import ctc as octc
from tests import lm_beam_reference as ref
from tests.beam_helpers import _logits, _random_scorer, _same_bits, _t, _tables, raw_beam
from tests.test_lm_host import TRUTH_CASES, check_truth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORMS = ['max', 'log_softmax']
MAX_WIDTH = 1024


def _run(hip, logits, seq_len, width, scorer, blank=None, norm='max'):
    out, out_len, logp = hip.ctc_beam_decode_lm(_t(logits), _t(np.asarray(seq_len), torch.int32),
                                                width, scorer, blank=blank, normalization=norm)
    return out.cpu().numpy(), out_len.cpu().numpy(), logp.cpu().numpy()


def _run_plain(hip, logits, seq_len, width, blank=None, norm='max'):
    out, out_len, logp = hip.ctc_beam_decode(_t(logits), _t(np.asarray(seq_len), torch.int32),
                                             width, blank=blank, normalization=norm)
    return out.cpu().numpy(), out_len.cpu().numpy(), logp.cpu().numpy()


def _zero_scorer(classes, final=False):
    return lm.LmScorer(np.zeros((1, classes), dtype=np.int32),
                       np.zeros((1, classes), dtype=np.float32),
                       np.zeros(1, dtype=np.float32) if final else None)


def _check(hip, logits, seq_len, width, scorer, blank, norm):
    """One call against the numpy reference, every row: out_len and path equal, the row zero
    beyond out_len, every label in [0, C) and never the blank, logp rtol 1e-5 / atol 1e-3."""
    num_steps, batch, classes = logits.shape
    seq_len = np.asarray(seq_len, dtype=np.int32)
    out, out_len, logp = _run(hip, logits, seq_len, width, scorer, blank, norm)
    ref_paths, ref_logp = ref.beam_search_decode(logits, seq_len, width, *_tables(scorer),
                                                 blank=blank, normalization=norm)
    assert out.shape == (batch, num_steps) and out_len.shape == (batch,)
    for b in range(batch):
        n = int(out_len[b])
        assert n == len(ref_paths[b]), (b, n, len(ref_paths[b]))
        assert out[b, :n].tolist() == ref_paths[b], (b, width, norm)
        assert (out[b, n:] == 0).all(), b
        assert ((out[b, :n] >= 0) & (out[b, :n] < classes) & (out[b, :n] != blank)).all(), b
    err = np.abs(np.where(logp == ref_logp, 0.0, logp.astype(np.float64) - ref_logp))
    print('T {} B {} C {} blank {} W {} S {} {}: max |logp - reference| {:.3g}'.format(
        num_steps, batch, classes, blank, width, scorer.num_states, norm, err.max()))
    assert np.allclose(logp, ref_logp, rtol=1e-5, atol=1e-3), (logp, ref_logp)
    return out, out_len, logp, ref_paths


# ------------------------------------------------------------------------------------------------
# 1. A scorer that scores nothing: the bits of the plain kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('shape', ['T 120 flat', 'T 120 peaked', 'T 500 B 16'])
def test_zero_scorer_equals_the_plain_kernel_bit_for_bit(hip, shape, norm):
    rng = np.random.default_rng(len(shape))
    if shape == 'T 500 B 16':
        logits = _logits(rng, 500, 16, 29, 28, scale=1.0)
        seq_len = np.full(16, 500, dtype=np.int32)
        seq_len[3], seq_len[9] = 317, 0
    else:
        flat = shape.endswith('flat')
        logits = _logits(rng, 120, 6, 29, 28, scale=0.3 if flat else 3.0,
                         blank_bias=0.0 if flat else 4.0)
        seq_len = np.array([120, 77, 1, 0, 120, 103], dtype=np.int32)
    for width in (1, 16, 64, MAX_WIDTH):
        plain = _run_plain(hip, logits, seq_len, width, 28, norm)
        for final in (False, True):
            fused = _run(hip, logits, seq_len, width, _zero_scorer(29, final), 28, norm)
            assert _same_bits(plain, fused), (width, final)


# ------------------------------------------------------------------------------------------------
# 2. Parity with the reference under real scorers
# ------------------------------------------------------------------------------------------------
def _corpus_rows(rng, classes, blank, count=40):
    labels = [c for c in range(classes) if c != blank]
    return [[labels[int(i)] for i in rng.integers(0, min(len(labels), 6),
                                                  size=int(rng.integers(1, 12)))]
            for _ in range(count)]


def _scorer_of(kind, rng, classes, blank):
    if kind == 'S 1':
        return _random_scorer(rng, 1, classes)
    if kind == 'S 4':
        return _random_scorer(rng, 4, classes)
    if kind == 'S 4, no final':
        return _random_scorer(rng, 4, classes, final=False)
    if kind == 'S 300, forbidden edges':
        return _random_scorer(rng, 300, classes, forbidden=0.05)
    model = lm.build_char_ngram(_corpus_rows(rng, classes, blank), 3, classes, blank=blank)
    if kind == 'order 3, weight 0.5':
        return model.scaled(0.5, 0.0)
    scaled = model.scaled(2.0, 0.75)
    if kind == 'order 3, weight 2, bonus, no final':
        return lm.LmScorer(scaled.next, scaled.score)
    raise ValueError(kind)


SCORERS = ['S 1', 'S 4', 'S 4, no final', 'S 300, forbidden edges', 'order 3, weight 0.5',
           'order 3, weight 2, bonus, no final']


@pytest.mark.parametrize('kind', SCORERS)
@pytest.mark.parametrize('classes,blank', [(29, 28), (3, 1), (64, 63)])
def test_parity_with_the_reference(hip, classes, blank, kind):
    """Ragged lengths with 0 and 1, widths 1, 8 and 32, both normalisations.  The n-grams are
    built over the labels of the decode (`build_char_ngram(..., blank=blank)`), so for C = 3
    with the blank at 1 both labels 0 and 2 carry n-gram scores."""
    rng = np.random.default_rng(1000 * classes + SCORERS.index(kind))
    logits = _logits(rng, 36, 5, classes, blank)
    seq_len = np.array([36, 0, 1, 19, 30], dtype=np.int32)
    scorer = _scorer_of(kind, rng, classes, blank)
    for width, norm in ((1, 'max'), (8, 'log_softmax'), (32, 'max')):
        _check(hip, logits, seq_len, width, scorer, blank, norm)


# ------------------------------------------------------------------------------------------------
# 3. Independent truth
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('classes,num_steps', TRUTH_CASES)
def test_unpruned_search_finds_the_best_fused_labelling(hip, classes, num_steps):
    """Width 1024 prunes nothing for these (C, T): the kernel must return the argmax of
    ln p_ctc + automaton score over all labellings, and that value (`check_truth` of
    test_lm_host.py: same generator, same near-tie cap, same bars)."""
    def decode(logits, seq_len, tables, blank):
        out, out_len, logp = _run(hip, logits, seq_len, MAX_WIDTH, lm.LmScorer(*tables), blank,
                                  'log_softmax')
        return [out[b, :out_len[b]].tolist() for b in range(len(out_len))], logp
    check_truth(decode, classes, num_steps)


# ------------------------------------------------------------------------------------------------
# 4. Forbidden edges
# ------------------------------------------------------------------------------------------------
LEXICON = ['ab', 'bad', 'cab']


def _word_list_scorer(words, classes=29):
    """Trie of ``words`` over the ids of `labels`: inside a word only the trie's edges exist, at
    a word's end only the space, which leads to state 1 - the start state again, but no place to
    end.  ``final`` is 0 at the start (state 0) and at word ends, -inf everywhere else."""
    from ctc_asr_amd.labels import ctoi
    nodes, ends = [{}, None], {0}
    for word in words:
        s = 0
        for ch in word:
            if ctoi(ch) not in nodes[s]:
                nodes[s][ctoi(ch)] = len(nodes)
                nodes.append({})
            s = nodes[s][ctoi(ch)]
        ends.add(s)
    nodes[1] = nodes[0]
    nxt = np.zeros((len(nodes), classes), dtype=np.int32)
    score = np.full((len(nodes), classes), -np.inf, dtype=np.float32)
    for s, edges in enumerate(nodes):
        for c, target in edges.items():
            nxt[s, c], score[s, c] = target, 0.0
        if s in ends and s != 0:
            nxt[s, ctoi(' ')], score[s, ctoi(' ')] = 1, 0.0
    final = np.array([0.0 if s in ends else -np.inf for s in range(len(nodes))],
                     dtype=np.float32)
    return lm.LmScorer(nxt, score, final)


def test_word_list_decodes_lexicon_words_only(hip):
    """Every decoded string is a sequence of lexicon words where the unconstrained decode of the
    same logits is not.  A beam can lose every complete hypothesis (all finals -inf: the winner
    is then an unfinished word); the inputs are fixed so that the reference's beam of 32 keeps
    one in every row, which the finite logp asserts."""
    from ctc_asr_amd.labels import decode
    rng = np.random.default_rng(43)
    logits = _logits(rng, 40, 6, 29, 28, blank_bias=3.0)
    # lean towards the letters of the lexicon, so that words do get decoded
    logits[:, :, [1, 2, 3, 4, 5]] += 2.0
    seq_len = np.array([40, 33, 40, 12, 40, 27], dtype=np.int32)
    scorer = _word_list_scorer(LEXICON)
    free = _run_plain(hip, logits, seq_len, 32, 28)
    free_text = [decode(free[0][b, :free[1][b]].tolist()) for b in range(6)]
    assert any(not all(w in LEXICON for w in text.split(' ')) for text in free_text), free_text
    out, out_len, logp, _ = _check(hip, logits, seq_len, 32, scorer, 28, 'max')
    texts = [decode(out[b, :out_len[b]].tolist()) for b in range(6)]
    print('word list: {} (unconstrained: {})'.format(texts, free_text))
    assert np.isfinite(logp).all()
    assert any(texts)
    for text in texts:
        assert text == '' or all(w in LEXICON for w in text.split(' ')), text


@pytest.mark.parametrize('norm', NORMS)
def test_everything_forbidden_decodes_to_the_empty_string(hip, norm):
    rng = np.random.default_rng(42)
    logits = _logits(rng, 25, 3, 29, 28)
    seq_len = np.array([25, 0, 9], dtype=np.int32)
    scorer = lm.LmScorer(np.zeros((2, 29), dtype=np.int32),
                         np.full((2, 29), -np.inf, dtype=np.float32),
                         np.array([0.625, -3.0], dtype=np.float32))
    for width in (1, 16):
        out, out_len, logp = _run(hip, logits, seq_len, width, scorer, 28, norm)
        assert (out_len == 0).all() and (out == 0).all()
        for b in range(3):
            x = logits[:seq_len[b], b].astype(np.float64)
            x = octc.log_softmax(x) if norm == 'log_softmax' else x - x.max(axis=1, keepdims=True)
            assert float(logp[b]) == pytest.approx(x[:, 28].sum() + 0.625, rel=1e-5, abs=1e-5)


# ------------------------------------------------------------------------------------------------
# 5. The model changes the answer where it should
# ------------------------------------------------------------------------------------------------
def test_a_scorer_flips_a_close_call_and_weight_zero_does_not(hip):
    classes, blank = 4, 3
    logits = np.full((5, 1, classes), -8.0, dtype=np.float32)
    logits[:, 0, blank] = 4.0
    logits[2, 0] = np.log([0.42, 0.30, 0.08, 0.20]).astype(np.float32)
    post = octc.brute_force_posteriors(logits[:, 0].astype(np.float64), blank)
    (best, p_best), (second, p_second) = sorted(post.items(), key=lambda kv: -kv[1])[:2]
    assert best == (0,) and second == (1,) and 1.0 < p_best / p_second < 2.0
    score = np.zeros((1, classes))
    score[0, 1] = np.log(4.0)
    favour = lm.LmScorer(np.zeros((1, classes), dtype=np.int32), score)
    for width in (4, 64):
        plain = _run_plain(hip, logits, [5], width, blank, 'log_softmax')
        assert plain[0][0, :plain[1][0]].tolist() == [0]
        out, out_len, logp = _run(hip, logits, [5], width, favour.scaled(1.0), blank,
                                  'log_softmax')
        assert out[0, :out_len[0]].tolist() == [1]
        assert float(logp[0]) == pytest.approx(np.log(p_second) + np.log(4.0), abs=1e-4)
        zero = _run(hip, logits, [5], width, favour.scaled(0.0), blank, 'log_softmax')
        assert _same_bits(zero, plain)


# ------------------------------------------------------------------------------------------------
# 6. Independence and hygiene
# ------------------------------------------------------------------------------------------------
def test_a_row_in_a_batch_of_64_is_the_row_alone(hip):
    rng = np.random.default_rng(64)
    logits = _logits(rng, 50, 64, 29, 28)
    seq_len = rng.integers(0, 51, size=64).astype(np.int32)
    seq_len[[0, 63]] = 50
    scorer = _random_scorer(rng, 7, 29, forbidden=0.03)
    for width in (16, 100):
        out, out_len, logp = _run(hip, logits, seq_len, width, scorer, 28)
        for b in (0, 17, 40, 63):
            one = _run(hip, logits[:, b:b + 1], seq_len[b:b + 1], width, scorer, 28)
            assert _same_bits(one, (out[b:b + 1], out_len[b:b + 1], logp[b:b + 1])), b
        for b in range(64):
            assert (out[b, out_len[b]:] == 0).all(), b


def test_two_scorers_on_one_workspace_give_each_its_own_result(hip):
    """The prefix tree of one launch is stale data for the next: everything a launch reads of
    it, it has written first.  Scorer A, then B with other states and other forbidden edges on
    the same bytes, then A again; also a workspace filled with 0xff first."""
    rng = np.random.default_rng(77)
    logits = _logits(rng, 30, 4, 29, 28)
    seq_len = np.array([30, 22, 30, 5], dtype=np.int32)
    a = _random_scorer(rng, 5, 29, forbidden=0.1)
    b = _random_scorer(rng, 300, 29, final=False, forbidden=0.1)
    need = hip.ctc_beam_lm_workspace_bytes(30, 4, 29, 32)
    workspace = torch.full((need,), 0xff, dtype=torch.uint8, device=DEV)
    lg, sl = _t(logits), _t(seq_len, torch.int32)
    results = []
    for scorer in (a, b, a):
        status, got = raw_beam(hip, lg, sl, 32, scorer, workspace)
        assert status == 0
        results.append(got)
        paths, logp = ref.beam_search_decode(logits, seq_len, 32, *_tables(scorer), blank=28)
        assert [got[0][r, :got[1][r]].tolist() for r in range(4)] == paths
        assert np.allclose(got[2], logp, rtol=1e-5, atol=1e-3)
        assert all((got[0][r, got[1][r]:] == 0).all() for r in range(4))
    assert _same_bits(results[0], results[2])
    assert not np.array_equal(results[0][2], results[1][2])
    # too small a workspace and bad scorer arguments are refused, nothing launched
    status, _ = raw_beam(hip, lg, sl, 32, a, workspace[:need - 1])
    assert status == -3
    lib = hip.load()
    nxt, score, _ = a.to(torch.device(DEV, torch.cuda.current_device()))
    for bad in ((None, score.data_ptr(), 5), (nxt.data_ptr(), None, 5),
                (nxt.data_ptr(), score.data_ptr(), 0), (nxt.data_ptr(), score.data_ptr(), -1)):
        assert lib.ctcasr_ctc_beam_decode_lm(
            lg.data_ptr(), sl.data_ptr(), 30, 4, 29, 28, 32, 0, bad[0], bad[1], None, bad[2],
            lg.data_ptr(), sl.data_ptr(), None, workspace.data_ptr(), need, None) == -1


def test_workspace_function_refuses_what_the_plain_one_refuses(hip):
    lib = hip.load()
    for args in ((0, 4, 29, 8), (30, 0, 29, 8), (30, 4, 0, 8), (30, 4, 29, 0), (-1, 4, 29, 8),
                 (30, 4, 29, -5)):
        assert lib.ctcasr_ctc_beam_workspace_bytes(*args) == 0
        assert lib.ctcasr_ctc_beam_lm_workspace_bytes(*args) == 0
    for args in ((30, 4, 29, 8), (500, 16, 29, 1024), (1, 1, 2, 1), (3200, 1, 64, 1024)):
        assert hip.ctc_beam_lm_workspace_bytes(*args) >= hip.ctc_beam_workspace_bytes(*args) > 0
    logits, seq_len = _t(np.zeros((6, 5, 29), dtype=np.float32)), _t(np.zeros(5), torch.int32)
    with pytest.raises(hip.CtcAsrError, match='4 lengths for a batch of 5'):
        hip.ctc_beam_decode_lm(logits, seq_len[:4], 8, _zero_scorer(29))
    with pytest.raises(hip.CtcAsrError, match='30 classes'):
        hip.ctc_beam_decode_lm(logits, seq_len, 8, _zero_scorer(30))
    for width in (0, 1025):
        with pytest.raises(hip.CtcAsrError):
            hip.ctc_beam_decode_lm(logits, seq_len, width, _zero_scorer(29))


@pytest.mark.timeout(160)
def test_pool_exhaustion_is_reported(hip):
    """The inputs of test_gpu_beam_edges.py's exhaustion case (the oracle counts 1.57 x 2^21
    prefixes there) under a scorer that scores nothing, so the search is that search:
    out_len = -1, the wrapper raises, and the next launch is sound."""
    classes, blank = 64, 63
    rng = np.random.default_rng(8)
    logits = _logits(rng, 3200, 1, classes, blank, scale=0.3, blank_bias=0.0)
    with pytest.raises(hip.CtcAsrError, match='pool exhausted'):
        _run(hip, logits, [3200], MAX_WIDTH, _zero_scorer(classes), blank)
    small = _logits(rng, 30, 3, 29, 28)
    _check(hip, small, [30, 12, 0], 32, _random_scorer(rng, 4, 29), 28, 'max')


# ------------------------------------------------------------------------------------------------
# 7. Through the model and the drivers
# ------------------------------------------------------------------------------------------------
def test_decode_many_with_a_scorer_equals_decode_fn_batch_by_batch():
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    cfg = ModelConfig(used_model='ds2', conv_filters=(4, 4), rnn_cell='lstm', cudnn=True,
                      num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0)
    model = CTCModel(cfg, 'cuda', params=init_params(cfg, 0))
    classes = cfg.num_classes
    rng = np.random.default_rng(91)
    scorer = _random_scorer(rng, 6, classes, forbidden=0.02)
    batches, host = [], []
    for steps, lengths in ((7, [7, 0, 3]), (40, [40]), (21, [0, 21, 1, 0]), (40, [33, 40, 0])):
        logits = _logits(rng, steps, len(lengths), classes, classes - 1, blank_bias=1.5)
        host.append((logits, np.array(lengths, dtype=np.int32)))
        batches.append((_t(logits), _t(np.array(lengths), torch.int32), None))
    assert model.decode_group_size(500, 16, scorer=scorer) == model.decode_group_size(500, 16)
    for width in (8, 32):
        joint = model.decode_many(batches, beam_width=width, scorer=scorer)
        plain = model.decode_many(batches, beam_width=width)
        for (logits, seq_len, _), (np_logits, np_len), got in zip(batches, host, joint):
            one = model.decode_fn(logits, seq_len, None, beam_width=width, scorer=scorer)
            assert got[0] == one[0] and list(got[1]) == list(one[1])
            assert got[0] == ref.beam_search_decode(np_logits, np_len, width,
                                                    *_tables(scorer))[0]
        assert [r[0] for r in joint] != [r[0] for r in plain]       # the scorer is in use


@pytest.fixture()
def trained(tmp_path):
    """The synthetic corpus and flags of test_gpu_pipeline.py, one epoch trained."""
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


def _printed_result(text):
    return re.search(r"\{'decoded'.*\}", text, flags=re.S).group(0)


def test_drivers_decode_with_the_model_of_lm_path(trained, capsys):
    from ctc_asr_amd import evaluate, input_functions, predict, storage
    from ctc_asr_amd.model import CTCModel, ModelConfig
    capsys.readouterr()
    lm_path = str(trained / 'chars.npz')
    assert lm.main(['--lm_corpus_csv', FLAGS.train_csv, '--lm_order', '3', '--lm_path',
                    lm_path]) == 0
    FLAGS.update(lm_path='')
    rows = input_functions.read_manifest(FLAGS.test_csv)
    wav = os.path.join(FLAGS.corpus_dir, rows[2]['path'])
    capsys.readouterr()
    # no --lm_path: what the driver printed before there was one
    assert predict.main(['--input', wav]) == 0
    unfused = _printed_result(capsys.readouterr().out)
    # weight 0, bonus 0: the n-gram has no forbidden label edge, so the text is the unfused text
    assert predict.main(['--input', wav, '--lm_path', lm_path, '--lm_weight', '0',
                         '--lm_bonus', '0']) == 0
    assert _printed_result(capsys.readouterr().out) == unfused
    # the model in use: predict() returns what decode_fn(scorer=...) returns, words aligned to it
    assert predict.main(['--input', wav, '--lm_path', lm_path, '--lm_weight', '2.0',
                         '--lm_bonus', '0.5', '--timestamps']) == 0
    out = capsys.readouterr().out
    assert "'words'" in out
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=1)
    storage.restore_checkpoint(storage.latest_checkpoint(FLAGS.train_dir), model)
    scorer = lm.from_flags(model.cfg.num_classes)
    assert scorer is not None and scorer.order == 3
    # ... and without --lm_path the driver printed the text of the plain kernel on its logits
    from ctc_asr_amd import hip
    from ctc_asr_amd.labels import decode
    feats, lengths = input_functions.features_from_pcm([input_functions.read_wav(wav)],
                                                       model.device)
    logits, seq_len = model.inference_fn(feats, lengths, training=False)
    plain_out, plain_len, _ = hip.ctc_beam_decode(logits, seq_len, FLAGS.beam_width)
    plain_ids = plain_out[0, :int(plain_len[0])].cpu().tolist()
    assert repr(decode(plain_ids)) in unfused
    assert predict.predict(model, wav)['decoded'].tolist() == plain_ids
    assert model.decode_fn(logits, seq_len, None)[0][0] == plain_ids
    assert model.decode_many([(logits, seq_len, None)])[0][0][0] == plain_ids
    got = predict.predict(model, wav, timestamps=True, scorer=scorer)
    assert repr(got['plaintext']) in out
    feats, lengths = input_functions.features_from_pcm([input_functions.read_wav(wav)],
                                                       model.device)
    logits, seq_len = model.inference_fn(feats, lengths, training=False)
    decoded, _, _ = model.decode_fn(logits, seq_len, None, scorer=scorer)
    assert decoded[0] == got['decoded'].tolist()
    path, logp = ref.beam_search_decode(logits.cpu().numpy(), seq_len.cpu().numpy(),
                                        FLAGS.beam_width, *_tables(scorer))
    assert decoded[0] == path[0]
    assert isinstance(got['words'], list)
    # evaluate: runs with the scorer; weight 0 reproduces the unfused figures
    plain = evaluate.evaluate_dataset(model, 'dev', report_samples=False)
    zero = evaluate.evaluate_dataset(model, 'dev', report_samples=False,
                                     scorer=lm.load(lm_path, 29).scaled(0.0, 0.0))
    assert zero == plain
    fused = evaluate.evaluate_dataset(model, 'dev', report_samples=False, scorer=scorer)
    assert fused['batches'] == plain['batches']
    assert fused['loss'] == pytest.approx(plain['loss'], rel=1e-6)
    assert np.isfinite(fused['word_error_rate']) and np.isfinite(fused['mean_edit_distance'])
    assert evaluate.main(['--dev', '--lm_path', lm_path]) == 0
    assert 'word_error_rate' in capsys.readouterr().out
    with pytest.raises(ValueError, match='29 classes'):
        lm.load(lm_path, 30)
