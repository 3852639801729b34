"""Which C entry point of csrc/beam.hip a Python decoding call reaches.

`hip.ctc_beam_search` is the one launch path; `hip.ctc_beam_decode`, `_lm`, `_nbest` and `_wordlm`
are shims over it and `CTCModel` calls it directly.  For no scorer, a dense scorer, and a word
scorer with and without a look-ahead table, a recording proxy around the loaded library names the
symbol every call launched; each older wrapper returns the bits of `ctc_beam_search` with the
matching arguments; and `decode_group_size` sizes its groups as the older sizers did."""

import numpy as np
import pytest
import torch

from ctc_asr_amd import lm
from tests.beam_helpers import _logits, _random_scorer, _t

pytestmark = pytest.mark.gpu
STEPS, BATCH, CLASSES, BLANK, WIDTH, TOP_PATHS = 4, 2, 5, 4, 2, 2
SPACE = 1
CORPUS = [[2, 1, 2, 3], [3, 1, 2], [2, 3, 1, 3]]        # the words 'a', 'ab' and 'b'
PREFIX = 'ctcasr_ctc_beam_decode'
KINDS = {'none': '', 'dense': '_lm', 'word': '_wordlm', 'look-ahead': '_wordlm_lookahead'}


class Recorder:
    """The loaded library, noting the beam-search entry points that are called."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith(PREFIX):
            return fn

        def noted(*args):
            self.calls.append(name[len(PREFIX):])
            return fn(*args)
        return noted


@pytest.fixture
def calls(hip, monkeypatch):
    recorder = Recorder(hip.load())
    monkeypatch.setattr(hip, '_lib', recorder)
    return recorder.calls


@pytest.fixture(scope='module')
def model():
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    cfg = ModelConfig(used_model='ds2', conv_filters=(4, 4), rnn_cell='lstm', cudnn=True,
                      num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0, num_classes_=CLASSES)
    return CTCModel(cfg, 'cuda', params=init_params(cfg, 0))


def _scorer(kind, rng):
    if kind == 'none':
        return None
    if kind == 'dense':
        return _random_scorer(rng, 2, CLASSES)
    words = lm.build_word_ngram(CORPUS, 2, CLASSES, SPACE, blank=BLANK)
    return words.scaled(1.0, 0.0, -4.0, lookahead=kind == 'look-ahead')


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32),
                                                                       y.view(torch.int32))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize('kind', list(KINDS))
def test_every_call_reaches_the_entry_point_of_its_model(hip, model, calls, kind):
    rng = np.random.default_rng(11)
    logits = _t(_logits(rng, STEPS, BATCH, CLASSES, BLANK))
    seq_len = _t(np.array([STEPS, 0]), torch.int32)
    scorer = _scorer(kind, rng)
    word = kind in ('word', 'look-ahead')
    top1_symbol = KINDS[kind]
    nbest_symbol = KINDS[kind] if word else '_nbest'

    def launched(symbol, count=1):
        assert calls == [symbol] * count, (kind, calls)
        del calls[:]

    # the one function, both forms
    top1 = hip.ctc_beam_search(logits, seq_len, WIDTH, scorer)
    launched(top1_symbol)
    nbest = hip.ctc_beam_search(logits, seq_len, WIDTH, scorer, TOP_PATHS)
    launched(nbest_symbol)
    assert [tuple(t.shape) for t in top1] == [(BATCH, STEPS), (BATCH,), (BATCH,)]
    assert [tuple(t.shape) for t in nbest] == [(BATCH, TOP_PATHS, STEPS), (BATCH, TOP_PATHS),
                                               (BATCH, TOP_PATHS), (BATCH,)]
    assert _same(top1, [t[:, 0] for t in nbest[:3]])
    # the older wrappers: the same symbol, the same bits
    if kind == 'none':
        assert _same(hip.ctc_beam_decode(logits, seq_len, WIDTH), top1)
        launched('')
    if kind == 'dense':
        assert _same(hip.ctc_beam_decode_lm(logits, seq_len, WIDTH, scorer), top1)
        launched('_lm')
    if word:
        assert _same(hip.ctc_beam_decode_wordlm(logits, seq_len, WIDTH, scorer, TOP_PATHS), nbest)
        one = hip.ctc_beam_decode_wordlm(logits, seq_len, WIDTH, scorer)
        assert _same([t[:, 0] for t in one[:3]], top1) and one[0].shape == (BATCH, 1, STEPS)
        launched(nbest_symbol, 2)
    else:
        assert _same(hip.ctc_beam_decode_nbest(logits, seq_len, WIDTH, TOP_PATHS, scorer=scorer),
                     nbest)
        launched('_nbest')
    # the model
    batches = [(logits, seq_len, None), (logits[:3, :1].contiguous(), seq_len[:1] - 1, None)]
    decoded = model.decode_fn(logits, seq_len, None, beam_width=WIDTH, scorer=scorer)
    launched(top1_symbol)
    many = model.decode_many(batches, beam_width=WIDTH, scorer=scorer)
    launched(top1_symbol)
    assert many[0][0] == decoded[0] == [top1[0][b, :top1[1][b]].tolist() for b in range(BATCH)]
    listed = model.nbest_fn(logits, seq_len, TOP_PATHS, beam_width=WIDTH, scorer=scorer)
    launched(nbest_symbol)
    assert model.nbest_many(batches, TOP_PATHS, beam_width=WIDTH, scorer=scorer)[0] == listed
    launched(nbest_symbol)
    if kind == 'none':
        model.mwer_loss_fn(logits, seq_len, [[2, 3], [3]], nbest=TOP_PATHS, beam_width=WIDTH,
                           check=False)
        launched('_nbest')
    # the sizer: a budget of 100 plain utterances holds fewer with the word model's larger pool
    older = {'none': hip.ctc_beam_workspace_bytes, 'dense': hip.ctc_beam_lm_workspace_bytes,
             'word': hip.ctc_beam_wordlm_workspace_bytes,
             'look-ahead': hip.ctc_beam_wordlm_workspace_bytes}[kind]
    per_utt = older(STEPS, 1, CLASSES, WIDTH)
    assert hip.ctc_beam_search_workspace_bytes(STEPS, 1, CLASSES, WIDTH, scorer) == per_utt > 0
    assert hip.ctc_beam_nbest_workspace_bytes(STEPS, 1, CLASSES, WIDTH) == \
        hip.ctc_beam_workspace_bytes(STEPS, 1, CLASSES, WIDTH)
    budget = 100 * hip.ctc_beam_workspace_bytes(STEPS, 1, CLASSES, WIDTH)
    group = model.decode_group_size(STEPS, BATCH, beam_width=WIDTH, budget_bytes=budget,
                                    scorer=scorer)
    assert group == max(BATCH, min(256, budget // per_utt)) // BATCH
    assert (group < 100 // BATCH) == word
