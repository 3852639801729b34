"""N-best decoding and rescoring through the model and the drivers (`CTCModel.nbest_fn` /
`nbest_many`, `predict --nbest`, `evaluate --nbest`, `--rescore_lm_path`), on a tiny model as in
test_gpu_beam_lm.py's driver test."""

import os
import re

import numpy as np
import pytest
import torch

from ctc_asr_amd import lm
from ctc_asr_amd.params import FLAGS

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _logits(rng, num_steps, batch, classes, blank_bias=1.5):
    logits = rng.normal(size=(num_steps, batch, classes)) * 2.0
    logits[:, :, classes - 1] += blank_bias
    return logits.astype(np.float32)


def _random_scorer(rng, states, classes, forbidden=0.0):
    score = rng.normal(size=(states, classes)).astype(np.float32)
    if forbidden:
        score[rng.random(size=score.shape) < forbidden] = -np.inf
    return lm.LmScorer(rng.integers(0, states, size=(states, classes)), score,
                       rng.normal(size=states).astype(np.float32))


def forbid_texts(label_rows, classes):
    """The automaton that scores every label sequence 0 except the given ones, whose end is
    forbidden: a trie over them, and one free state for everything that leaves it."""
    nodes = [{}]
    ends = set()
    for row in label_rows:
        s = 0
        for c in row:
            if c not in nodes[s]:
                nodes[s][c] = len(nodes)
                nodes.append({})
            s = nodes[s][c]
        ends.add(s)
    free = len(nodes)
    nxt = np.full((free + 1, classes), free, dtype=np.int32)
    for s, edges in enumerate(nodes):
        for c, target in edges.items():
            nxt[s, c] = target
    final = np.zeros(free + 1, dtype=np.float32)
    final[sorted(ends)] = -np.inf
    return lm.LmScorer(nxt, np.zeros((free + 1, classes), dtype=np.float32), final)


# ------------------------------------------------------------------------------------------------
def test_nbest_many_equals_nbest_fn_batch_by_batch(hip):
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    cfg = ModelConfig(used_model='ds2', conv_filters=(4, 4), rnn_cell='lstm', cudnn=True,
                      num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0)
    model = CTCModel(cfg, 'cuda', params=init_params(cfg, 0))
    classes = cfg.num_classes
    rng = np.random.default_rng(92)
    scorer = _random_scorer(rng, 6, classes, forbidden=0.02)
    rescorer = _random_scorer(rng, 4, classes)
    batches = []
    for steps, lengths in ((7, [7, 0, 3]), (40, [40]), (21, [0, 21, 1, 0]), (40, [33, 40, 0])):
        batches.append((_t(_logits(rng, steps, len(lengths), classes)),
                        _t(np.array(lengths), torch.int32),
                        np.array(['text {}'.format(i).encode() for i in range(len(lengths))],
                                 dtype=object)))
    for width, top_paths, first, second in ((8, 4, None, None), (32, 5, scorer, None),
                                            (32, 8, scorer, rescorer), (8, 8, None, rescorer)):
        joint = model.nbest_many(batches, top_paths, beam_width=width, scorer=first,
                                 rescorer=second)
        top1 = model.decode_many(batches, beam_width=width, scorer=first)
        for (logits, seq_len, originals), got, plain in zip(batches, joint, top1):
            one = model.nbest_fn(logits, seq_len, top_paths, originals, beam_width=width,
                                 scorer=first, rescorer=second)
            assert got == one
            assert [r['hypotheses'][0]['labels'] for r in got] == plain[0]
            assert list(model.nbest_top(got, originals)[1]) == list(plain[1])
            out, out_len, logp, n_paths = hip.ctc_beam_decode_nbest(logits, seq_len, width,
                                                                    top_paths, scorer=first)
            for b, result in enumerate(got):
                hyps = result['hypotheses']
                assert len(hyps) == int(n_paths[b]) and result['original'] == 'text {}'.format(b)
                assert [h['beam_logp'] for h in hyps] == logp[b, :len(hyps)].cpu().tolist()
                model_of = second if second is not None else first
                for h in hyps:
                    want = 0.0 if model_of is None else \
                        float(model_of.sequence_scores([h['labels']])[0])
                    assert h['lm_logp'] == want and h['total'] == h['ctc_logp'] + h['lm_logp']
                    assert h['status'] == 0
                totals = [h['total'] for h in hyps]
                if np.isfinite(totals).any():
                    assert result['selected'] == int(np.argmax(totals))
                    assert sum(h['posterior'] for h in hyps) == pytest.approx(1.0, abs=1e-12)


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """The synthetic corpus and flags of test_gpu_pipeline.py, one epoch trained."""
    from ctc_asr_amd import synth, train
    tmp_path = tmp_path_factory.mktemp('nbest')
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


def _printed(text, key):
    """The dict a driver printed: the last ``{...}`` of ``text`` that holds ``key``."""
    found = [m for m in re.findall(r'\{.*\}', text, flags=re.S) if key in m]
    return found[-1]


def _eval_result(text):
    body = _printed(text.split('Evaluation result: ')[-1], 'loss')
    return eval(body, {'nan': float('nan'), 'inf': float('inf')})      # (floats and dicts only)


def _wavs():
    from ctc_asr_amd import input_functions
    rows = input_functions.read_manifest(FLAGS.test_csv)
    return [os.path.join(FLAGS.corpus_dir, row['path']) for row in rows]


def _model():
    from ctc_asr_amd import storage
    from ctc_asr_amd.model import CTCModel, ModelConfig
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=1)
    storage.restore_checkpoint(storage.latest_checkpoint(FLAGS.train_dir), model)
    return model


def test_predict_nbest_keeps_the_text_and_adds_alternatives(trained, capsys, hip):
    from ctc_asr_amd import input_functions, predict
    wav = _wavs()[2]
    capsys.readouterr()
    assert predict.main(['--input', wav]) == 0
    plain = capsys.readouterr().out
    assert "'nbest'" not in plain and "'confidence'" not in plain
    assert predict.main(['--input', wav, '--nbest', '4']) == 0
    listed = capsys.readouterr().out
    FLAGS.update(nbest=0)
    head = re.search(r"\{'decoded'.*?'plaintext': '[^']*'", plain, flags=re.S).group(0)
    assert head in listed                    # 'decoded' and 'plaintext' printed as before
    model = _model()
    got = predict.predict(model, wav, nbest=4)
    base = predict.predict(model, wav)
    assert sorted(base) == ['decoded', 'plaintext']                  # --nbest 0: as it was
    assert got['decoded'].tolist() == base['decoded'].tolist()
    assert got['plaintext'] == base['plaintext']
    alternatives = got['nbest']
    assert len(alternatives) == 4 and repr(alternatives[1]['plaintext']) in listed
    assert sorted(alternatives[0]) == ['ctc_logp', 'lm_logp', 'logp', 'plaintext', 'posterior']
    assert sum(a['posterior'] for a in alternatives) == pytest.approx(1.0, abs=1e-9)
    assert alternatives[0]['plaintext'] == base['plaintext']
    assert got['confidence'] == alternatives[0]['posterior']
    assert all(a['lm_logp'] == 0.0 for a in alternatives)
    assert len({a['plaintext'] for a in alternatives}) == 4
    # --nbest 0 launches what the driver launched before: the plain kernel's answer
    feats, lengths = input_functions.features_from_pcm([input_functions.read_wav(wav)],
                                                       model.device)
    logits, seq_len = model.inference_fn(feats, lengths, training=False)
    out, out_len, logp = hip.ctc_beam_decode(logits, seq_len, FLAGS.beam_width)
    assert base['decoded'].tolist() == out[0, :int(out_len[0])].cpu().tolist()
    assert alternatives[0]['logp'] == float(logp[0])


def test_predict_with_a_rescorer_that_forbids_rank_0_prints_another(trained, capsys):
    from ctc_asr_amd import predict
    wav = _wavs()[2]
    model = _model()
    base = predict.predict(model, wav, nbest=4)
    path = str(trained / 'forbid_one.npz')
    forbid_texts([base['decoded'].tolist()], model.cfg.num_classes).save(path)
    capsys.readouterr()
    assert predict.main(['--input', wav, '--nbest', '4', '--rescore_lm_path', path,
                         '--timestamps']) == 0
    out = capsys.readouterr().out
    rescorer = lm.rescorer_from_flags(model.cfg.num_classes)
    FLAGS.update(nbest=0, rescore_lm_path='', timestamps=False)
    got = predict.predict(model, wav, timestamps=True, nbest=4, rescorer=rescorer)
    assert got['decoded'].tolist() != base['decoded'].tolist()
    assert repr(got['plaintext']) in out and "'words'" in out
    texts = [a['plaintext'] for a in got['nbest']]
    assert texts == [a['plaintext'] for a in base['nbest']]        # first-pass order kept
    assert got['plaintext'] in texts[1:]
    assert got['nbest'][0]['lm_logp'] == -np.inf and got['nbest'][0]['posterior'] == 0.0
    best = max(range(1, 4), key=lambda k: (got['nbest'][k]['ctc_logp'], -k))
    assert got['plaintext'] == texts[best]
    assert got['confidence'] == got['nbest'][best]['posterior'] > 0.0
    assert isinstance(got['words'], list)


def test_evaluate_nbest_keeps_every_key_and_adds_the_oracle(trained, capsys):
    from ctc_asr_amd import evaluate, predict
    model = _model()
    plain = evaluate.evaluate_dataset(model, 'test', report_samples=False)
    listed = evaluate.evaluate_dataset(model, 'test', report_samples=False, nbest=4)
    for key, value in plain.items():
        assert listed[key] == value or (value != value and listed[key] != listed[key]), key
    assert sorted(set(listed) - set(plain)) == ['nbest_mean_paths', 'oracle_label_error_rate',
                                                'oracle_word_error_rate']
    assert listed['oracle_label_error_rate'] <= listed['corpus_label_error_rate']
    assert listed['oracle_word_error_rate'] <= listed['corpus_word_error_rate']
    assert 1.0 <= listed['nbest_mean_paths'] <= 4.0
    # the driver, with and without the flag
    capsys.readouterr()
    assert evaluate.main([]) == 0
    without = _eval_result(capsys.readouterr().out)
    assert evaluate.main(['--nbest', '4']) == 0
    with_lists = _eval_result(capsys.readouterr().out)
    FLAGS.update(nbest=0)
    assert sorted(without) == sorted(plain)                          # --nbest 0: as it was
    assert {k: with_lists[k] for k in without} == without or \
        repr({k: with_lists[k] for k in without}) == repr(without)
    assert with_lists['oracle_label_error_rate'] == listed['oracle_label_error_rate']
    # a rescorer that forbids the rank-0 text of every utterance: other hypotheses are selected
    firsts = [predict.predict(model, wav)['decoded'].tolist() for wav in _wavs()]
    path = str(trained / 'forbid_all.npz')
    forbid_texts(firsts, model.cfg.num_classes).save(path)
    assert evaluate.main(['--nbest', '4', '--rescore_lm_path', path]) == 0
    rescored = _eval_result(capsys.readouterr().out)
    FLAGS.update(nbest=0, rescore_lm_path='')
    assert {k: rescored[k] for k in with_lists} == with_lists or \
        repr({k: rescored[k] for k in with_lists}) == repr(with_lists)
    for name in ('label', 'word'):
        assert rescored['rescored_{}_error_rate'.format(name)] >= \
            rescored['oracle_{}_error_rate'.format(name)]
    assert (rescored['rescored_label_error_rate'], rescored['rescored_word_error_rate']) != \
        (rescored['corpus_label_error_rate'], rescored['corpus_word_error_rate'])
    assert 'rescored_label_error_rate' not in with_lists
