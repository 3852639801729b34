"""``ctcasr_edit_distance`` on the GPU against the tuple reference (tests/edit_reference.py): all
four outputs, exact equality.  Strip seams, alphabets with many ties, layouts, status codes, and
the path through `CTCModel.error_counts_fn` and `evaluate_dataset`."""

import json
import os

import numpy as np
import pytest
import torch

from ctc_asr_amd import metrics
from ctc_asr_amd.params import FLAGS
from tests import edit_reference as ref

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'reference_python.json')))
SEAMS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 500)
POISON = -77


def _t(values):
    return torch.tensor(np.asarray(values, dtype=np.int64).astype(np.int32), dtype=torch.int32,
                        device='cuda')


def _pack(rows):
    lengths = [len(r) for r in rows]
    flat = [v for r in rows for v in r] or [0]
    return flat, (np.cumsum(lengths) - lengths).tolist(), lengths


def _run(hip, hyps, refs, **kwargs):
    """int array [B, 5] of (distance, S, D, I, status) for packed rows."""
    hyp, hyp_off, hyp_len = _pack(hyps)
    ref_, ref_off, ref_len = _pack(refs)
    out = hip.edit_distance(_t(hyp), _t(hyp_off), _t(hyp_len), _t(ref_), _t(ref_off), _t(ref_len),
                            **kwargs)
    return torch.stack(out, dim=1).cpu().numpy()


def _expected(hyps, refs):
    return np.array([ref.error_counts(h, r) + (0,) for h, r in zip(hyps, refs)], dtype=np.int64)


def _check(hip, hyps, refs, **kwargs):
    got = _run(hip, hyps, refs, **kwargs)
    want = _expected(hyps, refs)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(int(b), len(hyps[b]), len(refs[b]), got[b].tolist(),
                            want[b].tolist()) for b in bad[:5]]


def _symbols(rng, alphabet, size):
    if alphabet == 'wide':       # ids of 2^31 scale, both signs
        pool = rng.integers(-2 ** 31, 2 ** 31, size=24)
        return pool[rng.integers(0, len(pool), size=size)].tolist()
    return rng.integers(0, alphabet, size=size).tolist()


def test_golden_levenshtein_cases(hip):
    hyps = [[ord(c) for c in case['a']] for case in GOLD['levenshtein']]
    refs = [[ord(c) for c in case['b']] for case in GOLD['levenshtein']]
    got = _run(hip, hyps, refs)
    assert got[:, 0].tolist() == [case['distance'] for case in GOLD['levenshtein']]
    _check(hip, hyps, refs)


@pytest.mark.parametrize('alphabet', [2, 28, 'wide'])
def test_strip_seams(hip, alphabet):
    rng = np.random.default_rng(17)
    hyps, refs = [], []
    for hyp_len in SEAMS:
        for ref_len in SEAMS:
            hyps.append(_symbols(rng, alphabet, hyp_len))
            refs.append(_symbols(rng, alphabet, ref_len))
    _check(hip, hyps, refs)


def test_special_pairs(hip):
    rng = np.random.default_rng(23)
    same = _symbols(rng, 28, 200)
    long_a, long_b = _symbols(rng, 28, 3000), _symbols(rng, 2, 3000)
    hyps = [same, list(range(100)), [], [4, 5, 6], [], long_a, _symbols(rng, 28, 10),
            long_b, [1] * 10, same[:-1], same[1:]]
    refs = [same, list(range(100, 230)), [7, 8], [], [], _symbols(rng, 28, 10), long_a,
            [1] * 10, long_b, same, same]
    got = _run(hip, hyps, refs)
    assert got[0].tolist() == [0, 0, 0, 0, 0]                   # identical
    assert got[1].tolist() == [130, 100, 30, 0, 0]              # disjoint
    assert got[2].tolist() == [2, 0, 2, 0, 0] and got[3].tolist() == [3, 0, 0, 3, 0]
    assert got[4].tolist() == [0, 0, 0, 0, 0]                   # both empty
    _check(hip, hyps, refs)


def test_carry_columns_in_the_workspace(hip):
    """A reference side too long for four carry columns in LDS: the strips hand their column on
    through the workspace.  Short pairs share the launch."""
    rng = np.random.default_rng(29)
    hyps = [_symbols(rng, 3, 150), _symbols(rng, 28, 70), [], _symbols(rng, 28, 5000)]
    refs = [_symbols(rng, 3, 5000), _symbols(rng, 28, 64), _symbols(rng, 28, 5), [2]]
    assert hip.edit_distance_workspace_bytes(4, 5000, 5000) >= 4 * 5000 * 4
    _check(hip, hyps, refs)


def test_dense_and_packed_layouts_agree(hip):
    """The decoders' [B, T] rows with garbage beyond the length, against the packed rows."""
    rng = np.random.default_rng(31)
    batch, width = 37, 140
    lengths = rng.integers(0, width + 1, size=batch)
    lengths[:3] = (0, width, 64)
    dense = rng.integers(0, 28, size=(batch, width)).astype(np.int32)     # garbage included
    hyps = [dense[b, :lengths[b]].tolist() for b in range(batch)]
    refs = [_symbols(rng, 28, int(n)) for n in rng.integers(0, 150, size=batch)]
    ref_, ref_off, ref_len = _pack(refs)
    out = hip.edit_distance(_t(dense), _t(np.arange(batch) * width), _t(lengths), _t(ref_),
                            _t(ref_off), _t(ref_len))
    got = torch.stack(out, dim=1).cpu().numpy()
    assert (got == _run(hip, hyps, refs)).all()
    assert (got == _expected(hyps, refs)).all()


def test_overlapping_and_aliased_rows(hip):
    rng = np.random.default_rng(37)
    pool = _t(_symbols(rng, 4, 400))
    host = pool.cpu().tolist()
    hyp_off, hyp_len = [0, 10, 10, 200, 399, 0], [100, 150, 150, 200, 1, 400]
    ref_off, ref_len = [50, 10, 11, 0, 0, 0], [100, 150, 150, 300, 0, 400]
    out = hip.edit_distance(pool, _t(hyp_off), _t(hyp_len), pool, _t(ref_off), _t(ref_len))
    got = torch.stack(out, dim=1).cpu().numpy()
    hyps = [host[o:o + n] for o, n in zip(hyp_off, hyp_len)]
    refs = [host[o:o + n] for o, n in zip(ref_off, ref_len)]
    assert (got == _expected(hyps, refs)).all()
    assert got[1].tolist() == [0, 0, 0, 0, 0] and got[5].tolist() == [0, 0, 0, 0, 0]


def test_one_launch_of_600_mixed_pairs_and_a_single_pair(hip):
    rng = np.random.default_rng(41)
    hyp_lens = rng.choice([0, 1, 5, 30, 64, 65, 100, 160, 200, 260], size=600)
    ref_lens = rng.choice([0, 2, 7, 31, 63, 64, 110, 150, 190, 257], size=600)
    hyps = [_symbols(rng, (2, 28)[b % 2], int(n)) for b, n in enumerate(hyp_lens)]
    refs = [_symbols(rng, (2, 28)[b % 2], int(n)) for b, n in enumerate(ref_lens)]
    _check(hip, hyps, refs)
    for b in (7, 8):
        _check(hip, hyps[b:b + 1], refs[b:b + 1])           # B = 1
    # bit-reproducible
    assert (_run(hip, hyps, refs) == _run(hip, hyps, refs)).all()


def test_status_2_leaves_the_neighbours_alone(hip):
    rng = np.random.default_rng(43)
    rows = [_symbols(rng, 5, 90) for _ in range(7)]
    flat, offsets, lengths = _pack(rows)
    hyp_len = list(lengths)
    ref_len = list(lengths)
    hyp_len[1] = -1                  # the beam search's out_len of an exhausted pool
    ref_len[3] = -5
    hyp_len[5] = 70                  # above max_hyp_len = 64 (the row itself holds 90)
    hyp_len[0] = hyp_len[2] = hyp_len[4] = hyp_len[6] = 64
    ref_len[6] = 80                  # above max_ref_len = 75
    ref_len[0] = ref_len[1] = ref_len[2] = ref_len[4] = ref_len[5] = 75
    out = torch.full((5, 7), POISON, dtype=torch.int32, device='cuda')
    hip.edit_distance(_t(flat), _t(offsets), _t(hyp_len), _t(flat[::-1]), _t(offsets),
                      _t(ref_len), max_hyp_len=64, max_ref_len=75, out=out)
    got = out.t().cpu().numpy()
    assert not (got == POISON).any()
    reversed_flat = flat[::-1]
    for b in range(7):
        if b in (1, 3, 5, 6):
            assert got[b].tolist() == [-1, -1, -1, -1, 2], b
        else:
            hyp = flat[offsets[b]:offsets[b] + hyp_len[b]]
            ref_ = reversed_flat[offsets[b]:offsets[b] + ref_len[b]]
            assert got[b].tolist() == list(ref.error_counts(hyp, ref_)) + [0], b
    # the wrapper keeps every row inside its buffer before it launches
    packed = _t([1, 2, 3])
    with pytest.raises(hip.CtcAsrError, match='outside'):
        hip.edit_distance(packed, _t([0, 1, 2]), _t([1, 1, 2]), packed, _t([0, 1, 2]),
                          _t([1, 1, 1]))
    with pytest.raises(hip.CtcAsrError, match='outside'):
        hip.edit_distance(packed, _t([0, 1, 2]), _t([1, 1, 1]), packed, _t([-1, 1, 2]),
                          _t([1, 1, 1]))


def test_null_count_outputs_are_accepted(hip):
    rng = np.random.default_rng(47)
    hyps = [_symbols(rng, 3, n) for n in (70, 0, 5, 64)]
    refs = [_symbols(rng, 3, n) for n in (65, 3, 0, 200)]
    hyp, hyp_off, hyp_len = (_t(v) for v in _pack(hyps))
    ref_, ref_off, ref_len = (_t(v) for v in _pack(refs))
    hyp_len[2] = -1
    distance = torch.full((4,), POISON, dtype=torch.int32, device='cuda')
    status = torch.full((4,), POISON, dtype=torch.int32, device='cuda')
    code = hip.load().ctcasr_edit_distance(
        hyp.data_ptr(), hyp_off.data_ptr(), hyp_len.data_ptr(), ref_.data_ptr(),
        ref_off.data_ptr(), ref_len.data_ptr(), 4, 70, 200, distance.data_ptr(), None, None, None,
        status.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
    assert code == 0
    torch.cuda.synchronize()
    want = [ref.error_counts(h, r)[0] for h, r in zip(hyps, refs)]
    want[2] = -1
    assert distance.cpu().tolist() == want and status.cpu().tolist() == [0, 0, 2, 0]


def test_error_counts_packs_uploads_and_refuses_a_row_too_long(hip):
    rng = np.random.default_rng(53)
    hyps = [_symbols(rng, 28, int(n)) for n in rng.integers(0, 180, size=40)]
    refs = [_symbols(rng, 28, int(n)) for n in rng.integers(0, 180, size=40)]
    got = metrics.error_counts(hyps, refs, 'cuda')
    assert got.dtype == np.int32 and got.shape == (40, 4)
    assert (got == _expected(hyps, refs)[:, :4]).all()
    assert (metrics.error_counts([[], []], [[], []], 'cuda') == 0).all()
    assert metrics.error_counts([], [], 'cuda').shape == (0, 4)
    with pytest.raises(hip.CtcAsrError, match=r'\(-2\)'):
        metrics.error_counts([[1] * 32768], [[1]], 'cuda')


def _bits(array):
    return np.asarray(array, dtype=np.float32).view(np.uint32).tolist()


def test_error_counts_fn_equals_error_rates_fn(hip):
    from ctc_asr_amd.labels import decode, encode
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    cfg = ModelConfig(used_model='ds2', conv_filters=(4, 4), rnn_cell='lstm', cudnn=True,
                      num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0)
    model = CTCModel(cfg, 'cuda', params=init_params(cfg, 0))
    originals = ['the cat sat on the mat', 'a dog', 'speech is far away', 'ran', 'on and on']
    results = ['the cat sat on a mat', '', 'speech far a way', 'ran', 'no an no on']
    truths = [encode(text) for text in originals]
    decoded = [encode(text) for text in results]
    assert decoded[1] == [] and decode(decoded[0]) == results[0]
    labels = np.zeros((len(truths), max(len(t) for t in truths)), dtype=np.int32)
    for b, row in enumerate(truths):
        labels[b, :len(row)] = row
    want = CTCModel.error_rates_fn(labels, originals, decoded, results)
    for given in (labels, torch.tensor(labels, device='cuda')):
        got = model.error_counts_fn(given, originals, decoded, results)
        assert len(got) == 7
        for a, b in zip(got[:4], want):
            assert a.dtype == b.dtype and a.shape == b.shape and _bits(a) == _bits(b)
    _, _, _, _, label_counts, word_counts, reference = got
    assert reference.tolist() == [[len(t), len(o.split())] for t, o in zip(truths, originals)]
    assert label_counts.tolist() == [list(ref.error_counts(d, t)) for d, t in zip(decoded, truths)]
    assert word_counts.tolist() == [list(ref.error_counts(r.split(), o.split()))
                                    for o, r in zip(originals, results)]
    assert word_counts[1].tolist() == [2, 0, 2, 0]              # the empty decode: all deleted
    with pytest.raises(ZeroDivisionError):
        model.error_counts_fn(labels[:1], [''], decoded[:1], results[:1])


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


def test_evaluate_dataset_with_and_without_gpu_metrics(trained, monkeypatch, hip):
    from ctc_asr_amd import evaluate, storage
    from ctc_asr_amd.input_functions import input_fn_generator
    from ctc_asr_amd.model import CTCModel, ModelConfig

    def fresh(switch):
        monkeypatch.setenv('CTCASR_GPU_METRICS', switch)
        model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=1)
        storage.restore_checkpoint(storage.latest_checkpoint(FLAGS.train_dir), model)
        return model

    model = fresh('1')
    assert model.gpu_metrics
    on = evaluate.evaluate_dataset(model, 'dev', report_samples=False)
    host_model = fresh('0')
    assert not host_model.gpu_metrics
    off = evaluate.evaluate_dataset(host_model, 'dev', report_samples=False)
    assert sorted(off) == ['batches', 'loss', 'mean_edit_distance', 'word_error_rate']
    for key in off:
        assert on[key] == off[key], key
    monkeypatch.delenv('CTCASR_GPU_METRICS')
    assert CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=1).gpu_metrics   # default on

    # the new keys against a host recomputation over the same decodes
    totals = {'label': np.zeros(4, dtype=np.int64), 'word': np.zeros(4, dtype=np.int64)}
    for features, labels in input_fn_generator('dev', device=model.device)():
        logits, seq_len = model.inference_fn(features['spectrogram'],
                                             features['spectrogram_length'], training=False)
        decoded, plaintext, _ = model.decode_fn(logits, seq_len, None)
        rows = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels
        for row, text, dec, dec_text in zip(rows, features['label_plaintext'], decoded,
                                            plaintext):
            truth = [int(v) for v in row if int(v) != 0]
            for name, counts, length in (
                    ('label', ref.error_counts(dec, truth), len(truth)),
                    ('word', ref.error_counts(dec_text.split(), text.split()),
                     len(text.split()))):
                totals[name] += np.array(list(counts[1:]) + [length])
    for name in ('label', 'word'):
        errors = on[name + '_errors']
        assert sorted(errors) == ['deletions', 'insertions', 'reference', 'substitutions']
        assert all(isinstance(v, int) for v in errors.values())
        assert [errors['substitutions'], errors['deletions'], errors['insertions'],
                errors['reference']] == totals[name].tolist()
        assert errors['reference'] > 0
        assert on['corpus_{}_error_rate'.format(name)] == \
            (errors['substitutions'] + errors['deletions'] + errors['insertions']) / \
            errors['reference']
