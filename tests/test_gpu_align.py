"""CTC forced alignment (csrc/ctc_align.hip, `hip.ctc_align`, `CTCModel.align_fn`) on the MI355X.

Every row the kernel returns is checked (`_check`): a valid path (monotone, legal moves, starts in
{0, 1}, ends in {S - 1, S - 2}, collapses to the label) and -1 past seq_len; the score equal to the
float64 rescoring of the kernel's own path (rel. 1e-5) and that rescoring within 1e-4 * len of the
float64 reference's best score (tests/align_reference.py); the path identical to the reference's
wherever the reference's best path beats every other alignment by more than 1e-3; frame_logp the
log-softmax of the emitted class; and the status, score and outputs of rows without a path.

Edge shapes mirror test_gpu_ctc_edges.py: utterances of 0-1 frames and L = 0, the tight bound
len = L + repeats and one frame below it, L at the lattice ceiling (575) and a row past
max_label_len, bad ids and lengths, non-finite logits, a blank other than C - 1, C = 2 ... 64,
B on both sides of 32 / 64 / 128 with empty rows, T on both sides of every LDS-tier boundary
(table and back-pointer slab), frame_logp = NULL, garbage in every output and the workspace, and
changing data on one workspace.  Then through the model: a memorised batch, predict --timestamps,
and the corpus aligner."""

import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import ctc as octc
from tests import align_reference as ref
from tests.helpers import pack_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ctcasr_ctc_align's launcher: s_pad = 2 * max_label_len + 1 lattice states, at most 384 * 3 of
# them; LDS = fixed + (slab) + (table), fixed = two fp64 lattice rows, int ext[s_pad] (16-byte
# aligned), 16 int words, 64 int path stage, 64 x 3 x 16 B back-pointer stage.  Slab and table
# in LDS while everything fits 150 KB; then the table alone; then neither.
MAX_LABEL_LEN = (384 * 3 - 1) // 2          # 575
LDS_MAX = 150 * 1024


def _fixed(max_label_len):
    s_pad = 2 * max_label_len + 1
    return 2 * s_pad * 8 + (s_pad * 4 + 15) // 16 * 16 + 64 + 256 + 64 * 3 * 16


def _words(max_label_len):
    return (2 * max_label_len + 1 + 63) // 64


def _tier_bounds(classes, max_label_len):
    """The largest T with slab + table in LDS, and with the table alone in LDS."""
    room = LDS_MAX - _fixed(max_label_len)
    return room // (classes * 4 + _words(max_label_len) * 16), room // (classes * 4)


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _run(hip, logits, labels, seq_len, max_label_len, blank=None, offsets=None, **kw):
    """The wrapper on host arrays (``offsets`` given: ``labels`` is already flat).  Returns host
    (path, score, frame_logp or None, status)."""
    if offsets is None:
        flat, offsets = pack_labels(labels)
    else:
        flat = np.asarray(labels, dtype=np.int32)
    path, score, frame_logp, status = hip.ctc_align(
        _t(logits), _t(flat, torch.int32), _t(offsets, torch.int32),
        _t(np.asarray(seq_len), torch.int32), max_label_len, blank=blank, **kw)
    return (path.cpu().numpy(), score.cpu().numpy(),
            None if frame_logp is None else frame_logp.cpu().numpy(), status.cpu().numpy())


def _expected_status(logits, labels, seq_len, max_label_len, blank):
    num_steps, _, classes = logits.shape
    out = []
    for b, label in enumerate(labels):
        length = int(seq_len[b])
        if len(label) > max_label_len or length > num_steps or length < 0 or \
                any(v < 0 or v >= classes or v == blank for v in label):
            out.append(2)
        elif length < octc.required_time(label):
            out.append(1)
        elif not np.isfinite(logits[:length, b]).all():
            out.append(3)
        else:
            out.append(0)
    return out


def _log_num_alignments(label, blank, length):
    ext = octc.extended_labels(label, blank)
    size = len(ext)
    skip = np.zeros(size, dtype=bool)
    for s in range(2, size):
        skip[s] = ext[s] != blank and ext[s] != ext[s - 2]
    a = np.full(size, -np.inf)
    a[0] = 0.0
    if size > 1:
        a[1] = 0.0
    for _ in range(1, length):
        n = a.copy()
        n[1:] = np.logaddexp(n[1:], a[:-1])
        n[2:] = np.where(skip[2:], np.logaddexp(n[2:], a[:-2]), n[2:])
        a = n
    return np.logaddexp(a[-1], a[-2] if size > 1 else -np.inf)


MEASURED = {'rows': 0, 'compared_paths': 0}


def _check(hip, logits, labels, seq_len, max_label_len=None, blank=None, result=None, **kw):
    """One call checked row by row (see the module docstring); returns the host outputs."""
    num_steps, batch, classes = logits.shape
    blank = classes - 1 if blank is None else blank
    seq_len = np.asarray(seq_len, dtype=np.int32)
    if max_label_len is None:
        max_label_len = max([len(row) for row in labels] + [1])
    path, score, frame_logp, status = result if result is not None else \
        _run(hip, logits, labels, seq_len, max_label_len, blank, **kw)
    assert status.tolist() == _expected_status(logits, labels, seq_len, max_label_len, blank)
    for b, label in enumerate(labels):
        MEASURED['rows'] += 1
        if status[b] != 0:
            assert (path[b] == -1).all(), b
            assert np.isnan(score[b]) if status[b] == 3 else score[b] == -np.inf, (b, score[b])
            if frame_logp is not None:
                assert (frame_logp[b] == 0).all(), b
            continue
        length = int(seq_len[b])
        row = [int(s) for s in path[b, :length]]
        assert (path[b, length:] == -1).all(), b
        if frame_logp is not None:
            assert (frame_logp[b, length:] == 0).all(), b
        if length == 0:
            assert score[b] == 0.0 and not label, b
            continue
        why = ref.is_valid_path(row, label, blank, length)
        assert why is None, (b, why)
        x = logits[:length, b].astype(np.float64)
        mine = ref.rescore(x, label, row, blank)
        assert abs(score[b] - mine) <= 1e-5 * max(1.0, abs(mine)), (b, score[b], mine)
        best, best_path = ref.viterbi(x, label, blank)
        assert mine <= best + 1e-9 * max(1.0, abs(best)) and mine >= best - 1e-4 * length, \
            (b, mine, best)
        if ref.margin(x, label, best_path, blank) > 1e-3:
            MEASURED['compared_paths'] += 1
            assert row == best_path, b
        if frame_logp is not None:
            ext = octc.extended_labels(label, blank)
            lp = octc.log_softmax(x)[np.arange(length), [ext[s] for s in row]]
            assert np.abs(frame_logp[b, :length] - lp).max() <= 1e-5, b
    return path, score, frame_logp, status


def _random_labels(rng, length, classes, blank, repeat_p=0.2):
    ids = [c for c in range(classes) if c != blank]
    out = []
    for _ in range(length):
        out.append(out[-1] if out and rng.random() < repeat_p else int(rng.choice(ids)))
    return out


def _peaked(rng, logits, labels, seq_len, blank, boost=6.0):
    """Add ``boost`` to the class a reference alignment emits at each frame, so that one path
    wins by a wide margin."""
    logits = logits.copy()
    for b, label in enumerate(labels):
        length = int(seq_len[b])
        if length < octc.required_time(label) or length == 0:
            continue
        _, path = ref.viterbi(rng.normal(size=(length, logits.shape[2])), label, blank)
        for t, c in enumerate(ref.path_classes(path, label, blank)):
            logits[t, b, c] += boost
    return logits


@pytest.fixture(scope='module')
def hip():
    from ctc_asr_amd import hip as module
    module.load()
    return module


# ------------------------------------------------------------------------------------------------
# Correctness
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('num_steps,batch,max_len', [(50, 6, 12), (200, 5, 60), (500, 4, 150)])
def test_random_and_peaked_logits_match_the_reference(hip, num_steps, batch, max_len):
    rng = np.random.default_rng(num_steps + batch)
    classes, blank = 29, 28
    labels = [_random_labels(rng, int(rng.integers(0, max_len + 1)), classes, blank)
              for _ in range(batch)]
    seq_len = np.array([max(octc.required_time(l), int(rng.integers(num_steps // 2, num_steps + 1)))
                        for l in labels], dtype=np.int32)
    logits = (rng.normal(size=(num_steps, batch, classes)) * 2.0).astype(np.float32)
    before = MEASURED['compared_paths']
    _check(hip, logits, labels, seq_len, max_len)
    _check(hip, _peaked(rng, logits, labels, seq_len, blank), labels, seq_len, max_len)
    assert MEASURED['compared_paths'] - before >= batch     # every peaked row compares its path


def test_uniform_logits_take_the_reference_tie_path(hip):
    """Every path ties: the kernel's comparisons must follow the documented order exactly."""
    rng = np.random.default_rng(11)
    classes, blank = 29, 28
    labels = [_random_labels(rng, n, classes, blank, 0.3) for n in (0, 1, 5, 20, 40, 3)]
    seq_len = np.array([7, 1, 30, 90, 100, 6], dtype=np.int32)
    logits = np.zeros((100, len(labels), classes), dtype=np.float32)
    path, _, _, status = _check(hip, logits, labels, seq_len)
    assert (status == 0).all()
    for b, label in enumerate(labels):
        _, want = ref.viterbi(logits[:seq_len[b], b].astype(np.float64), label, blank)
        assert path[b, :seq_len[b]].tolist() == want, b


def test_score_lies_between_the_loss_and_the_loss_over_the_number_of_alignments(hip):
    rng = np.random.default_rng(12)
    classes, blank, num_steps = 29, 28, 120
    labels = [_random_labels(rng, n, classes, blank) for n in (3, 10, 30, 50)]
    seq_len = np.array([120, 90, 110, 120], dtype=np.int32)
    logits = (rng.normal(size=(num_steps, 4, classes)) * 3.0).astype(np.float32)
    _, score, _, status = _check(hip, logits, labels, seq_len)
    flat, offsets = pack_labels(labels)
    loss, _, _ = hip.ctc_loss_fwd_bwd(_t(logits), _t(flat, torch.int32),
                                      _t(offsets, torch.int32), _t(seq_len, torch.int32), 50)
    loss = loss.cpu().numpy()
    for b, label in enumerate(labels):
        count = _log_num_alignments(label, blank, int(seq_len[b]))
        assert -loss[b] - count - 1e-3 <= score[b] <= -loss[b] + 1e-3, (b, score[b], loss[b])


# ------------------------------------------------------------------------------------------------
# Edge shapes
# ------------------------------------------------------------------------------------------------
def test_short_rows_and_empty_labels(hip):
    rng = np.random.default_rng(20)
    classes, blank = 29, 28
    labels = [[], [], [3], [3], [4, 5], [], [7, 7]]
    seq_len = np.array([0, 1, 1, 0, 2, 6, 3], dtype=np.int32)
    logits = rng.normal(size=(6, len(labels), classes)).astype(np.float32)
    path, score, _, status = _check(hip, logits, labels, seq_len, max_label_len=2)
    assert status.tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert score[0] == 0.0 and (path[0] == -1).all()
    assert path[1, 0] == 0 and path[5, :6].tolist() == [0] * 6       # L = 0: all blank
    assert path[2, 0] == 1 and path[6, :3].tolist() == [1, 2, 3]


def test_tight_rows_have_exactly_one_alignment_and_one_frame_less_none(hip):
    rng = np.random.default_rng(21)
    classes, blank = 29, 28
    labels = [_random_labels(rng, n, classes, blank, 0.4) for n in (1, 4, 17, 60, 200)]
    need = [octc.required_time(l) for l in labels]
    num_steps = max(need) + 2
    logits = rng.normal(size=(num_steps, 2 * len(labels), classes)).astype(np.float32)
    rows = labels + labels
    seq_len = np.array(need + [n - 1 for n in need], dtype=np.int32)
    path, _, _, status = _check(hip, logits, rows, seq_len, max_label_len=200)
    assert status.tolist() == [0] * len(labels) + [1] * len(labels)
    for b, label in enumerate(labels):
        # the only alignment: every label for one frame, a blank between each repeat
        ext = octc.extended_labels(label, blank)
        want = [1]
        for k in range(1, len(label)):
            if label[k] == label[k - 1]:
                want.append(2 * k)
            want.append(2 * k + 1)
        assert path[b, :need[b]].tolist() == want, b
        assert ext[want[-1]] == label[-1]


def test_labels_at_the_ceiling_and_rows_past_max_label_len(hip):
    rng = np.random.default_rng(22)
    classes, blank = 29, 28
    labels = [_random_labels(rng, MAX_LABEL_LEN, classes, blank, 0.05),
              _random_labels(rng, 300, classes, blank), _random_labels(rng, 40, classes, blank)]
    num_steps = octc.required_time(labels[0]) + 30
    logits = (rng.normal(size=(num_steps, 3, classes)) * 2.0).astype(np.float32)
    seq_len = np.array([num_steps, num_steps - 5, 200], dtype=np.int32)
    _check(hip, logits, labels, seq_len, max_label_len=MAX_LABEL_LEN)
    _check(hip, _peaked(rng, logits, labels, seq_len, blank), labels, seq_len, MAX_LABEL_LEN)
    # max_label_len 299: row 1 (300 labels) and row 0 do not fit and are refused
    _, _, _, status = _check(hip, logits, labels, seq_len, max_label_len=299)
    assert status.tolist() == [2, 2, 0]
    with pytest.raises(Exception):
        _run(hip, logits, labels, seq_len, MAX_LABEL_LEN + 1)          # s_pad > 1152


def test_bad_ids_lengths_and_non_finite_logits(hip):
    rng = np.random.default_rng(23)
    classes, blank, num_steps = 29, 28, 40
    labels = [[1, 2], [29], [28], [-1], [3, 4], [3, 4], [5], [5], [6], [1]]
    seq_len = np.array([40, 40, 40, 40, 41, -1, 30, 30, 30, 20], dtype=np.int32)
    logits = rng.normal(size=(num_steps, len(labels), classes)).astype(np.float32)
    logits[5, 6, 3] = np.nan
    logits[29, 7, 0] = np.inf
    logits[0, 8, 28] = -np.inf
    logits[25, 9, 2] = np.nan            # past seq_len 20: does not count
    _, _, _, status = _check(hip, logits, labels, seq_len)
    assert status.tolist() == [0, 2, 2, 2, 2, 2, 3, 3, 3, 0]


@pytest.mark.parametrize('classes,blank', [(2, 0), (2, 1), (3, 0), (17, 5), (29, 0), (63, 62),
                                           (64, 0), (64, 63)])
def test_class_counts_and_blanks(hip, classes, blank):
    rng = np.random.default_rng(classes * 7 + blank)
    labels = [_random_labels(rng, n, classes, blank) for n in (0, 1, 8, 25)]
    seq_len = np.array([10, 5, 40, 80], dtype=np.int32)
    logits = (rng.normal(size=(80, 4, classes)) * 2.0).astype(np.float32)
    _check(hip, logits, labels, seq_len, blank=blank)
    _check(hip, _peaked(rng, logits, labels, seq_len, blank), labels, seq_len, blank=blank)


@pytest.mark.parametrize('batch', [31, 33, 63, 65, 127, 129])
def test_batches_with_empty_rows(hip, batch):
    rng = np.random.default_rng(batch)
    classes, blank, num_steps = 29, 28, 30
    labels = [[] if b % 5 == 0 else _random_labels(rng, int(rng.integers(1, 10)), classes, blank)
              for b in range(batch)]
    seq_len = np.array([0 if b % 7 == 3 else int(rng.integers(20, num_steps + 1))
                        for b in range(batch)], dtype=np.int32)
    logits = (rng.normal(size=(num_steps, batch, classes)) * 2.0).astype(np.float32)
    _check(hip, logits, labels, seq_len, max_label_len=10)


@pytest.mark.parametrize('max_len', [20, 150])
def test_t_on_both_sides_of_every_lds_tier(hip, max_len):
    classes, blank = 29, 28
    slab_t, table_t = _tier_bounds(classes, max_len)
    plain_t = (64 * 1024 - _fixed(max_len)) // (classes * 4 + _words(max_len) * 16)
    rng = np.random.default_rng(max_len)
    for num_steps in (plain_t, plain_t + 1, slab_t, slab_t + 1, table_t, table_t + 1):
        labels = [_random_labels(rng, max_len, classes, blank), _random_labels(rng, 3, classes,
                                                                               blank)]
        seq_len = np.array([num_steps, num_steps - 1], dtype=np.int32)
        logits = (rng.normal(size=(num_steps, 2, classes)) * 2.0).astype(np.float32)
        _check(hip, _peaked(rng, logits, labels, seq_len, blank), labels, seq_len, max_len)


def test_null_frame_logp_and_garbage_everywhere(hip):
    rng = np.random.default_rng(30)
    classes, blank, num_steps, batch = 29, 28, 300, 6
    labels = [_random_labels(rng, n, classes, blank) for n in (0, 5, 40, 80, 80, 3)]
    seq_len = np.array([0, 300, 250, 300, 90, 2], dtype=np.int32)
    logits = (rng.normal(size=(num_steps, batch, classes)) * 2.0).astype(np.float32)
    result = _check(hip, logits, labels, seq_len, frame_logp=False)
    assert result[2] is None
    ws_bytes = hip.ctc_align_workspace_bytes(num_steps, batch, classes, 80)
    garbage = dict(
        path=torch.full((batch, num_steps), 12345, dtype=torch.int32, device=DEV),
        score=torch.full((batch,), 7.0, device=DEV),
        frame_logp=torch.full((batch, num_steps), 99.0, device=DEV),
        status=torch.full((batch,), 77, dtype=torch.int32, device=DEV),
        workspace=torch.randint(0, 256, (ws_bytes,), dtype=torch.uint8, device=DEV))
    dirty = _check(hip, logits, labels, seq_len, **garbage)
    for a, b in zip(result, dirty):
        if a is not None:
            assert np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------
# Changing data on one workspace
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('num_steps,max_len', [(400, 60), (900, 300), (1400, 100)])
def test_changing_data_on_one_workspace(hip, num_steps, max_len):
    """Three calls with different logits, labels and lengths on one workspace (LDS slab; slab in
    the workspace; slab and table in the workspace) are each bit-equal to a fresh workspace."""
    classes, blank, batch = 29, 28, 5
    slab_t, table_t = _tier_bounds(classes, max_len)
    assert (num_steps <= slab_t, num_steps <= table_t) in ((True, True), (False, True),
                                                           (False, False))
    shared = torch.randint(0, 256, (hip.ctc_align_workspace_bytes(num_steps, batch, classes,
                                                                   max_len),),
                           dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(num_steps)
    for _ in range(3):
        labels = [_random_labels(rng, int(rng.integers(0, max_len + 1)), classes, blank)
                  for _ in range(batch)]
        seq_len = np.array([max(octc.required_time(l), int(rng.integers(1, num_steps + 1)))
                            for l in labels], dtype=np.int32)
        logits = (rng.normal(size=(num_steps, batch, classes)) * 3.0).astype(np.float32)
        got = _run(hip, logits, labels, seq_len, max_len, workspace=shared)
        fresh = _run(hip, logits, labels, seq_len, max_len)
        for a, b in zip(got, fresh):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
        _check(hip, logits, labels, seq_len, max_len, result=got)


# ------------------------------------------------------------------------------------------------
# Through the model
# ------------------------------------------------------------------------------------------------
def test_a_memorised_batch_aligns_along_its_greedy_path():
    """The DS2 BiLSTM model of tools/overfit_check.py memorises 8 utterances; aligning each
    transcript then emits greedy's argmax on every frame where it wins clearly (the greedy path
    collapses to the transcript, so it is itself the best alignment), and the words join to the
    transcript."""
    from ctc_asr_amd import alignment
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.labels import BLANK_ID, decode
    from ctc_asr_amd.model import CTCModel, ModelConfig
    from ctc_asr_amd.synth import synthetic_batch

    class Flags:
        learning_rate, adam_beta1, adam_beta2, adam_epsilon = 3e-4, 0.9, 0.999, 1e-8

    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32), num_units_dense=512,
                      num_layers_rnn=2, num_units_rnn=1024, rnn_cell='lstm', cudnn=True,
                      dense_dropout_rate=0.0)
    trainer = Trainer(cfg, flags=Flags, device='cuda', seed=3)
    feats, lengths, labels, texts = synthetic_batch(8, 2.0, seed=5, chars_per_second=6.0)
    feats_d, len_d = torch.tensor(feats, device='cuda'), torch.tensor(lengths, device='cuda')
    packed = CTCModel.pack_labels(labels, trainer.model.device)
    for step in range(400):
        trainer.train_step(feats_d, len_d, packed, check=(step % 50 == 0))
    model = trainer.model
    model.check_rnn_error()
    logits, seq_len = model.inference_fn(feats_d, len_d, training=False)
    greedy, _, _ = model.decode_fn(logits, seq_len, None, greedy=True)
    assert [decode(g) for g in greedy] == texts
    path, score, frame_logp, status = model.align_fn(logits, seq_len, labels)
    assert (status.cpu().numpy() == 0).all()
    path, frame_logp = path.cpu().numpy(), frame_logp.cpu().numpy()
    lp = torch.log_softmax(logits.double(), dim=-1).cpu().numpy()
    seq_len = seq_len.cpu().numpy()
    hop = alignment.frame_seconds(cfg, False)
    clear = 0
    for b, text in enumerate(texts):
        row = [int(v) for v in labels[b] if v != 0]
        ext = octc.extended_labels(row, BLANK_ID)
        top2 = np.sort(lp[:seq_len[b], b], axis=-1)[:, -2:]
        for t in np.nonzero(top2[:, 1] - top2[:, 0] > 1.0)[0]:
            assert ext[path[b, t]] == int(np.argmax(lp[t, b])), (b, t)
            clear += 1
        words = alignment.segments(path[b], row, hop, frame_logp[b])
        assert ' '.join(w['word'] for w in words) == text
        assert all(w['confidence'] <= 0.0 for w in words)
    assert clear > 0.25 * int(seq_len.sum())


@pytest.fixture()
def corpus(tmp_path):
    from ctc_asr_amd import synth
    from ctc_asr_amd.params import FLAGS
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
                 rnn_cell='lstm', max_epochs=2, learning_rate=1e-3, beam_width=8,
                 log_frequency=2, random_seed=7, dense_dropout_rate=0.0)
    yield tmp_path
    FLAGS.reset()


def test_predict_with_timestamps(corpus, capsys):
    from ctc_asr_amd import alignment, input_functions, predict, storage, train
    from ctc_asr_amd.model import CTCModel, ModelConfig
    from ctc_asr_amd.params import FLAGS
    FLAGS.max_epochs = 1
    assert train.main([]) == 0
    capsys.readouterr()
    rows = input_functions.read_manifest(FLAGS.test_csv)
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=1)
    storage.restore_checkpoint(storage.latest_checkpoint(FLAGS.train_dir), model)
    hop = alignment.frame_seconds(model.cfg, False)
    for row in rows[:4]:
        wav = os.path.join(FLAGS.corpus_dir, row['path'])
        assert predict.main(['--input', wav, '--timestamps']) == 0
        out = capsys.readouterr().out
        assert "'words'" in out and "'plaintext'" in out
        got = predict.predict(model, wav, timestamps=True)
        assert repr(got['plaintext']) in out
        duration = len(input_functions.read_wav(wav)) / 16000.0
        words = got['words']
        feats, lengths = input_functions.features_from_pcm([input_functions.read_wav(wav)],
                                                           model.device)
        logits, seq_len = model.inference_fn(feats, lengths, training=False)
        ids = [v for v in got['decoded'].tolist() if v != 0]
        status = int(model.align_fn(logits, seq_len, [ids])[3][0])
        # a decode the alignment cannot place gives no words; any other gives the plaintext's
        joined = ' '.join(got['plaintext'].split()) if status == 0 else ''
        assert ' '.join(w['word'] for w in words) == joined
        ends = [0.0] + [x for w in words for x in (w['start'], w['end'])]
        assert ends == sorted(ends), words
        # the last logit frame may reach up to half a frame past the last sample
        assert all(w['end'] <= duration + hop / 2 and w['start'] < w['end'] for w in words)
    # without the flag: no words
    assert 'words' not in predict.predict(model, wav)


def test_align_driver_writes_one_line_per_row_in_order(corpus):
    from ctc_asr_amd import align, train
    from ctc_asr_amd.csv_helper import read_csv_rows
    from ctc_asr_amd.params import FLAGS
    FLAGS.max_epochs = 1
    assert train.main([]) == 0
    out = str(corpus / 'aligned.jsonl')
    assert align.main(['--align_csv', FLAGS.test_csv, '--align_output', out]) == 0
    rows = read_csv_rows(FLAGS.test_csv)[1:]          # every row: no [1:-1] quirk
    lines = [json.loads(line) for line in open(out, encoding='utf-8')]
    assert [r['path'] for r in lines] == [r['path'] for r in rows]
    assert len(rows) == 10 and len({r['path'] for r in rows}) == 9
    for line, row in zip(lines, rows):
        assert set(line) == {'path', 'status', 'score', 'score_per_frame', 'words'}
        assert line['status'] == 'ok', line
        assert math.isfinite(line['score']) and line['score'] <= 0.0
        assert line['score_per_frame'] <= 0.0
        assert ' '.join(w['word'] for w in line['words']) == row['label']
        times = [x for w in line['words'] for x in (w['start'], w['end'])]
        assert times == sorted(times)
    # a transcript outside the alphabet raises, as training does
    bad = corpus / 'bad.csv'
    text = open(FLAGS.test_csv, encoding='utf-8').read().splitlines()
    path = text[1].split(';')[0]
    bad.write_text('\n'.join([text[0], '{};Hello;1.0'.format(path)]) + '\n')
    with pytest.raises(ValueError):
        align.main(['--align_csv', str(bad), '--align_output', str(corpus / 'bad.jsonl')])
