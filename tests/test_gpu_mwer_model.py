"""Minimum word error rate training through `CTCModel.mwer_loss_fn`, `forward_backward` and
`engine.Trainer`, on the tiny model of tests/test_gpu_nbest_model.py with four utterances.

The accumulation bar is that of tests/test_gpu_schedule_model.py (``1e-5 * max(1, max |want|)``
between a gradient arena filled by two accumulated passes and the sum of two separate ones)."""

import numpy as np
import pytest
import torch

from ctc_asr_amd import labels as alphabet
from ctc_asr_amd import metrics

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_TOL = 1e-5         # tests/test_gpu_schedule_model.py
TEXTS = ['ab cd', 'e f', 'g', 'hi jk l']
MWER = {'nbest': 4, 'beam_width': 8, 'ctc_weight': 0.3}


def _cfg():
    from ctc_asr_amd.model import ModelConfig
    return ModelConfig(used_model='ds2', conv_filters=(4, 4), rnn_cell='lstm', cudnn=True,
                       num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                       dense_dropout_rate=0.0)


def _batch(seed=3, frames=61):
    rng = np.random.default_rng(seed)
    feats = torch.tensor(rng.normal(size=(4, frames, 80)).astype(np.float32))
    return feats, torch.full((4,), frames, dtype=torch.int32), \
        [alphabet.encode(text) for text in TEXTS]


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _trainer(**kwargs):
    from ctc_asr_amd.engine import Trainer
    trainer = Trainer(_cfg(), device=DEV, seed=3, **kwargs)
    trainer.lr = 1e-3
    return trainer


@pytest.mark.parametrize('risk', ['label', 'word'])
def test_loss_fn_is_the_weighted_ctc_gradient_plus_a_direct_call(hip, risk):
    from ctc_asr_amd.model import CTCModel
    model = CTCModel(_cfg(), DEV, seed=5)
    feats, flen, labels = _batch()
    logits, seq_len = model.inference_fn(feats, flen, training=True)
    loss = model.mwer_loss_fn(logits, seq_len, labels, originals=TEXTS, risk=risk, **MWER)
    got, last = model._acts['dlogits'].clone(), model.last_mwer
    batch, nbest = 4, MWER['nbest']
    flat, offsets, max_len, rows = model.pack_labels(labels, DEV)
    ctc_loss, want, status = hip.ctc_loss_fwd_bwd(logits, flat, offsets, seq_len, max_len,
                                                  grad_scale=MWER['ctc_weight'] / batch)
    ctc_only = want.clone()
    want, expected, score, posterior, hyp_status = hip.ctc_mwer(
        logits, seq_len, last['labels'], last['label_offsets'], last['n_hyps'], last['risk'],
        scale=1.0 / batch, accumulate=True, grad=want)
    assert _bits(got, want)
    if risk == 'label':
        # (the hypotheses of an untrained model differ in their label errors; in word errors
        # they need not: every word of every one of them is wrong)
        assert not _bits(got, ctc_only)
    assert _bits(expected, last['expected_risk']) and _bits(score, last['score'])
    assert torch.equal(model.last_status, status) and bool((status == 0).all())
    total = expected + MWER['ctc_weight'] * ctc_loss
    assert _bits(model.last_per_utterance_loss, total) and float(loss) == float(total.mean())
    assert bool(torch.isfinite(total).all())
    # the risks are the error counts of the decoded lists
    out, out_len, n_paths = (t.cpu().numpy() for t in (last['out'], last['out_len'],
                                                       last['n_hyps']))
    assert (n_paths >= 2).all()
    used = [(b, k) for b in range(batch) for k in range(int(n_paths[b]))]
    hyps = [out[b, k, :out_len[b, k]].tolist() for b, k in used]
    if risk == 'label':
        counts = metrics.error_counts(hyps, [rows[b] for b, _ in used], DEV)
    else:
        ref_words, hyp_words = metrics.word_ids([TEXTS[b] for b, _ in used],
                                                [alphabet.decode(h) for h in hyps])
        counts = metrics.error_counts(hyp_words, ref_words, DEV)
    risks = last['risk'].cpu().numpy().reshape(batch, nbest)
    assert [risks[b, k] for b, k in used] == counts[:, 0].astype(np.float32).tolist()
    # the kernel's rows are the decoder's: the exact scores of `hip.ctc_score` on the list
    assert bool((hyp_status.reshape(batch, nbest)[:, :2] == 0).all())
    # without transcripts the word risk scores against the references decoded
    if risk == 'word':
        again = model.mwer_loss_fn(logits, seq_len, labels, risk='word', **MWER)
        assert float(again) == float(loss) and _bits(model._acts['dlogits'], got)


def test_forward_backward_accumulates_like_the_ctc_loss(hip):
    """Two accumulated passes fill the arena with the sum of the two separate ones."""
    from ctc_asr_amd.model import CTCModel
    model = CTCModel(_cfg(), DEV, seed=5)
    settings = dict(MWER, risk='label')
    batch_a, batch_b = _batch(3), _batch(4)
    model.forward_backward(*batch_a, mwer=settings, originals=TEXTS)
    grad_a = model.arena.grad.clone()
    model.forward_backward(*batch_b, mwer=settings, originals=TEXTS)
    want = (grad_a + model.arena.grad).cpu().numpy().astype(np.float64)
    model.arena.grad.fill_(123.0)
    model.forward_backward(*batch_a, mwer=settings, originals=TEXTS)
    model.forward_backward(*batch_b, mwer=settings, originals=TEXTS, accumulate=True)
    torch.cuda.synchronize()
    got = model.arena.grad.cpu().numpy().astype(np.float64)
    limit = GRAD_TOL * max(1.0, np.abs(want).max())
    worst = np.abs(got - want).max()
    print('max |accumulated - sum| {:.3g} against {:.3g} (max |grad| {:.3g})'.format(
        worst, limit, np.abs(want).max()))
    assert np.isfinite(want).all() and np.abs(want).max() > 0 and worst < limit


@pytest.mark.parametrize('risk', ['label', 'word'])
def test_a_train_step_moves_the_parameters_and_reports_the_risk(hip, risk):
    trainer = _trainer(mwer_nbest=4, mwer_beam_width=8, mwer_ctc_weight=0.3, mwer_risk=risk)
    feats, flen, labels = _batch()
    before = trainer.model.arena.param.clone()
    loss = trainer.train_step(feats, flen, labels, originals=TEXTS)
    trainer.drain_checks()
    assert np.isfinite(float(loss)) and not _bits(before, trainer.model.arena.param)
    assert trainer.last_expected_risk.is_cuda and trainer.last_expected_risk.shape == (4,)
    assert bool(torch.isfinite(trainer.last_expected_risk).all())
    assert trainer.last_mwer_paths.is_cuda and int(trainer.last_mwer_paths.min()) >= 2
    assert trainer.skipped_step_count() == 0 and trainer.model.step_count == 1


def test_accumulated_micro_steps_are_one_update(hip):
    """grad_accum_steps = 2: the update applies the sum of its two micro-steps' gradients."""
    halves = _trainer(mwer_nbest=4, mwer_beam_width=8, mwer_ctc_weight=0.3, mwer_risk='label',
                      grad_accum_steps=2)
    single = _trainer(mwer_nbest=4, mwer_beam_width=8, mwer_ctc_weight=0.3, mwer_risk='label')
    batch_a, batch_b = _batch(3), _batch(4)
    model = single.model
    model.forward_backward(*batch_a, mwer=single.mwer)
    grad_a = model.arena.grad.clone()
    model.forward_backward(*batch_b, mwer=single.mwer)
    want = (grad_a + model.arena.grad).cpu().numpy().astype(np.float64)
    before = halves.model.arena.param.clone()
    halves.train_step(*batch_a)
    assert halves.accumulating and _bits(before, halves.model.arena.param)
    halves.train_step(*batch_b)
    halves.drain_checks()
    got = halves.model.arena.grad.cpu().numpy().astype(np.float64)
    limit = GRAD_TOL * max(1.0, np.abs(want).max())
    print('max |two micro-steps - sum| {:.3g} against {:.3g}'.format(np.abs(got - want).max(),
                                                                    limit))
    assert np.abs(got - want).max() < limit and np.abs(want).max() > 0
    assert halves.model.step_count == 1 and not _bits(before, halves.model.arena.param)


def test_a_non_finite_feature_drops_the_update_on_the_device(hip):
    trainer = _trainer(mwer_nbest=4, mwer_beam_width=8, mwer_risk='label')
    feats, flen, labels = _batch()
    trainer.train_step(feats, flen, labels, check=False)
    torch.cuda.synchronize()
    a = trainer.model.arena
    before = [t.clone() for t in (a.param, a.m, a.v)]
    assert trainer.skipped_step_count() == 0
    bad = feats.clone()
    bad[2, 17, 5] = float('nan')
    trainer.train_step(bad, flen, labels, check=False)
    torch.cuda.synchronize()
    for got, want in zip((a.param, a.m, a.v), before):
        assert _bits(got, want)
    assert trainer.skipped_step_count() == 1
    assert not bool(torch.isfinite(trainer.model.last_per_utterance_loss).all())


def test_switched_off_nothing_changes(hip, monkeypatch):
    """mwer_nbest = 0: a trainer built with the new keyword arguments and one built without, from
    one seed, three steps each.

    Two runs of a training step do not give bit-identical gradients (the bias sums use atomics:
    tests/test_gpu_clip_model.py), so the bits of two trainers cannot be held against each other
    directly.  What is held, bit for bit, is each trainer against itself, as that file does it:
    every update is `hip.adam_step` of the parameters and moments before the step with the
    gradients the step left in the arena - nothing else touched them -, the model is called with
    the arguments it was always called with, and no entry point of the MWER path is ever
    reached.  The two trainers' parameters then agree within the bar of "one update computed two
    ways" (tests/test_gpu_schedule_model.py: 1e-6 per update at lr 1e-3); whether they also agree
    in every bit is printed."""
    lib = hip.load()
    reached = []
    for name in ('ctcasr_ctc_mwer', 'ctcasr_ctc_beam_decode_nbest', 'ctcasr_edit_distance'):
        def spy(*args, _real=getattr(lib, name), _name=name):
            reached.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, name, spy)
    plain = _trainer()
    off = _trainer(mwer_nbest=0, mwer_beam_width=64, mwer_ctc_weight=0.01, mwer_risk='word')
    assert off.mwer is None and plain.mwer is None
    assert _bits(plain.model.arena.param, off.model.arena.param)
    seen = []
    for trainer in (plain, off):
        def watched(*args, _real=trainer.model.forward_backward, **kwargs):
            seen.append(sorted(kwargs))
            return _real(*args, **kwargs)
        monkeypatch.setattr(trainer.model, 'forward_backward', watched)
    for step in range(1, 4):
        feats, flen, labels = _batch(10 + step)
        for trainer in (plain, off):
            a = trainer.model.arena
            p, m, v = a.param.clone(), a.m.clone(), a.v.clone()
            if trainer is off:
                trainer.train_step(feats, flen, labels, originals=TEXTS)
            else:
                trainer.train_step(feats, flen, labels)
            hip.adam_step(p, a.grad, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1.0)
            assert _bits(p, a.param) and _bits(m, a.m) and _bits(v, a.v), step
    plain.drain_checks()
    off.drain_checks()
    assert not reached and seen == [['check', 'reduce_hook']] * 6
    diff = float((plain.model.arena.param - off.model.arena.param).abs().max())
    print('two trainers after 3 updates: max |param difference| {:.3g} (bit-identical: {})'
          .format(diff, _bits(plain.model.arena.param, off.model.arena.param)))
    assert diff < 3 * 1e-6
    assert off.last_expected_risk is None and not hasattr(off.model, 'last_mwer')
    with pytest.raises(ValueError, match='mwer_nbest'):
        _trainer(mwer_nbest=1)
    with pytest.raises(ValueError, match='mwer_beam_width'):
        _trainer(mwer_nbest=8, mwer_beam_width=4)
