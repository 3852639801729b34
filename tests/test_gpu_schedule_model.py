"""Accumulated micro-batches, the parameters' moving average and the learning-rate schedule through
`CTCModel` and `engine.Trainer`, on the tiny model of tests/test_gpu_clip_model.py.

Tolerances.  A gradient arena filled by two accumulated micro-batches against the sum of two
separate passes is the comparison tests/test_gpu_dp_rccl.py makes between gradient arenas of the
same step computed two ways (line 204: ``1e-5 * max(1, max |want|)``; two runs differ by the order
of the bias sums' atomics and of the partial sums).  Parameters after an update of accumulated
micro-batches against the update of the whole batch is that file's "two ranks equal one rank"
(line 109: ``1e-6`` after one step at lr 1e-3), times the number of updates."""

import types

import numpy as np
import pytest
import torch

from tests import adam_ema_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_TOL = 1e-5         # tests/test_gpu_dp_rccl.py:204
PARAM_TOL = 1e-6        # tests/test_gpu_dp_rccl.py:109, per update at lr = 1e-3


def _cfg(**kwargs):
    from ctc_asr_amd.model import ModelConfig
    return ModelConfig(num_units_rnn=64, num_layers_rnn=1, num_units_dense=32, **kwargs)


def _batch(seed=3, rows=2, frames=41):
    rng = np.random.default_rng(seed)
    feats = torch.tensor(rng.normal(size=(rows, frames, 80)).astype(np.float32))
    labels = [[1, 2, 3], [4, 5], [6], [7, 8, 9, 9]][:rows]
    return feats, torch.full((rows,), frames, dtype=torch.int32), labels


def _trainer(cfg=None, **kwargs):
    from ctc_asr_amd.engine import Trainer
    return Trainer(cfg or _cfg(), device=DEV, seed=3, **kwargs)


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _accumulation_is_a_sum(cfg, batch_a, batch_b, seed=3):
    from ctc_asr_amd.model import CTCModel
    model = CTCModel(cfg, DEV, seed=seed)
    model.forward_backward(*batch_a)
    grad_a = model.arena.grad.clone()
    model.forward_backward(*batch_b)
    want = (grad_a + model.arena.grad).cpu().numpy().astype(np.float64)
    model.arena.grad.fill_(123.0)                    # the first pass clears, the second adds
    model.forward_backward(*batch_a)
    model.forward_backward(*batch_b, accumulate=True)
    torch.cuda.synchronize()
    model.check_rnn_error()
    got = model.arena.grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    worst = {}
    for name, start, stop in model.arena.layer_slices:
        worst[name] = float(np.abs(got[start:stop] - want[start:stop]).max())
        assert np.abs(want[start:stop]).max() > 0, name
    limit = GRAD_TOL * max(1.0, np.abs(want).max())
    print('max |accumulated - sum| per layer {} against {:.3g} (max |grad| {:.3g})'.format(
        worst, limit, np.abs(want).max()))
    assert max(worst.values()) < limit, worst
    return model


def test_accumulation_is_a_sum_streaming_shape(hip):
    _accumulation_is_a_sum(_cfg(dense_dropout_rate=0.0), _batch(3), _batch(4))


def test_accumulation_is_a_sum_persistent_shape(hip):
    """LSTM-1024, 16 rows, T' = 9: the persistent recurrences and the own weight-gradient kernel,
    whose tiles add into the arena."""
    from ctc_asr_amd.model import ModelConfig
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32), num_units_dense=64,
                      num_layers_rnn=2, num_units_rnn=1024, rnn_cell='lstm', cudnn=True,
                      dense_dropout_rate=0.0)
    assert hip.rnn_persistent_supported('lstm', 9, 16, 1024)

    def batch(seed):
        rng = np.random.default_rng(seed)
        feats = torch.tensor(rng.normal(size=(16, 17, 80)).astype(np.float32))
        labels = [list(rng.integers(1, 28, size=rng.integers(1, 4))) for _ in range(16)]
        return feats, torch.full((16,), 17, dtype=torch.int32), labels

    model = _accumulation_is_a_sum(cfg, batch(1), batch(2), seed=1)
    assert model._acts['t_out'] == 9


def test_two_micro_batches_of_two_rows_are_one_batch_of_four(hip):
    cfg = _cfg(dense_dropout_rate=0.0)
    feats, flen, labels = _batch(5, rows=4)
    whole, halves = _trainer(cfg), _trainer(cfg, grad_accum_steps=2)
    whole.lr = halves.lr = 1e-3
    assert _bits(whole.model.arena.param, halves.model.arena.param)
    assert halves.accumulating is False
    for update in range(3):
        loss = whole.train_step(feats, flen, labels)
        first = halves.train_step(feats[:2], flen[:2], labels[:2])
        assert halves.accumulating and halves.model.step_count == update
        with pytest.raises(RuntimeError, match='open'):
            halves.drain_checks()
        with pytest.raises(RuntimeError, match='open'):
            halves.save_checkpoint('/nonexistent', 1)
        second = halves.train_step(feats[2:], flen[2:], labels[2:])
        assert not halves.accumulating and halves.model.step_count == update + 1
        assert abs(float(loss) - (float(first) + float(second)) / 2) < 1e-5
    whole.drain_checks()
    halves.drain_checks()
    assert whole.model.step_count == halves.model.step_count == 3
    diff = float((whole.model.arena.param - halves.model.arena.param).abs().max())
    print('max |param difference| after 3 updates: {:.3g} against {:.3g}'.format(
        diff, 3 * PARAM_TOL))
    assert diff < 3 * PARAM_TOL
    assert halves.skipped_step_count() == 0
    # a ragged group: one micro-step, then dropped - nothing was counted, nothing applied
    before = halves.model.arena.param.clone()
    halves.train_step(feats[:2], flen[:2], labels[:2])
    halves.abandon_update()
    halves.drain_checks()
    assert halves.model.step_count == 3 and _bits(before, halves.model.arena.param)


def test_an_infeasible_row_in_the_first_micro_step_drops_the_whole_update(hip):
    trainer = _trainer(grad_accum_steps=2, ema_decay=0.9)
    feats, flen, labels = _batch(3)
    trainer.train_step(feats, flen, labels)
    trainer.train_step(feats, flen, labels)
    trainer.drain_checks()
    a = trainer.model.arena
    before = [t.clone() for t in (a.param, a.m, a.v, a.ema)]
    assert not _bits(a.param, a.ema)
    # 21 output steps cannot carry 30 labels: where tf.nn.ctc_loss raises
    trainer.train_step(feats, flen, [list(range(1, 28)) + [1, 2, 3], [4, 5]])
    # (a clean second micro-step; unchecked, so that the first one's report waits for the drain)
    trainer.train_step(feats, flen, labels, check=False)
    torch.cuda.synchronize()
    for got, want in zip((a.param, a.m, a.v, a.ema), before):
        assert _bits(got, want)
    assert trainer.skipped_step_count() == 1
    with pytest.raises(ValueError, match=r'training step 2 \(micro-step 1 of 2\); its update '
                                         r'was not applied'):
        trainer.drain_checks()
    with pytest.warns(RuntimeWarning, match='dropped on the device'):
        trainer.drain_checks()
    assert trainer.model.step_count == 1
    trainer.train_step(feats, flen, labels)
    trainer.train_step(feats, flen, labels)
    trainer.drain_checks()
    assert trainer.model.step_count == 2 and not _bits(a.param, before[0])


def test_the_average_follows_the_trainers_own_parameters(hip, tmp_path):
    from ctc_asr_amd import storage
    from ctc_asr_amd.model import CTCModel
    trainer = _trainer(ema_decay=0.9)
    trainer.lr = 1e-3
    model, a = trainer.model, trainer.model.arena
    assert a.ema is not None and _bits(a.ema, a.param)
    assert a.ema.data_ptr() != a.param.data_ptr()
    feats, flen, labels = _batch(3)
    exact = a.ema.cpu().numpy().astype(np.float64)
    budget = np.zeros(a.size)
    for k in range(5):
        ema_old = a.ema.cpu().numpy()
        trainer.train_step(feats, flen, labels)
        param = a.param.cpu().numpy()
        exact = ref.ema_update(exact, param, ref.alpha32(0.9, k))
        budget = np.maximum(budget, ref.ema_bound(ema_old, param))
    trainer.drain_checks()
    err = np.abs(a.ema.cpu().numpy().astype(np.float64) - exact)
    print('5 updates, error / (5 x bound): {:.4f}'.format(
        float((err / np.maximum(5 * budget, 1e-300)).max())))
    assert (err <= 5 * budget).all() and not _bits(a.ema, a.param)

    # swap and restore, bit for bit, also when the body raises
    param, ema, version = a.param.clone(), a.ema.clone(), a.version
    with model.ema_weights():
        assert _bits(a.param, ema) and _bits(a.ema, param) and a.version == version + 1
        logits_ema, _ = model.inference_fn(feats, flen, training=False)
        logits_ema = logits_ema.clone()
    assert _bits(a.param, param) and _bits(a.ema, ema) and a.version == version + 2
    with pytest.raises(KeyError, match='inside'):
        with model.ema_weights():
            raise KeyError('inside')
    assert _bits(a.param, param) and _bits(a.ema, ema) and a.version == version + 4

    # the checkpoint's average, restored as the parameters, gives the same logits
    path = trainer.save_checkpoint(str(tmp_path), 1)
    other = CTCModel(_cfg(), DEV, seed=9)
    assert other.arena.ema is None
    storage.restore_checkpoint(path, other, weights='ema')
    assert _bits(other.arena.param, ema)
    logits, _ = other.inference_fn(feats, flen, training=False)
    assert torch.equal(logits, logits_ema)
    with pytest.raises(hip.CtcAsrError):
        other.apply_gradients(1e-3, ema_decay=0.9)               # built without an average
    with pytest.raises(hip.CtcAsrError):
        with other.ema_weights():
            pass


def test_defaults_allocate_nothing_and_launch_what_they_launched(hip, monkeypatch):
    lib = hip.load()
    calls = []
    real = lib.ctcasr_adam_step_ema

    def counted(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(lib, 'ctcasr_adam_step_ema', counted)
    trainer = _trainer()
    assert (trainer.grad_accum_steps, trainer.ema_decay, trainer.lr_schedule,
            trainer.lr_scheduled, trainer.accumulating) == (1, 0.0, 'constant', False, False)
    model, a = trainer.model, trainer.model.arena
    assert a.ema is None
    trainer.lr = 1e-3
    feats, flen, labels = _batch(3)
    for step in range(1, 4):
        p, m, v = a.param.clone(), a.m.clone(), a.v.clone()
        trainer.train_step(feats, flen, labels)
        # forward_backward left the step's gradients in the arena (Adam only reads them): what
        # apply_gradients(lr, beta1, beta2, eps, grad_scale=1 / world) launched before
        hip.adam_step(p, a.grad, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1.0)
        assert _bits(p, a.param) and _bits(m, a.m) and _bits(v, a.v), step
        assert not trainer.accumulating and model.step_count == step
    trainer.drain_checks()
    assert not calls and a.ema is None and trainer.lr == 1e-3
    # the spy does see the entry once an average is kept
    averaged = _trainer(ema_decay=0.5)
    averaged.train_step(feats, flen, labels)
    averaged.drain_checks()
    assert calls == [1]


def test_a_staircase_hands_the_kernel_learning_rate_at(hip, monkeypatch):
    from ctc_asr_amd.params import learning_rate_at
    flags = types.SimpleNamespace(learning_rate=1e-3, learning_rate_decay_factor=0.5,
                                  steps_per_decay=2, minimum_lr=1e-5, lr_schedule='staircase')
    seen = []
    real = hip.adam_step

    def spy(param, grad, m, v, step, lr, *args, **kwargs):
        seen.append((step, lr))
        return real(param, grad, m, v, step, lr, *args, **kwargs)

    monkeypatch.setattr(hip, 'adam_step', spy)
    trainer = _trainer(flags=flags)
    assert trainer.lr_scheduled and trainer.lr_schedule == 'staircase'
    a = trainer.model.arena
    feats, flen, labels = _batch(3)
    rates = [learning_rate_at(u, flags) for u in (1, 2, 3)]
    assert rates == [1e-3, 1e-3, 5e-4]
    for update in range(3):
        p, m, v = a.param.clone(), a.m.clone(), a.v.clone()
        trainer.train_step(feats, flen, labels)
        # the manual run: the step's own gradients (Adam only reads them) at that rate
        real(p, a.grad, m, v, update + 1, rates[update], 0.9, 0.999, 1e-8, 1.0)
        assert _bits(p, a.param) and _bits(m, a.m) and _bits(v, a.v), update
    trainer.drain_checks()
    assert seen == [(1, rates[0]), (2, rates[1]), (3, rates[2])] and trainer.lr == rates[2]
    # the keyword wins over the flag; an incomplete schedule is refused when the trainer is built
    assert _trainer(flags=flags, lr_schedule='constant').lr_scheduled is False
    with pytest.raises(ValueError, match='lr_total_steps'):
        _trainer(lr_schedule='cosine')
    with pytest.raises(ValueError):
        _trainer(grad_accum_steps=0)
    with pytest.raises(ValueError):
        _trainer(ema_decay=1.0)
