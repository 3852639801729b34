"""`CTCModel` with ``rnn_batch_norm`` against the float64 torch restatement
(tests/batchnorm_reference.py: `oracle.torch_ref.TorchRefModel` with the input of layers 2..L
normalised): logits, loss, every gradient, training steps, the running statistics, checkpoints,
dropped steps and accumulated micro-batches.

Tolerances are those of tests/test_gpu_model.py (lines 195-219) for this very comparison: 1e-3 on
logits and loss, ``1e-3 * max(1, max |ref|)`` per gradient tensor; accumulated gradients use
``GRAD_TOL`` of tests/test_gpu_schedule_model.py."""

import numpy as np
import pytest
import torch

from tests import batchnorm_reference as ref
from tests.test_gpu_schedule_model import GRAD_TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _streaming_cfg(**kwargs):
    """ds1, the tanh BasicRNNCell path (per-row lengths: the masked counting rule) on the
    streaming kernels."""
    from ctc_asr_amd.model import ModelConfig
    return ModelConfig(used_model='ds1', rnn_cell='rnn_tanh', cudnn=False, num_units_dense=32,
                       num_layers_rnn=2, num_units_rnn=64, dense_dropout_rate=0.0, **kwargs)


def _persistent_cfg(**kwargs):
    """The persistent shape of tests/test_gpu_schedule_model.py."""
    from ctc_asr_amd.model import ModelConfig
    return ModelConfig(used_model='ds2', conv_filters=(32, 32), num_units_dense=64,
                       num_layers_rnn=2, num_units_rnn=1024, rnn_cell='lstm', cudnn=True,
                       dense_dropout_rate=0.0, **kwargs)


def _params(cfg, seed):
    """Livelier weights than the initialiser's, gamma and beta away from 1 and 0."""
    from ctc_asr_amd.model import init_params
    rng = np.random.default_rng(seed)
    flat = init_params(cfg, seed)
    for name in flat:
        flat[name] = (flat[name] + rng.normal(size=flat[name].shape) * 0.05).astype(np.float32)
        if name.endswith('bn_gamma') or name.endswith('bn_beta'):
            flat[name] = (flat[name] + rng.normal(size=flat[name].shape) * 0.2).astype(np.float32)
    return flat


def _streaming_batch(seed=3):
    rng = np.random.default_rng(seed)
    feats = rng.normal(size=(2, 41, 80)).astype(np.float32)
    flen = np.array([41, 30], dtype=np.int32)
    feats[1, 30:] = 0.0
    return feats, flen, [[1, 2, 3], [4, 5]]


def _persistent_batch(seed=1):
    rng = np.random.default_rng(seed)
    feats = rng.normal(size=(16, 17, 80)).astype(np.float32)
    labels = [list(rng.integers(1, 28, size=rng.integers(1, 4))) for _ in range(16)]
    return feats, np.full(16, 17, dtype=np.int32), labels


def _reference(cfg, flat):
    from ctc_asr_amd.model import to_oracle_layout
    bn = [(flat['rnn{}/bn_gamma'.format(i)], flat['rnn{}/bn_beta'.format(i)])
          for i in range(1, cfg.num_layers_rnn)]
    return ref.BatchNormRefModel(to_oracle_layout(flat, cfg), bn, cfg.used_model, cfg.rnn_cell,
                                 cfg.cudnn, decay=cfg.rnn_bn_decay)


def _reference_gradients(model_ref, cfg):
    grads = model_ref.grads_in_shared_layout()
    front = 'conv' if cfg.used_model == 'ds2' else 'dense'
    pairs = []
    for i, (gk, gb) in enumerate(grads[front]):
        pairs += [('{}{}/kernel'.format(front, i), gk), ('{}{}/bias'.format(front, i), gb)]
    for i, layer in enumerate(grads['rnn']):
        pairs += [('rnn{}/{}'.format(i, k), layer[k]) for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')]
        if i > 0:
            pairs += [('rnn{}/bn_gamma'.format(i), model_ref.bn_gamma[i - 1].grad),
                      ('rnn{}/bn_beta'.format(i), model_ref.bn_beta[i - 1].grad)]
    pairs += [('dense4/kernel', grads['dense4'][0]), ('dense4/bias', grads['dense4'][1]),
              ('logits/kernel', grads['logits'][0]), ('logits/bias', grads['logits'][1])]
    return pairs


def _logits_loss_and_gradients(cfg, flat, feats, flen, labels):
    from ctc_asr_amd.model import CTCModel
    model = CTCModel(cfg, DEV, params=flat)
    logits, seq_len = model.inference_fn(torch.tensor(feats), torch.tensor(flen), training=True)
    loss = model.loss_fn(logits, seq_len, labels)
    model.backward()
    torch.cuda.synchronize()

    model_ref = _reference(cfg, flat)
    t_logits, t_len = model_ref(torch.tensor(feats, dtype=torch.float64), flen)
    t_loss, _ = model_ref.loss(t_logits, t_len, labels)
    t_loss.backward()
    assert (seq_len.cpu().numpy() == t_len.numpy()).all()
    err = np.abs(logits.cpu().numpy() - t_logits.detach().numpy()).max()
    print('max |logits - ref| {:.3g}, loss {:.6f} against {:.6f}'.format(
        err, float(loss), float(t_loss.detach())))
    assert err < 1e-3
    assert abs(float(loss) - float(t_loss)) < 1e-3
    got = model.arena.export('grad')
    pairs = _reference_gradients(model_ref, cfg)
    assert {name for name, _ in pairs} == set(got)
    for name, ref_g in pairs:
        ref_g = ref_g.numpy()
        err = np.abs(got[name] - ref_g).max()
        print('{}: max |grad - ref| {:.3g}, max |ref| {:.3g}'.format(name, err,
                                                                     np.abs(ref_g).max()))
        assert err < 1e-3 * max(1.0, np.abs(ref_g).max()), (name, err)
        assert np.abs(got[name]).max() > 0, name
    # the running statistics have moved, by the batch's own
    for i, (run_mean, run_var) in enumerate(model_ref.running):
        state = model.bn_state[i].cpu().numpy().astype(np.float64)
        assert np.abs(state[0] - run_mean.numpy()).max() < 1e-5 * max(1.0, float(run_mean.abs().max()))
        assert np.abs(state[1] - run_var.numpy()).max() < 1e-5 * max(1.0, float(run_var.abs().max()))
        assert np.abs(state[0]).max() > 0 and (state[1] != 1.0).all()
    return model


def test_a_masked_batch_on_the_streaming_kernels():
    """(a) two rows of 41 frames, lengths 41 and 30: rows past a length are not counted."""
    cfg = _streaming_cfg(rnn_batch_norm=True)
    model = _logits_loss_and_gradients(cfg, _params(cfg, 0), *_streaming_batch())
    assert model._acts['rnn_len'] is not None and model._acts['bn_saved'][0] is None
    assert model._acts['bn_saved'][1] is not None


def test_the_persistent_shape(hip):
    """(b) ds2, two convolutions, 2 x LSTM-1024, 16 rows of 17 frames, T' = 9: the persistent
    recurrences; the paths that step aside for a dropout between the layers step aside here."""
    cfg = _persistent_cfg(rnn_batch_norm=True)
    assert hip.rnn_persistent_supported('lstm', 9, 16, 1024)
    model = _logits_loss_and_gradients(cfg, _params(cfg, 1), *_persistent_batch())
    model.check_rnn_error()
    acts = model._acts
    assert acts['t_out'] == 9 and acts['rnn_len'] is None
    assert acts['layer_in'][1] is not acts['layer_out'][0]
    assert not model._pipeline_forward(0, 'lstm', 64, 16, 1024, None, 0.0)
    assert model._predicted_bounds(True)[1] is None
    assert model.arithmetic()['rnn1/input_projection'] in ('fp16x3 (row / column scales)',
                                                           'bf16x6', 'fp32')


def test_training_steps_running_statistics_checkpoint_and_dropped_step(hip, tmp_path):
    """(c) three `Trainer.train_step`s against three TF-form Adam steps of the restatement, then
    evaluation with the running statistics; (d) a checkpoint carries them; (e) a dropped update
    leaves gamma and beta alone (the running statistics have moved in its forward pass)."""
    from ctc_asr_amd import storage
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.model import CTCModel
    from oracle import torch_ref
    cfg = _streaming_cfg(rnn_batch_norm=True, rnn_bn_decay=0.9)
    flat = _params(cfg, 2)
    feats, flen, labels = _streaming_batch(4)
    trainer = Trainer(cfg, device=DEV, params=flat)
    trainer.lr = 1e-3
    model = trainer.model
    model_ref = _reference(cfg, flat)
    opt = torch_ref.TFAdam(model_ref.parameters(), lr=1e-3)
    t_feats = torch.tensor(feats, dtype=torch.float64)
    for _ in range(3):
        loss = trainer.train_step(torch.tensor(feats), torch.tensor(flen), labels)
        opt.zero_grad()
        t_logits, t_len = model_ref(t_feats, flen)
        t_loss, _ = model_ref.loss(t_logits, t_len, labels)
        t_loss.backward()
        opt.step()
        print('loss {:.6f} against {:.6f}'.format(float(loss), float(t_loss)))
        assert abs(float(loss) - float(t_loss)) < 1e-3
    trainer.drain_checks()
    state = model.bn_state.cpu().numpy().astype(np.float64)
    for k in range(2):
        want = model_ref.running[0][k].numpy()
        err = np.abs(state[0, k] - want)
        print('running {}: max error {:.3g}'.format(('mean', 'variance')[k], err.max()))
        assert (err <= 1e-5 * np.maximum(1.0, np.abs(want))).all()
    gamma = model.arena.export('param')['rnn1/bn_gamma']
    assert np.abs(gamma - model_ref.bn_gamma[0].detach().numpy()).max() < 1e-4
    assert np.abs(gamma - flat['rnn1/bn_gamma']).max() > 1e-4           # it has been trained

    # evaluation: the running statistics, twice the same bits, and the restatement's
    before = model.bn_state.clone()
    first, _ = model.inference_fn(torch.tensor(feats), torch.tensor(flen), training=False)
    first = first.clone()
    second, _ = model.inference_fn(torch.tensor(feats), torch.tensor(flen), training=False)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert torch.equal(before, model.bn_state)
    model_ref.bn_training = False
    with torch.no_grad():
        t_logits, _ = model_ref(t_feats, flen)
    assert np.abs(first.cpu().numpy() - t_logits.numpy()).max() < 1e-3
    model_ref.bn_training = True
    with torch.no_grad():
        t_train, _ = model_ref(t_feats, flen)
    assert np.abs(t_train.numpy() - t_logits.numpy()).max() > 1e-2      # the modes differ

    # (d) save, restore into a fresh model
    path = trainer.save_checkpoint(str(tmp_path), 1)
    other = CTCModel(cfg, DEV, seed=9)
    assert not torch.equal(other.bn_state, model.bn_state)
    storage.restore_checkpoint(path, other)
    assert torch.equal(other.bn_state.view(torch.int32), model.bn_state.view(torch.int32))
    logits, _ = other.inference_fn(torch.tensor(feats), torch.tensor(flen), training=False)
    assert torch.equal(logits.view(torch.int32), first.view(torch.int32))
    with pytest.raises(ValueError, match='different network layout'):
        storage.restore_checkpoint(path, CTCModel(_streaming_cfg(), DEV, seed=9))

    # (e) 41 output steps cannot carry 45 labels: the update is dropped on the device
    names = ('rnn1/bn_gamma', 'rnn1/bn_beta')
    kept = [model.arena.p[name].clone() for name in names]
    moments = model.arena.m.clone()
    state = model.bn_state.clone()
    assert trainer.skipped_step_count() == 0
    trainer.train_step(torch.tensor(feats), torch.tensor(flen),
                       [list(range(1, 28)) + list(range(1, 19)), [4, 5]], check=False)
    torch.cuda.synchronize()
    for name, want in zip(names, kept):
        assert torch.equal(model.arena.p[name].view(torch.int32), want.view(torch.int32)), name
    assert torch.equal(model.arena.m, moments)
    assert trainer.skipped_step_count() == 1
    assert not torch.equal(model.bn_state, state) and torch.isfinite(model.bn_state).all()
    with pytest.warns(RuntimeWarning, match='dropped on the device'):
        trainer.drain_checks()


def test_accumulated_micro_batches_are_a_sum(hip):
    """(f) two micro-batches with ``accumulate=True`` against the sum of two passes."""
    from ctc_asr_amd.model import CTCModel
    cfg = _streaming_cfg(rnn_batch_norm=True)
    flat = _params(cfg, 5)
    batch_a = [torch.tensor(v) if isinstance(v, np.ndarray) else v for v in _streaming_batch(6)]
    batch_b = [torch.tensor(v) if isinstance(v, np.ndarray) else v for v in _streaming_batch(7)]
    model = CTCModel(cfg, DEV, params=flat)
    model.forward_backward(*batch_a)
    grad_a = model.arena.grad.clone()
    model.forward_backward(*batch_b)
    want = (grad_a + model.arena.grad).cpu().numpy().astype(np.float64)
    model.arena.grad.fill_(123.0)                    # the first pass clears, the second adds
    model.forward_backward(*batch_a)
    model.forward_backward(*batch_b, accumulate=True)
    torch.cuda.synchronize()
    got = model.arena.grad.cpu().numpy().astype(np.float64)
    limit = GRAD_TOL * max(1.0, np.abs(want).max())
    for name in ('rnn1/bn_gamma', 'rnn1/bn_beta'):
        start = model.arena.offsets[name]
        stop = start + 2 * cfg.num_units_rnn
        err = np.abs(got[start:stop] - want[start:stop]).max()
        print('{}: max |accumulated - sum| {:.3g} against {:.3g}'.format(name, err, limit))
        assert np.abs(want[start:stop]).max() > 0 and err < limit
    assert np.abs(got - want).max() < limit


def test_the_flag_off_is_the_model_without_the_flag(hip):
    """(g) bit-equal logits and gradients, no new parameter, no state."""
    from ctc_asr_amd.model import CTCModel
    feats, flen, labels = _persistent_batch(2)
    out = []
    for kwargs in ({}, dict(rnn_batch_norm=False, rnn_bn_decay=0.5)):
        cfg = _persistent_cfg(**kwargs)
        model = CTCModel(cfg, DEV, seed=4)
        assert model.bn_state is None and not any('bn_' in n for n in model.arena.offsets)
        logits, _ = model.inference_fn(torch.tensor(feats), torch.tensor(flen), training=True)
        assert all(saved is None for saved in model._acts['bn_saved'])
        out.append((logits.clone(), model.arena.size, model.arithmetic()))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert out[0][1:] == out[1][1:]
