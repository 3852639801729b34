"""Gradient clipping through `CTCModel` and `engine.Trainer` on the tiny model.

Two runs of a training step do not give bit-identical gradients (the bias sums use atomics), so
every check is made WITHIN one model, from the gradient arena the step itself left behind:
`CTCModel.backward` clears `arena.grad` at its start and Adam only reads it
(`test_adam_leaves_the_gradients_of_the_step_in_the_arena` confirms that first).  Parameters and
moments are snapshotted before the step; afterwards the norms are recomputed from `arena.grad` in
float64 and a plain `hip.adam_step` with the expected float32 scale is applied to the snapshots.
Parameters and moments must then match bit for bit, the norms within one float32 ulp
(tests/test_gpu_grad_norm.py derives that bound)."""

import numpy as np
import pytest
import torch

from tests import gradnorm_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _cfg():
    from ctc_asr_amd.model import ModelConfig
    return ModelConfig(num_units_rnn=64, num_layers_rnn=1, num_units_dense=32)


def _batch(seed=3):
    rng = np.random.default_rng(seed)
    feats = torch.tensor(rng.normal(size=(2, 21, 80)).astype(np.float32))
    return feats, torch.tensor([21, 21], dtype=torch.int32), [[1, 2, 3], [4, 5]]


def _trainer(**kwargs):
    from ctc_asr_amd.engine import Trainer
    return Trainer(_cfg(), device=DEV, seed=3, **kwargs)


def _snapshot(trainer):
    a = trainer.model.arena
    return a.param.clone(), a.m.clone(), a.v.clone()


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _table(model):
    slices = model.arena.layer_slices
    return [slices[0][1]] + [stop for _, _, stop in slices]


def _verify_step(hip, trainer, snapshot, max_norm):
    """The step that has just run, re-derived from its own gradients; returns (norms, factor) as
    the trainer holds them."""
    torch.cuda.synchronize()
    model, a = trainer.model, trainer.model.arena
    grad = a.grad.cpu().numpy()
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    norms = trainer.last_grad_norms.cpu().numpy()
    factor = trainer.last_clip_factor.cpu().numpy()[0]
    table = _table(model)
    assert table[0] == 0 and table[-1] == a.size == a.grad.numel()
    assert len(model.grad_norm_names) + 1 == trainer.last_grad_norms.numel() == len(table)
    assert model.grad_norm_names == [name for name, _, _ in a.layer_slices]
    want = ref.exact_norms(grad, table, 1.0 / trainer.world)
    assert ref.ulps32(norms, want).max() <= 1, (norms, want)
    assert norms[-1] > 0
    expect = ref.clip_factor(norms[-1], max_norm)
    assert np.float32(factor).view(np.uint32) == expect.view(np.uint32), (factor, expect)
    scale = float(np.float32(1.0 / trainer.world) * expect)
    p, m, v = (t.clone() for t in snapshot)
    hip.adam_step(p, a.grad, m, v, model.step_count, trainer.lr, trainer.beta1, trainer.beta2,
                  trainer.eps, grad_scale=scale)
    assert _bits_equal(p, a.param) and _bits_equal(m, a.m) and _bits_equal(v, a.v)
    assert not _bits_equal(a.param, snapshot[0])
    return norms, factor


def test_adam_leaves_the_gradients_of_the_step_in_the_arena(hip):
    """What every check below relies on."""
    trainer = _trainer()
    feats, flen, labels = _batch()
    model = trainer.model
    model.forward_backward(feats, flen, labels)
    grad = model.arena.grad.clone()
    assert float(grad.abs().max()) > 0
    model.apply_gradients(1e-3)
    assert _bits_equal(grad, model.arena.grad)
    model.arena.grad.fill_(123.0)           # stale values do not leak into the next step
    model.forward_backward(feats, flen, labels)
    torch.cuda.synchronize()
    assert float(model.arena.grad.abs().max()) < 123.0


def test_a_bound_nobody_reaches_then_half_the_measured_norm(hip):
    trainer = _trainer(max_grad_norm=1e30)
    assert trainer.last_grad_norms is None and trainer.clipped_step_count() == 0
    feats, flen, labels = _batch()
    snapshot = _snapshot(trainer)
    trainer.train_step(feats, flen, labels)
    norms, factor = _verify_step(hip, trainer, snapshot, 1e30)
    assert factor == 1.0 and trainer.clipped_step_count() == 0
    # the same batch again, one tiny update later: its norm is close to the one just measured, so
    # half of that clips with a factor near 0.5 - what it is exactly, _verify_step pins
    trainer.max_grad_norm = float(norms[-1]) / 2
    snapshot = _snapshot(trainer)
    trainer.train_step(feats, flen, labels)
    norms, factor = _verify_step(hip, trainer, snapshot, trainer.max_grad_norm)
    assert 0.25 < factor < 1.0
    assert trainer.clipped_step_count() == 1 and trainer.skipped_step_count() == 0
    trainer.drain_checks()


def test_report_alone_fills_the_norms_and_changes_no_update(hip):
    trainer = _trainer(report_grad_norms=True)
    assert trainer.max_grad_norm == 0.0
    feats, flen, labels = _batch()
    for _ in range(2):
        snapshot = _snapshot(trainer)
        trainer.train_step(feats, flen, labels)
        norms, factor = _verify_step(hip, trainer, snapshot, 0.0)       # plain Adam, scale 1
        assert factor == 1.0
    assert trainer.clipped_step_count() == 0
    model = trainer.model
    assert len(model.grad_norm_names) + 1 == trainer.last_grad_norms.numel()
    assert model.grad_norm_names[0] == 'conv0' and 'rnn0' in model.grad_norm_names
    # the global norm is the norm of the layer norms
    assert float(norms[-1]) == pytest.approx(float(np.sqrt((norms[:-1].astype(np.float64) ** 2)
                                                           .sum())), rel=1e-6)
    trainer.drain_checks()


def test_flags_switch_it_on(hip):
    import types
    trainer = _trainer(flags=types.SimpleNamespace(max_grad_norm=1e-3, report_grad_norms=False))
    feats, flen, labels = _batch()
    snapshot = _snapshot(trainer)
    trainer.train_step(feats, flen, labels)
    norms, factor = _verify_step(hip, trainer, snapshot, 1e-3)
    assert factor < 1.0 and trainer.clipped_step_count() == 1


def test_the_norm_is_taken_behind_the_all_reduce(hip):
    """`force_reducer=True` puts the real bucketed all-reduce under the backward pass of one rank
    (a one-rank sum is the identity): the step must still be the step its own gradients give."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group('gloo', store=dist.HashStore(), rank=0, world_size=1)
    try:
        trainer = _trainer(max_grad_norm=1e-3, force_reducer=True, bucket_bytes=1 << 16)
        assert trainer.reducer.active
        feats, flen, labels = _batch()
        for _ in range(2):
            snapshot = _snapshot(trainer)
            trainer.train_step(feats, flen, labels)
            norms, factor = _verify_step(hip, trainer, snapshot, 1e-3)
            assert factor < 1.0
        assert trainer.reducer.launched > 0 and trainer.clipped_step_count() == 2
        trainer.drain_checks()
    finally:
        dist.destroy_process_group()


def test_a_non_finite_norm_drops_the_update_on_the_device(hip):
    """No kernel is made to misbehave: one inf is written into the gradient arena."""
    trainer = _trainer()
    model, a = trainer.model, trainer.model.arena
    feats, flen, labels = _batch()
    model.forward_backward(feats, flen, labels)
    a.grad[a.size // 2] = float('inf')
    snapshot = _snapshot(trainer)
    guard = model.step_guard()
    assert guard.tolist()[0] == 0
    second = int(guard[1])
    norms, factor = model.grad_norms(1.0, 1.0, guard)
    model.apply_gradients(1e-3, skip=guard, grad_factor=factor)
    torch.cuda.synchronize()
    assert guard.tolist() == [1, second] and float(factor) == 0.0
    assert torch.isposinf(norms[-1]) and int(torch.isinf(norms[:-1]).sum()) == 1
    for got, want in zip((a.param, a.m, a.v), snapshot):
        assert _bits_equal(got, want)
    # a finite arena again: the word stays raised (never cleared here), the norms are finite
    a.grad[a.size // 2] = 0.0
    norms, factor = model.grad_norms(1.0, 0.0, guard)
    assert guard.tolist()[0] == 1 and torch.isfinite(norms).all() and float(factor) == 1.0


def test_the_trainer_names_the_gradient_norm_when_it_raises(hip, monkeypatch):
    from ctc_asr_amd.engine import NanLossDuringTrainingError
    trainer = _trainer(report_grad_norms=True)
    model, a = trainer.model, trainer.model.arena
    feats, flen, labels = _batch()
    trainer.train_step(feats, flen, labels)
    trainer.drain_checks()
    snapshot = _snapshot(trainer)
    real = model.forward_backward

    def poisoned(*args, **kwargs):
        loss = real(*args, **kwargs)
        a.grad[7] = float('nan')
        return loss

    monkeypatch.setattr(model, 'forward_backward', poisoned)
    loss = trainer.train_step(feats, flen, labels)       # does not raise here: deferred
    monkeypatch.setattr(model, 'forward_backward', real)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for got, want in zip((a.param, a.m, a.v), snapshot):
        assert _bits_equal(got, want)
    assert torch.isnan(trainer.last_grad_norms[-1]) and float(trainer.last_clip_factor) == 0.0
    with pytest.raises(NanLossDuringTrainingError,
                       match='non-finite gradient norm in training step 2; its update was not '
                             'applied'):
        trainer.drain_checks()
    with pytest.warns(RuntimeWarning, match='dropped on the device'):
        trainer.drain_checks()
    assert trainer.skipped_step_count() == 1 and trainer.clipped_step_count() == 0
    assert model.step_count == 1
    snapshot = _snapshot(trainer)
    trainer.train_step(feats, flen, labels)             # a clean step moves them again
    _verify_step(hip, trainer, snapshot, 0.0)
    trainer.drain_checks()


def test_both_switches_off_launch_nothing_new(hip, monkeypatch):
    hip.load()
    calls = []
    real = hip.grad_norm
    monkeypatch.setattr(hip, 'grad_norm', lambda *a, **k: calls.append(1) or real(*a, **k))
    trainer = _trainer()
    assert trainer.max_grad_norm == 0.0 and trainer.report_grad_norms is False
    feats, flen, labels = _batch()
    snapshot = _snapshot(trainer)
    trainer.train_step(feats, flen, labels)
    trainer.train_step(feats, flen, labels, check=False)
    trainer.drain_checks()
    assert trainer.last_grad_norms is None and trainer.last_clip_factor is None
    assert trainer.clipped_step_count() == 0 and not calls
    assert trainer.model._grad_norm_state is None
    assert not _bits_equal(trainer.model.arena.param, snapshot[0])
    # the spy does see a call once a switch is on
    trainer.report_grad_norms = True
    trainer.train_step(feats, flen, labels)
    assert calls == [1] and trainer.last_grad_norms is not None
    trainer.drain_checks()
