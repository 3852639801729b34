"""The host side of the training schedule: `params.learning_rate_at`, the flags around it, the
EMA decay of `params.ema_decay_at`, the summary row, and the averaged parameters' way through a
checkpoint (on CPU tensors: `storage` only copies)."""

import json
import math
import os
import types

import numpy as np
import pytest
import torch

from ctc_asr_amd import params, storage
from ctc_asr_amd.params import FLAGS, ema_alpha_at, ema_decay_at, learning_rate_at
from tests import adam_ema_reference as ref

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'reference_python.json')))


@pytest.fixture(autouse=True)
def _fresh_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def _flags(**kwargs):
    base = dict(learning_rate=1e-3, learning_rate_decay_factor=0.5, steps_per_decay=4,
                minimum_lr=1e-5, lr_schedule='constant', lr_warmup_steps=0, lr_total_steps=0)
    base.update(kwargs)
    return types.SimpleNamespace(**base)


def test_constant_is_the_flag_itself():
    assert learning_rate_at(1) is FLAGS.learning_rate
    flags = _flags()
    for update in (1, 2, 75000, 10 ** 9):
        assert learning_rate_at(update, flags) is flags.learning_rate
    with pytest.raises(ValueError):
        learning_rate_at(0, flags)


def test_staircase():
    flags = _flags(lr_schedule='staircase')
    s = flags.steps_per_decay
    assert learning_rate_at(1, flags) == 1e-3
    assert learning_rate_at(s, flags) == 1e-3
    assert learning_rate_at(s + 1, flags) == 1e-3 * 0.5
    assert learning_rate_at(2 * s + 1, flags) == 1e-3 * 0.5 ** 2
    # 1e-3 * 0.5^7 = 7.8e-6 is below the floor: updates from 7 s + 1 on stay at minimum_lr
    assert learning_rate_at(6 * s + 1, flags) == 1e-3 * 0.5 ** 6 > 1e-5
    for update in (7 * s + 1, 100 * s, 10 ** 7):
        assert learning_rate_at(update, flags) == 1e-5
    # the reference's defaults: what the formerly inert flags now say
    FLAGS.update(lr_schedule='staircase')
    assert learning_rate_at(75000) == 1e-5
    assert learning_rate_at(75001) == max(1e-6, 1e-5 * 0.8)
    assert learning_rate_at(75000 * 40 + 1) == 1e-6


def test_cosine():
    flags = _flags(lr_schedule='cosine', lr_total_steps=101)
    assert learning_rate_at(1, flags) == pytest.approx(1e-3, rel=1e-15)
    assert learning_rate_at(51, flags) == pytest.approx((1e-3 + 1e-5) / 2, rel=1e-12)   # midpoint
    assert learning_rate_at(101, flags) == 1e-5
    assert learning_rate_at(102, flags) == 1e-5
    rates = [learning_rate_at(u, flags) for u in range(1, 103)]
    assert all(a >= b for a, b in zip(rates, rates[1:]))
    for total in (0, -3):
        with pytest.raises(ValueError, match='lr_total_steps'):
            learning_rate_at(1, _flags(lr_schedule='cosine', lr_total_steps=total))
    with pytest.raises(ValueError):
        learning_rate_at(1, _flags(lr_schedule='linear'))


@pytest.mark.parametrize('schedule', ['constant', 'staircase', 'cosine'])
def test_warm_up_multiplies_any_schedule(schedule):
    w = 8
    plain = _flags(lr_schedule=schedule, lr_total_steps=40)
    warm = _flags(lr_schedule=schedule, lr_total_steps=40, lr_warmup_steps=w)
    assert learning_rate_at(1, warm) == learning_rate_at(1, plain) * (1.0 / w)
    assert learning_rate_at(3, warm) == learning_rate_at(3, plain) * (3.0 / w)
    assert learning_rate_at(w, warm) == learning_rate_at(w, plain)
    assert learning_rate_at(w + 1, warm) == learning_rate_at(w + 1, plain)
    assert learning_rate_at(1, warm) < learning_rate_at(2, warm) < learning_rate_at(w, plain) * 1.01


def test_bad_values_are_refused_when_parsed():
    for argv in (['--lr_schedule=linear'], ['--lr_schedule', ''], ['--lr_warmup_steps=-1'],
                 ['--grad_accum_steps=0'], ['--grad_accum_steps=1025'], ['--ema_decay=1.0'],
                 ['--ema_decay=-0.1'], ['--ema_decay=nan'], ['--grad_accum_steps=two']):
        FLAGS.reset()
        with pytest.raises(ValueError):
            FLAGS.parse(argv)
    with pytest.raises(ValueError):
        FLAGS.update(ema_decay=1.5)
    FLAGS.reset()
    assert FLAGS.parse(['--lr_schedule=cosine', '--lr_warmup_steps=0', '--lr_total_steps', '9',
                        '--grad_accum_steps=1024', '--ema_decay=0.9999', '--eval_ema']) == []
    assert (FLAGS.lr_schedule, FLAGS.lr_total_steps, FLAGS.grad_accum_steps, FLAGS.ema_decay,
            FLAGS.eval_ema) == ('cosine', 9, 1024, 0.9999, True)


def test_defaults_are_off_and_the_decay_flags_say_what_they_do():
    defaults = FLAGS.defaults_dict()
    assert (defaults['lr_schedule'], defaults['lr_warmup_steps'], defaults['lr_total_steps'],
            defaults['grad_accum_steps'], defaults['ema_decay'], defaults['eval_ema']) == \
        ('constant', 0, 0, 1, 0.0, False)
    for name in ('learning_rate_decay_factor', 'steps_per_decay', 'minimum_lr'):
        assert 'inert' not in FLAGS._flags[name].help
        assert defaults[name] == GOLD['flags'][name]


@pytest.mark.parametrize('decay', [0.9, 0.9999])
def test_decay_t(decay):
    want = {0: min(decay, 1 / 10), 1: min(decay, 2 / 11), 89: min(decay, 90 / 99),
            90: min(decay, 91 / 100), 10 ** 6: min(decay, (1 + 1e6) / (10 + 1e6))}
    for k, value in want.items():
        assert ema_decay_at(decay, k) == value == ref.decay_t(decay, k)
        assert ema_alpha_at(decay, k) == 1.0 - value
        assert np.float32(ema_alpha_at(decay, k)) == ref.alpha32(decay, k)
    # 0.9: the ramp (1 + k) / (10 + k) passes 0.9 between k = 80 and 81 - capped from there on
    assert ema_decay_at(0.9, 80) == 0.9 and ema_decay_at(0.9, 79) == 80 / 89 < 0.9
    assert ema_decay_at(0.9, 89) == ema_decay_at(0.9, 90) == ema_decay_at(0.9, 10 ** 6) == 0.9
    # 0.9999: still on the ramp at 90, capped at 10^6 ((1 + k) / (10 + k) > 0.9999 from 89990)
    assert ema_decay_at(0.9999, 90) == 0.91 and ema_decay_at(0.9999, 10 ** 6) == 0.9999
    with pytest.raises(ValueError):
        ema_decay_at(decay, -1)


def test_the_summary_of_a_default_run_is_unchanged_line_for_line():
    assert params.get_parameters() == GOLD['get_parameters']
    lines = params.get_parameters().split('\n')
    for change in (dict(lr_schedule='staircase'), dict(lr_warmup_steps=10),
                   dict(grad_accum_steps=4), dict(ema_decay=0.999), dict(eval_ema=True)):
        FLAGS.reset()
        FLAGS.update(**change)
        got = params.get_parameters().split('\n')
        assert got[:-1] == lines and len(got) == len(lines) + 1
        assert got[-1].startswith('\tSchedule (') and got[-1].endswith(');')
        for name, value in change.items():
            assert '{}={}'.format(name.replace('lr_warmup', 'warmup'), value) in got[-1]


# ---- checkpoints -----------------------------------------------------------------------------
class _Arena:
    def __init__(self, n, ema, seed):
        gen = torch.Generator().manual_seed(seed)
        self.param, self.m, self.v = (torch.randn(n, generator=gen) for _ in range(3))
        self.ema = torch.randn(n, generator=gen) if ema else None
        self.shapes, self.offsets = {'w': (n,)}, {'w': 0}
        self.touched = 0

    def touch(self):
        self.touched += 1


def _model(n=37, ema=True, seed=0):
    return types.SimpleNamespace(arena=_Arena(n, ema, seed), step_count=11 + seed,
                                 dropout_seed=5 + seed)


def test_a_checkpoint_carries_the_average(tmp_path):
    src = _model(ema=True, seed=1)
    path = storage.save_checkpoint(str(tmp_path), src, epoch=3)
    assert torch.equal(torch.load(path, weights_only=False)['ema'], src.arena.ema)
    dst = _model(ema=True, seed=2)
    assert storage.restore_checkpoint(path, dst) == 3
    for name in ('param', 'm', 'v', 'ema'):
        assert torch.equal(getattr(dst.arena, name), getattr(src.arena, name)), name
    assert (dst.step_count, dst.dropout_seed, dst.arena.touched) == (12, 6, 1)
    # the averaged parameters in place of the trained ones; the arena's own average follows
    dst = _model(ema=True, seed=3)
    storage.restore_checkpoint(path, dst, weights='ema')
    assert torch.equal(dst.arena.param, src.arena.ema) and dst.arena.touched == 1
    assert torch.equal(dst.arena.ema, src.arena.ema)
    # ... also into a model that keeps none (evaluate / predict / align --eval_ema)
    dst = _model(ema=False, seed=4)
    storage.restore_checkpoint(path, dst, weights='ema')
    assert torch.equal(dst.arena.param, src.arena.ema) and dst.arena.ema is None
    dst = _model(ema=False, seed=5)
    storage.restore_checkpoint(path, dst)
    assert torch.equal(dst.arena.param, src.arena.param) and dst.arena.ema is None
    with pytest.raises(ValueError, match='weights'):
        storage.restore_checkpoint(path, dst, weights='average')


def test_a_checkpoint_without_an_average(tmp_path):
    src = _model(ema=False, seed=1)
    path = storage.save_checkpoint(str(tmp_path), src, epoch=1)
    assert 'ema' not in torch.load(path, weights_only=False)
    dst = _model(ema=False, seed=2)
    assert storage.restore_checkpoint(path, dst) == 1
    assert torch.equal(dst.arena.param, src.arena.param) and dst.arena.ema is None
    # --ema_decay switched on later: the average starts from the file's parameters
    dst = _model(ema=True, seed=3)
    storage.restore_checkpoint(path, dst)
    assert torch.equal(dst.arena.ema, src.arena.param)
    assert dst.arena.ema.data_ptr() != dst.arena.param.data_ptr()
    before = dst.arena.param.clone()
    with pytest.raises(ValueError, match=os.path.basename(path).replace('.', r'\.')):
        storage.restore_checkpoint(path, dst, weights='ema')
    assert torch.equal(dst.arena.param, before)         # refused before anything was copied


def test_reference_update_is_the_tensorflow_form():
    """assign_sub(ema, (1 - decay) * (ema - param)) and ema + alpha * (param - ema) agree."""
    rng = np.random.default_rng(0)
    ema, param = rng.normal(size=64), rng.normal(size=64)
    alpha = 1.0 - ref.decay_t(0.999, 500)
    assert np.allclose(ref.ema_update(ema, param, alpha), ema - alpha * (ema - param),
                       rtol=0, atol=1e-15)
    assert math.isclose(float(ref.alpha32(0.9, 10 ** 6)), 0.1, rel_tol=1e-7)
    assert (ref.ema_bound(np.float32([1.0]), np.float32([-2.0])) == 9 * 2.0 ** -24).all()
