"""The parts of gradient clipping that need no GPU: the float64 reference of the norm kernel
against exactly rounded sums, the two flags, and how `engine.Trainer` reads them."""

import math
import os
import re
import types

import numpy as np
import pytest

from tests import gradnorm_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mixed(rng, n):
    """Normal deviates with a few 3e19 (their squares overflow float32), runs of 1e-30 (their
    squares underflow it) and exact zeros."""
    x = rng.normal(size=n).astype(np.float32)
    x[1::5] = 0.0
    x[2::97] = 1e-30
    x[rng.permutation(n)[:min(3, n)]] = 3e19
    return x


@pytest.mark.parametrize('n', [1, 3, 4, 5, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1,
                               2 * ref.CHUNK + 3, 70 * ref.CHUNK + 13])
def test_the_fixed_order_sums_are_within_an_ulp_of_the_exact_ones(n):
    rng = np.random.default_rng(n)
    cut = (n // 3) & ~3
    offsets = [0, cut, cut, n]
    for x in (rng.normal(size=n).astype(np.float32), _mixed(rng, n)):
        for scale in (1.0, 1.0 / 8):
            got, _ = ref.grad_norm(x, offsets, scale)
            want = ref.exact_norms(x, offsets, scale)
            assert np.isfinite(got).all() and got[1] == 0.0
            assert ref.ulps32(got, want).max() <= 1, (n, scale, got, want)
    # the float64 sum itself: a relative error far below one float32 ulp (2^-24)
    x = rng.normal(size=n).astype(np.float32)
    exact = math.fsum(x.astype(np.float64) ** 2)
    assert abs(ref.segment_sum(x) - exact) <= exact * 2.0 ** -45


def test_small_and_huge_values_survive_the_float64_squares():
    tiny = np.full(16, 1e-30, dtype=np.float32)
    norms, _ = ref.grad_norm(tiny, [0, 16])
    assert norms[0] == np.float32(4e-30) and norms[1] == norms[0]
    huge = np.array([3e19, 0, 0, 3e19], dtype=np.float32)
    norms, factor = ref.grad_norm(huge, [0, 4], max_norm=1.0)
    assert np.isfinite(norms).all()
    assert ref.ulps32(norms, ref.exact_norms(huge, [0, 4])).max() <= 1
    assert factor == np.float32(1.0) / norms[1]


def test_a_segment_does_not_depend_on_where_it_sits():
    rng = np.random.default_rng(7)
    seg = rng.normal(size=ref.CHUNK + 8).astype(np.float32)
    alone, _ = ref.grad_norm(seg, [0, seg.size])
    x = np.concatenate([rng.normal(size=12).astype(np.float32), seg,
                        rng.normal(size=5).astype(np.float32)])
    inside, _ = ref.grad_norm(x, [0, 12, 12, 12 + seg.size, x.size])
    assert inside[2].view(np.uint32) == alone[0].view(np.uint32) and inside[1] == 0.0


def test_factor_and_non_finite_norms():
    one = np.float32(1.0)
    assert ref.clip_factor(2.0, 0.0) == one and ref.clip_factor(2.0, -1.0) == one
    assert ref.clip_factor(2.0, 2.0) == one and ref.clip_factor(0.0, 1.0) == one
    below = np.nextafter(np.float32(2.0), np.float32(0))
    assert ref.clip_factor(2.0, below) == below / np.float32(2.0) < one
    assert ref.clip_factor(np.inf, 0.0) == 0.0 and ref.clip_factor(np.nan, 5.0) == 0.0
    x = np.ones(12, dtype=np.float32)
    x[5] = np.nan
    norms, factor = ref.grad_norm(x, [0, 4, 8, 12], max_norm=1.0)
    assert norms[0] == 2.0 and norms[2] == 2.0 and np.isnan(norms[1]) and np.isnan(norms[3])
    assert factor == 0.0
    x[5] = np.inf
    norms, factor = ref.grad_norm(x, [0, 4, 8, 12])
    assert norms[0] == 2.0 and np.isposinf(norms[1]) and np.isposinf(norms[3]) and factor == 0.0
    zeros, factor = ref.grad_norm(np.zeros(9, dtype=np.float32), [0, 4, 9], max_norm=1.0)
    assert not zeros.any() and factor == one


def test_offset_tables_are_clamped_into_the_vector():
    assert ref.sanitize_offsets([0, 8, 8, 21], 21) == [0, 8, 8, 21]
    assert ref.sanitize_offsets([0, 100, 40, 64], 64) == [0, 64, 64, 64]
    assert ref.sanitize_offsets([-5, 10 ** 12, 7, 90], 50) == [0, 48, 48, 50]
    assert ref.sanitize_offsets([3, 7, 30], 21) == [0, 4, 21]


def test_the_binding_exports_the_constants_of_the_header():
    from ctc_asr_amd import hip
    text = open(os.path.join(ROOT, 'include', 'ctcasr.h')).read()
    defines = dict(re.findall(r'#define (CTCASR_GRAD_NORM_[A-Z_]+) (\d+)', text))
    assert int(defines['CTCASR_GRAD_NORM_CHUNK']) == hip.GRAD_NORM_CHUNK == ref.CHUNK
    assert int(defines['CTCASR_GRAD_NORM_MAX_SEGMENTS']) == hip.GRAD_NORM_MAX_SEGMENTS \
        == ref.MAX_SEGMENTS >= 64
    for name in ('ctcasr_grad_norm', 'ctcasr_grad_norm_workspace_bytes',
                 'ctcasr_adam_step_clipped'):
        assert name in hip.SIGNATURES


def test_flags_parse_and_show_in_the_summary_only_when_set():
    from ctc_asr_amd import params
    flags = params.FLAGS
    flags.reset()
    try:
        assert flags.max_grad_norm == 0.0 and flags.report_grad_norms is False
        plain = params.get_parameters()
        assert 'max_grad_norm' not in plain
        flags.parse(['--max_grad_norm=400', '--report_grad_norms'])
        assert flags.max_grad_norm == 400.0 and flags.report_grad_norms is True
        shown = params.get_parameters()
        assert 'max_grad_norm=400.0' in shown and 'report_grad_norms=True' in shown
        assert shown.startswith(plain)
        flags.parse(['--noreport_grad_norms', '--max_grad_norm', '0.5'])
        assert flags.max_grad_norm == 0.5 and flags.report_grad_norms is False
        assert 'max_grad_norm=0.5' in params.get_parameters()
    finally:
        flags.reset()


def test_trainer_reads_the_switches_with_defaults(monkeypatch):
    """From ``flags`` by `getattr` (a bare object has neither: both off), overridden by the keyword
    arguments.  The model and the reducer are stand-ins: nothing here touches a device."""
    from ctc_asr_amd import engine

    class Model:
        def __init__(self, *args, **kwargs):
            self.arena = types.SimpleNamespace(grad=None, param=None)

    monkeypatch.setattr(engine, 'CTCModel', Model)
    monkeypatch.setattr(engine, 'GradientReducer', lambda *args, **kwargs: None)
    cfg = types.SimpleNamespace(cell='lstm', num_units_rnn=64)

    def build(flags=None, **kwargs):
        return engine.Trainer(cfg, flags=flags, device='cpu', **kwargs)

    for trainer in (build(), build(object()), build(types.SimpleNamespace(learning_rate=1e-3))):
        assert trainer.max_grad_norm == 0.0 and trainer.report_grad_norms is False
        assert trainer.last_grad_norms is None and trainer.last_clip_factor is None
        assert trainer.clipped_step_count() == 0
    flags = types.SimpleNamespace(max_grad_norm=25, report_grad_norms=True)
    trainer = build(flags)
    assert trainer.max_grad_norm == 25.0 and trainer.report_grad_norms is True
    trainer = build(flags, max_grad_norm=0.0, report_grad_norms=False)
    assert trainer.max_grad_norm == 0.0 and trainer.report_grad_norms is False
    trainer = build(max_grad_norm=3.5)
    assert trainer.max_grad_norm == 3.5 and trainer.report_grad_norms is False
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    assert build(FLAGS).max_grad_norm == 0.0 and build(FLAGS).report_grad_norms is False
