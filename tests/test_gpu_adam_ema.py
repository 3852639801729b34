"""`ctcasr_adam_step_ema` through the C ABI: Adam and the parameters' exponential moving average
in one launch.

param, m and v are compared bit for bit with the plain call on copies of the same inputs (the
contract is an identity).  The average is compared with the float64 restatement of
tests/adam_ema_reference.py evaluated from the kernel's OWN float32 ``param_new``, elementwise
within 3 * 2^-24 * (|param_new| + |ema_old|): three float32 roundings - the difference, the
product, the sum - each at most half an ulp of a value no larger than that sum; a fused
multiply-add drops one of them, so the bound holds with or without contraction."""

import numpy as np
import pytest
import torch

from tests import adam_ema_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)
# one element, a tail only, one float4, float4 + tail, under / at one workgroup's 1024 floats,
# several workgroups with a tail, and more float4s than one pass of 256 workgroups
SIZES = [1, 3, 4, 5, 1023, 1024, 4099, 262144 + 7]


def _state(n, seed):
    """Device (param, grad, m, v, ema): gradients whose magnitudes span 1e-12 .. 1e3 with both
    signs and exact zeros, moments of a run in progress, an average near the parameters."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    exponent = torch.rand(n, device=DEV, generator=gen) * 15.0 - 12.0
    g = torch.pow(10.0, exponent) * torch.sign(torch.randn(n, device=DEV, generator=gen))
    g[0::13] = 0.0
    if n > 2:
        g[1], g[2] = 1e-12, -1e3
    m = torch.randn(n, device=DEV, generator=gen).mul_(1e-2)
    v = torch.rand(n, device=DEV, generator=gen).mul_(1e-3)
    p = torch.randn(n, device=DEV, generator=gen)
    p[5::11] = 0.0
    e = p + torch.randn(n, device=DEV, generator=gen).mul_(0.05)
    return p, g, m, v, e


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fused(hip, state, step, alpha, **kwargs):
    p, g, m, v, e = state
    p, m, v, e = p.clone(), m.clone(), v.clone(), e.clone()
    hip.adam_step(p, g, m, v, step, **HYPER, ema=e, ema_alpha=alpha, **kwargs)
    return p, m, v, e


def _plain(hip, state, step, **kwargs):
    p, g, m, v, _ = state
    p, m, v = p.clone(), m.clone(), v.clone()
    hip.adam_step(p, g, m, v, step, **HYPER, **kwargs)
    return p, m, v


def _check_ema(ema_new, ema_old, param_new, alpha, slack=1.0):
    want = ref.ema_update(ema_old.cpu().numpy(), param_new.cpu().numpy(), np.float32(alpha))
    bound = slack * ref.ema_bound(ema_old.cpu().numpy(), param_new.cpu().numpy())
    err = np.abs(ema_new.cpu().numpy().astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print('ema error / bound: {:.3f}'.format(worst))
    assert (err <= bound).all(), worst


@pytest.mark.parametrize('n', SIZES)
def test_param_and_moments_are_the_plain_call_bit_for_bit_and_the_ema_is_within_its_bound(hip, n):
    state = _state(n, n % 997)
    grad_before = state[1].clone()
    for step in (1, 1000):
        for factor in (None, 0.37):
            extra = {} if factor is None else \
                {'grad_factor': torch.tensor([factor], dtype=torch.float32, device=DEV)}
            for alpha in (0.9, 1e-4):
                got = _fused(hip, state, step, alpha, grad_scale=0.5, **extra)
                want = _plain(hip, state, step, grad_scale=0.5, **extra)
                for name, a, b in zip('pmv', got, want):
                    assert _bits(a, b), (n, step, factor, name)
                assert not _bits(got[0], state[0]) or n < 3
                _check_ema(got[3], state[4], got[0], alpha)
    assert torch.equal(state[1], grad_before)


def test_fifty_updates_track_the_float64_recursion(hip):
    n, decay = 4099, 0.9
    p, g, m, v, e = (t.clone() for t in _state(n, 7))
    exact = e.cpu().numpy().astype(np.float64)
    budget = np.zeros(n)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for k in range(50):
        g = torch.randn(n, device=DEV, generator=gen)
        alpha = ref.alpha32(decay, k)
        ema_old = e.cpu().numpy()
        hip.adam_step(p, g, m, v, k + 1, **HYPER, ema=e, ema_alpha=float(alpha))
        exact = ref.ema_update(exact, p.cpu().numpy(), alpha)
        budget = np.maximum(budget, ref.ema_bound(ema_old, p.cpu().numpy()))
    err = np.abs(e.cpu().numpy().astype(np.float64) - exact)
    print('50 updates, error / (50 x bound): {:.4f}'.format(float((err / (50 * budget)).max())))
    assert (err <= 50 * budget).all()
    assert float((e - p).abs().max()) > 0


def test_a_raised_skip_word_leaves_all_four_arrays_their_bits(hip):
    state = list(_state(1027, 3))
    nan_payload = torch.tensor([0x7FC12345], dtype=torch.int32, device=DEV).view(torch.float32)
    for t in (state[0], state[2], state[3], state[4]):
        t[17] = nan_payload[0]
    factor = torch.tensor([0.5], device=DEV)
    for words, applied in (([0, 9], True), ([1, 0], False), ([-5, 0], False)):
        skip = torch.tensor(words, dtype=torch.int32, device=DEV)
        got = _fused(hip, state, 2, 0.25, grad_scale=0.5, skip=skip, grad_factor=factor)
        assert skip.tolist() == words
        kept = [_bits(a, b) for a, b in zip(got, (state[0], state[2], state[3], state[4]))]
        assert kept == ([False] * 4 if applied else [True] * 4), (words, kept)


def test_nothing_is_hidden_and_alpha_zero_keeps_the_average(hip):
    state = list(_state(1030, 5))
    state[0][3], state[0][1029] = float('nan'), float('inf')     # float4 body and tail
    got = _fused(hip, state, 1, 0.1)
    assert torch.isnan(got[3][3]) and torch.isinf(got[3][1029])
    assert int(torch.isfinite(got[3]).logical_not().sum()) == 2
    clean = _state(1030, 6)
    got = _fused(hip, clean, 1, 0.0)
    assert _bits(got[3], clean[4]) and not _bits(got[0], clean[0])
    got = _fused(hip, clean, 1, 1.0)                             # alpha 1: the parameters
    assert np.abs((got[3] - got[0]).cpu().numpy()).max() <= \
        ref.ema_bound(clean[4].cpu().numpy(), got[0].cpu().numpy()).max()


def test_argument_errors_leave_the_arrays_untouched(hip):
    p, g, m, v, e = _state(64, 1)
    before = [t.clone() for t in (p, m, v, e)]
    for alpha in (-0.1, 1.5, float('nan')):
        with pytest.raises(hip.CtcAsrError):
            hip.adam_step(p, g, m, v, 1, ema=e, ema_alpha=alpha)
    with pytest.raises(hip.CtcAsrError, match='ema_alpha'):
        hip.adam_step(p, g, m, v, 1, ema=e)                      # no alpha
    with pytest.raises(hip.CtcAsrError):
        hip.adam_step(p, g, m, v, 1, ema_alpha=0.1)              # no average to move
    with pytest.raises(hip.CtcAsrError, match='ema holds 60'):
        hip.adam_step(p, g, m, v, 1, ema=e[:60], ema_alpha=0.1)
    with pytest.raises(hip.CtcAsrError, match='CPU'):
        hip.adam_step(p, g, m, v, 1, ema=e.cpu(), ema_alpha=0.1)
    with pytest.raises(hip.CtcAsrError):
        hip.adam_step(p, g, m, v, 1, ema=e.double(), ema_alpha=0.1)
    lib = hip.load()
    ptr = [t.data_ptr() for t in (p, g, m, v)]
    assert lib.ctcasr_adam_step_ema(*ptr, None, 64, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None, None,
                                    0.1, None) == -1              # null ema
    assert lib.ctcasr_adam_step_ema(*ptr, e.data_ptr(), 64, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, None,
                                    None, 0.1, None) == -1        # step counts from 1
    assert lib.ctcasr_adam_step_ema(*ptr, e.data_ptr() + 4, 60, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0,
                                    None, None, 0.1, None) == -1  # alignment
    torch.cuda.synchronize()
    for got, want in zip((p, m, v, e), before):
        assert _bits(got, want)
