"""`hip.adam_step(grad_factor=...)` - `ctcasr_adam_step_clipped`: the same kernel as
`ctcasr_adam_step` with a factor read on the device.  Its contract is an identity, so everything
here is compared bit for bit: gradients scaled by ``grad_scale * grad_factor[0]``, ONE float32
product, are the gradients of the plain call with that product as its scale."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)
# 65536 workgroups x 256 threads of float4, three more workgroups' worth, and a tail of 3
STRIDES = 4 * 256 * 65536 + 4 * 256 * 3 + 3
FACTORS = (1.0, 0.5, 0.3, 1e-6, 0.0)


def _state(n, seed):
    """Device tensors (param, grad, m, v): normal deviates with exact zeros, 1e-20 and 1e+10
    among the gradients, moments of a run in progress, a few parameters at exactly 0."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    g = torch.randn(n, device=DEV, generator=gen)
    g[0::7], g[1::7], g[2::7] = 0.0, 1e-20, 1e10
    g[3::14] *= -1
    m = torch.randn(n, device=DEV, generator=gen).abs_().mul_(1e-2).mul_(torch.sign(g))
    v = torch.rand(n, device=DEV, generator=gen).mul_(1e-3)
    p = torch.randn(n, device=DEV, generator=gen)
    p[5::11] = 0.0
    return p, g, m, v


def _step(hip, state, step, **kwargs):
    """One Adam step on copies of (param, m, v); returns them."""
    p, g, m, v = state
    p, m, v = p.clone(), m.clone(), v.clone()
    hip.adam_step(p, g, m, v, step, **HYPER, **kwargs)
    return p, m, v


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize('n', [1, 5, 1027, STRIDES])
def test_a_device_factor_is_the_plain_call_with_the_product_as_its_scale(hip, n):
    state = _state(n, n % 1000)
    grad_before = state[1].clone()
    for scale in (1.0, 1.0 / 3):
        for f in FACTORS:
            factor = torch.tensor([f], dtype=torch.float32, device=DEV)
            got = _step(hip, state, 3, grad_scale=scale, grad_factor=factor)
            product = float(np.float32(scale) * np.float32(f))
            want = _step(hip, state, 3, grad_scale=product)
            assert _same(got, want), (n, scale, f)
            assert factor.item() == np.float32(f)
            if f == 0.0:    # nothing of the gradient, but an update all the same: v decays
                assert not _same(got[2:3], state[3:4])
    assert torch.equal(state[1], grad_before)


@pytest.mark.parametrize('n', [1, 5, 1027])
def test_no_factor_and_a_factor_of_one_are_todays_call(hip, n):
    state = _state(n, 50 + n)
    one = torch.ones(1, device=DEV)
    for scale in (1.0, 0.125, 1.0 / 3):
        plain = _step(hip, state, 7, grad_scale=scale)
        assert _same(plain, _step(hip, state, 7, grad_scale=scale, grad_factor=None))
        assert _same(plain, _step(hip, state, 7, grad_scale=scale, grad_factor=one))
        assert not _same(plain, state[:1] + state[2:])
    # ... and the entry point of the plain call itself, next to the new one with a null factor
    lib = hip.load()
    args = lambda t: [x.data_ptr() for x in t]                           # noqa: E731
    a = [x.clone() for x in state]
    b = [x.clone() for x in state]
    assert lib.ctcasr_adam_step(*args(a), n, 1e-3, 0.9, 0.999, 1e-8, 7, 0.5, None, None) == 0
    assert lib.ctcasr_adam_step_clipped(*args(b), n, 1e-3, 0.9, 0.999, 1e-8, 7, 0.5, None, None,
                                        None) == 0
    torch.cuda.synchronize()
    assert _same(a, b)


def test_the_skip_word_wins_over_a_factor(hip):
    state = _state(1027, 9)
    factor = torch.tensor([0.5], device=DEV)
    for words, applied in (([0, 9], True), ([1, 0], False), ([-5, 0], False)):
        skip = torch.tensor(words, dtype=torch.int32, device=DEV)
        got = _step(hip, state, 2, grad_scale=0.5, skip=skip, grad_factor=factor)
        assert skip.tolist() == words and factor.item() == 0.5
        if applied:
            assert _same(got, _step(hip, state, 2, grad_scale=0.25))
        else:
            assert _same(got, state[:1] + state[2:])


def test_refusals(hip):
    p, g, m, v = _state(64, 1)
    before = p.clone()
    for bad in (torch.ones(1), torch.ones(1, device=DEV, dtype=torch.float64),
                torch.ones(1, device=DEV, dtype=torch.int32), torch.ones(2, device=DEV),
                torch.ones(0, device=DEV)):
        with pytest.raises(hip.CtcAsrError):
            hip.adam_step(p, g, m, v, 1, grad_factor=bad)
    lib = hip.load()
    factor = torch.ones(1, device=DEV)
    assert lib.ctcasr_adam_step_clipped(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0,
                                        None, factor.data_ptr(), None) == -1
    assert lib.ctcasr_adam_step_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 64,
                                        1e-3, 0.9, 0.999, 1e-8, 0, 1.0, None, factor.data_ptr(),
                                        None) == -1                      # step counts from 1
    torch.cuda.synchronize()
    assert torch.equal(p, before)
