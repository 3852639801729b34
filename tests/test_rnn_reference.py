"""The float64 recurrence reference (tests/rnn_reference.py) the kernel tests compare with: the
vectorised form against the row-by-row loop, and both against torch.nn's own bidirectional
cells over packed sequences.  CPU only."""

import pytest
import torch

from tests import rnn_reference as ref

CELLS = ['lstm', 'gru', 'rnn_relu', 'rnn_tanh']


def _data(cell, num_steps, batch, hidden, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    gh = ref.GATES[cell] * hidden
    xw = torch.randn(num_steps, batch, 2, gh, generator=g, dtype=torch.float64)
    w = torch.randn(2, gh, hidden, generator=g, dtype=torch.float64) / hidden ** 0.5
    b_hh = torch.randn(2, gh, generator=g, dtype=torch.float64) * 0.3
    bias = torch.randn(2 * gh, generator=g, dtype=torch.float64) * 0.2
    dy = torch.randn(num_steps, batch, 2 * hidden, generator=g, dtype=torch.float64)
    sl = None
    if lengths:
        sl = torch.randint(1, num_steps + 1, (batch,), generator=g, dtype=torch.int32)
        sl[0], sl[-1] = num_steps, 1
    return xw, w, b_hh, bias, dy, sl


@pytest.mark.parametrize('cell', CELLS)
@pytest.mark.parametrize('lengths', [False, True])
@pytest.mark.parametrize('num_steps,batch', [(1, 1), (3, 2), (6, 5)])
def test_vectorised_reference_equals_the_loop(cell, lengths, num_steps, batch):
    xw, w, b_hh, bias, dy, sl = _data(cell, num_steps, batch, 8, lengths, 7 * num_steps + batch)
    got = ref.forward_backward(cell, xw, w, dy, b_hh, sl, bias)
    want = ref.forward_backward(cell, xw, w, dy, b_hh, sl, bias, fn=ref.recurrence_loop)
    for name, a, b in zip(('y', 'dxw', 'dbias'), got, want):
        assert a.shape == b.shape, name
        assert float((a - b).abs().max()) < 1e-12, name
    if sl is not None and int(sl[-1]) < num_steps:     # past a row's end: no output, no gradient
        assert float(got[0][int(sl[-1]):, -1].abs().max()) == 0.0
        assert float(got[1][int(sl[-1]):, -1].abs().max()) == 0.0


def _torch_nn(cell, xw, w, b_hh, bias, sl):
    """The same recurrence through torch.nn's bidirectional cells: the input is [xw_fwd | xw_bwd]
    with W_ih = [I 0] / [0 I], so that each direction's pre-activation is exactly its xw."""
    num_steps, batch, _, gh = xw.shape
    hidden = w.shape[2]
    kind = {'lstm': torch.nn.LSTM, 'gru': torch.nn.GRU}.get(cell, torch.nn.RNN)
    extra = {} if kind is not torch.nn.RNN else dict(nonlinearity=cell[4:])
    net = kind(2 * gh, hidden, bidirectional=True, **extra).double()
    eye = torch.eye(gh, dtype=torch.float64)
    zero = torch.zeros(gh, gh, dtype=torch.float64)
    with torch.no_grad():
        for d, suffix in enumerate(('', '_reverse')):
            getattr(net, 'weight_ih_l0' + suffix).copy_(torch.cat([eye, zero] if d == 0
                                                                  else [zero, eye], dim=1))
            getattr(net, 'weight_hh_l0' + suffix).copy_(w[d])
            getattr(net, 'bias_ih_l0' + suffix).copy_(bias.view(2, gh)[d])
            rec = torch.zeros(gh, dtype=torch.float64)
            if cell == 'gru':
                rec[2 * hidden:] = b_hh[d, 2 * hidden:]
            getattr(net, 'bias_hh_l0' + suffix).copy_(rec)
    x = xw.reshape(num_steps, batch, 2 * gh)
    lens = torch.full((batch,), num_steps) if sl is None else sl.long()
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, enforce_sorted=False)
    out, _ = net(packed)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=num_steps)
    return y


@pytest.mark.parametrize('cell', CELLS)
@pytest.mark.parametrize('lengths', [False, True])
def test_reference_equals_torch_nn(cell, lengths):
    xw, w, b_hh, bias, _, sl = _data(cell, 5, 4, 8, lengths, 3)
    with torch.no_grad():
        got = ref.recurrence(cell, xw, w, b_hh, sl, bias)
        want = _torch_nn(cell, xw, w, b_hh, bias, sl)
    assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize('lengths', [False, True])
def test_relu_backward_from_a_given_y_equals_autograd(lengths):
    xw, w, _, bias, dy, sl = _data('rnn_relu', 4, 3, 8, lengths, 5)
    y, dxw, _ = ref.forward_backward('rnn_relu', xw, w, dy, None, sl, bias)
    assert float((ref.relu_backward(y, dy, w, sl) - dxw).abs().max()) < 1e-12
