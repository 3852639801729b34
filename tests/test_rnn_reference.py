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


def test_relu_backward_selects_on_the_mask():
    """A NaN gradient where y <= 0 is dropped and a NaN y counts as dead (TensorFlow's ReluGrad,
    the kernels' `y > 0 ? acc : 0`) - a product with the mask would keep both as NaN."""
    xw, w, _, bias, dy, _ = _data('rnn_relu', 4, 3, 8, False, 5)
    y = ref.recurrence('rnn_relu', xw, w, None, None, bias)
    dead = (y[3, 1, :8] == 0).nonzero()
    assert len(dead), 'the data has no dead unit at the last frame'
    poisoned = dy.clone()
    poisoned[3, 1, int(dead[0])] = float('nan')
    assert torch.equal(ref.relu_backward(y, poisoned, w), ref.relu_backward(y, dy, w))
    y_nan = y.clone()
    y_nan[3, 1, 0] = float('nan')
    got = ref.relu_backward(y_nan, dy, w)
    assert not got.isnan().any() and float(got[3, 1, 0, 0]) == 0.0


_POISONS = [(t0, row, d, unit) for t0 in (0, 1, 3) for row in (0, 2) for d in (0, 1)
            for unit in (0, 3, 7)]


@pytest.mark.parametrize('cell', CELLS)
@pytest.mark.parametrize('lengths', [False, True])
def test_one_nan_forward_spreads_as_the_closed_form_says(cell, lengths):
    """One NaN in xw: isnan(y) of `recurrence` is `nan_mask_forward` - its unit at that frame,
    every unit of the row and direction at the frames visited later inside the row's length,
    nothing else (H = 8, T = 4; every gate of the unit; the last row has length 1)."""
    hidden, gates = 8, ref.GATES[cell]
    xw, w, b_hh, bias, _, sl = _data(cell, 4, 3, hidden, lengths, 11)
    with torch.no_grad():
        for t0, row, d, unit in _POISONS:
            for gate in range(gates):
                x = xw.clone()
                x[t0, row, d, gate * hidden + unit] = float('nan')
                got = ref.recurrence(cell, x, w, b_hh, sl, bias).isnan().view(4, 3, 2, hidden)
                want = ref.nan_mask_forward(4, 3, hidden, t0, row, d, unit, sl)
                assert torch.equal(got, want), (t0, row, d, unit, gate)
                assert lengths or want.any()


@pytest.mark.parametrize('cell', CELLS)
@pytest.mark.parametrize('lengths', [False, True])
def test_one_nan_backward_spreads_as_the_closed_form_says(cell, lengths):
    """One NaN in dy after a clean forward pass: isnan(dxw) of autograd is `nan_mask_backward`
    (LSTM, GRU, tanh); the ReLU cell keeps of that mask the entries with y > 0 (`relu_backward`:
    a select), the poisoned unit chosen alive."""
    hidden, gates = 8, ref.GATES[cell]
    xw, w, b_hh, bias, dy, sl = _data(cell, 4, 3, hidden, lengths, 13)
    y = ref.recurrence(cell, xw, w, b_hh, sl, bias)
    alive = (y > 0).view(4, 3, 2, hidden)
    for t0, row, d, unit in _POISONS:
        if cell == 'rnn_relu':
            live_units = alive[t0, row, d].nonzero()
            if len(live_units):
                unit = int(live_units[len(live_units) // 2])
        g = dy.clone()
        g[t0, row, d * hidden + unit] = float('nan')
        want = ref.nan_mask_backward(4, 3, hidden, gates, t0, row, d, unit, sl)
        if cell == 'rnn_relu':
            got = ref.relu_backward(y, g, w, sl).isnan()
            want &= alive
        else:
            got = ref.forward_backward(cell, xw, w, g, b_hh, sl, bias)[1].isnan()
        assert torch.equal(got, want), (t0, row, d, unit)


@pytest.mark.parametrize('cell', ['lstm', 'gru', 'rnn_tanh'])
@pytest.mark.parametrize('lengths', [False, True])
@pytest.mark.parametrize('value', [float('inf'), float('-inf')])
def test_an_infinite_pre_activation_saturates_the_gate(cell, lengths, value):
    """+-inf in one xw entry of a gated cell or the tanh cell: sigmoid and tanh saturate, y, dxw
    and the bias gradients of the float64 reference stay finite everywhere."""
    hidden, gates = 8, ref.GATES[cell]
    xw, w, b_hh, bias, dy, sl = _data(cell, 4, 3, hidden, lengths, 17)
    for t0, row, d, unit in _POISONS[::5]:
        for gate in range(gates):
            x = xw.clone()
            x[t0, row, d, gate * hidden + unit] = value
            for name, got in zip(('y', 'dxw', 'dbias'),
                                 ref.forward_backward(cell, x, w, dy, b_hh, sl, bias)):
                assert torch.isfinite(got).all(), (name, t0, row, d, unit, gate)


@pytest.mark.parametrize('cell', CELLS)
def test_garbage_past_a_rows_length_is_never_read(cell):
    """NaN in every xw and dy frame past a row's length: y, dxw and the bias gradients are those of
    clean padding, bit for bit (autograd through a masked-out NaN would give 0 * NaN)."""
    xw, w, b_hh, bias, dy, sl = _data(cell, 4, 3, 8, True, 19)
    past = torch.arange(4).view(4, 1) >= sl.view(1, -1)
    assert past.any()
    x, g = xw.clone(), dy.clone()
    x[past] = float('nan')
    g[past] = float('nan')
    want = ref.forward_backward(cell, xw, w, dy, b_hh, sl, bias)
    for fn in (ref.recurrence, ref.recurrence_loop):
        for a, b in zip(ref.forward_backward(cell, x, w, g, b_hh, sl, bias, fn=fn), want):
            assert torch.equal(a, b) or fn is ref.recurrence_loop and \
                float((a - b).abs().max()) < 1e-12
    y = want[0]
    if cell == 'rnn_relu':
        assert torch.equal(ref.relu_backward(y, g, w, sl), ref.relu_backward(y, dy, w, sl))
