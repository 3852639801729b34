"""Float64 reference of the bidirectional recurrence the HIP kernels compute (`hip.rnn_fwd` /
`hip.rnn_bwd`), written with plain torch ops so that autograd gives dxw and the bias gradients.

Layouts are the kernels': xw [T, B, 2, G*H], w_hh [2, G*H, H], y [T, B, 2H] (forward direction in
the first H columns), ``seq_len`` int[B] (rows past their length: y = 0, no gradient).  Gate order
i, f, g, o for the LSTM; r, z, n for the GRU, whose candidate adds the recurrent bias ``b_hh_n``
(columns 2H..3H of a [2, 3H] tensor) inside r * (...).  The backward direction walks each row's
own length from its last frame down.

`recurrence` handles every row at once under a length mask; `recurrence_loop` is the same
recurrence one row and one step at a time, kept as the plain statement the vectorised form is
checked against (tests/test_rnn_reference.py)."""

import torch

GATES = {'rnn_relu': 1, 'rnn_tanh': 1, 'lstm': 4, 'gru': 3}


def _cell(cell, x, rec, h, c, b_n, hidden):
    """One step of every row: x, rec [B, G*H] (rec = h W^T + recurrent bias) -> h', c'."""
    if cell == 'rnn_relu':
        return torch.relu(x + rec), c
    if cell == 'rnn_tanh':
        return torch.tanh(x + rec), c
    if cell == 'lstm':
        i, f, g, o = (x + rec).split(hidden, dim=-1)
        c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c_new), c_new
    xr, xz, xn = x.split(hidden, dim=-1)
    rr, rz, rn = rec.split(hidden, dim=-1)
    r, z = torch.sigmoid(xr + rr), torch.sigmoid(xz + rz)
    n = torch.tanh(xn + r * (rn + b_n))
    return (1 - z) * n + z * h, c


def _inputs(cell, xw, w_hh, b_hh_n, xw_bias, rec_bias):
    hidden = w_hh.shape[2]
    gh = GATES[cell] * hidden
    x = xw.double()
    if xw_bias is not None:
        x = x + xw_bias.double().reshape(1, 1, 2, gh)
    w = w_hh.double()
    b_n = [torch.zeros(hidden, dtype=torch.float64, device=xw.device)] * 2
    if cell == 'gru':
        b_n = [b_hh_n[d, 2 * hidden:].double() for d in (0, 1)]
    rb = [None, None] if rec_bias is None else [rec_bias.double().reshape(2, gh)[d] for d in (0, 1)]
    return x, w, b_n, rb, hidden


def recurrence(cell, xw, w_hh, b_hh_n=None, seq_len=None, xw_bias=None, rec_bias=None):
    """y f64[T, B, 2H].  ``xw_bias`` f[2*G*H] is added to xw (as the kernels' ``xw_bias``);
    ``rec_bias`` f[2*G*H] (normally zeros) is added to h W^T - its gradient is the column sums of
    the recurrent pre-activation gradients (the GRU's drec).  Differentiable in every input."""
    num_steps, batch = xw.shape[0], xw.shape[1]
    x, w, b_n, rb, hidden = _inputs(cell, xw, w_hh, b_hh_n, xw_bias, rec_bias)
    dev = xw.device
    steps = torch.full((batch,), num_steps, dtype=torch.long, device=dev) if seq_len is None \
        else torch.as_tensor(seq_len, device=dev).long()
    s_idx = torch.arange(num_steps, device=dev).view(-1, 1)
    active = s_idx < steps.view(1, -1)                                    # [T, B]
    # the backward direction: step s of row b reads time L_b - 1 - s; past the row's end the index
    # stays put (it is its own inverse, so the same gather puts the outputs back in time order)
    rev = torch.where(active, steps.view(1, -1) - 1 - s_idx, s_idx.expand(num_steps, batch))
    cols = torch.arange(batch, device=dev).view(1, -1).expand(num_steps, batch)
    halves = []
    for d in (0, 1):
        xd = x[:, :, d] if d == 0 else x[rev, cols, 1]
        h = torch.zeros(batch, hidden, dtype=torch.float64, device=dev)
        c = torch.zeros_like(h)
        outs = []
        for s in range(num_steps):
            rec = h @ w[d].t()
            if rb[d] is not None:
                rec = rec + rb[d]
            m = active[s].view(-1, 1)
            # (a frame past its row's length is never read: garbage there, a NaN included, reaches
            # neither y nor - as 0 * NaN through the masked-out branch - any gradient)
            h_new, c_new = _cell(cell, torch.where(m, xd[s], torch.zeros_like(xd[s])), rec, h, c,
                                 b_n[d], hidden)
            outs.append(torch.where(m, h_new, torch.zeros_like(h_new)))
            h = torch.where(m, h_new, h)
            c = torch.where(m, c_new, c)
        out = torch.stack(outs)
        halves.append(out if d == 0 else out[rev, cols])
    return torch.cat(halves, dim=2)


def recurrence_loop(cell, xw, w_hh, b_hh_n=None, seq_len=None, xw_bias=None, rec_bias=None):
    """The same y, one row and one step at a time (slow: for checking `recurrence`)."""
    num_steps, batch = xw.shape[0], xw.shape[1]
    x, w, b_n, rb, hidden = _inputs(cell, xw, w_hh, b_hh_n, xw_bias, rec_bias)
    zero = torch.zeros(hidden, dtype=torch.float64, device=xw.device)
    cols = [[[zero] * num_steps for _ in range(batch)] for _ in (0, 1)]
    for d in (0, 1):
        for b in range(batch):
            steps = num_steps if seq_len is None else int(seq_len[b])
            h, c = zero, zero
            for s in range(steps):
                t = s if d == 0 else steps - 1 - s
                rec = w[d] @ h
                if rb[d] is not None:
                    rec = rec + rb[d]
                h, c = _cell(cell, x[t, b, d], rec, h, c, b_n[d], hidden)
                cols[d][b][t] = h
    return torch.stack([torch.stack([torch.cat([cols[0][b][t], cols[1][b][t]])
                                     for b in range(batch)]) for t in range(num_steps)])


def relu_backward(y, dy, w_hh, seq_len=None):
    """dxw f64[T, B, 2, H] of the ReLU recurrence with the mask y > 0 taken from a GIVEN y: the
    backward kernels read the mask off the y they are handed, and where a pre-activation is
    ~1e-7 the float64 forward pass may have the other sign (an O(1) change of that entry's
    gradient).  dpre = y > 0 ? dy + dpre_next W : 0, walked against each direction's order - a
    select as in the kernels (and TensorFlow's ReluGrad), not a product with the mask: a NaN
    gradient where y <= 0 (or y is NaN) gives 0, never NaN * 0."""
    num_steps, batch, _ = y.shape
    hidden = w_hh.shape[2]
    dev = y.device
    y64 = y.double().view(num_steps, batch, 2, hidden)
    dy64 = dy.double().view(num_steps, batch, 2, hidden)
    steps = torch.full((batch,), num_steps, dtype=torch.long, device=dev) if seq_len is None \
        else torch.as_tensor(seq_len, device=dev).long()
    dxw = [[None] * num_steps for _ in (0, 1)]
    for d in (0, 1):
        w64 = w_hh[d].double()
        carry = torch.zeros(batch, hidden, dtype=torch.float64, device=dev)
        # (the backward direction's step after time t is time t - 1 of the same row)
        for t in (range(num_steps - 1, -1, -1) if d == 0 else range(num_steps)):
            live = (y64[t, :, d] > 0) & (t < steps).view(-1, 1)
            dpre = torch.where(live, dy64[t, :, d] + carry, torch.zeros_like(carry))
            dxw[d][t] = dpre
            carry = dpre @ w64
    return torch.stack([torch.stack([dxw[0][t], dxw[1][t]], dim=1) for t in range(num_steps)])


def forward_backward(cell, xw, w_hh, dy, b_hh_n=None, seq_len=None, xw_bias=None,
                     fn=recurrence):
    """(y, dxw, dbias) in float64 for the loss sum(y * dy): dxw [T, B, 2, G*H] (the gradient of
    the pre-activations xw (+ xw_bias)), dbias in the layout `hip.rnn_bwd` fills - the column sums
    of dxw [2*G*H], then for the GRU those of drec [2*G*H]."""
    gh = GATES[cell] * w_hh.shape[2]
    x = xw.detach().double().requires_grad_(True)
    rec_bias = torch.zeros(2 * gh, dtype=torch.float64, device=xw.device, requires_grad=True)
    y = fn(cell, x, w_hh.detach(), b_hh_n, seq_len, xw_bias, rec_bias)
    (y * dy.double()).sum().backward()
    dbias = x.grad.sum(dim=(0, 1)).reshape(-1)
    if cell == 'gru':
        dbias = torch.cat([dbias, rec_bias.grad])
    return y.detach(), x.grad, dbias


def _row_steps(num_steps, batch, seq_len):
    return [num_steps] * batch if seq_len is None else [int(n) for n in seq_len]


def nan_mask_forward(num_steps, batch, hidden, t0, row, d, unit, seq_len=None):
    """Closed form of isnan(y) bool[T, B, 2, H] after ONE NaN in xw[t0, row, d, a gate column of
    ``unit``]: that unit at t0, then every unit of (row, d) at the frames the direction visits
    after t0 inside the row's length (d = 0: later frames, d = 1: earlier ones); nothing when t0
    is past the row's length, nothing in any other row or direction."""
    mask = torch.zeros(num_steps, batch, 2, hidden, dtype=torch.bool)
    steps = _row_steps(num_steps, batch, seq_len)[row]
    if t0 < steps:
        mask[t0, row, d, unit] = True
        later = range(t0 + 1, steps) if d == 0 else range(0, t0)
        for t in later:
            mask[t, row, d] = True
    return mask


def nan_mask_backward(num_steps, batch, hidden, gates, t0, row, d, unit, seq_len=None):
    """Closed form of isnan(dxw) bool[T, B, 2, G*H] after ONE NaN in dy[t0, row, d * H + unit] for
    the LSTM, GRU and tanh cells (whose derivatives multiply the incoming gradient; the ReLU
    cell's selects on y > 0: `relu_backward`): all G gate columns of the unit at t0, then every
    column of (row, d) at the frames the backward walk visits after t0 (d = 0: earlier frames,
    d = 1: later ones inside the row's length)."""
    mask = torch.zeros(num_steps, batch, 2, gates * hidden, dtype=torch.bool)
    steps = _row_steps(num_steps, batch, seq_len)[row]
    if t0 < steps:
        mask[t0, row, d, unit::hidden] = True
        later = range(0, t0) if d == 0 else range(t0 + 1, steps)
        for t in later:
            mask[t, row, d] = True
    return mask
