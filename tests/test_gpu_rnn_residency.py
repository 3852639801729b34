"""The residency hand-shake of the persistent recurrence on the device: `resident_signal` at the
head of all seven persistent kernels, `resident_gate_kernel`, and the ticket count that
`CTCModel` keeps for them (include/ctcasr.h).

A wrong gate costs time, never a result, so these tests time gates.  A gate is enqueued on a side
stream between two events.  With the bound it is given (`max_wait_us`) it is

  shut   when it took at least 0.9 x the bound and at most the bound + SLACK_MS,
  open   when it took less than a quarter of the bound.

Gates that must be shut get 5 ms, gates that must be open 100 ms (the ABI's maximum): both
thresholds come from the bound passed in.  SLACK_MS is what an event bracket costs beyond the
kernel in it - the bracket itself plus the launch of a one-lane kernel - measured on the MI355X
(MEASURED below), not anything the gate under test reports.

MEASURED on one MI355X (300 brackets each; ms):
  empty bracket                 median 0.0045   worst 0.025
  gate with max_wait_us = 0     median 0.0086   worst 0.029     (nothing is enqueued)
  open gate, 100 ms bound       median 0.0094   worst 0.0137    (the first one: 0.026)
  shut gate, 5 ms bound         5.003 .. 5.013                  (1 ms bound: 1.003 .. 1.012)
  SLACK_MS: bracket + launch, worst case 0.025 + 0.029 = 0.054 -> 0.2 (a shared machine; 4 % of
  the 5 ms bound, far below the 10 % the lower limit leaves)
  OPEN_GATE_MS: 0.03 - the open-gate latency with the kernel's first launch
  RUNNING_T = 160 steps of LSTM-1024 at 16 rows, at least 20 x OPEN_GATE_MS = 0.6 ms per launch:
    backward, default flags   launch 1.187   gate 0.033   gate's end -> launch's end 1.169
    forward, RNN_HALF_CHIP    launch 0.978   gate 0.032   gate's end -> launch's end 0.960
    (the gate's 0.03 ms is the host's time to enqueue the launch behind it; at T = 64 the launches
    last 0.48 / 0.39 ms and the order still holds, six times out of six each)
"""

import numpy as np
import pytest
import torch

from tests.test_gpu_model import _setup
from tests.test_gpu_rnn_edges import CASES, _bwd_kernels, _case, _flags

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SHUT_US, OPEN_US = 5000, 100000
SLACK_MS = 0.2
OPEN_GATE_MS = 0.03
RUNNING_T = 160
STEPS = 3
BATCHES = {1024: (1, 17, 24, 33, 64), 2048: (1, 17, 33)}
LAST = 0xFFFFFF

_SIDE = []


def _side():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _bracket_ms(fn):
    """Milliseconds between two events around ``fn``'s work on the (idle) side stream."""
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(_side()):
        start.record()
        fn()
        stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


class _Gates:
    """Timed gates on one workspace."""

    def __init__(self, hip, cell, ws, num_steps, batch, hidden):
        self.hip, self.args, self.ws = hip, (num_steps, batch, hidden), ws
        self.cell = cell

    def ms(self, ticket, bound_us):
        return _bracket_ms(lambda: self.hip.rnn_resident_gate(self.cell, self.ws, *self.args,
                                                              ticket, bound_us))

    def shut(self, ticket, what=None):
        took = self.ms(ticket, SHUT_US)
        assert 0.9 * SHUT_US / 1000 <= took <= SHUT_US / 1000 + SLACK_MS, \
            ('gate should be shut', hex(ticket), took, what)

    def open(self, ticket, what=None):
        took = self.ms(ticket, OPEN_US)
        assert took < 0.25 * OPEN_US / 1000, ('gate should be open', hex(ticket), took, what)
        return took


@pytest.fixture(scope='module', autouse=True)
def _gate_kernel_loaded(hip):
    """The first launch of a kernel pays for loading it: not inside a timed bracket."""
    ws = hip.rnn_workspace('lstm', 1, 1, 1024, DEV)
    with torch.cuda.stream(_side()):
        hip.rnn_resident_gate('lstm', ws, 1, 1, 1024, 1, 1)
    torch.cuda.synchronize()


class _Buffers:
    """Outputs of one pass over a case of `_case`, pre-filled so that an untouched one shows."""

    def __init__(self, hip, cell, c, colmax_ok, fill=float('nan')):
        num_steps, batch = c['xw'].shape[:2]
        hidden = c['w'].shape[2]
        gh = hip.CELL_GATES[cell] * hidden
        self.hip, self.cell, self.c = hip, cell, c
        self.y = torch.full((num_steps, batch, 2 * hidden), fill, device=DEV)
        self.reserve = torch.zeros(hip.rnn_reserve_bytes(cell, num_steps, batch, hidden),
                                   dtype=torch.uint8, device=DEV)
        self.dxw = torch.full((num_steps, batch, 2, gh), fill, device=DEV)
        self.dbias = torch.zeros(2 * gh * (2 if cell == 'gru' else 1), device=DEV)
        self.colmax = torch.zeros(2 * gh, dtype=torch.int32, device=DEV) if colmax_ok else None

    def fwd(self, ws, flags, ticket=0, steps=None, y=None):
        c = self.c
        self.hip.rnn_fwd(self.cell, c['xw'], c['w'], c['sl'], b_hh_n=c['b_hh'],
                         y=self.y if y is None else y, reserve=self.reserve, workspace=ws,
                         steps=steps, flags=flags, xw_bias=c['bias'], ticket=ticket)

    def bwd(self, ws, flags, ticket=0, steps=None, y=None):
        c = self.c
        self.hip.rnn_bwd(self.cell, c['dy'], self.y if y is None else y, c['wt'], self.reserve,
                         c['sl'], b_hh_n=c['b_hh'], dxw=self.dxw, dbias=self.dbias, workspace=ws,
                         steps=steps, flags=flags, ticket=ticket, colmax=self.colmax)


def _colmax_ok(hip, cell, num_steps, batch, hidden, bwd_flags, forms):
    return forms != ['stream'] and hip.rnn_bwd_f16_supported(cell, num_steps, batch, hidden,
                                                             bwd_flags)


def _same_backward(got, want, what):
    """dxw and the column maxima bit for bit, the bias gradients to the rounding of their atomics
    (1e-5 of the largest: the bar of the cut pass in test_gpu_rnn_edges.py)."""
    assert torch.equal(got.dxw, want.dxw), (what, 'dxw', int((got.dxw != want.dxw).sum()))
    assert float((got.dbias - want.dbias).abs().max()) <= \
        1e-5 * max(1.0, float(want.dbias.abs().max())), (what, 'dbias')
    assert (got.colmax is None) == (want.colmax is None), what
    if got.colmax is not None:
        assert torch.equal(got.colmax, want.colmax), (what, 'colmax')


def _untagged(hip, cell, c, fwd_flags, bwd_flags, colmax_ok):
    """The pass without tickets on a fresh workspace."""
    num_steps, batch = c['xw'].shape[:2]
    hidden = c['w'].shape[2]
    ws = hip.rnn_workspace(cell, num_steps, batch, hidden, DEV)
    want = _Buffers(hip, cell, c, colmax_ok)
    want.fwd(ws, fwd_flags)
    want.bwd(ws, bwd_flags)
    hip.rnn_poll_error(cell, ws, num_steps, batch, hidden)
    assert torch.isfinite(want.y).all() and torch.isfinite(want.dxw).all()
    return want


def _expected_forms(hip, cell, hidden, variant, batch, bwd_flags):
    """Which backward kernel each 32-row block must run - written out per variant, next to the
    rule `_bwd_kernels` restates."""
    blocks = [min(32, batch - b0) for b0 in range(0, batch, 32)]
    if not bwd_flags & hip.RNN_F16:
        return ['fp32'] * len(blocks)
    if cell == 'rnn_relu':
        return ['prnn_relu16_kernel' if batch <= 16 else 'fp32'] * len(blocks)
    if cell != 'lstm':
        return ['fp32'] * len(blocks)
    if hidden == 2048:
        return ['prnn_bwd16w_kernel<k-pair>' if variant == 'f16 k-pair' else
                'prnn_bwd16w_kernel'] * len(blocks)
    return ['prnn_bwd16s_kernel' if variant == 'f16 stagger' and rows in (24, 32) else
            'prnn_bwd16_kernel' for rows in blocks]


@pytest.mark.parametrize('cell,hidden,variant', [c for c in CASES if c[2] != 'stream'])
def test_every_kernel_family_posts_its_ticket_and_cleans_up(hip, cell, hidden, variant):
    """Per (cell, H, variant) and batch, on one zeroed workspace: a gate for ticket 5 is shut; a
    forward pass with ticket 5 opens it and leaves 6 shut; a backward pass with ticket 6 opens 6;
    a forward pass with ticket 7 opens 7 - the third post happens only if every launch of the
    passes before (H = 2048: one per direction and tile; B > 32: the first row block's) put
    `resident[0]` back to zero.  Results are those of the same calls without tickets."""
    fwd_flags, bwd_flags = _flags(hip, variant)
    for batch in BATCHES[hidden]:
        what = (cell, hidden, variant, batch)
        assert hip.rnn_persistent_supported(cell, STEPS, batch, hidden), what
        forms = _bwd_kernels(hip, cell, hidden, STEPS, batch, bwd_flags, False)
        assert forms == _expected_forms(hip, cell, hidden, variant, batch, bwd_flags), what
        fwd_f16 = hip.rnn_f16_recurrence(cell, STEPS, batch, hidden, fwd_flags, backward=False)
        assert fwd_f16 == bool(fwd_flags & hip.RNN_F16 and (
            cell in ('lstm', 'gru') or (cell == 'rnn_relu' and batch <= 16))), what
        c = _case(hip, cell, hidden, STEPS, batch, False)
        colmax_ok = _colmax_ok(hip, cell, STEPS, batch, hidden, bwd_flags, forms)
        want = _untagged(hip, cell, c, fwd_flags, bwd_flags, colmax_ok)

        ws = hip.rnn_workspace(cell, STEPS, batch, hidden, DEV)
        gates = _Gates(hip, cell, ws, STEPS, batch, hidden)
        got = _Buffers(hip, cell, c, colmax_ok)
        gates.shut(5, what)
        got.fwd(ws, fwd_flags, ticket=5)
        gates.open(5, what)
        gates.shut(6, what)
        got.bwd(ws, bwd_flags, ticket=6)
        gates.open(6, what)
        y_again = torch.full_like(got.y, float('nan'))
        got.fwd(ws, fwd_flags, ticket=7, y=y_again)
        gates.open(7, what)
        hip.rnn_poll_error(cell, ws, STEPS, batch, hidden)
        assert torch.equal(got.y, want.y), (what, 'y')
        assert torch.equal(y_again, want.y), (what, 'y of the second forward pass')
        _same_backward(got, want, what)


@pytest.mark.parametrize('cell,hidden,variant,batch', [('lstm', 1024, 'f16 stagger', 24),
                                                       ('gru', 2048, 'fp32', 17),
                                                       ('rnn_tanh', 2048, 'whole chip', 33)])
def test_every_launch_of_a_cut_pass_posts_its_own_ticket(hip, cell, hidden, variant, batch):
    """T = 3 as three forward and three backward launches of one step, tickets 11 .. 16: after
    each launch its own gate is open and the next one's still shut."""
    fwd_flags, bwd_flags = _flags(hip, variant)
    c = _case(hip, cell, hidden, STEPS, batch, False)
    forms = _bwd_kernels(hip, cell, hidden, STEPS, batch, bwd_flags, False)
    colmax_ok = _colmax_ok(hip, cell, STEPS, batch, hidden, bwd_flags, forms)
    want = _untagged(hip, cell, c, fwd_flags, bwd_flags, colmax_ok)
    ws = hip.rnn_workspace(cell, STEPS, batch, hidden, DEV)
    gates = _Gates(hip, cell, ws, STEPS, batch, hidden)
    got = _Buffers(hip, cell, c, colmax_ok)
    ticket = 11
    gates.shut(ticket)
    for step in range(STEPS):
        got.fwd(ws, fwd_flags, ticket=ticket, steps=(step, step + 1))
        gates.open(ticket, ('fwd', step))
        gates.shut(ticket + 1, ('fwd', step))
        ticket += 1
    for step in reversed(range(STEPS)):
        got.bwd(ws, bwd_flags, ticket=ticket, steps=(step, step + 1))
        gates.open(ticket, ('bwd', step))
        gates.shut(ticket + 1, ('bwd', step))
        ticket += 1
    assert ticket == 17
    hip.rnn_poll_error(cell, ws, STEPS, batch, hidden)
    assert torch.equal(got.y, want.y)
    _same_backward(got, want, (cell, hidden, variant, batch))


def test_the_gate_compares_modulo_two_to_the_24_over_half_the_range(hip):
    """After one launch with ticket X = 0x400123 the gate is open for X, X - 1 and
    X - (2^23 - 1) (= X + 2^23 + 1 modulo 2^24: the far end of what counts as "posted at or after
    mine"), and shut for X + 1, X + 2^23 - 1 and X + 2^23.  (X + 2^24 - 1 is X - 1 modulo 2^24:
    open, by the predicate of include/ctcasr.h.)"""
    cell, hidden, batch, x = 'lstm', 1024, 1, 0x400123
    c = _case(hip, cell, hidden, STEPS, batch, False)
    ws = hip.rnn_workspace(cell, STEPS, batch, hidden, DEV)
    gates = _Gates(hip, cell, ws, STEPS, batch, hidden)
    got = _Buffers(hip, cell, c, False)
    # nothing posted yet: shut for every ticket, also above 2^23 where 0 - ticket passes the
    # modular comparison
    for ticket in (x, 0x800001, LAST):
        gates.shut(ticket)
    got.fwd(ws, 0, ticket=x)
    for ticket in (x, x - 1, (x - (2 ** 23 - 1)) % 2 ** 24, (x + 2 ** 24 - 1) % 2 ** 24):
        assert 0 < ticket <= LAST
        gates.open(ticket)
    assert (x - (2 ** 23 - 1)) % 2 ** 24 == 0xC00124
    for ticket in (x + 1, (x + 2 ** 23 - 1) % 2 ** 24, (x + 2 ** 23) % 2 ** 24):
        assert 0 < ticket <= LAST
        gates.shut(ticket)
    hip.rnn_poll_error(cell, ws, STEPS, batch, hidden)


def test_tickets_with_the_sign_bit_of_flags_and_the_wrap_to_one(hip):
    """Tickets 0x7FFFFF, 0x800000 (from here on the `flags` word is negative as an int),
    0xFFFFFE, 0xFFFFFF and then 1, on LSTM-1024 at 24 rows under RNN_F16 | RNN_XCD_SPLIT |
    RNN_STAGGER: every launch is accepted, computes what the untagged call computes (the low
    bits of `flags` still select the staggered kernel) and opens its own gate; after 0xFFFFFF the
    gate for 1 stays shut until the launch with ticket 1 has run.  The retired bit 8 is refused
    with a ticket above it as it is without."""
    cell, hidden, batch = 'lstm', 1024, 24
    fwd_flags, bwd_flags = _flags(hip, 'f16 stagger')
    assert bwd_flags == hip.RNN_F16 | hip.RNN_XCD_SPLIT | hip.RNN_STAGGER
    assert _bwd_kernels(hip, cell, hidden, STEPS, batch, bwd_flags, False) == \
        ['prnn_bwd16s_kernel']
    c = _case(hip, cell, hidden, STEPS, batch, False)
    want = _untagged(hip, cell, c, fwd_flags, bwd_flags, True)
    ws = hip.rnn_workspace(cell, STEPS, batch, hidden, DEV)
    gates = _Gates(hip, cell, ws, STEPS, batch, hidden)
    got = _Buffers(hip, cell, c, True)
    got.fwd(ws, fwd_flags)
    for ticket in (0x7FFFFF, 0x800000, 0xFFFFFE, 0xFFFFFF, 1):
        if ticket == 1:
            gates.shut(1)
        got.dxw.fill_(float('nan'))
        got.dbias.zero_()
        got.colmax.zero_()
        got.bwd(ws, bwd_flags, ticket=ticket)
        gates.open(ticket)
        _same_backward(got, want, hex(ticket))
    # the forward launch takes a negative `flags` word as well
    for ticket in (0x800000, LAST):
        ws_f = hip.rnn_workspace(cell, STEPS, batch, hidden, DEV)
        y = torch.full_like(got.y, float('nan'))
        got.fwd(ws_f, fwd_flags, ticket=ticket, y=y)
        _Gates(hip, cell, ws_f, STEPS, batch, hidden).open(ticket)
        hip.rnn_poll_error(cell, ws_f, STEPS, batch, hidden)
        assert torch.equal(y, want.y), hex(ticket)
    for ticket in (1, 0x800000, LAST):
        with pytest.raises(hip.CtcAsrError, match='bad argument'):
            got.fwd(ws, fwd_flags | 8, ticket=ticket)
        with pytest.raises(hip.CtcAsrError, match='bad argument'):
            got.bwd(ws, bwd_flags | 8, ticket=ticket)
    hip.rnn_poll_error(cell, ws, STEPS, batch, hidden)


@pytest.mark.parametrize('backward', [True, False])
def test_the_gate_opens_while_the_launch_is_still_running(hip, backward):
    """What the mechanism is for.  LSTM-1024, 16 rows, RUNNING_T steps: the backward pass under the
    default flags (128 CUs), the forward pass under RNN_HALF_CHIP.  The gate (100 ms bound) is
    enqueued on the side stream FIRST, the ticketed launch on the main stream after it: the
    gate's end event precedes the launch's, and the gate was open."""
    cell, hidden, batch, num_steps = 'lstm', 1024, 16, RUNNING_T
    g = torch.Generator(device=DEV).manual_seed(16)
    xw = torch.randn(num_steps, batch, 2, 4 * hidden, device=DEV, generator=g) * 0.5
    w = torch.randn(2, 4 * hidden, hidden, device=DEV, generator=g) / np.sqrt(hidden)
    ws = hip.rnn_workspace(cell, num_steps, batch, hidden, DEV)
    y, reserve, _ = hip.rnn_fwd(cell, xw, w, workspace=ws)
    if backward:
        dy = torch.randn(num_steps, batch, 2 * hidden, device=DEV, generator=g)
        wt = hip.transpose_batched(w)
        dxw = torch.empty(num_steps, batch, 2, 4 * hidden, device=DEV)
    ticket = 41
    torch.cuda.synchronize()
    events = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.stream(_side()):
        events[0].record()
        hip.rnn_resident_gate(cell, ws, num_steps, batch, hidden, ticket, OPEN_US)
        events[1].record()
    events[2].record()
    if backward:
        hip.rnn_bwd(cell, dy, y, wt, reserve, dxw=dxw, workspace=ws, ticket=ticket)
    else:
        hip.rnn_fwd(cell, xw, w, y=y, reserve=reserve, workspace=ws, flags=hip.RNN_HALF_CHIP,
                    ticket=ticket)
    events[3].record()
    torch.cuda.synchronize()
    gate_ms, launch_ms = events[0].elapsed_time(events[1]), events[2].elapsed_time(events[3])
    ahead_ms = events[1].elapsed_time(events[3])
    print('backward' if backward else 'forward', 'T', num_steps, 'gate', gate_ms, 'launch',
          launch_ms, 'gate end -> launch end', ahead_ms)
    hip.rnn_poll_error(cell, ws, num_steps, batch, hidden)
    assert launch_ms >= 20 * OPEN_GATE_MS, launch_ms
    assert gate_ms < 0.25 * OPEN_US / 1000, gate_ms
    assert ahead_ms > 0, (gate_ms, launch_ms, ahead_ms)


@pytest.mark.parametrize('cell,hidden,batch,flags,want_form', [
    # prnn_fwd_kernel and prnn_bwd_kernel; prnn_fwd16_kernel and prnn_bwd16_kernel;
    # prnn_bwd16s_kernel; prnn_bwd16w_kernel (four launches a pass); prnn_relu16_kernel
    ('lstm', 1024, 16, 'RNN_DEFAULT', 'fp32'),
    ('lstm', 1024, 16, 'RNN_F16', 'prnn_bwd16_kernel'),
    ('lstm', 1024, 24, 'RNN_F16 | RNN_STAGGER', 'prnn_bwd16s_kernel'),
    ('lstm', 2048, 17, 'RNN_F16', 'prnn_bwd16w_kernel'),
    ('rnn_relu', 2048, 1, 'RNN_F16', 'prnn_relu16_kernel')])
def test_a_poisoned_launch_still_posts_and_a_poll_forgets_the_ticket(hip, cell, hidden, batch,
                                                                      flags, want_form):
    """The time-out word set by hand (as in
    test_a_set_time_out_word_ends_every_later_launch_at_once): a ticketed launch leaves at once,
    its outputs untouched, but has posted - side-stream work behind its gate is not held for the
    whole bound on top of a failed step.  The poll reports the time-out and clears the block,
    the posted ticket with it: a gate for the old ticket is shut again.  The next ticketed launch
    is whole and posts."""
    flags = sum(getattr(hip, name) for name in flags.split(' | '))
    c = _case(hip, cell, hidden, STEPS, batch, False)
    forms = _bwd_kernels(hip, cell, hidden, STEPS, batch, flags, False)
    assert forms == [want_form]
    colmax_ok = _colmax_ok(hip, cell, STEPS, batch, hidden, flags, forms)
    want = _untagged(hip, cell, c, flags, flags, colmax_ok)
    ws = hip.rnn_workspace(cell, STEPS, batch, hidden, DEV)
    gates = _Gates(hip, cell, ws, STEPS, batch, hidden)
    address = hip.rnn_timeout_words(cell, ws, STEPS, batch, hidden)[0]
    offset = address - ws.data_ptr()
    ws[offset:offset + 4].view(torch.int32).fill_(1)
    got = _Buffers(hip, cell, c, colmax_ok, fill=7.0)
    got.fwd(ws, flags, ticket=21)
    gates.open(21)
    gates.shut(22)
    got.bwd(ws, flags, ticket=22, y=want.y)
    gates.open(22)
    torch.cuda.synchronize()
    assert bool((got.y == 7.0).all()) and bool((got.dxw == 7.0).all())      # nothing ran
    with pytest.raises(hip.CtcAsrError, match='time'):
        hip.rnn_poll_error(cell, ws, STEPS, batch, hidden)
    gates.shut(22)
    gates.shut(21)
    got.fwd(ws, flags, ticket=23)
    gates.open(23)
    gates.shut(24)
    got.dbias.zero_()
    got.bwd(ws, flags, ticket=24)
    gates.open(24)
    hip.rnn_poll_error(cell, ws, STEPS, batch, hidden)
    assert torch.equal(got.y, want.y)
    _same_backward(got, want, (cell, hidden, batch))


def test_gates_that_are_no_ops(hip, monkeypatch):
    """Shapes that take the streaming kernels (H = 64; H = 1024 under CTCASR_RNN_MODE=stream) and
    `max_wait_us` = 0: OK and no wait, even for a ticket nobody posts; a ticket on a streaming
    launch changes nothing."""
    quick = 0.25 * SHUT_US / 1000
    ws = hip.rnn_workspace('lstm', STEPS, 2, 64, DEV)
    assert not hip.rnn_persistent_supported('lstm', STEPS, 2, 64)
    assert _bracket_ms(lambda: hip.rnn_resident_gate('lstm', ws, STEPS, 2, 64, 9, OPEN_US)) < quick
    # a persistent shape, bound 0
    ws = hip.rnn_workspace('lstm', STEPS, 2, 1024, DEV)
    assert hip.rnn_persistent_supported('lstm', STEPS, 2, 1024)
    assert _bracket_ms(lambda: hip.rnn_resident_gate('lstm', ws, STEPS, 2, 1024, 9, 0)) < quick
    _Gates(hip, 'lstm', ws, STEPS, 2, 1024).shut(9)     # (the same gate with a bound does wait)
    monkeypatch.setenv('CTCASR_RNN_MODE', 'stream')
    assert not hip.rnn_persistent_supported('lstm', STEPS, 2, 1024)
    ws = hip.rnn_workspace('lstm', STEPS, 2, 1024, DEV)
    assert _bracket_ms(lambda: hip.rnn_resident_gate('lstm', ws, STEPS, 2, 1024, 9, OPEN_US)) < quick
    for hidden in (64, 1024):
        g = torch.Generator(device=DEV).manual_seed(hidden)
        xw = torch.randn(STEPS, 2, 2, 4 * hidden, device=DEV, generator=g) * 0.5
        w = torch.randn(2, 4 * hidden, hidden, device=DEV, generator=g) / np.sqrt(hidden)
        dy = torch.randn(STEPS, 2, 2 * hidden, device=DEV, generator=g)
        wt = hip.transpose_batched(w)
        out = []
        for ticket in (0, 77, LAST):
            y, reserve, ws = hip.rnn_fwd('lstm', xw, w, ticket=ticket)
            dxw = hip.rnn_bwd('lstm', dy, y, wt, reserve, workspace=ws, ticket=ticket)
            hip.rnn_poll_error('lstm', ws, STEPS, 2, hidden)
            out.append((y, dxw))
        for y, dxw in out[1:]:
            assert torch.equal(y, out[0][0]) and torch.equal(dxw, out[0][1]), hidden


def test_gates_that_are_refused_enqueue_nothing(hip):
    """Ticket 0 and 2^24, a bound of -1 and of 100001 us: `bad argument`; a workspace one byte
    short: the workspace error - each before anything is enqueued: the bracket around all of them,
    which would hold a 100 ms wait for a ticket nobody posts, is over at once."""
    cell, num_steps, batch, hidden = 'lstm', STEPS, 2, 1024
    ws = hip.rnn_workspace(cell, num_steps, batch, hidden, DEV)
    assert ws.numel() == hip.rnn_workspace_bytes(cell, num_steps, batch, hidden)

    def refusals():
        for ticket, bound in ((0, OPEN_US), (2 ** 24, OPEN_US), (9, -1), (9, OPEN_US + 1)):
            with pytest.raises(hip.CtcAsrError, match='bad argument'):
                hip.rnn_resident_gate(cell, ws, num_steps, batch, hidden, ticket, bound)
        with pytest.raises(hip.CtcAsrError, match='workspace'):
            hip.rnn_resident_gate(cell, ws[:-1], num_steps, batch, hidden, 9, OPEN_US)
    assert _bracket_ms(refusals) < 0.25 * OPEN_US / 1000
    # (the largest ticket and the largest bound are taken)
    _Gates(hip, cell, ws, num_steps, batch, hidden).shut(LAST)
    took = _bracket_ms(lambda: hip.rnn_resident_gate(cell, ws, num_steps, batch, hidden, 9, OPEN_US))
    assert 0.9 * OPEN_US / 1000 <= took <= OPEN_US / 1000 + SLACK_MS, took


def _launches_per_pass(cell, hidden, batch):
    """By the dispatch rules of `prnn_fwd` / `prnn_bwd`: one launch per block of at most 32 rows;
    the LSTM and the GRU at H = 2048 hold one direction's weights at a time - one launch per
    direction and 16-row tile of the block."""
    count = 0
    for b0 in range(0, batch, 32):
        rows = min(32, batch - b0)
        count += 2 * ((rows + 15) // 16) if hidden == 2048 and cell in ('lstm', 'gru') else 1
    return count


def test_kernel_events_count_the_persistent_launches(hip):
    """`set_option('rnn_kernel_events', 1)`: launches and their summed kernel times per direction
    of passes of known shape; a second read returns zeros; with the option off nothing is kept."""
    shapes = [('lstm', 1024, 24, 0), ('lstm', 1024, 40, 0), ('lstm', 2048, 17, 0),
              ('lstm', 2048, 33, hip.RNN_F16 | hip.RNN_KPAIR), ('gru', 2048, 33, 0),
              ('rnn_tanh', 2048, 33, 0), ('gru', 1024, 64, 0)]
    assert [_launches_per_pass(*s[:3]) for s in shapes] == [1, 2, 4, 6, 6, 2, 2]
    zeros = {'fwd': (0, 0.0), 'bwd': (0, 0.0)}
    hip.rnn_kernel_events()                 # (whatever an earlier test of this process left)
    try:
        hip.set_option('rnn_kernel_events', 1)
        assert hip.rnn_kernel_events() == zeros
        for cell, hidden, batch, flags in shapes:
            what = (cell, hidden, batch)
            c = _case(hip, cell, hidden, STEPS, batch, False)
            ws = hip.rnn_workspace(cell, STEPS, batch, hidden, DEV)
            got = _Buffers(hip, cell, c, False)
            want = _launches_per_pass(cell, hidden, batch)
            got.fwd(ws, flags)
            seen = hip.rnn_kernel_events()
            assert seen['fwd'][0] == want and seen['bwd'] == (0, 0.0), (what, seen)
            assert 0.0 < seen['fwd'][1] < 1000.0, (what, seen)
            assert hip.rnn_kernel_events() == zeros, what
            got.bwd(ws, flags)
            # a pass cut in two: twice the launches
            got.fwd(ws, flags, steps=(0, 1))
            got.fwd(ws, flags, steps=(1, STEPS))
            seen = hip.rnn_kernel_events()
            assert seen['bwd'][0] == want and seen['fwd'][0] == 2 * want, (what, seen)
            assert 0.0 < seen['bwd'][1] < 1000.0 and 0.0 < seen['fwd'][1] < 1000.0, (what, seen)
            assert hip.rnn_kernel_events() == zeros, what
            hip.rnn_poll_error(cell, ws, STEPS, batch, hidden)
        # with the option off nothing is recorded
        c = _case(hip, 'lstm', 1024, STEPS, 24, False)
        hip.set_option('rnn_kernel_events', 0)
        ws = hip.rnn_workspace('lstm', STEPS, 24, 1024, DEV)
        got = _Buffers(hip, 'lstm', c, False)
        got.fwd(ws, 0)
        got.bwd(ws, 0)
        hip.rnn_poll_error('lstm', ws, STEPS, 24, 1024)
        assert hip.rnn_kernel_events() == zeros
    finally:
        hip.set_option('rnn_kernel_events', 0)
        hip.rnn_kernel_events()


# ------------------------------------------------------------------ the model's bookkeeping
def _next(ticket):
    return ticket % 0xFFFFFF + 1


_STEPS_RUN = {}


def _model_step(hip, monkeypatch, env=(), hidden=1024, frames=71, first_ticket=None, key=None):
    """One training step (forward, loss, backward) of ds2_lstm_2conv at two rows on a fresh model
    built as tests/test_gpu_model.py builds it, CTCASR_FWD_CHUNKS=4 and CTCASR_BWD_CHUNKS=3, with
    `hip.rnn_fwd`, `hip.rnn_bwd` and `hip.rnn_resident_gate` recorded in enqueue order."""
    if key is not None and key in _STEPS_RUN:
        return _STEPS_RUN[key]
    from ctc_asr_amd.model import CTCModel
    cfg, flat, feats, flen, labels = _setup('ds2_lstm_2conv', hidden=hidden, frames=frames, batch=2)
    with monkeypatch.context() as patch:        # (the model reads these when it is built)
        patch.setenv('CTCASR_FWD_CHUNKS', '4')
        patch.setenv('CTCASR_BWD_CHUNKS', '3')
        for name, value in env:
            patch.setenv(name, value)
        model = CTCModel(cfg, 'cuda', params=flat)
    assert (model.fwd_chunks, model.bwd_chunks, cfg.num_layers_rnn) == (4, 3, 2)
    if first_ticket is not None:
        model._ticket = first_ticket
    start = model._ticket
    record = []
    real = {name: getattr(hip, name) for name in ('rnn_fwd', 'rnn_bwd', 'rnn_resident_gate')}

    def fwd(*args, **kwargs):
        record.append(('fwd', kwargs.get('ticket', 0), kwargs['workspace'].data_ptr()))
        return real['rnn_fwd'](*args, **kwargs)

    def bwd(*args, **kwargs):
        record.append(('bwd', kwargs.get('ticket', 0), kwargs['workspace'].data_ptr()))
        return real['rnn_bwd'](*args, **kwargs)

    def gate(cell, workspace, num_steps, batch, hid, ticket, max_wait_us=200):
        record.append(('gate', ticket, workspace.data_ptr()))
        assert max_wait_us == model.side_gate_max_us
        return real['rnn_resident_gate'](cell, workspace, num_steps, batch, hid, ticket,
                                         max_wait_us)

    with monkeypatch.context() as patch:
        patch.setattr(hip, 'rnn_fwd', fwd)
        patch.setattr(hip, 'rnn_bwd', bwd)
        patch.setattr(hip, 'rnn_resident_gate', gate)
        logits, seq_len = model.inference_fn(torch.tensor(feats), torch.tensor(flen),
                                             training=True)
        loss = model.loss_fn(logits, seq_len, labels)
        model.backward()
    torch.cuda.synchronize()
    assert model.step_guard().tolist() == [0, 0]
    model.check_rnn_error()
    out = dict(record=record, start=start, end=model._ticket, logits=logits.cpu().numpy(),
               loss=float(loss), grads=model.arena.export('grad'))
    if key is not None:
        _STEPS_RUN[key] = out
    return out


def _check_record(run):
    """The rules of the ticket count, on a step's record.  -> (forward gates, backward gates)."""
    record = run['record']
    ticket = run['start']
    for kind, carried, _ in record:
        if kind != 'gate' and carried:
            ticket = _next(ticket)
            assert carried == ticket and 1 <= carried <= LAST, (kind, hex(carried), hex(ticket))
    assert ticket == run['end']
    gates = {'fwd': 0, 'bwd': 0}
    for at, (kind, named, workspace) in enumerate(record):
        if kind != 'gate':
            continue
        assert 1 <= named <= LAST
        later = [r for r in record[at + 1:] if r[0] != 'gate' and r[1] and r[2] == workspace]
        assert later, ('a gate for a launch that never comes', at, hex(named))
        assert later[0][1] == named, (at, hex(named), hex(later[0][1]))
        gates[later[0][0]] += 1
    return gates['fwd'], gates['bwd']


def _same_step(got, want, bits):
    """The bars of test_pipelined_forward_equals_single_launch_forward; ``bits``: bit for bit."""
    assert np.abs(got['logits'] - want['logits']).max() < 1e-5
    assert abs(got['loss'] - want['loss']) < 1e-4
    for name, ref_g in want['grads'].items():
        err = np.abs(got['grads'][name] - ref_g).max()
        assert err < 1e-5 * max(1.0, np.abs(ref_g).max()), (name, err)
    if bits:
        assert np.array_equal(got['logits'], want['logits']) and got['loss'] == want['loss']
        for name, ref_g in want['grads'].items():
            assert np.array_equal(got['grads'][name], ref_g), name


def _default_steps(hip, monkeypatch):
    """Two fresh default steps, and whether they agree bit for bit (on the MI355X they did not:
    the bias gradients' atomics have no fixed order - then the bars alone decide)."""
    first = _model_step(hip, monkeypatch, key='default 1')
    second = _model_step(hip, monkeypatch, key='default 2')
    bits = (np.array_equal(first['logits'], second['logits']) and
            first['loss'] == second['loss'] and
            all(np.array_equal(first['grads'][n], second['grads'][n]) for n in first['grads']))
    print('two default steps agree bit for bit:', bits)
    return first, second, bits


def test_the_model_gates_each_side_stream_batch_on_the_next_launch(hip, monkeypatch):
    """Pipelined forward (layer 0 in four launches) and chunked backward (both layers in three):
    tickets rise by one per ticketed launch, every gate names the NEXT ticketed launch on its
    workspace, and that launch comes within the step."""
    first, second, _ = _default_steps(hip, monkeypatch)
    for run in (first, second):
        assert run['start'] == 0
        fwd_gates, bwd_gates = _check_record(run)
        launches = [r for r in run['record'] if r[0] != 'gate']
        # layer 0 forward: 4 ticketed half-chip launches, 3 gates between them; layer 1: one launch
        # without a ticket; backward: 2 layers x 3 ticketed launches, a gate in front of each
        assert [r[1] != 0 for r in launches if r[0] == 'fwd'] == [True] * 4 + [False]
        assert [r[1] != 0 for r in launches if r[0] == 'bwd'] == [True] * 6
        assert (fwd_gates, bwd_gates) == (3, 6), run['record']
        assert run['end'] == 10
    _same_step(second, first, False)


def test_the_model_without_gates_and_without_the_side_stream(hip, monkeypatch):
    first, _, bits = _default_steps(hip, monkeypatch)
    run = _model_step(hip, monkeypatch, env=[('CTCASR_SIDE_GATE_US', '0')])
    assert not [r for r in run['record'] if r[0] == 'gate']
    assert _check_record(run) == (0, 0) and run['end'] == first['end']
    _same_step(run, first, bits)
    run = _model_step(hip, monkeypatch, env=[('CTCASR_OVERLAP_WGRAD', '0')])
    fwd_gates, bwd_gates = _check_record(run)
    assert fwd_gates == 3 and bwd_gates == 0
    _same_step(run, first, False)


def test_the_whole_chip_backward_carries_no_ticket(hip, monkeypatch):
    """LSTM-2048: the backward recurrence takes all 256 CUs one direction at a time - nothing runs
    beside it, no backward launch carries a ticket and no gate waits for one."""
    run = _model_step(hip, monkeypatch, hidden=2048, frames=39)
    assert _check_record(run)[1] == 0
    backward = [r for r in run['record'] if r[0] == 'bwd']
    assert len(backward) == 2 and not any(r[1] for r in backward)
    assert not [r for r in run['record'] if r[0] == 'gate']


def test_a_step_across_the_wrap_of_the_ticket_count(hip, monkeypatch):
    """A step that starts two tickets before 0xFFFFFF: the count goes ... 0xFFFFFE, 0xFFFFFF, 1,
    2 ... - never 0 - the record obeys the same rules and the step computes what a fresh model's
    does."""
    first, _, bits = _default_steps(hip, monkeypatch)
    run = _model_step(hip, monkeypatch, first_ticket=LAST - 2)
    carried = [r[1] for r in run['record'] if r[0] != 'gate' and r[1]]
    assert carried == [LAST - 1, LAST] + list(range(1, 9))
    assert _check_record(run) == (3, 6)
    assert run['end'] == 8
    _same_step(run, first, bits)
