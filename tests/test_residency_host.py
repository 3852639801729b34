"""The arithmetic of the residency hand-shake, restated in plain Python integers and held against
`CTCModel`'s own ticket count (no device).

Two rules.  The gate (`resident_gate_kernel`, include/ctcasr.h) opens iff the workspace's posted
word `seen` is not 0 and ``((seen - ticket) & 0xFFFFFF) < 0x800000``.  The model numbers its
persistent launches ``next = t % 0xFFFFFF + 1``: 1 .. 2^24 - 1 and round again, never 0 - 0 is
"no ticket" in a launch's flags and "nothing posted" in the workspace."""

import random

import numpy as np
import pytest

from ctc_asr_amd.model import CTCModel, ModelConfig

LAST = 0xFFFFFF          # the largest ticket
HALF = 0x800000          # tickets the gate looks back over


def gate_opens(seen, ticket):
    return seen != 0 and ((seen - ticket) & 0xFFFFFF) < HALF


def next_ticket(t):
    return t % 0xFFFFFF + 1


class _Count:
    """What `_upcoming_ticket` / `_take_ticket` need of a model: the count (and each other - the
    model's own functions, borrowed)."""
    _upcoming_ticket = CTCModel._upcoming_ticket
    _take_ticket = CTCModel._take_ticket

    def __init__(self, ticket):
        self._ticket = ticket


def _model_next(t):
    return CTCModel._upcoming_ticket(_Count(t))


def _some_tickets():
    rng = random.Random(24)
    near_wrap = list(range(LAST - 63, LAST + 1)) + list(range(1, 65))
    return near_wrap + [rng.randint(1, LAST) for _ in range(1000)]


def test_the_sequence_visits_every_ticket_but_zero_and_wraps_to_one():
    assert next_ticket(0) == 1 and next_ticket(LAST) == 1 and next_ticket(LAST - 1) == LAST
    # one cycle over 1 .. 2^24 - 1: every ticket but the last is followed by the one above it,
    # the last by 1 (all 2^24 - 1 of them, in int64)
    tickets = np.arange(1, LAST + 1, dtype=np.int64)
    after = tickets % 0xFFFFFF + 1
    assert np.array_equal(after[:-1], tickets[1:]) and after[-1] == 1
    assert after.min() == 1 and after.max() == LAST
    for t in (1, 2, HALF - 1, HALF, LAST - 1, LAST):
        assert next_ticket(t) == after[t - 1]


def test_the_model_counts_as_the_rule_says():
    for t in [0] + _some_tickets():
        assert _model_next(t) == next_ticket(t), t
        assert 1 <= _model_next(t) <= LAST
    count = _Count(LAST - 2)
    took = [CTCModel._take_ticket(count) for _ in range(5)]
    assert took == [LAST - 1, LAST, 1, 2, 3] and count._ticket == 3
    # looking ahead moves nothing
    assert CTCModel._upcoming_ticket(count) == 4 and count._ticket == 3


def test_a_gate_waits_for_its_own_launch_and_not_for_an_earlier_one():
    for t in _some_tickets():
        nxt = _model_next(t)
        assert not gate_opens(t, nxt), t          # launch t has posted, the gate is for the next
        assert gate_opens(nxt, nxt), t            # ... which has now posted
        assert gate_opens(nxt, t), t              # a stale gate for the launch before
        assert gate_opens(t, t), t


def test_a_fresh_word_opens_for_no_ticket():
    # (the modular comparison alone would pass every ticket above 2^23: 0 - ticket mod 2^24 is
    # then below 2^23)
    for t in _some_tickets() + [HALF - 1, HALF, HALF + 1, LAST]:
        assert not gate_opens(0, t), t
    assert ((0 - (HALF + 1)) & 0xFFFFFF) < HALF


def test_the_gate_looks_back_over_two_to_the_23_tickets():
    """The comparison is modular, so "posted at or after my ticket" can only mean "up to 2^23 - 1
    tickets after it".  A gate for a ticket that lies 2^23 or more AHEAD of the posted word - the
    same as a word last posted more than 2^23 tickets ago, seen from the ticket count going round -
    opens at once instead of waiting: the side-stream work then starts without its head start, a
    late start of the recurrence, never a wrong result."""
    rng = random.Random(23)
    for seen in [1, 2, HALF - 1, HALF, HALF + 1, LAST] + [rng.randint(1, LAST) for _ in range(200)]:
        def ahead(k):        # the ticket k launches after `seen`, in the model's order
            return (seen + k - 1) % LAST + 1
        # the model's order skips 0, the gate's arithmetic does not: the ticket k launches ahead of
        # the posted word is k (no wrap between them) or k + 1 (a wrap) ahead of it modulo 2^24 -
        # shut up to k = 2^23 - 1, open from k = 2^23 + 1, either at k = 2^23
        for k in (1, 2, 1000, HALF - 2, HALF - 1):
            assert not gate_opens(seen, ahead(k)), (seen, k)
        for k in (HALF + 1, HALF + 1000, LAST - 1):
            assert gate_opens(seen, ahead(k)), (seen, k)
        # in the gate's own arithmetic the window is exact: open from seen - (2^23 - 1) up to
        # seen, shut from seen + 1 up to seen + 2^23
        for back in (0, 1, HALF - 1):
            ticket = (seen - back) & 0xFFFFFF
            assert ticket == 0 or gate_opens(seen, ticket), (seen, back)
        for fwd in (1, HALF - 1, HALF):
            ticket = (seen + fwd) & 0xFFFFFF
            assert ticket == 0 or not gate_opens(seen, ticket), (seen, fwd)
        ticket = (seen + HALF + 1) & 0xFFFFFF
        assert ticket == 0 or gate_opens(seen, ticket), (seen, ticket)


def _tiny_config():
    return ModelConfig(used_model='ds2', conv_filters=(4, 4), num_units_dense=8, num_layers_rnn=1,
                       num_units_rnn=64, rnn_cell='lstm', cudnn=True)


class _Reached(Exception):
    pass


def test_a_gate_bound_the_library_refuses_is_refused_when_the_model_is_built(monkeypatch):
    """CTCASR_SIDE_GATE_US above the 100 ms that `ctcasr_rnn_resident_gate` takes: a ValueError
    from the constructor, before the device is touched - not `bad argument` out of the first
    training step.  100 ms itself, 0 (no gates) and the default pass that check."""
    from ctc_asr_amd import hip, model

    def stop():
        raise _Reached()
    monkeypatch.setattr(model.hip, 'load', stop)
    assert hip.RESIDENT_GATE_MAX_US == 100000
    for value in ('100001', '1000000', str(2 ** 31)):
        monkeypatch.setenv('CTCASR_SIDE_GATE_US', value)
        with pytest.raises(ValueError, match='CTCASR_SIDE_GATE_US'):
            CTCModel(_tiny_config())
    for value in ('100000', '300', '0'):
        monkeypatch.setenv('CTCASR_SIDE_GATE_US', value)
        with pytest.raises(_Reached):
            CTCModel(_tiny_config())
    monkeypatch.delenv('CTCASR_SIDE_GATE_US')
    with pytest.raises(_Reached):
        CTCModel(_tiny_config())
