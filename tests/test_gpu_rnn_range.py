"""Every recurrence variant across the float range - the values the edge-shape tests never feed:
one NaN (it must stay in its row and direction and reach everything after it, so that the loss
turns NaN and the step is dropped), +-inf, NaN in the frames past a row's length, saturated
gates, gradients scaled by powers of two (the fp16-pipe kernels pick every scale from an exponent:
a pass is linear in dy bit for bit), all-zero gradient rows.

Shapes: T = 3; H = 1024 at batches 3 (one padded tile), 24 (two tiles, a multiple of 8: the
staggered kernel) and 40 (two row blocks), H = 2048 at 3, 17 and 40; with and without
per-row lengths.  References: tests/rnn_reference.py in float64 (NaN masks also in closed form,
tests/test_rnn_reference.py checks those on the CPU), and the SAME kernel's pass without the
special value - rows are independent recurrences, so everything outside the touched row and
direction is compared bit for bit.  No bar of its own: bit equality, or the bars of
`_check_pass` (tests/test_gpu_rnn_edges.py).  `_pass` polls the time-out words after every pass."""

import pytest
import torch

from tests import rnn_reference
from tests.test_gpu_rnn_edges import (FAMILIES, VARIANTS, _bwd_kernels, _case, _check_pass, _flags,
                                      _fwd_is_f16, _pass)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = 3
BATCHES = {1024: (3, 24, 40), 2048: (3, 17, 40)}
NAN, INF = float('nan'), float('inf')


def _must_run(cell, hidden, variant):
    """The kernel forms a (family, variant) has to reach over the batches of this file (without
    per-row lengths), else the variant no longer tests the kernel it exists for: backward forms as
    `_bwd_kernels` names them, 'fwd16' for an fp16-pipe forward pass."""
    if variant == 'stream':
        return {'stream'}
    if variant in ('fp32', 'whole chip', 'one barrier'):
        return {'fp32'}
    if cell == 'lstm' and hidden == 1024:
        # ('f16 k-pair': the bit is ignored at this size, the plain kernel runs)
        return {'fwd16', 'prnn_bwd16_kernel'} | {'f16 stagger': {'prnn_bwd16s_kernel'}}.get(
            variant, set())
    if cell == 'lstm':
        return {'fwd16', 'prnn_bwd16w_kernel<k-pair>' if variant == 'f16 k-pair'
                else 'prnn_bwd16w_kernel'}
    if cell == 'gru':
        return {'fwd16', 'fp32'}
    if cell == 'rnn_relu':
        return {'fwd16', 'prnn_relu16_kernel', 'fp32'}
    return {'fp32'}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b, keep=None):
    """a and b bit for bit (where ``keep``, a bool mask that broadcasts, is set)."""
    a, b = _bits(a), _bits(b)
    if keep is None:
        return torch.equal(a, b)
    return bool(((a == b) | ~keep).all())


def _frames(reserve, cell, batch, hidden):
    """The reserve as float32 [part][T, B, 2, columns]: LSTM gates and cells; GRU r, z, n, q and
    drec (include/ctcasr.h); the plain cells keep none."""
    if cell not in ('lstm', 'gru'):
        return []
    words = reserve.view(torch.float32)
    cut = T * batch * 2 * 4 * hidden
    return [words[:cut].view(T, batch, 2, 4 * hidden),
            words[cut:].view(T, batch, 2, -1)]


def _colmax_of(dxw):
    """What `colmax_kernel` (split.hip) finds in a pass over dxw: fmaxf skips a NaN."""
    return torch.nan_to_num(dxw.abs(), nan=0.0, posinf=INF).amax(dim=(0, 1)).reshape(-1)


class _Family:
    """One (cell, H, variant) at one (batch, lengths): the clean pass and the checks against it."""

    def __init__(self, hip, cell, hidden, variant, batch, lengths):
        self.hip, self.cell, self.hidden, self.variant = hip, cell, hidden, variant
        self.batch, self.lengths = batch, lengths
        self.gates = hip.CELL_GATES[cell]
        self.fwd_flags, self.bwd_flags = _flags(hip, variant)
        self.c = _case(hip, cell, hidden, T, batch, lengths)
        assert hip.rnn_persistent_supported(cell, T, batch, hidden) == (variant != 'stream')
        self.forms = _bwd_kernels(hip, cell, hidden, T, batch, self.bwd_flags, lengths)
        self.fwd16 = self.forms != ['stream'] and _fwd_is_f16(hip, cell, hidden, T, batch,
                                                              self.fwd_flags, lengths)
        self.colmax_ok = self.forms != ['stream'] and hip.rnn_bwd_f16_supported(
            cell, T, batch, hidden, self.bwd_flags) and not (cell == 'rnn_relu' and lengths)
        self.what = (cell, hidden, variant, batch, lengths)
        self.clean = self.run(self.c)
        for part in self.clean[:3]:
            assert torch.isfinite(part).all(), self.what

    def run(self, c):
        return _pass(self.hip, self.cell, c, self.fwd_flags, self.bwd_flags, self.colmax_ok)

    def check(self, c, got, check_y=True):
        _check_pass(self.hip, self.cell, self.hidden, c, self.variant, self.fwd_flags,
                    self.bwd_flags, self.forms, got, check_y=check_y)

    def reference(self, c, y):
        """(y, dxw, NaN mask of dbias) in float64; the ReLU cell's dxw by the select on the
        kernel's own ``y``."""
        ref_y, ref_dxw, ref_dbias = rnn_reference.forward_backward(
            self.cell, c['xw'], c['w'], c['dy'], c['b_hh'], c['sl'], c['bias'])
        if self.cell != 'rnn_relu':
            return ref_y, ref_dxw, ~torch.isfinite(ref_dbias)
        ref_dxw = rnn_reference.relu_backward(y, c['dy'], c['w'], c['sl'])
        return ref_y, ref_dxw, (~torch.isfinite(ref_dxw)).any(dim=(0, 1)).reshape(-1)

    def rows(self):
        """Row 0, the last row, the first row of the second tile and of the second block."""
        return sorted({0, self.batch - 1} | {r for r in (16, 32) if r < self.batch})

    def units(self):
        return (0, self.hidden // 2 + 5, self.hidden - 1)

    def check_touched(self, c, got, row, d, exact, why, moved=False):
        """A pass with one special value in (row, d) against the float64 reference and the clean
        pass.  ``exact``: the kernel's NaN masks ARE the reference's, and everything outside them
        equals the clean pass bit for bit - unless the value ``moved`` finite results inside
        (row, d) (a saturated gate), which the caller then checks against float64; the ReLU
        cell's dxw inside (row, d) follows a changed y: the bars of `_check_pass` on the kernel's
        own y.  Not ``exact`` (inf: the fp16 pieces
        of inf are inf and NaN): the kernel's non-finite set contains the reference's and stays
        inside (row, d).  Either way every other row and direction equals the clean pass bit for
        bit, the bias gradients of untouched columns are within 1e-4 of the clean pass, and the
        column maxima are those of a NaN-skipping pass over dxw."""
        y, dxw, dbias, colmax, reserve, _ = got
        cy, cdxw, cdbias, _, creserve, _ = self.clean
        hidden, gh = self.hidden, self.gates * self.hidden
        why = self.what + why
        ref_y, ref_dxw, ref_dbias_bad = self.reference(c, y)
        y4 = y.view(T, self.batch, 2, hidden)
        bad_y, bad_dxw = ~torch.isfinite(y4), ~torch.isfinite(dxw)
        ref_bad_y = ~torch.isfinite(ref_y).view(T, self.batch, 2, hidden)
        ref_bad_dxw = ~torch.isfinite(ref_dxw)
        inside = torch.zeros(T, self.batch, 2, 1, dtype=torch.bool, device=DEV)
        inside[:, row, d] = True
        if exact:
            assert torch.equal(y4.isnan(), ref_bad_y), (why, 'isnan(y)')
            assert torch.equal(dxw.isnan(), ref_bad_dxw), (why, 'isnan(dxw)')
            assert torch.equal(bad_y, ref_bad_y) and torch.equal(bad_dxw, ref_bad_dxw), why
            keep_y, keep_dxw = ~ref_bad_y, ~ref_bad_dxw
            relu_moved = self.cell == 'rnn_relu' and bool(ref_bad_y.any())
            if moved:
                keep_y = keep_y & ~inside
            if moved or relu_moved:
                keep_dxw = keep_dxw & ~inside
        else:
            assert bool((bad_y | ~ref_bad_y).all()), (why, 'y: a non-finite value lost')
            assert bool((bad_dxw | ~ref_bad_dxw).all()), (why, 'dxw: a non-finite value lost')
            assert not bool((bad_y & ~inside).any()), (why, 'y: left its row')
            assert not bool((bad_dxw & ~inside).any()), (why, 'dxw: left its row')
            keep_y = keep_dxw = ~inside
        assert _same_bits(y4, cy.view(T, self.batch, 2, hidden), keep_y), (why, 'y')
        assert _same_bits(dxw, cdxw, keep_dxw), (why, 'dxw')
        # the reserve, frame by frame: a frame is touched where y or (the GRU's drec) dxw is
        whole = moved or not exact
        touched_fwd = inside if whole else ref_bad_y.any(dim=3, keepdim=True)
        touched_bwd = inside if whole else touched_fwd | ref_bad_dxw.any(dim=3, keepdim=True)
        parts, cparts = _frames(reserve, self.cell, self.batch, hidden), \
            _frames(creserve, self.cell, self.batch, hidden)
        for k, (part, cpart) in enumerate(zip(parts, cparts)):
            touched = touched_bwd if (self.cell, k) == ('gru', 1) else touched_fwd
            assert _same_bits(part, cpart, ~touched), (why, 'reserve', k)
        # the bias gradients: a column that sums a NaN is NaN; the others as the clean pass
        half = torch.zeros(2, dbias.numel() // (2 * gh), gh, dtype=torch.bool, device=DEV)
        half[d] = True                            # the columns of direction d ([part][dir][G*H])
        half = half.transpose(0, 1).reshape(-1)
        bad_dbias = ~torch.isfinite(dbias)
        if exact:
            assert torch.equal(dbias.isnan(), ref_dbias_bad), (why, 'dbias')
            untouched = ~ref_dbias_bad
            if moved or relu_moved:
                untouched = untouched & ~half
        else:
            assert bool((bad_dbias | ~ref_dbias_bad).all()), (why, 'dbias')
            assert not bool((bad_dbias & ~half).any()), (why, 'dbias: left its direction')
            untouched = ~half
        err = ((dbias - cdbias).abs() * untouched).nan_to_num(nan=0.0, posinf=0.0).max()
        assert float(err) < 1e-4 * max(1.0, float(cdbias.abs().max())), (why, 'dbias', float(err))
        if exact and relu_moved:
            self.check(c, got, check_y=False)
        if colmax is not None:
            assert torch.equal(_bits(colmax), _bits(_colmax_of(dxw))), (why, 'colmax')

    # ---- a. one NaN ----------------------------------------------------------------------------
    def one_nan(self):
        c, hidden, sl = self.c, self.hidden, self.c['sl']
        cy = self.clean[0].view(T, self.batch, 2, hidden)
        k = 0
        for row in self.rows():
            for d in (0, 1):
                for unit in self.units():
                    # forward: xw[1, row, d, a gate column of the unit]
                    xw = c['xw'].clone()
                    xw[1, row, d, (k % self.gates) * hidden + unit] = NAN
                    k += 1
                    p = dict(c, xw=xw)
                    got = self.run(p)
                    want = rnn_reference.nan_mask_forward(T, self.batch, hidden, 1, row, d, unit,
                                                          sl).to(DEV)
                    assert torch.equal(got[0].view(T, self.batch, 2, hidden).isnan(), want), \
                        self.what + ('xw', row, d, unit)
                    self.check_touched(p, got, row, d, True, ('NaN in xw', row, d, unit))
                    # backward: dy[1, row, d H + unit] after a clean forward pass; the ReLU
                    # cell's derivative is a select on y > 0: a live unit nearest to this one
                    if self.cell == 'rnn_relu':
                        live = (cy[1, row, d] > 0).nonzero().view(-1)
                        if live.numel():
                            unit = int(live[(live - unit).abs().argmin()])
                    dy = c['dy'].clone()
                    dy[1, row, d * hidden + unit] = NAN
                    p = dict(c, dy=dy)
                    got = self.run(p)
                    assert _same_bits(got[0], self.clean[0]), self.what
                    want = rnn_reference.nan_mask_backward(T, self.batch, hidden, self.gates, 1,
                                                           row, d, unit, sl).to(DEV)
                    if self.cell == 'rnn_relu':
                        want &= cy > 0
                    assert torch.equal(got[1].isnan(), want), self.what + ('dy', row, d, unit)
                    self.check_touched(p, got, row, d, True, ('NaN in dy', row, d, unit))

    # ---- b. +-inf ------------------------------------------------------------------------------
    def infinities(self):
        c, hidden = self.c, self.hidden
        row, unit = self.rows()[-2], self.units()[1]
        for d, value in ((0, INF), (1, -INF)):
            xw = c['xw'].clone()
            xw[1, row, d, (self.gates - 1 - d) * hidden + unit] = value
            if self.cell != 'rnn_relu':
                # the gate saturates: finite everywhere, inside the bars against float64
                ref_y, ref_dxw, _ = rnn_reference.forward_backward(
                    self.cell, xw, c['w'], c['dy'], c['b_hh'], c['sl'], c['bias'])
                assert torch.isfinite(ref_y).all() and torch.isfinite(ref_dxw).all()
                p = dict(c, xw=xw, ref_y=ref_y, ref_dxw=ref_dxw)
                got = self.run(p)
                for part in got[:3]:
                    assert torch.isfinite(part).all(), self.what + ('inf in xw', value)
                self.check(p, got)
                self.check_touched(p, got, row, d, True, ('inf in xw', value), moved=True)
            elif value > 0:
                p = dict(c, xw=xw)
                self.check_touched(p, self.run(p), row, d, False, ('inf in xw',))
            dy = c['dy'].clone()
            dy[1, row, d * hidden + unit] = value
            p = dict(c, dy=dy)
            self.check_touched(p, self.run(p), row, d, False, ('inf in dy', value))

    # ---- c. garbage past a row's length -----------------------------------------------------------
    def garbage_past_the_length(self):
        c = self.c
        if c['sl'] is None:
            return
        past = torch.arange(T, device=DEV).view(T, 1) >= c['sl'].view(1, -1)       # [T, B]
        assert bool(past[1:, -1].all()) and not bool(past[:, 0].any())
        xw, dy = c['xw'].clone(), c['dy'].clone()
        xw[past] = NAN
        dy[past] = NAN
        got = self.run(dict(c, xw=xw, dy=dy))
        for name, a, b in zip(('y', 'dxw'), got[:2], self.clean[:2]):
            assert _same_bits(a, b), self.what + ('garbage past the length', name)
        # (the bias gradients are atomic adds in no fixed order - include/ctcasr.h; the streaming
        # path's differ in the last bit from run to run on the SAME input: to rounding, as below)
        assert float((got[2] - self.clean[2]).abs().max()) <= \
            1e-5 * float(self.clean[2].abs().max()), self.what + ('garbage past the length', 'dbias')
        if got[3] is not None:
            assert torch.equal(got[3], self.clean[3]), self.what
        assert bool((got[0][past] == 0).all()) and bool((got[1][past] == 0).all()), self.what

    # ---- d. saturated gates ---------------------------------------------------------------------
    def saturated_gates(self):
        c = self.c
        if self.cell == 'rnn_relu':
            return
        for factor in (40.0, 1e4):
            xw = c['xw'] * factor
            ref_y, ref_dxw, _ = rnn_reference.forward_backward(
                self.cell, xw, c['w'], c['dy'], c['b_hh'], c['sl'], c['bias'])
            p = dict(c, xw=xw, ref_y=ref_y, ref_dxw=ref_dxw)
            got = self.run(p)
            for part in got[:3]:
                assert torch.isfinite(part).all(), self.what + ('xw x', factor)
            self.check(p, got)

    # ---- e. powers of two -----------------------------------------------------------------------
    def powers_of_two(self):
        c = self.c
        y, dxw, dbias, colmax = self.clean[:4]
        for k in (48, -48, 90, -90):
            f = 2.0 ** k
            why = self.what + ('dy x 2^', k)
            p = dict(c, dy=c['dy'] * f, ref_dxw=c['ref_dxw'] * f)
            got = self.run(p)
            assert _same_bits(got[0], y), why
            if abs(k) == 90:
                # (some rows' scale sits at the clamp of +-100 binades: accuracy only)
                self.check(p, got)
                continue
            assert _same_bits(got[1], dxw * f), why
            assert float((got[2] - dbias * f).abs().max()) <= 1e-5 * float((dbias * f).abs().max()), \
                why
            if colmax is not None:
                assert _same_bits(got[3].view(torch.float32), colmax.view(torch.float32) * f), why
        if self.cell == 'rnn_relu':
            # the ReLU cell's forward pass is positively homogeneous
            for k in (48, -48):
                f = 2.0 ** k
                y_k, _, ws = self.hip.rnn_fwd(self.cell, c['xw'] * f, c['w'], c['sl'],
                                              flags=self.fwd_flags, xw_bias=c['bias'] * f)
                self.hip.rnn_poll_error(self.cell, ws, T, self.batch, self.hidden)
                assert _same_bits(y_k, y * f), self.what + ('xw x 2^', k)

    # ---- f. all-zero gradients ---------------------------------------------------------------
    def zero_gradients(self):
        c, row = self.c, self.rows()[-2]
        others = torch.ones(1, self.batch, 1, 1, dtype=torch.bool, device=DEV)
        others[:, row] = False
        dy = c['dy'].clone()
        dy[:, row] = 0
        got = self.run(dict(c, dy=dy))
        why = self.what + ('zero dy row', row)
        assert bool((got[1][:, row] == 0).all()), why
        assert _same_bits(got[0], self.clean[0]), why
        assert _same_bits(got[1], self.clean[1], others), why
        if got[3] is not None:
            assert torch.equal(_bits(got[3]), _bits(_colmax_of(got[1]))), why
        got = self.run(dict(c, dy=torch.zeros_like(dy)))
        why = self.what + ('zero dy',)
        assert _same_bits(got[0], self.clean[0]), why
        assert bool((got[1] == 0).all()) and bool((got[2] == 0).all()), why
        if got[3] is not None:
            assert bool((got[3] == 0).all()), why


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cell,hidden', FAMILIES)
def test_every_variant_across_the_float_range(hip, cell, hidden, variant, monkeypatch):
    """Groups a - f of the module docstring for one (cell, H, variant), at every batch of
    BATCHES with and without per-row lengths.

    The power-of-two identity dxw(2^k dy) == 2^k dxw(dy) and, for the ReLU cell,
    y(2^k xw, 2^k bias) == 2^k y are asserted bit for bit at k = +-48 for every variant (measured:
    they hold in all 42 cases, the fp32 and streaming kernels included); at k = +-90 (the per-row
    scale clamps at +-100 binades) the bars of `_check_pass` hold against the float64 result
    times 2^k.  The bias gradients are compared to rounding (1e-5 of their largest) wherever
    two passes are compared, group c included: their atomic adds have no fixed order
    (include/ctcasr.h), and the streaming path's sums differed in the last bit between two passes
    over the same dxw."""
    if variant == 'stream':
        monkeypatch.setenv('CTCASR_RNN_MODE', 'stream')
    ran = set()
    for batch in BATCHES[hidden]:
        for lengths in (False, True):
            fam = _Family(hip, cell, hidden, variant, batch, lengths)
            if not lengths:
                ran |= set(fam.forms) | ({'fwd16'} if fam.fwd16 else set())
            fam.one_nan()
            fam.infinities()
            fam.garbage_past_the_length()
            fam.saturated_gates()
            fam.powers_of_two()
            fam.zero_gradients()
    assert _must_run(cell, hidden, variant) <= ran, (cell, hidden, variant, sorted(ran))
