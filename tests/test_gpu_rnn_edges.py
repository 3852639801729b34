"""Every persistent recurrence variant (and the streaming kernels) at the shapes where a pipelined
kernel goes wrong first: T = 1 (each step is the pipeline's prologue and epilogue at once: the
prefetch guards, the all-zero h(-1) block and the stagger's half-step offset meet), T = 2 and 3
(odd step counts against the K-pair tag parity), batches of one and two rows, a tile of one row,
and two row blocks - where `prnn_bwd` hands each 32-row block its own rows as B and the whole batch
as the row stride (block 1 of B = 56 and both blocks of B = 64 take the staggered kernel with
B != BS).  Per pass: y and dxw against the float64 recurrence and autograd
(tests/rnn_reference.py) inside the bars of each kernel's own test, the column maxima bit for bit,
the bias gradients against the kernel's own dxw, which kernel form ran, a clean time-out poll;
T = 3 cut into single-step launches; one workspace across T = 3, 1, 2, 3, 1."""

import numpy as np
import pytest
import torch

from tests import rnn_reference
from tests.test_gpu_kernels import _Pass, _assert_same_pass

pytestmark = pytest.mark.gpu
DEV = 'cuda'

FAMILIES = [('lstm', 1024), ('gru', 1024), ('lstm', 2048), ('gru', 2048), ('rnn_relu', 2048),
            ('rnn_tanh', 2048)]
VARIANTS = ['fp32', 'whole chip', 'one barrier', 'f16 stagger', 'f16 k-pair',
            'f16 half-chip forward', 'stream']
# (the K-pair form exists at H = 2048 only)
CASES = [(cell, hidden, variant) for variant in VARIANTS for cell, hidden in FAMILIES
         if variant != 'f16 k-pair' or hidden == 2048]
STEPS = (1, 2, 3)
BATCHES = {1024: (1, 2, 8, 15, 16, 17, 24, 31, 32, 33, 40, 48, 56, 64),
           2048: (1, 2, 16, 17, 32, 33, 56, 64)}
# the batches at which a variant must take the kernel it exists for (no per-row lengths)
MUST_RUN = {('lstm', 1024, 'f16 stagger'): ('prnn_bwd16s_kernel', {24, 32, 56, 64}),
            ('lstm', 2048, 'f16 k-pair'): ('prnn_bwd16w_kernel<k-pair>', set(BATCHES[2048]))}


def _flags(h, variant):
    """(forward flags, backward flags) of a variant (those of
    test_no_persistent_kernel_reads_the_pass_before; 'stream' forces the per-step kernels)."""
    f16 = h.RNN_F16 | h.RNN_XCD_SPLIT
    return {'fp32': (0, 0), 'whole chip': (0, h.RNN_WHOLE_CHIP),
            'one barrier': (h.RNN_ONE_BARRIER, h.RNN_ONE_BARRIER),
            'f16 stagger': (f16, f16 | h.RNN_STAGGER), 'f16 k-pair': (f16, f16 | h.RNN_KPAIR),
            'f16 half-chip forward': (h.RNN_F16 | h.RNN_HALF_CHIP, h.RNN_F16),
            'stream': (0, 0)}[variant]


def _bwd_kernels(h, cell, hidden, num_steps, batch, flags, ragged):
    """The backward kernel each 32-row block runs, by the rule of `prnn_bwd`: the LSTM-1024
    fp16-pipe call takes the staggered kernel on half of the chip, without per-row
    lengths, for a block of two 16-row tiles whose row count is a multiple of 8; at LSTM-2048
    RNN_F16 | RNN_KPAIR alone takes the K-pair kernel for every tile."""
    if not h.rnn_persistent_supported(cell, num_steps, batch, hidden):
        return ['stream']
    f16 = h.rnn_f16_recurrence(cell, num_steps, batch, hidden, flags, backward=True, ragged=ragged)
    # (the predicate against the rule it states: fp16 backward for the LSTM at both sizes and for
    # the ReLU cell at one tile without lengths)
    assert f16 == bool(flags & h.RNN_F16 and (
        cell == 'lstm' or (cell == 'rnn_relu' and batch <= 16 and not ragged))), \
        (cell, hidden, batch, flags, ragged)
    forms = []
    for b0 in range(0, batch, 32):
        rows = min(32, batch - b0)
        if not f16:
            forms.append('fp32')
        elif cell == 'rnn_relu':
            forms.append('prnn_relu16_kernel')
        elif hidden == 2048:
            forms.append('prnn_bwd16w_kernel<k-pair>' if flags & h.RNN_KPAIR
                         else 'prnn_bwd16w_kernel')
        else:
            apart = ((rows + 15) // 16 == 2 and not flags & h.RNN_WHOLE_CHIP and not ragged and
                     rows % 8 == 0)
            forms.append('prnn_bwd16s_kernel' if apart and flags & h.RNN_STAGGER else
                         'prnn_bwd16_kernel')
    return forms


def _fwd_is_f16(h, cell, hidden, num_steps, batch, flags, ragged):
    f16 = h.rnn_f16_recurrence(cell, num_steps, batch, hidden, flags, backward=False,
                               ragged=ragged)
    assert f16 == bool(flags & h.RNN_F16 and h.rnn_persistent_supported(
        cell, num_steps, batch, hidden) and (
        cell in ('lstm', 'gru') or (cell == 'rnn_relu' and batch <= 16 and not ragged))), \
        (cell, hidden, batch, flags, ragged)
    return f16


_WEIGHTS, _CASES = {}, {}


def _case(h, cell, hidden, num_steps, batch, lengths):
    """Inputs and the float64 y / dxw of one (cell, H, T, B, lengths), shared by every variant.
    Gradients over three decades of rows; GRU with a non-zero b_hh_n, every cell with xw_bias;
    per-row lengths with a row of length T first and a row of length 1 last."""
    if (cell, hidden) not in _WEIGHTS:
        _WEIGHTS.clear()
        _CASES.clear()
        gh = h.CELL_GATES[cell] * hidden
        g = torch.Generator(device=DEV).manual_seed(hidden + h.CELL_IDS[cell])
        w = torch.randn(2, gh, hidden, device=DEV, generator=g) / np.sqrt(hidden)
        b_hh = torch.randn(2, gh, device=DEV, generator=g) * 0.3 if cell == 'gru' else None
        bias = torch.randn(2 * gh, device=DEV, generator=g) * 0.1
        _WEIGHTS[(cell, hidden)] = (w, h.transpose_batched(w), b_hh, bias)
    key = (cell, hidden, num_steps, batch, lengths)
    if key not in _CASES:
        w, wt, b_hh, bias = _WEIGHTS[(cell, hidden)]
        gh = h.CELL_GATES[cell] * hidden
        g = torch.Generator(device=DEV).manual_seed(1000 * num_steps + 10 * batch + lengths)
        xw = torch.randn(num_steps, batch, 2, gh, device=DEV, generator=g) * 0.5
        dy = torch.randn(num_steps, batch, 2 * hidden, device=DEV, generator=g) * \
            torch.logspace(-3, 0, batch, device=DEV).view(1, batch, 1)
        sl = None
        if lengths:
            sl = torch.randint(1, num_steps + 1, (batch,), device=DEV, generator=g).int()
            sl[0], sl[-1] = num_steps, 1
        ref_y, ref_dxw, _ = rnn_reference.forward_backward(cell, xw, w, dy, b_hh, sl, bias)
        _CASES[key] = dict(xw=xw, dy=dy, sl=sl, w=w, wt=wt, b_hh=b_hh, bias=bias, ref_y=ref_y,
                           ref_dxw=ref_dxw)
    return _CASES[key]


def _pass(h, cell, c, fwd_flags, bwd_flags, colmax_ok, fwd_cuts=None, bwd_cuts=None):
    """One forward + backward pass on a fresh workspace -> y, dxw, dbias, colmax, reserve, ws."""
    num_steps, batch = c['xw'].shape[:2]
    hidden = c['w'].shape[2]
    gh = h.CELL_GATES[cell] * hidden
    ws = h.rnn_workspace(cell, num_steps, batch, hidden, DEV)
    y = torch.full((num_steps, batch, 2 * hidden), float('nan'), device=DEV)
    reserve = torch.zeros(h.rnn_reserve_bytes(cell, num_steps, batch, hidden), dtype=torch.uint8,
                          device=DEV)
    fwd_cuts = fwd_cuts or [0, num_steps]
    bwd_cuts = bwd_cuts or [num_steps, 0]
    for lo, hi in zip(fwd_cuts[:-1], fwd_cuts[1:]):
        h.rnn_fwd(cell, c['xw'], c['w'], c['sl'], b_hh_n=c['b_hh'], y=y, reserve=reserve,
                  workspace=ws, steps=(lo, hi), flags=fwd_flags, xw_bias=c['bias'])
    h.rnn_poll_error(cell, ws, num_steps, batch, hidden)
    colmax = torch.zeros(2 * gh, dtype=torch.int32, device=DEV) if colmax_ok else None
    dbias = torch.zeros(2 * gh * (2 if cell == 'gru' else 1), device=DEV)
    dxw = torch.full((num_steps, batch, 2, gh), float('nan'), device=DEV)
    for hi, lo in zip(bwd_cuts[:-1], bwd_cuts[1:]):
        h.rnn_bwd(cell, c['dy'], y, c['wt'], reserve, c['sl'], b_hh_n=c['b_hh'], dxw=dxw,
                  dbias=dbias, workspace=ws, steps=(lo, hi), flags=bwd_flags, colmax=colmax)
    h.rnn_poll_error(cell, ws, num_steps, batch, hidden)
    return y, dxw, dbias, colmax, reserve, ws


def _row_err(got, ref):
    """Each row's (utterance's) largest error relative to its largest gradient; the largest."""
    err = (got.double() - ref).abs().amax(dim=(0, 2, 3))
    return float((err / ref.abs().amax(dim=(0, 2, 3)).clamp_min(1e-30)).max())


def _check_y(h, cell, hidden, c, fwd_flags, forms, y, what):
    num_steps, batch = y.shape[:2]
    ragged = c['sl'] is not None
    ref_y = c['ref_y']
    # forward: fp32 kernels 2e-5 (test_rnn_fwd_bwd); fp16 pipe within 2e-5 and 3x the fp32
    # kernel's error + 2e-6 (test_rnn_fwd_on_the_fp16_matrix_pipe; ReLU: + 1e-6 x the scale of y,
    # test_relu_recurrence_on_the_fp16_matrix_pipe)
    scale_y = max(1.0, float(ref_y.abs().max()))
    err = float((y.double() - ref_y).abs().max())
    if forms != ['stream'] and _fwd_is_f16(h, cell, hidden, num_steps, batch, fwd_flags, ragged):
        y32, _, ws32 = h.rnn_fwd(cell, c['xw'], c['w'], c['sl'], b_hh_n=c['b_hh'],
                                 xw_bias=c['bias'])
        h.rnn_poll_error(cell, ws32, num_steps, batch, hidden)
        err32 = float((y32.double() - ref_y).abs().max())
        if cell == 'rnn_relu':
            assert err < 3 * err32 + 1e-6 * scale_y, (what, err, err32)
        else:
            assert err < 2e-5 and err < 3 * err32 + 2e-6, (what, err, err32)
    else:
        assert err < 2e-5 * scale_y, (what, err)


def _check_pass(h, cell, hidden, c, variant, fwd_flags, bwd_flags, forms, got, check_y=True):
    """y, dxw, dbias and the column maxima of one pass against the float64 reference, to the bars
    of the existing test of each kernel family.  ``check_y=False`` leaves y out (a pass whose y is
    judged elsewhere: the backward bars alone, the ReLU cell's against the y it was handed)."""
    y, dxw, dbias, colmax, reserve, ws = got
    num_steps, batch = y.shape[:2]
    ragged = c['sl'] is not None
    what = (cell, hidden, variant, num_steps, batch, ragged)
    if check_y:
        _check_y(h, cell, hidden, c, fwd_flags, forms, y, what)
    # backward: the ReLU cell differentiates through the mask y > 0 of the y it is handed
    ref = c['ref_dxw'] if cell != 'rnn_relu' else \
        rnn_reference.relu_backward(y, c['dy'], c['w'], c['sl'])
    if all(f in ('fp32', 'stream') for f in forms):
        err = float((dxw.double() - ref).abs().max())
        assert err < 1e-4 * max(1.0, float(ref.abs().max())), (what, err)
    else:
        # fp16 pipe: each row within 3x the fp32 kernel's error (on the same reserve) + 1e-6
        dxw32 = h.rnn_bwd(cell, c['dy'], y, c['wt'], reserve, c['sl'], b_hh_n=c['b_hh'],
                          workspace=ws)
        h.rnn_poll_error(cell, ws, num_steps, batch, hidden)
        e16, e32 = _row_err(dxw, ref), _row_err(dxw32, ref)
        assert e16 < 3 * e32 + 1e-6, (what, e16, e32)
    # the bias gradients: column sums of dxw (GRU: then of drec), to 1e-4 (test_rnn_fwd_bwd)
    want = [dxw.double().sum(dim=(0, 1)).reshape(-1)]
    if cell == 'gru':
        want.append(h.rnn_gru_drec(reserve, num_steps, batch, hidden).double()
                    .sum(dim=(0, 1)).reshape(-1))
    want = torch.cat(want)
    assert float((dbias.double() - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max())), \
        what
    if colmax is not None:
        assert torch.equal(colmax.view(torch.float32), dxw.abs().amax(dim=(0, 1)).reshape(-1)), \
            what


@pytest.mark.parametrize('cell,hidden,variant', CASES)
def test_every_variant_at_the_edge_shapes(hip, cell, hidden, variant, monkeypatch):
    fwd_flags, bwd_flags = _flags(hip, variant)
    if variant == 'stream':
        monkeypatch.setenv('CTCASR_RNN_MODE', 'stream')
    ran = set()
    for num_steps in STEPS:
        for batch in BATCHES[hidden]:
            for lengths in (False, True):
                c = _case(hip, cell, hidden, num_steps, batch, lengths)
                assert hip.rnn_persistent_supported(cell, num_steps, batch, hidden) == \
                    (variant != 'stream')
                forms = _bwd_kernels(hip, cell, hidden, num_steps, batch, bwd_flags, lengths)
                ran |= {(f, num_steps, batch, lengths) for f in forms}
                colmax_ok = forms != ['stream'] and hip.rnn_bwd_f16_supported(
                    cell, num_steps, batch, hidden, bwd_flags) and not \
                    (cell == 'rnn_relu' and lengths)
                got = _pass(hip, cell, c, fwd_flags, bwd_flags, colmax_ok)
                _check_pass(hip, cell, hidden, c, variant, fwd_flags, bwd_flags, forms, got)
                dxw = got[1]
                # the staggered / K-pair forms against the plain fp16 kernel on the same reserve:
                # staggered bit for bit; K pairs within 1.5x its row error + 2e-7
                # (test_rnn_bwd_k_pairs_at_2048); blocks that fall back are the plain kernel
                if bwd_flags & (hip.RNN_STAGGER | hip.RNN_KPAIR) and cell == 'lstm':
                    plain = hip.rnn_bwd(cell, c['dy'], got[0], c['wt'], got[4], c['sl'],
                                        workspace=got[5],
                                        flags=bwd_flags & ~(hip.RNN_STAGGER | hip.RNN_KPAIR))
                    hip.rnn_poll_error(cell, got[5], num_steps, batch, hidden)
                    ref = c['ref_dxw']
                    for blk, form in enumerate(forms):
                        rows = slice(32 * blk, min(batch, 32 * blk + 32))
                        if 'k-pair' in form:
                            e_pair = _row_err(dxw[:, rows], ref[:, rows])
                            e_plain = _row_err(plain[:, rows], ref[:, rows])
                            assert e_pair < 1.5 * e_plain + 2e-7, \
                                (variant, num_steps, batch, blk, e_pair, e_plain)
                        else:
                            assert torch.equal(dxw[:, rows], plain[:, rows]), \
                                (variant, num_steps, batch, blk, form)
                if num_steps == 3:
                    # single-step launches, each way: bit for bit one whole launch (the bias
                    # gradients: one atomic per launch and column - to rounding)
                    cut = _pass(hip, cell, c, fwd_flags, bwd_flags, colmax_ok,
                                fwd_cuts=[0, 1, 2, 3], bwd_cuts=[3, 2, 1, 0])
                    what = (cell, hidden, variant, batch, lengths)
                    assert torch.equal(cut[0], got[0]), what
                    assert torch.equal(cut[1], got[1]), what
                    assert float((cut[2] - got[2]).abs().max()) <= \
                        1e-5 * max(1.0, float(got[2].abs().max())), what
                    assert (cut[3] is None) == (got[3] is None)
                    if got[3] is not None:
                        assert torch.equal(cut[3], got[3]), what
    rule = MUST_RUN.get((cell, hidden, variant))
    if rule is not None:
        form, batches = rule
        for num_steps in STEPS:
            took = {b for f, t, b, ragged in ran if f == form and t == num_steps and not ragged}
            assert batches <= took, (variant, num_steps, sorted(took))
        # per-row lengths: the LSTM-1024 staggered kernel is not taken
        if hidden == 1024:
            assert not {r for r in ran if r[0] == form and r[3]}


@pytest.mark.parametrize('cell,hidden,variant', CASES)
def test_one_workspace_down_to_a_single_step(hip, cell, hidden, variant, monkeypatch):
    """test_one_workspace_serves_every_shorter_pass down to T = 1 and out to two full row blocks:
    passes at T = 3, 1, 2, 3, 1 on ONE workspace created for T = 3, new data each pass (the T = 2
    pass with per-row lengths where the variant takes them), each equal bit for bit to the same
    pass on a fresh workspace of exactly its T; the time-out words read clear at both T."""
    fwd_flags, bwd_flags = _flags(hip, variant)
    if variant == 'stream':
        monkeypatch.setenv('CTCASR_RNN_MODE', 'stream')
    gates = hip.CELL_GATES[cell]
    g = torch.Generator(device=DEV).manual_seed(71)
    w = torch.randn(2, gates * hidden, hidden, device=DEV, generator=g) / np.sqrt(hidden)
    wt = hip.transpose_batched(w)
    b_hh = torch.randn(2, gates * hidden, device=DEV, generator=g) * 0.3 if cell == 'gru' else None
    lengths_ok = not (cell == 'rnn_relu' and bwd_flags & hip.RNN_F16)
    for batch in (1, 24, 56, 64):
        ws = hip.rnn_workspace(cell, 3, batch, hidden, DEV)
        for k, num_steps in enumerate((3, 1, 2, 3, 1)):
            p = _Pass(hip, cell, hidden, batch, num_steps, 7000 + 100 * k + batch, w, wt, b_hh,
                      lengths_ok and num_steps == 2)
            got = p.run(ws, fwd_flags, bwd_flags)
            hip.rnn_poll_error(cell, ws, 3, batch, hidden)
            hip.rnn_poll_error(cell, ws, num_steps, batch, hidden)
            fresh = hip.rnn_workspace(cell, num_steps, batch, hidden, DEV)
            want = p.run(fresh, fwd_flags, bwd_flags)
            hip.rnn_poll_error(cell, fresh, num_steps, batch, hidden)
            _assert_same_pass(got, want, (variant, batch, num_steps))


def test_the_retired_variant_bit_is_a_bad_argument(hip):
    """Value 8 of `flags` selected the reduce-scatter backward form up to ABI v7.  It is an unknown
    bit now: both recurrence calls refuse it before anything is enqueued, outputs untouched."""
    num_steps, batch, hidden = 2, 1, 64
    g = torch.Generator(device=DEV).manual_seed(8)
    xw = torch.randn(num_steps, batch, 2, 4 * hidden, device=DEV, generator=g)
    w = torch.randn(2, 4 * hidden, hidden, device=DEV, generator=g) / np.sqrt(hidden)
    dy = torch.randn(num_steps, batch, 2 * hidden, device=DEV, generator=g)
    y, reserve, ws = hip.rnn_fwd('lstm', xw, w)
    wt = hip.transpose_batched(w)
    y_out = torch.full_like(y, 7.0)
    reserve_out = torch.full_like(reserve, 7)
    with pytest.raises(hip.CtcAsrError, match='bad argument'):
        hip.rnn_fwd('lstm', xw, w, y=y_out, reserve=reserve_out, workspace=ws, flags=8)
    dxw = torch.full((num_steps, batch, 2, 4 * hidden), 7.0, device=DEV)
    dbias = torch.full((2 * 4 * hidden,), 7.0, device=DEV)
    with pytest.raises(hip.CtcAsrError, match='bad argument'):
        hip.rnn_bwd('lstm', dy, y, wt, reserve, dxw=dxw, dbias=dbias, workspace=ws, flags=8)
    torch.cuda.synchronize()
    assert bool((y_out == 7.0).all()) and bool((reserve_out == 7).all())
    assert bool((dxw == 7.0).all()) and bool((dbias == 7.0).all())
    # (the calls themselves are whole: the same arguments without the bit)
    hip.rnn_bwd('lstm', dy, y, wt, reserve, dxw=dxw, dbias=dbias, workspace=ws)
    assert torch.isfinite(dxw).all() and not bool((dxw == 7.0).all())


def test_the_k_pair_bit_is_ignored_at_1024(hip):
    """LSTM-1024 has no K-pair form: RNN_KPAIR changes nothing there.  At the smallest shape that
    took the removed kernel (two tiles, rows a multiple of 8, no lengths) the call runs the
    staggered kernel where RNN_STAGGER is set, else the one-barrier kernel - dxw, the bias
    gradients and the column maxima bit for bit those of the same call without the bit."""
    num_steps, batch, hidden = 3, 24, 1024
    c = _case(hip, 'lstm', hidden, num_steps, batch, False)
    base = hip.RNN_F16 | hip.RNN_XCD_SPLIT
    y, reserve, ws = hip.rnn_fwd('lstm', c['xw'], c['w'], xw_bias=c['bias'], flags=base)

    def run(flags):
        dbias = torch.zeros(2 * 4 * hidden, device=DEV)
        colmax = torch.zeros(2 * 4 * hidden, dtype=torch.int32, device=DEV)
        dxw = torch.full((num_steps, batch, 2, 4 * hidden), float('nan'), device=DEV)
        hip.rnn_bwd('lstm', c['dy'], y, c['wt'], reserve, dxw=dxw, dbias=dbias, workspace=ws,
                    flags=flags, colmax=colmax)
        hip.rnn_poll_error('lstm', ws, num_steps, batch, hidden)
        return dxw, dbias, colmax

    for flags in (base, base | hip.RNN_STAGGER):
        want, got = run(flags), run(flags | hip.RNN_KPAIR)
        assert torch.isfinite(want[0]).all()
        for name, a, b in zip(('dxw', 'dbias', 'colmax'), got, want):
            assert torch.equal(a, b), (flags, name)
