"""The kernels of csrc/elementwise.hip at the places where they go wrong first: every grid-stride
loop taken at least twice (the float4 epilogue beyond 2^21 elements, the scalar one and `dropout`
beyond 2^19, `absmax` beyond 2^20, Adam beyond 2^26), the tails behind the float4 bodies, the
dropout mask pinned bit for bit to the host generator (tests/elementwise_reference.py) at every
flat index and in all three kernels that draw it, the clip at exactly 0 / the cutoff / +-inf /
NaN, the column sums of the backward epilogue on its narrow, partial and capped grids, the step
guard on both sides of its 256 threads, the transpose away from multiples of 32, and the
refusals of the Python wrappers (an argument of the wrong length never reaches the library).

What an operation defines exactly is compared exactly: bit patterns, except where the clip has
produced a zero (the sign of max(-0, 0) is nobody's contract; values and NaN positions are
compared there).  The two places with a tolerance derive it: the column sums (any-order float32
summation bound) and Adam (error against float64 no worse than 4 x the error of the same update
evaluated in float32 operation by operation, + 1 ulp)."""

import time

import numpy as np
import pytest
import torch

from oracle import nn as onn
from tests import elementwise_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CUTOFF = 20.0
INF = float('inf')

# what whoever runs the module reads to report it (the asserts do not depend on it)
MEASURED = {}


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(got, want):
    got, want = _np(got), np.asarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _same_values(got, want):
    """Equal values and NaNs in the same places (+0 == -0)."""
    return np.array_equal(_np(got), np.asarray(want, dtype=np.float32), equal_nan=True)


# ============================================================================ bias_act_fwd
FWD_SHAPES = [(r, c) for r in (1, 2, 33, 4097) for c in (1, 3, 4, 29, 64, 65, 2048)]
# 4097 x 2048 = 2^23 + 2048 elements: the float4 kernel (2048 x 256 threads x 4) strides four
# times.  The scalar kernel covers 2048 x 256 = 2^19 elements per trip:
FWD_SHAPES.append((8200, 65))           # 533 000 elements, cols % 4 != 0: the scalar kernel strides
FWD_SHAPES.append((1030, 2052))         # 2^21 + 16 408 elements, cols % 4 == 0: a short second trip


def _epilogue_case(rng, rows, cols, with_bias):
    """Pre-activations that straddle both bounds, and where they sit: sums that are exactly 0,
    exactly the cutoff, one ulp on either side of it, +-inf and -0."""
    y = (rng.normal(size=(rows, cols)) * 12.0).astype(np.float32)
    # (quarters: y + bias is exact for the planted values)
    bias = (rng.integers(-8, 9, size=cols) / 4.0).astype(np.float32) if with_bias else None
    shift = bias if with_bias else np.zeros(cols, dtype=np.float32)
    flat, n = y.reshape(-1), y.size
    targets = [0.0, CUTOFF, np.nextafter(np.float32(CUTOFF), np.float32(INF)),
               np.nextafter(np.float32(CUTOFF), np.float32(0)), INF, -INF, -0.0, 1.0]
    spots = rng.permutation(n)[:min(n, 64 * len(targets))]
    for k, i in enumerate(spots):
        target = np.float32(targets[k % len(targets)])
        flat[i] = target - shift[i % cols] if np.isfinite(target) and target != 0 else target
    if with_bias:       # (-0 and 0 survive only where nothing is added; planted sums: 0 = -b + b)
        zero = spots[0::len(targets)]
        flat[zero] = -shift[zero % cols]
    return y, bias


@pytest.mark.parametrize('rows,cols', FWD_SHAPES)
def test_bias_act_fwd_equals_the_float32_reference(hip, rows, cols):
    rng = np.random.default_rng(rows * 10007 + cols)
    seed = int(rng.integers(0, 1 << 63)) * 2 + 1
    for with_bias in (False, True):
        y, bias = _epilogue_case(rng, rows, cols, with_bias)
        dev_bias = None if bias is None else _t(bias)
        # cutoff 0: the add alone, whatever the rate says - defined to the bit
        got = hip.bias_act_fwd(_t(y), dev_bias, 0.0, 0.5, seed)
        assert _same_bits(got, ref.bias_act_fwd_f32(y, bias, 0.0)[0]), (with_bias, 'add only')
        for rate in (0.0, 0.1, 0.5):
            want, mask = ref.bias_act_fwd_f32(y, bias, CUTOFF, rate, seed)
            got = hip.bias_act_fwd(_t(y), dev_bias, CUTOFF, rate, seed)
            assert _same_values(got, want), (with_bias, rate)
            assert 0.0 <= float(got.min()) and float(got.max()) <= CUTOFF * 2
            if mask is not None and not with_bias:
                # the mask itself: ones go in, 1 / keep or 0 comes out, at every flat index
                ones = hip.bias_act_fwd(torch.ones(rows, cols, device=DEV), None, CUTOFF, rate,
                                        seed)
                assert np.array_equal(_np(ones) != 0, mask), rate
                assert _same_bits(ones, np.where(mask, ref.inv_keep_f32(rate), np.float32(0)))


def test_scalar_and_float4_kernels_draw_the_same_mask(hip):
    """One matrix through the float4 kernel (aligned, cols % 4 == 0), through the scalar kernel
    (the same values at a 4-byte offset; the same buffer seen with cols % 4 != 0) and through
    `dropout`: the mask belongs to the flat index, not to the kernel.  2^23 + 2048 elements: all
    three stride."""
    rows, cols, rate, seed = 4097, 2048, 0.5, (1 << 64) - 3
    n = rows * cols
    rng = np.random.default_rng(11)
    y = rng.uniform(0.5, 19.0, size=(rows, cols)).astype(np.float32)
    bias = (rng.integers(-1, 2, size=cols) / 4.0).astype(np.float32)
    want, mask = ref.bias_act_fwd_f32(y, bias, CUTOFF, rate, seed)
    aligned = hip.bias_act_fwd(_t(y), _t(bias), CUTOFF, rate, seed)
    assert aligned.data_ptr() % 16 == 0 and _same_bits(aligned, want)
    buf = torch.empty(n + 4, device=DEV)
    shifted = buf[1:1 + n].view(rows, cols)
    shifted.copy_(_t(y))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    hip.bias_act_fwd(shifted, _t(bias), CUTOFF, rate, seed)
    assert torch.equal(shifted.view(torch.int32), aligned.view(torch.int32))
    # cols % 4 != 0 over the same flat range (no bias: its column would move)
    plain = ref.bias_act_fwd_f32(y, None, CUTOFF, rate, seed)[0]
    narrow = hip.bias_act_fwd(_t(y).view(cols, rows), None, CUTOFF, rate, seed)
    assert _same_bits(narrow.view(rows, cols), plain)
    dropped = hip.dropout(_t(y), rate, seed)
    assert np.array_equal(_np(dropped) != 0, mask) and _same_bits(dropped, plain)


def test_bias_act_fwd_without_rows_returns(hip):
    bias = torch.ones(8, device=DEV)
    empty = torch.empty(0, 8, device=DEV)
    assert hip.bias_act_fwd(empty, bias, CUTOFF, 0.5, 3) is empty
    assert hip.bias_act_fwd(torch.empty(2, 0, 8, device=DEV), None, 0.0).numel() == 0
    assert float(bias.min()) == float(bias.max()) == 1.0


# ---------------------------------------------------------------------------- NaN
@pytest.mark.parametrize('cols,offset', [(64, 0), (65, 0), (64, 1)])
def test_nan_leaves_the_epilogue_as_nan(hip, cols, offset):
    """fmaxf(NaN, 0) is 0: a clip written with it alone turns a NaN pre-activation into a finite
    activation, the loss stays finite and the step guard lets the update through.  Both forward
    kernels (float4: 64 columns aligned; scalar: 65 columns, and 64 at a 4-byte offset)."""
    rows = 33
    rng = np.random.default_rng(cols + offset)
    y = (rng.normal(size=(rows, cols)) * 12.0).astype(np.float32)
    bias = rng.normal(size=cols).astype(np.float32)
    nan_at = [(0, 0), (0, 3), (7, cols - 1), (rows - 1, cols - 1), (16, 5)]
    for k, (r, c) in enumerate(nan_at):
        y[r, c] = np.nan if k % 2 == 0 else -np.nan
    y[1, 1], y[2, 2] = INF, -INF
    for rate in (0.0, 0.5):
        buf = torch.zeros(rows * cols + 4, device=DEV)
        view = buf[offset:offset + rows * cols].view(rows, cols)
        view.copy_(_t(y))
        got = _np(hip.bias_act_fwd(view, _t(bias), CUTOFF, rate, 99))
        want, mask = ref.bias_act_fwd_f32(y, bias, CUTOFF, rate, 99)
        kept = np.ones_like(y, dtype=bool) if mask is None else mask
        for r, c in nan_at:
            assert np.isnan(got[r, c]) == bool(kept[r, c]), (rate, r, c, got[r, c])
        assert rate > 0 or all(np.isnan(got[r, c]) for r, c in nan_at)
        assert got[1, 1] == (want[1, 1] if rate else CUTOFF) and got[2, 2] == 0.0
        assert np.array_equal(got, want, equal_nan=True)
        assert int(np.isnan(got).sum()) == sum(bool(kept[r, c]) for r, c in nan_at)


def test_a_nan_weight_in_dense4_drops_the_step(hip):
    """A NaN in the last dense layer's kernel reaches the loss (the epilogue used to turn the NaN
    pre-activations into zeros: finite logits, finite loss, update applied): the step guard is
    set, `Trainer.train_step` leaves parameters and moments as they were, and the deferred check
    raises what a NaN loss raises."""
    from ctc_asr_amd.engine import NanLossDuringTrainingError, Trainer
    from ctc_asr_amd.model import ModelConfig
    cfg = ModelConfig(used_model='ds2', conv_filters=(4, 4), num_units_dense=32, num_layers_rnn=1,
                      num_units_rnn=64, rnn_cell='lstm', cudnn=True, dense_dropout_rate=0.0)
    trainer = Trainer(cfg, device=DEV, seed=3)
    rng = np.random.default_rng(5)
    feats = torch.tensor(rng.normal(size=(2, 21, 80)).astype(np.float32))
    flen = torch.tensor([21, 21], dtype=torch.int32)
    labels = [[1, 2, 3], [4, 5]]
    trainer.train_step(feats, flen, labels)
    trainer.drain_checks()
    assert trainer.model.step_guard().tolist() == [0, 0]
    arena = trainer.model.arena
    arena.p['dense4/kernel'][3, 0] = float('nan')
    arena.touch()
    before = [t.clone().view(torch.int32) for t in (arena.param, arena.m, arena.v)]
    loss = trainer.train_step(feats, flen, labels)
    torch.cuda.synchronize()
    assert not np.isfinite(float(loss))
    assert int(trainer.model.step_guard()[0]) == 1
    for was, now in zip(before, (arena.param, arena.m, arena.v)):
        assert torch.equal(was, now.view(torch.int32))
    with pytest.raises(NanLossDuringTrainingError):
        trainer.drain_checks()


# ============================================================================ bias_act_bwd
BWD_COLS = [1, 2, 4, 32,            # narrow: 64 / cols rows per wave access
            3, 29, 63,              # below 64 and not narrow
            64, 65, 2048, 4096]
# rows 17: two row blocks of 9 rows (9 is no multiple of 4 x rows-per-wave-access for any width);
# 33: three of 11; 1000: 63 blocks of 16
BWD_ROWS = [1, 15, 16, 17, 33, 1000]
# (64 columns also run 16 x 2048 + 100 rows: ceil(rows / 16) exceeds the 2048 row blocks the
# launch allows itself, rows_per_block becomes 17)
BWD_CAPPED_ROWS = 16 * 2048 + 100


def _bwd_case(rng, rows, cols, rate):
    """y as a forward pass leaves it (0 .. cutoff / keep) with the boundary values planted, dy
    bounded away from 0 so that the column-sum bound below is about sums, not about noise."""
    upper = np.float32(CUTOFF) * ref.inv_keep_f32(rate)
    y = rng.uniform(0.0, float(upper), size=(rows, cols)).astype(np.float32)
    specials = np.array([0.0, -0.0, upper, np.nextafter(upper, np.float32(0)),
                         np.nextafter(np.float32(0), np.float32(1)), 2 * upper, -1.0,
                         np.float32(1.17549435e-38)], dtype=np.float32)
    pick = rng.random(size=y.shape) < 0.3
    y[pick] = specials[rng.integers(0, len(specials), size=int(pick.sum()))]
    dy = (rng.uniform(0.5, 2.0, size=y.shape) * rng.choice([-1.0, 1.0], size=y.shape))
    return y, dy.astype(np.float32)


def _check_colsum(got, start, dz, rows, what):
    """|dbias - (start + sum_r dz)| <= (rows + 3) 2^-24 sum_r |dz| per column: rows + 1 terms
    added in any order in float32 (the wave's partial sums, the shared-memory fold, the atomics
    of the row blocks), each addition within 2^-24 of its partial sum.  `start` is kept below
    2^-6 and every kept |dz| is at least 0.5, so that the start value's share of the partial sums
    stays inside the three spare terms."""
    exact = dz.astype(np.float64).sum(axis=0) + start.astype(np.float64)
    bound = (rows + 3) * 2.0 ** -24 * np.abs(dz.astype(np.float64)).sum(axis=0)
    err = np.abs(_np(got).astype(np.float64) - exact)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if bound.any() else 0.0
    MEASURED[what] = max(MEASURED.get(what, 0.0), worst)
    assert (err <= bound).all(), (what, rows, worst)


@pytest.mark.parametrize('cols', BWD_COLS)
def test_bias_act_bwd_and_column_sums(hip, cols):
    rng = np.random.default_rng(cols)
    for rows in BWD_ROWS + ([BWD_CAPPED_ROWS] if cols == 64 else []):
        for rate in (0.0, 0.1):
            y, dy = _bwd_case(rng, rows, cols, rate)
            want = ref.bias_act_bwd_f32(y, dy, CUTOFF, rate)
            start = rng.uniform(-2.0 ** -6, 2.0 ** -6, size=cols).astype(np.float32)
            dbias = _t(start)
            dz = hip.bias_act_bwd(_t(y), _t(dy), CUTOFF, rate, dbias=dbias)
            assert _same_bits(dz, want), (rows, rate)
            _check_colsum(dbias, start, want, rows, 'bias_act_bwd dbias / bound')
            # the float64 form agrees on which elements pass
            assert np.array_equal(ref.bias_act_bwd_f64(y, dy, CUTOFF, rate) != 0, want != 0)
            # the sum alone, over what the kernel wrote
            again = _t(-start)
            assert hip.colsum_accumulate(dz, again) is again
            _check_colsum(again, -start, want, rows, 'colsum_accumulate / bound')
            # no dbias: dz and nothing else (guard words on both sides of dz)
            n, pad = rows * cols, 64
            buf = torch.full((n + 2 * pad,), -7.0, device=DEV)
            out = hip.bias_act_bwd(_t(y), _t(dy), CUTOFF, rate, dz=buf[pad:pad + n].view(rows, cols))
            assert _same_bits(out, want)
            assert float(buf[:pad].max()) == float(buf[:pad].min()) == -7.0
            assert float(buf[pad + n:].max()) == float(buf[pad + n:].min()) == -7.0
    print('bias_act_bwd cols {}: {}'.format(cols, MEASURED))


# ============================================================================ dropout
@pytest.mark.parametrize('n', [1, 255, 256, 257, 524288 + 5, (1 << 24) + 3])
def test_dropout_is_the_reference_mask(hip, n):
    """2048 x 256 threads cover 2^19 elements per trip: 2^19 + 5 strides once, 2^24 + 3 strides 32
    times and passes the last index a float32 counter could hold."""
    rng = np.random.default_rng(n)
    src = rng.normal(size=n).astype(np.float32)
    src[rng.integers(0, n, size=min(n, 8))] = [0.0, -0.0, INF, -INF, 1e-40, -1e-40, 3e38, 1.0][:min(n, 8)]
    dev = _t(src)
    for seed, rate in ((77, 0.25), ((1 << 64) - 1, 0.9)):
        mask = ref.dropout_mask(seed, n, rate)
        want = np.where(mask, src * ref.inv_keep_f32(rate), np.float32(0))
        got = hip.dropout(dev, rate, seed)
        assert _same_bits(got, want), (seed, rate)
        assert np.array_equal(_np(got)[src != 0] != 0, mask[src != 0])
        if n > (1 << 20):
            break                       # (one seed of the largest size is enough host time)
    # in place
    alias = dev.clone()
    assert hip.dropout(alias, 0.25, 77, out=alias) is alias
    assert _same_bits(alias, np.where(ref.dropout_mask(77, n, 0.25),
                                      src * ref.inv_keep_f32(0.25), np.float32(0)))
    # rate 0 keeps everything, bit for bit
    assert _same_bits(hip.dropout(dev, 0.0, 5), src)


def test_dropout_index_does_not_wrap_at_32_bits(hip):
    """2^32 + 2^20 elements in place (17 GB): the draws beyond element 2^32 are those of their
    own 64-bit index - with a 32-bit one they would repeat the mask from element 0.  The host
    checks both ends of the vector; every element was 1."""
    n, edge, rate, seed = (1 << 32) + (1 << 20), 1 << 32, 0.5, 0x0123456789ABCDEF
    x = torch.ones(n, device=DEV)
    assert hip.dropout(x, rate, seed, out=x) is x
    two = np.float32(2.0)
    head = ref.dropout_mask(seed, 1 << 20, rate)
    tail = ref.dropout_mask(seed, (1 << 20) + 4096, rate, start=edge - 4096)
    assert not np.array_equal(head, tail[4096:])            # (the two masks do differ)
    assert _same_bits(x[:1 << 20], np.where(head, two, np.float32(0)))
    assert _same_bits(x[edge - 4096:], np.where(tail, two, np.float32(0)))
    kept = float(x.sum(dtype=torch.float64)) / 2.0
    assert abs(kept - n * 0.5) < 5 * (n * 0.25) ** 0.5


# ============================================================================ Adam
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)
ADAM_BIG = 4 * 256 * 65536 + 4 * 256 * 3 + 3        # 65536 x 256 float4: strides, + a tail of 3


def _ulps(got, want):
    """Largest |got - want| in float32 units in the last place of `want` (float64 tensors /
    arrays of the float64 result; 2^-149 at zero)."""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    mag = want.abs().float()
    ulp = (torch.nextafter(mag, torch.full_like(mag, INF)) - mag).double()
    return float(((got.double() - want).abs() / ulp).max())


def _adam_state(n, rng):
    """Gradients with zeros, 1e-20 and 1e+10 among normal deviates; first moments on the side of
    their gradient (an update whose two terms cancel has no meaningful error in ulps of the
    result); a few parameters at exactly 0, where the update is all there is."""
    g = rng.normal(size=n).astype(np.float32)
    g[0::7], g[1::7], g[2::7] = 0.0, 1e-20, 1e10
    g[3::14] *= -1
    m = (np.abs(rng.normal(size=n)) * 1e-2 * np.sign(g)).astype(np.float32)
    v = (rng.random(size=n) * 1e-3).astype(np.float32)
    p = rng.normal(size=n).astype(np.float32)
    p[5::11] = 0.0
    return p, g, m, v


def _hyper32():
    return {k: float(np.float32(x)) for k, x in HYPER.items()}


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024 * 4 + 1])
def test_adam_against_float64_no_worse_than_float32_arithmetic(hip, n):
    h = _hyper32()
    worst = {}
    for scale in (1.0, 1.0 / 16):
        for base in (1, 100000):
            p, g, m, v = _adam_state(n, np.random.default_rng(n + base))
            dp, dg, dm, dv = _t(p), _t(g), _t(m), _t(v)
            for step in range(base, base + 5):
                p, m, v = _np(dp), _np(dm), _np(dv)
                want = onn.adam_step(p.astype(np.float64), g.astype(np.float64) * scale,
                                     m.astype(np.float64), v.astype(np.float64), step, h['lr'],
                                     h['beta1'], h['beta2'], h['epsilon'])
                plain = ref.adam_f32(p, g, m, v, step, h['lr'], h['beta1'], h['beta2'],
                                     h['epsilon'], scale)
                hip.adam_step(dp, dg, dm, dv, step, grad_scale=scale, **HYPER)
                for name, got, f32, f64 in zip('pmv', (dp, dm, dv), plain, want):
                    kernel, floor = _ulps(_np(got), f64), _ulps(f32, f64)
                    worst[name] = tuple(map(max, worst.get(name, (0, 0)), (kernel, floor)))
                    assert kernel <= 4 * floor + 1, (name, n, step, scale, kernel, floor)
                assert _same_bits(dg, g)
    MEASURED['adam n={}'.format(n)] = worst
    print('adam n {}: worst (kernel ulps, float32 ulps) {}'.format(n, worst))


def test_adam_strides_and_reaches_its_tail(hip):
    """n = 4 * 256 * 65536 + 4 * 256 * 3 + 3: the 65536 workgroups stride (three more workgroups'
    worth of float4) and three elements are left for the tail.  Five steps, the float64 reference
    on the device, the float32 one on the host as everywhere."""
    n, h = ADAM_BIG, _hyper32()
    gen = torch.Generator(device=DEV).manual_seed(4)
    g = torch.randn(n, device=DEV, generator=gen)
    g[0::7], g[1::7], g[2::7] = 0.0, 1e-20, 1e10
    m = torch.randn(n, device=DEV, generator=gen).abs_().mul_(1e-2).mul_(torch.sign(g))
    v = torch.rand(n, device=DEV, generator=gen).mul_(1e-3)
    p = torch.randn(n, device=DEV, generator=gen)
    p[5::11] = 0.0
    g_host = _np(g)
    worst = {}
    started = time.time()
    for step, scale in ((1, 1.0), (2, 1.0 / 16), (100000, 1.0), (100001, 1.0 / 16), (100002, 1.0)):
        plain = ref.adam_f32(_np(p), g_host, _np(m), _np(v), step, h['lr'], h['beta1'],
                             h['beta2'], h['epsilon'], scale)
        lr_t = ref.adam_lr_t(step, h['lr'], h['beta1'], h['beta2'])
        gs = g.double() * scale
        m64 = h['beta1'] * m.double() + (1.0 - h['beta1']) * gs
        v64 = h['beta2'] * v.double() + (1.0 - h['beta2']) * gs * gs
        p64 = p.double() - lr_t * m64 / (v64.sqrt() + h['epsilon'])
        del gs
        hip.adam_step(p, g, m, v, step, grad_scale=scale, **HYPER)
        for name, got, f32, f64 in zip('pmv', (p, m, v), plain, (p64, m64, v64)):
            kernel, floor = _ulps(got, f64), _ulps(_t(f32), f64)
            worst[name] = tuple(map(max, worst.get(name, (0, 0)), (kernel, floor)))
            assert kernel <= 4 * floor + 1, (name, step, scale, kernel, floor)
        del p64, m64, v64
    MEASURED['adam n={}'.format(n)] = worst
    print('adam n {}: worst (kernel ulps, float32 ulps) {}, {:.1f} s'.format(
        n, worst, time.time() - started))


@pytest.mark.parametrize('n', [5, 1024 * 4 + 1])
def test_adam_skip_word(hip, n):
    p, g, m, v = _adam_state(n, np.random.default_rng(n))
    runs = {}
    for name, skip in (('none', None), ('clear', [0, 9]), ('set', [1, 0]), ('set2', [-5, 0])):
        dev = [_t(a) for a in (p, g, m, v)]
        word = None if skip is None else torch.tensor(skip, dtype=torch.int32, device=DEV)
        hip.adam_step(*dev, 3, grad_scale=0.5, skip=word, **HYPER)
        runs[name] = [_np(t) for t in dev]
        assert word is None or word.tolist() == skip
    for k, orig in enumerate((p, g, m, v)):
        bits = {name: arrays[k].view(np.uint32) for name, arrays in runs.items()}
        assert np.array_equal(bits['none'], bits['clear'])
        assert np.array_equal(bits['set'], orig.view(np.uint32))
        assert np.array_equal(bits['set2'], orig.view(np.uint32))
    for k in (0, 2, 3):
        assert not np.array_equal(runs['none'][k], (p, g, m, v)[k])


def test_adam_refuses_a_misaligned_view_and_step_zero(hip):
    n = 64
    buf = torch.zeros(n + 4, device=DEV)
    ok = [torch.zeros(n, device=DEV) for _ in range(4)]
    for k in range(4):
        args = list(ok)
        args[k] = buf[1:1 + n]
        with pytest.raises(hip.CtcAsrError):
            hip.adam_step(*args, 1)
    with pytest.raises(hip.CtcAsrError):
        hip.adam_step(*ok, 0)
    assert all(float(t.abs().max()) == 0.0 for t in ok)


# ============================================================================ absmax
ABSMAX_BIG = 4 * 256 * 1024 + 7         # 1024 x 256 float4 per trip: one more float4, a tail of 3


def _absmax_bits(hip, x, start=0):
    out = torch.tensor([start], dtype=torch.int32, device=DEV)
    assert hip.absmax(x, out) is out
    return int(out.item()) & 0xFFFFFFFF


def _bits_of(value):
    return int(np.float32(value).view(np.uint32))


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, ABSMAX_BIG])
def test_absmax_finds_the_peak_wherever_it_is(hip, n):
    rng = np.random.default_rng(n)
    base = rng.uniform(-1.0, 1.0, size=n).astype(np.float32)
    base[rng.integers(0, n, size=min(n, 6))] = [0.0, -0.0, 1e-40, -1e-40, 0.5, -0.5][:min(n, 6)]
    body = 4 * (n // 4)
    spots = {0, n - 1, n // 2} | set(range(body, n))            # first, last, every tail element
    if body:
        spots |= {body - 1, body - 4}                           # the last float4 of the body
    if n == ABSMAX_BIG:
        spots |= {4 * 256 * 1024 - 1, 4 * 256 * 1024, 4 * 256 * 1024 + 3}      # the trip seam
    for k, at in enumerate(sorted(spots)):
        for peak in (3.5, INF):
            x = base.copy()
            if n > 2:
                x[(at + 1) % n] = np.nan                         # ignored, wherever it sits
            x[at] = peak if k % 2 == 0 else -peak
            assert _absmax_bits(hip, _t(x)) == _bits_of(peak), (n, at, x[at])
    # a starting word is kept when it is larger, replaced when it is not
    x = base.copy()
    x[n - 1] = -3.5
    assert _absmax_bits(hip, _t(x), _bits_of(7.0)) == _bits_of(7.0)
    assert _absmax_bits(hip, _t(x), _bits_of(1.0)) == _bits_of(3.5)
    # nothing but denormals, zeros and NaNs: the largest denormal, not a flushed zero
    tiny = np.where(np.arange(n) % 3 == 0, np.nan, 1e-42).astype(np.float32)
    tiny[n - 1] = -3e-39
    assert _absmax_bits(hip, _t(tiny)) == _bits_of(3e-39)
    assert _absmax_bits(hip, torch.full((n,), float('nan'), device=DEV)) == 0
    assert _absmax_bits(hip, torch.full((n,), -0.0, device=DEV)) == 0


def test_absmax_refuses_a_misaligned_vector(hip):
    buf = torch.ones(64, device=DEV)
    out = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(hip.CtcAsrError):
        hip.absmax(buf[1:33], out)
    assert int(out.item()) == 0
    # a matrix is read flat
    assert _absmax_bits(hip, torch.full((3, 5), -2.0, device=DEV)) == _bits_of(2.0)


# ============================================================================ step_guard
@pytest.mark.parametrize('batch', [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_step_guard_sees_one_bad_entry_anywhere(hip, batch):
    status = torch.zeros(batch, dtype=torch.int32, device=DEV)
    loss = torch.full((batch,), 2.5, device=DEV)
    assert hip.step_guard(status, loss, wgrad_word=False).tolist() == [0, 0]
    for at in sorted({0, batch - 1, 255, 256}):
        if not 0 <= at < batch:
            continue
        for bad in (3, -1):
            status[at] = bad
            assert hip.step_guard(status, loss, wgrad_word=False).tolist() == [1, 0], (at, bad)
            status[at] = 0
        for bad in (float('nan'), INF, -INF):
            loss[at] = bad
            assert hip.step_guard(status, loss, wgrad_word=False).tolist() == [1, 0], (at, bad)
            loss[at] = 2.5
    assert hip.step_guard(status, loss, wgrad_word=False).tolist() == [0, 0]
    # a loss of the largest finite magnitude is a loss
    if batch:
        loss[batch - 1] = -3.4e38
        assert hip.step_guard(status, loss, wgrad_word=False).tolist() == [0, 0]


def test_step_guard_time_out_words(hip, monkeypatch):
    status = torch.zeros(65, dtype=torch.int32, device=DEV)
    loss = torch.ones(65, device=DEV)
    w0 = torch.tensor([5], dtype=torch.int32, device=DEV)
    w1 = torch.tensor([2], dtype=torch.int32, device=DEV)
    clear = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((4,), -9, dtype=torch.int32, device=DEV)
    guard = lambda words, **kw: hip.step_guard(status, loss, words, wgrad_word=False, **kw).tolist()
    assert guard((clear.data_ptr(), clear.data_ptr())) == [0, 0]
    assert guard((w0.data_ptr(), 0)) == [1, 5]
    assert guard((0, w1.data_ptr())) == [1, 2]
    assert guard((w0.data_ptr(), w1.data_ptr())) == [1, 7]
    assert guard((w0.data_ptr(), clear.data_ptr()), out=out) == [1, 5, -9, -9]
    status[64] = 1
    assert guard((w0.data_ptr(), w1.data_ptr())) == [1, 7]
    status[64] = 0
    # the weight-gradient kernel's give-up word: bit 30, unless the caller opts out
    index = status.device.index
    monkeypatch.setitem(hip._WGRAD16_SYNC, index, torch.tensor([1, 0, 0, 0], dtype=torch.int32,
                                                               device=DEV))
    assert hip.step_guard(status, loss).tolist() == [1, 1 << 30]
    assert hip.step_guard(status, loss, (w0.data_ptr(), 0)).tolist() == [1, (1 << 30) | 5]
    assert hip.step_guard(status, loss, wgrad_word=False).tolist() == [0, 0]
    monkeypatch.setitem(hip._WGRAD16_SYNC, index, torch.zeros(4, dtype=torch.int32, device=DEV))
    assert hip.step_guard(status, loss).tolist() == [0, 0]


# ============================================================================ transpose
def test_transpose_batched_away_from_multiples_of_32(hip):
    gen = torch.Generator(device=DEV).manual_seed(2)
    for batch in (1, 3):
        for rows in (1, 31, 32, 33, 100):
            for cols in (1, 31, 32, 33, 2049):
                src = torch.randn(batch, rows, cols, device=DEV, generator=gen)
                want = src.permute(0, 2, 1).contiguous()
                got = hip.transpose_batched(src)
                assert got.shape == want.shape and got.is_contiguous()
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
                    (batch, rows, cols)
                # into a range of a bigger buffer, nothing written around it
                n, pad = src.numel(), 32
                buf = torch.full((n + 2 * pad,), -7.0, device=DEV)
                out = buf[pad:pad + n].view(batch, cols, rows)
                assert hip.transpose_batched(src, out=out) is out
                assert torch.equal(out.view(torch.int32), want.view(torch.int32))
                assert bool((buf[:pad] == -7.0).all()) and bool((buf[pad + n:] == -7.0).all())
    # a weight matrix and its scratch, the way the model transposes them
    matrix = torch.randn(96, 40, device=DEV, generator=gen)
    scratch = torch.empty(40, 96, device=DEV)
    hip.transpose_batched(matrix.view(1, 96, 40), out=scratch.view(1, 40, 96))
    assert torch.equal(scratch, matrix.t().contiguous())


# ============================================================================ refusals
# Every call below hands the library an argument of the wrong length.  The wrappers compare
# lengths before anything crosses the ABI, so none of these launches anything.
def _f(*shape):
    return torch.zeros(*shape, device=DEV)


def _i(*shape):
    return torch.zeros(*shape, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('name,delta', [(a, d) for a in ('grad', 'm', 'v') for d in (-1, 1)])
def test_adam_step_refuses_unequal_lengths(hip, name, delta):
    args = {k: _f(64) for k in ('param', 'grad', 'm', 'v')}
    args[name] = _f(64 + delta)
    with pytest.raises(hip.CtcAsrError, match=r'adam_step: {} holds'.format(name)):
        hip.adam_step(args['param'], args['grad'], args['m'], args['v'], 1)


@pytest.mark.parametrize('bias_len', [7, 9, 16, 1])
def test_bias_act_fwd_refuses_a_bias_of_another_length(hip, bias_len):
    with pytest.raises(hip.CtcAsrError, match='bias_act_fwd: bias holds'):
        hip.bias_act_fwd(_f(4, 8), _f(bias_len), CUTOFF)
    with pytest.raises(hip.CtcAsrError, match='bias_act_fwd: y'):
        hip.bias_act_fwd(torch.zeros((), device=DEV), None, CUTOFF)


@pytest.mark.parametrize('name,shape', [('dy', (3, 8)), ('dy', (5, 8)), ('dz', (3, 8)),
                                        ('dz', (4, 9)), ('dbias', (7,)), ('dbias', (9,))])
def test_bias_act_bwd_refuses_unequal_lengths(hip, name, shape):
    args = dict(dy=_f(4, 8), dz=_f(4, 8), dbias=_f(8))
    args[name] = _f(*shape)
    with pytest.raises(hip.CtcAsrError, match='bias_act_bwd: {} holds'.format(name)):
        hip.bias_act_bwd(_f(4, 8), args['dy'], CUTOFF, 0.0, dbias=args['dbias'], dz=args['dz'])


@pytest.mark.parametrize('length', [7, 9, 1])
def test_colsum_accumulate_refuses_a_dbias_of_another_length(hip, length):
    with pytest.raises(hip.CtcAsrError, match='colsum_accumulate: dbias holds'):
        hip.colsum_accumulate(_f(4, 8), _f(length))


@pytest.mark.parametrize('length', [99, 101])
def test_dropout_refuses_an_out_of_another_length(hip, length):
    with pytest.raises(hip.CtcAsrError, match='dropout: out holds'):
        hip.dropout(_f(100), 0.5, 1, out=_f(length))


@pytest.mark.parametrize('src,out', [((2, 3, 4), (2, 3, 4)), ((2, 3, 4), (2, 4, 2)),
                                     ((2, 3, 4), (1, 4, 3)), ((2, 3, 4), (24,)),
                                     ((3, 4), None), ((1, 2, 3, 4), None)])
def test_transpose_batched_refuses_other_shapes(hip, src, out):
    with pytest.raises(hip.CtcAsrError, match='transpose_batched: (src|out) must be'):
        hip.transpose_batched(_f(*src), out=None if out is None else _f(*out))


@pytest.mark.parametrize('loss_len,out_len', [(4, 2), (6, 2), (5, 1), (5, 0)])
def test_step_guard_refuses_unequal_lengths(hip, loss_len, out_len):
    with pytest.raises(hip.CtcAsrError, match='step_guard: (per_utterance_loss|out) holds'):
        hip.step_guard(_i(5), _f(loss_len), out=_i(out_len), wgrad_word=False)


def test_absmax_refuses_an_empty_out(hip):
    with pytest.raises(hip.CtcAsrError, match='absmax: out holds'):
        hip.absmax(_f(16), _i(0))


@pytest.mark.parametrize('name,length', [('scale', 15), ('scale', 17), ('inv_scale', 15),
                                         ('inv_scale', 8)])
def test_colmax_scale_refuses_short_scale_vectors(hip, name, length):
    args = dict(scale=_f(16), inv_scale=_f(16))
    args[name] = _f(length)
    with pytest.raises(hip.CtcAsrError, match='colmax_scale: {} holds'.format(name)):
        hip.colmax_scale(_f(4, 16), **args)


@pytest.mark.parametrize('length', [15, 17, 8, None])
def test_split_f16_cols_refuses_a_col_scale_of_another_length(hip, length):
    with pytest.raises(hip.CtcAsrError, match='split_f16_cols: col_scale'):
        hip.split_f16_cols(_f(4, 16), None if length is None else _f(length), 1.0, (0, 1))
