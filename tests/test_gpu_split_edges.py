"""The operand splits and their scales (csrc/split.hip) on the inputs random data never produces:
low halves that sit exactly on a bfloat16 rounding tie (with bit 16 clear and set, one above,
one below, both signs), fp16 ties (2049 / 2051 x 2^k), fp16 denormal results, values whose second
and third pieces are empty, zeros, -0, float32 denormals, saturation at +-65504, column and row
maxima at 2^e, just below 2^(e+1), at the smallest denormal and at the top of the exponent range,
the 16384-column limit of `split_f16_rows`, row / column ranges of bigger buffers on both sides,
and every block order of a fixed list of lengths 1 to 6.  Every piece and every scale is
compared bit for bit with tests/elementwise_reference.py."""

import numpy as np
import pytest
import torch

from tests import elementwise_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SHAPES = [(r, c) for r in (1, 2, 257) for c in (8, 2040, 2048)]
BF16_ORDERS = [(2,), (1, 0), (0, 1, 2), (2, 2, 0, 1), (0, 1, 2, 0, 1), (0, 1, 2, 0, 1, 0)]
F16_ORDERS = [(1,), (1, 0), (0, 1, 0), (1, 1, 0, 0), (0, 1, 0, 0, 1), (0, 0, 1, 0, 1, 1)]
F16_SCALE = 2048.0


def _t(a, dtype=torch.float32):
    a = np.ascontiguousarray(a)
    if a.size == 0:                     # (numpy gives an empty array strides of its own)
        return torch.zeros(a.shape, dtype=dtype, device=DEV)
    return torch.as_tensor(a, dtype=dtype).to(DEV)


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bits32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _bf16_specials():
    out = []
    for sign in (0, 0x80000000):
        for top in (0x3F80, 0x3F81, 0x4049, 0x4B00, 0x2F01, 0x7F00):
            for low in (0x8000, 0x8001, 0x7FFF, 0x0080, 0x0001):
                out.append(sign | (top << 16) | low)
        # a tie in the SECOND piece: the remainder after the first piece ends in 0x8000 too
        out += [sign | 0x3F800080, sign | 0x3F800180, sign | 0x3F80007F]
    values = _f32(np.array(out, dtype=np.uint32))
    plain = np.array([0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0, 1.5, -2.0, 1.00390625,    # one piece
                      1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -15),                         # two pieces
                      65504.0, 3.0e38, -3.0e38, 1.17549435e-38], dtype=np.float32)
    return np.concatenate([values, plain, _f32([1, 0x80000001, 0x007FFFFF])])


def _f16_specials(scale):
    """x with x * scale on the fp16 ties, at the fp16 denormals, at +-65504, exact in fp16."""
    t = []
    for k in (-14, -3, 0, 4):
        t += [2049.0 * 2.0 ** k, 2051.0 * 2.0 ** k, -2049.0 * 2.0 ** k, -2051.0 * 2.0 ** k,
              2050.0 * 2.0 ** k, 2049.5 * 2.0 ** k]
    t += [2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -26, 2.0 ** -14,
          2.0 ** -14 - 2.0 ** -25, 65504.0, -65504.0, 65503.99, 1.0, -0.5, 1024.0, 0.0, -0.0]
    x = (np.array(t, dtype=np.float64) / scale).astype(np.float32)
    return np.concatenate([x, _f32([1, 0x80000001])])


def _matrix(rng, rows, cols, specials, spread):
    """Three quarters specials (every one of them whenever the matrix has room), one quarter the
    random matrix of the older tests, shuffled."""
    n = rows * cols
    flat = (rng.normal(size=n) * spread(rng, n)).astype(np.float32)
    k = max(min(n, len(specials)), (3 * n) // 4)
    flat[:k] = np.resize(np.roll(specials, rows + cols), k)
    return rng.permutation(flat).reshape(rows, cols)


def _wide(rng, n):
    return 10.0 ** rng.uniform(-30, 20, size=n)


def _bounded(rng, n):
    return np.full(n, 4.0)            # |x| * 2048 stays far below 65504


def _in_a_bigger_buffer(x, kernel_out_dtype, blocks):
    """x as a row / column range of a bigger f32 buffer and an output range of a bigger one
    (16-byte aligned starts, rows longer than cols on both sides)."""
    rows, cols = x.shape
    big = torch.full((rows + 3, cols + 24), 7.0, device=DEV)
    big[2:2 + rows, 12:12 + cols] = x
    out = torch.zeros(rows + 2, blocks, cols + 16, dtype=kernel_out_dtype, device=DEV)
    return big[2:2 + rows, 12:12 + cols], out, out[1:1 + rows, :, 8:8 + cols]


def _check_blocks(got, pieces, order, what):
    bits = _bits16(got)
    for block, piece in enumerate(order):
        assert np.array_equal(bits[:, block], pieces[piece]), (what, order, block)


def _check_untouched(whole, rows, cols):
    assert float(whole[0].float().abs().max()) == 0 and float(whole[1 + rows:].float().abs().max()) == 0
    assert float(whole[:, :, :8].float().abs().max()) == 0
    assert float(whole[:, :, 8 + cols:].float().abs().max()) == 0


@pytest.mark.parametrize('rows,cols', SHAPES)
def test_split_bf16_on_ties_and_empty_pieces(hip, rows, cols):
    rng = np.random.default_rng(rows * 4099 + cols)
    x = _matrix(rng, rows, cols, _bf16_specials(), _wide)
    pieces = ref.bf16_split3(x)
    dev = _t(x)
    for order in BF16_ORDERS:
        _check_blocks(hip.split_bf16(dev, order), pieces, order, 'split_bf16')
        view, whole, out = _in_a_bigger_buffer(dev, torch.bfloat16, len(order))
        assert hip.split_bf16(view, order, out=out) is out
        _check_blocks(out, pieces, order, 'split_bf16, ranges')
        _check_untouched(whole, rows, cols)


@pytest.mark.parametrize('rows,cols', SHAPES)
def test_split_f16_on_ties_denormals_and_the_range_end(hip, rows, cols):
    rng = np.random.default_rng(rows * 4099 + cols + 1)
    x = _matrix(rng, rows, cols, _f16_specials(F16_SCALE), _bounded)
    pieces = ref.f16_split2(x, F16_SCALE, saturate=True)
    assert not np.isinf(pieces[0].view(np.float16)).any()
    dev = _t(x)
    for order in F16_ORDERS:
        _check_blocks(hip.split_f16(dev, F16_SCALE, order), pieces, order, 'split_f16')
        view, whole, out = _in_a_bigger_buffer(dev, torch.float16, len(order))
        assert hip.split_f16(view, F16_SCALE, order, out=out) is out
        _check_blocks(out, pieces, order, 'split_f16, ranges')
        _check_untouched(whole, rows, cols)


def test_split_f16_saturates_instead_of_overflowing(hip):
    top = np.array([65504.0, 65519.0, 65520.0, 65536.0, 1e6, 3e38 * F16_SCALE], dtype=np.float64)
    x = np.concatenate([top, -top, [1.0, -1.0, 0.0, 65503.0]]) / F16_SCALE
    x = np.resize(x.astype(np.float32), (2, 16))
    got = hip.split_f16(_t(x), F16_SCALE, (0, 1))
    h1, h2 = ref.f16_split2(x, F16_SCALE, saturate=True)
    assert np.array_equal(_bits16(got)[:, 0], h1) and np.array_equal(_bits16(got)[:, 1], h2)
    assert bool(torch.isfinite(got).all())
    over = np.abs(x.astype(np.float64)) * F16_SCALE >= 65504.0
    first, second = got[:, 0].cpu().numpy(), got[:, 1].cpu().numpy()
    assert over.sum() >= 20
    assert np.array_equal(first[over], np.where(x[over] > 0, 65504.0, -65504.0).astype(np.float16))
    assert not second[over].any()


def _column_maxima():
    """Bit patterns of column maxima: zero, powers of two, one below the next power of two, both
    ends of the denormals, both ends of the exponent range."""
    bits = [0, 1, 0x007FFFFF, 0x00800000, 0x00FFFFFF, 0x7F7FFFFF, 0x7F000000, 0x7EFFFFFF]
    bits.append(int(np.float32(3e38).view(np.uint32)))
    for e in (-126, -115, -114, -113, -20, -1, 0, 1, 13, 14, 100, 127):
        at = int(np.float32(2.0 ** e).view(np.uint32))
        bits += [at, at + 1] + ([at + 0x7FFFFF] if e < 127 else [])
    return np.array(bits, dtype=np.uint32)


def _check_scales(scale, inv, maxima_bits, what):
    want = ref.scale_for_max(maxima_bits)
    got = _bits32(scale).view(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
    assert np.isfinite(got).all() and (got > 0).all()
    product = _bits32(inv).view(np.float32).astype(np.float64) * got.astype(np.float64)
    assert (product == 1.0).all(), (what, product[product != 1.0])


@pytest.mark.parametrize('rows', [0, 1, 128, 129, 300])
def test_colmax_scale_is_the_rule_on_the_bits(hip, rows):
    maxima = _column_maxima()
    cols = 4 * ((len(maxima) + 3) // 4 + 1)             # trailing columns stay all zero
    x = np.zeros((rows, cols), dtype=np.float32)
    want = np.zeros(cols, dtype=np.uint32)
    rng = np.random.default_rng(rows)
    for c, b in enumerate(maxima[:cols] if rows else []):
        peak = _f32([b])[0]
        x[:, c] = peak * rng.uniform(0.0, 0.999, size=rows).astype(np.float32) * \
            rng.choice([-1.0, 1.0], size=rows).astype(np.float32)
        x[:, c][np.abs(x[:, c]) > peak] = 0.0           # (rounding of a denormal product)
        # the peak alone in the last row of the last 128-row block, or wherever c points
        x[(rows - 1) if c % 2 else (c % rows), c] = -peak if c % 3 else peak
        want[c] = b
    dev = torch.full((rows + 2, cols + 8), 9e37, device=DEV)
    dev[1:1 + rows, 4:4 + cols] = _t(x)
    for view in (_t(x), dev[1:1 + rows, 4:4 + cols]):
        scale, inv = hip.colmax_scale(view)
        _check_scales(scale, inv, want, 'colmax_scale rows {}'.format(rows))
    # buffers of the caller are filled, whatever they held
    scale, inv = torch.full((cols,), 5.0, device=DEV), torch.full((cols,), 5.0, device=DEV)
    assert hip.colmax_scale(_t(x), scale=scale, inv_scale=inv)[0] is scale
    _check_scales(scale, inv, want, 'colmax_scale into buffers')


def test_colscale_from_max_on_every_kind_of_bit_pattern(hip):
    rng = np.random.default_rng(0)
    bits = np.concatenate([_column_maxima(), [0x7F800000, 0x7FC00000],        # inf, NaN: finite
                           rng.integers(0, 0x7F800000, size=600).astype(np.uint32)])
    assert len(bits) % 256 not in (0, 255)
    scale, inv = hip.colscale_from_max(_t(bits.astype(np.int64), torch.int32))
    _check_scales(scale, inv, bits, 'colscale_from_max')
    one = hip.colscale_from_max(torch.tensor([0x3F800000], dtype=torch.int32, device=DEV))
    assert one[0].tolist() == [8192.0] and one[1].tolist() == [1.0 / 8192.0]


@pytest.mark.parametrize('rows,cols', SHAPES)
def test_split_f16_cols_and_rows_under_their_own_scales(hip, rows, cols):
    rng = np.random.default_rng(rows * 4099 + cols + 2)
    x = _matrix(rng, rows, cols, _bf16_specials(), _wide)
    # columns / rows whose maximum is each of the hard cases
    maxima = _f32(_column_maxima())
    for c in range(0, min(cols, 2 * len(maxima)), 2):
        x[:, c] = np.clip(x[:, c], -maxima[c // 2], maxima[c // 2])
        x[rows - 1, c] = -maxima[c // 2]
    dev = _t(x)
    scale, inv = hip.colmax_scale(dev)
    col_scale = ref.scale_for_max(np.abs(x).max(axis=0).view(np.uint32))
    assert np.array_equal(_bits32(scale), col_scale.view(np.uint32))
    pieces = ref.f16_split2(x, 1.0, col_scale=col_scale)
    top = np.abs(pieces[0].view(np.float16).astype(np.float64))
    assert np.isfinite(top).all() and top.max() <= 2.0 ** 14
    for order in F16_ORDERS:
        _check_blocks(hip.split_f16_cols(dev, scale, 1.0, order), pieces, order, 'split_f16_cols')
    view, whole, out = _in_a_bigger_buffer(dev, torch.float16, 2)
    hip.split_f16_cols(view, scale, 1.0, (1, 0), out=out)
    _check_blocks(out, pieces, (1, 0), 'split_f16_cols, ranges')
    _check_untouched(whole, rows, cols)
    # an extra power of two rides along exactly
    half = ref.f16_split2(x, 0.5, col_scale=col_scale)
    _check_blocks(hip.split_f16_cols(dev, scale, 0.5, (0, 1)), half, (0, 1), 'split_f16_cols / 2')

    # rows: maxima along the rows instead
    xr = _matrix(rng, rows, cols, _bf16_specials(), _wide)
    for r in range(rows):
        peak = maxima[(r + cols) % len(maxima)]
        xr[r] = np.clip(xr[r], -peak, peak)
        xr[r, (r * 37) % cols] = peak
    if rows > 1:
        xr[1] = 0.0                                     # an all-zero row: scale 1, inverse 1
    row_scale = ref.scale_for_max(np.abs(xr).max(axis=1).view(np.uint32))
    with np.errstate(over='ignore', under='ignore'):
        scaled = xr * row_scale[:, None]
    pieces = ref.f16_split2(scaled, 1.0)
    top = np.abs(pieces[0].view(np.float16).astype(np.float64))
    assert np.isfinite(top).all() and top.max() <= 2.0 ** 14
    dev = _t(xr)
    for order in F16_ORDERS:
        got, inv_rows = hip.split_f16_rows(dev, order)
        _check_blocks(got, pieces, order, 'split_f16_rows')
        got_inv = _bits32(inv_rows).view(np.float32)
        assert (got_inv.astype(np.float64) * row_scale.astype(np.float64) == 1.0).all()
    if rows > 1:
        assert got_inv[1] == 1.0
    view, whole, out = _in_a_bigger_buffer(dev, torch.float16, 3)
    inv_rows = torch.full((rows,), -3.0, device=DEV)
    hip.split_f16_rows(view, (0, 1, 0), out=out, inv_scale=inv_rows)
    _check_blocks(out, pieces, (0, 1, 0), 'split_f16_rows, ranges')
    _check_untouched(whole, rows, cols)
    assert np.array_equal(_bits32(inv_rows), got_inv.view(np.uint32))


def test_split_f16_rows_at_its_column_limit(hip):
    """256 threads x 8 vectors x 8 columns = 16384 columns is the most one workgroup holds: taken
    and right, with the row's maximum in the last vector of the last thread; one vector more is
    refused."""
    rows, cols = 3, 16384
    rng = np.random.default_rng(3)
    x = rng.normal(size=(rows, cols)).astype(np.float32)
    x[0, cols - 1] = -1000.0
    x[1, cols - 8] = 3e38
    x[2] = 0.0
    row_scale = ref.scale_for_max(np.abs(x).max(axis=1).view(np.uint32))
    assert row_scale.tolist() == [2.0 ** 4, 2.0 ** -114, 1.0]
    pieces = ref.f16_split2(x * row_scale[:, None], 1.0)
    got, inv = hip.split_f16_rows(_t(x), (0, 1))
    _check_blocks(got, pieces, (0, 1), 'split_f16_rows 16384')
    assert (_bits32(inv).view(np.float32).astype(np.float64) * row_scale == 1.0).all()
    assert inv[2].item() == 1.0
    with pytest.raises(hip.CtcAsrError):
        hip.split_f16_rows(torch.zeros(2, cols + 8, device=DEV), (0, 1))


@pytest.mark.parametrize('rows,cols', [(1, 4), (1, 2052), (300, 4), (300, 2052)])
def test_rescale_rows_rounds_twice(hip, rows, cols):
    """out (+)= t * (row_factor * alpha): the factor is rounded, the product is rounded, the sum is
    rounded - no fused multiply-add, which would not be what the fp32 path it stands in for does."""
    rng = np.random.default_rng(rows + cols)
    t = (rng.normal(size=(rows, cols)) * 10.0 ** rng.uniform(-3, 3, size=(rows, 1))).astype(np.float32)
    factor = (2.0 ** rng.integers(-20, 20, size=rows) * rng.choice([1.0, 1.5], size=rows)) \
        .astype(np.float32)
    alpha = np.float32(1.0 / 3.0)
    prior = rng.normal(size=(rows, cols)).astype(np.float32)
    k = (factor * alpha).astype(np.float32)
    product = (t * k[:, None]).astype(np.float32)
    total = (product + prior).astype(np.float32)
    dev_t, dev_f = _t(t), _t(factor)

    def bits(a):
        return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

    out = hip.rescale_rows(dev_t, dev_f, float(alpha), torch.full((rows, cols), 5.0, device=DEV))
    assert np.array_equal(_bits32(out), bits(product))
    out = hip.rescale_rows(dev_t, dev_f, float(alpha), _t(prior), accumulate=True)
    assert np.array_equal(_bits32(out), bits(total))
    # rows longer than cols on either side, then on both
    big_t = torch.full((rows + 1, cols + 8), 3.0, device=DEV)
    big_t[1:, 4:4 + cols] = dev_t
    big_o = torch.full((rows + 2, cols + 4), -7.0, device=DEV)
    for src, dst in ((big_t[1:, 4:4 + cols], None), (dev_t, big_o[1:1 + rows, 4:]),
                     (big_t[1:, 4:4 + cols], big_o[1:1 + rows, 4:])):
        big_o.fill_(-7.0)
        target = torch.empty(rows, cols, device=DEV) if dst is None else dst
        hip.rescale_rows(src, dev_f, float(alpha), target)
        assert np.array_equal(_bits32(target), bits(product))
        if dst is not None:
            assert bool((big_o[:, :4] == -7.0).all()) and bool((big_o[0] == -7.0).all())
            assert bool((big_o[1 + rows:] == -7.0).all())
            dst.copy_(_t(prior))
            hip.rescale_rows(src, dev_f, float(alpha), dst, accumulate=True)
            assert np.array_equal(_bits32(dst), bits(total))
    # in place
    same = dev_t.clone()
    assert hip.rescale_rows(same, dev_f, float(alpha), same) is same
    assert np.array_equal(_bits32(same), bits(product))
    with pytest.raises(hip.CtcAsrError):
        hip.rescale_rows(dev_t, _t(factor[:-1]) if rows > 1 else _t(np.ones(2)), 1.0, same)
