"""tests/gemm_reference.py against itself and against float64, on the CPU: the packed layouts
invert, the emulated MFMA walk over two packed buffers gives the float64 product on exact data
(which pins the layout restatement independently of the kernels), the clamp keeps a NaN, the
exactness precondition rejects data that is not exact, and the restated tile orders are
bijections."""

import numpy as np
import pytest
import torch

from tests import gemm_reference as ref

H = ref.H


def _f64(h):
    return h.astype(np.float64)


@pytest.mark.parametrize('cols', [1, 15, 16, 17, 65])
@pytest.mark.parametrize('rows_total,row0,stages', [(40, 0, 2), (33, -5, 1), (64, 30, 2), (7, 40, 1)])
def test_wgrad16_pack_then_unpack_is_the_identity_on_the_pieces(cols, rows_total, row0, stages):
    rng = np.random.default_rng(cols + rows_total)
    x = (ref.f16_two_piece(rng, (rows_total + 3, cols)) / 2048.0).astype(np.float32)
    col_scale = np.exp2(rng.integers(-2, 3, size=cols)).astype(np.float32)
    packed = ref.wgrad16_pack_reference(x, rows_total, row0, stages, col_scale, 2048.0)
    assert packed.dtype == np.uint8 and packed.size == ref.wgrad16_packed_bytes(stages, cols)
    h1, h2 = ref.wgrad16_unpack(packed, stages, cols)
    want = np.zeros((32 * stages, 16 * ((cols + 15) // 16)))
    for r in range(32 * stages):
        if 0 <= row0 + r < rows_total:
            want[r, :cols] = x[row0 + r].astype(np.float64) * col_scale * 2048.0
    assert np.array_equal(_f64(h1) + _f64(h2), want)
    assert np.array_equal(ref.wgrad16_layout(h1, h2), packed)
    if row0 >= rows_total:
        assert not packed.any()
    # lane l of chunk (stage 0, tile 0, piece 0): rows 8 (l >> 4) .. + 7, column l & 15
    chunk = packed.view(np.float16).reshape(-1, 2, 64, 8)[0, 0]
    for lane in (0, 5, 17, 63):
        assert np.array_equal(chunk[lane], h1[8 * (lane >> 4):8 * (lane >> 4) + 8, lane & 15])


@pytest.mark.parametrize('n', [1, 17, 40])
def test_dgrad16_pack_then_unpack_is_the_identity_on_the_pieces(n):
    rng = np.random.default_rng(n)
    w = (ref.f16_two_piece(rng, (8 * H, n)) / 2048.0).astype(np.float32)
    packed = ref.dgrad16_pack_reference(w, 2048.0)
    assert packed.size == ref.dgrad16_packed_bytes(n)
    h1, h2 = ref.dgrad16_unpack(packed, n)
    assert np.array_equal((_f64(h1) + _f64(h2))[:, :n], w.astype(np.float64) * 2048.0)
    assert not (_f64(h1)[:, n:].any() or _f64(h2)[:, n:].any())
    assert np.array_equal(ref.dgrad16_layout(h1, h2), packed)
    # stage (dir 1, P 3, m 1), lane (q 2, column 5), element e = 6: unit 16 P + 8 m + 2 q + 1, gate 2
    nt = (n + 15) // 16
    chunks = packed.view(np.float16).reshape(2, 64, 2, nt, 2, 64, 8)
    if n > 5:
        unit = 16 * 3 + 8 + 2 * 2 + 1
        assert chunks[1, 3, 1, 0, 0, 2 * 16 + 5, 6] == h1[4 * H + 2 * H + unit, 5]


def test_clamp_keeps_nan_and_saturates_infinities():
    v = np.array([np.nan, np.inf, -np.inf, 60000.0, 60001.0, -7e4, 3.0, -0.0], dtype=np.float32)
    c = ref.clamp_keep_nan(v)
    assert np.isnan(c[0]) and np.array_equal(c[1:], np.float32([6e4, -6e4, 6e4, 6e4, -6e4, 3.0, -0.0]))
    h1, h2 = ref.f16_split2(c)
    assert np.isnan(h1[0]) and np.isfinite(_f64(h1[1:])).all() and np.isfinite(_f64(h2[1:])).all()
    x = np.zeros((32, 3), dtype=np.float32)
    x[4, 1], x[5, 2], x[6, 0] = np.nan, np.inf, -1e30
    g1, g2 = ref.wgrad16_unpack(ref.wgrad16_pack_reference(x, 32, 0, 1, None, 2048.0), 1, 3)
    assert np.isnan(g1[4, 1]) and g1[5, 2] == np.float16(60000.0) and g1[6, 0] == np.float16(-60000.0)
    assert int(np.isnan(_f64(g1)).sum()) == 1


def test_two_piece_forms_split_as_constructed():
    rng = np.random.default_rng(0)
    v = ref.f16_two_piece(rng, (500,))
    h1, h2 = ref.f16_split2(v)
    assert np.array_equal(_f64(h1), np.round(v / 2048.0) * 2048.0) and np.abs(_f64(h2)).min() >= 1
    assert np.array_equal(_f64(h1) + _f64(h2), v)
    assert not _f64(ref.f16_split2(ref.f16_one_piece(rng, (500,), 7))[1]).any()
    p = ref.bf16_pieces(ref.bf16_three_piece(rng, (500,)))
    assert all(np.abs(q).min() > 0 for q in p)
    p = ref.bf16_pieces(ref.bf16_two_piece(rng, (500,)))
    assert np.abs(p[0]).min() > 0 and np.abs(p[1]).min() > 0 and not p[2].any()
    p = ref.bf16_pieces(ref.bf16_one_piece(rng, (500,)))
    assert not p[1].any() and not p[2].any()
    a, b = ref.bf16_piece_case(5, 7, 48, 1)
    ref.distinct(ref.exact_product(a, b))


def test_precondition_rejects_data_that_is_not_exact():
    # 320 rows of (a 2^11 + b) x 8 (in units of 2^11) are too many; 95 are not
    rng = np.random.default_rng(1)
    d = np.abs(ref.f16_two_piece(rng, (320, 4)))
    x = np.full((320, 4), 8.0 * 2048.0)
    with pytest.raises(ref.InexactData):
        ref.exact_product(d.T, x, 1.0, 2048.0)
    ref.exact_product(d[:95].T, x[:95], 1.0, 2048.0)
    with pytest.raises(ref.InexactData):
        ref.exact_product(np.array([[0.5]]), np.array([[1.0]]))           # no multiple of the granule
    with pytest.raises(ref.InexactData):
        ref.exact_product(np.array([[np.nan]]), np.array([[1.0]]))
    with pytest.raises(ref.InexactData):
        ref.exact_product(np.full((1, 2), 4096.0), np.full((2, 1), 2048.0))  # 2 x 2^23
    # two-piece against two-piece in fp16 form drops d2 x2: the generator never pairs them
    ds, xs = ref.f16_pair_case(95, 17, 33, 3)
    d2, x2 = _f64(ref.f16_split2(ds)[1]), _f64(ref.f16_split2(xs)[1])
    assert not (np.abs(d2).T @ np.abs(x2)).any()
    assert (np.abs(d2).T @ np.abs(xs - x2))[:, :].all() and (np.abs(ds - d2).T @ np.abs(x2)).all()
    ref.distinct(ref.f16_pair_product(ds, xs))
    with pytest.raises(ref.InexactData):
        ref.exact_product(ds.T, xs, 1.0, 1.0)              # (in units of 1 it would not be exact)
    with pytest.raises(AssertionError):
        ref.distinct(np.array([[1.0, 2.0], [1.0, 2.0]]))
    with pytest.raises(AssertionError):
        ref.distinct(np.array([[1.0, 1.0], [2.0, 2.0]]))


@pytest.mark.parametrize('rows,m,n,row0,x_stage0', [(33, 17, 20, 0, 0), (64, 16, 33, 0, 1),
                                                   (31, 1, 1, 0, 0)])
def test_emulated_wgrad16_walk_is_the_float64_product(rows, m, n, row0, x_stage0):
    """Packed d and packed x as MFMA fragments, three products per stage: D^T X exactly - with x
    packed for more rows than the range (x_stage0) and per-column scales of d."""
    ds, xs = ref.f16_pair_case(rows, m, n, rows + m)
    rng = np.random.default_rng(5)
    col_scale = np.exp2(rng.integers(8, 14, size=m)).astype(np.float32)
    d = (ds / col_scale).astype(np.float32)
    x = (xs / 2048.0).astype(np.float32)
    assert np.array_equal(d.astype(np.float64) * col_scale, ds)
    stages = (rows + 31) // 32
    x_all = np.concatenate([np.full((32 * x_stage0, n), 9.0, dtype=np.float32), x])
    d_pk = ref.wgrad16_pack_reference(d, rows, 0, stages, col_scale, 1.0)
    x_pk = ref.wgrad16_pack_reference(x_all, x_all.shape[0], 0, stages + x_stage0, None, 2048.0)
    got = ref.wgrad16_emulated(d_pk, m, stages, 1.0 / col_scale, x_pk, x_stage0, n, 2048.0)
    want = ref.f16_pair_product(ds, xs) / col_scale.astype(np.float64)[:, None] / 2048.0
    assert np.array_equal(want, d.astype(np.float64).T @ x.astype(np.float64))
    assert np.array_equal(got, want)
    # without the d2 x1 product the answer differs: the data needs it
    h1, _ = ref.wgrad16_unpack(d_pk, stages, m)
    short = ref.wgrad16_emulated(ref.wgrad16_layout(h1, np.zeros_like(h1)), m, stages,
                                 1.0 / col_scale, x_pk, x_stage0, n, 2048.0)
    assert (short != want).any()


@pytest.mark.parametrize('steps,batch,n', [(2, 3, 17), (1, 17, 5)])
def test_emulated_dgrad16_walk_is_the_float64_product(steps, batch, n):
    """Published dxw and packed W_ih as MFMA fragments with a fresh accumulator per stage and the
    row's inverse block scale: dxw @ W_ih exactly, with block scales that differ per (t, b, dir,
    P) - the step order of direction 1, both halves m, the first and the last producer."""
    rng = np.random.default_rng(steps + batch)
    dxw = np.zeros((steps, batch, 2, 4, H))
    units = [0, 9, 17, 24, 1008, 1023]
    dxw[..., units] = ref._nonzero_ints(rng, (steps, batch, 2, 4, len(units)), 7)
    dxw *= np.repeat(np.exp2(rng.integers(-2, 3, size=(steps, batch, 2, 1, 64))), 16, axis=-1)
    w = ref._nonzero_ints(rng, (8 * H, n), 3)
    pieces, inv = ref.publish_blocks(torch.tensor(dxw.reshape(steps, batch, 2, 4 * H),
                                                  dtype=torch.float32))
    assert tuple(pieces.shape) == (steps, 2, 64, 2, 2, 4, batch, 2, 4)
    packed = ref.dgrad16_pack_reference(w.astype(np.float32), 2048.0)
    got = ref.dgrad16_emulated(pieces, inv, packed, n, 2048.0)
    want = ref.distinct(ref.exact_product(dxw.reshape(steps * batch, 8 * H), w, 0.25, 1.0))
    assert np.array_equal(got, want)


def test_tile_orders_are_bijections():
    """Every tile exactly once for tile counts up to 19 x 19: the grouped order of the split GEMM
    and the block-scaled data gradient, and the two orders of the weight-gradient kernel - whose
    blocked branch (4 x 4 tiles per XCD) is taken per operand: at (m, nx, ny) = (1024, 1024,
    1024) by both operands, at (769, 1000, 300) by operand 0 only, at (1024, 512, 1024) by
    operand 1 only, at (1024, 256, 1024) by neither (operand 0's four tiles are no multiple
    of 8, which forbids it for operand 1 too), at (2048, 1024, none) by operand 0."""
    for tm in range(1, 20):
        for tn in range(1, 20):
            taken = [t for t in ref.tile_order_maps(tm, tn) if t is not None]
            assert sorted(taken) == [(i, j) for i in range(tm) for j in range(tn)], (tm, tn)
            for tn1 in (0, 1, 4, tn):
                order = ref.wgrad16_tile_order(tm, tn, tn1)
                want = [(0, i, j) for i in range(tm) for j in range(tn)] + \
                       [(1, i, j) for i in range(tm) for j in range(tn1)]
                assert sorted(t[:3] for t in order) == want, (tm, tn, tn1)
    t256 = lambda v: (v + 255) // 256
    blocked = lambda m, nx, ny: tuple(
        any(t[0] == w and t[3] for t in ref.wgrad16_tile_order(t256(m), t256(nx), t256(ny)))
        for w in (0, 1))
    assert blocked(1024, 1024, 1024) == (True, True)
    assert blocked(769, 1000, 300) == (True, False)
    assert blocked(1024, 512, 1024) == (False, True)
    assert blocked(1024, 256, 1024) == (False, False)
    assert blocked(2048, 1024, 0) == (True, False)
    # a full group of four tile rows then a partial one; a grid padded with idle workgroups
    order = ref.tile_order_maps(5, 2)
    assert len(order) == 16 and order.count(None) == 6
