"""The own MFMA GEMM kernels at their seams, compared exactly: the bf16 split GEMM in both forms
(csrc/split_gemm.hip), the weight-gradient pack and kernel (csrc/wgrad16.hip), the weight pack and
the block-scaled data gradient (csrc/dgrad16.hip).

Operands come from tests/gemm_reference.py: integers times powers of two with so few significant
bits that every fp16 / bf16 piece holds them exactly, every dropped piece product exactly zero,
and - checked by the reference before it hands out an expectation - sum_k |a_k| |b_k| below 2^24
granules for every output.  Every partial sum in any order is then an fp32 number, and the kernel
has to give the float64 product at EVERY element: `torch.equal` on values, 32-bit words for what
must stay untouched, no tolerance anywhere.  The expectations have no two equal rows or columns
(asserted), so a misplaced tile, row or column cannot pass.  The packed operands are compared byte
for byte with the layouts restated in the reference (which tests/test_gemm_host.py pins on the CPU
by an emulated MFMA walk).

Shapes are the smallest that reach each branch: M, N at 255 / 256 / 257 / 513, one to five K
steps, tile grids with a full group of four tile rows and a partial one and with idle workgroups
in the padded grid, both tile orders of the weight-gradient kernel per operand, one to three
stages cut into one to three parts, stage offsets, step ranges that end inside a tile.  Around
that: operands are views inside NaN-filled buffers (rows / columns past a matrix are read
clamped, never from outside), outputs are views between NaN words that must stay as they were,
`accumulate = 0` lands on NaN, a NaN or inf in an operand reaches exactly its row / column of
the output, and the wrappers refuse short buffers before anything is launched.

Second operands of the weight gradient are shifted by EVEN numbers of rows only: the pair data
alternates two-piece and one-piece rows, and an odd shift would pair two second pieces."""

import functools

import numpy as np
import pytest
import torch

from tests import gemm_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H = ref.H
NAN_WORD = 0x7FC0BEEF
NAN_HALF = 0x7E00
PAD = 64
W_SCALE = 2048.0
INF = float('inf')
MN = [(1, 1), (255, 257), (256, 256), (257, 255), (513, 1), (1, 513)]
GRIDS = [(5, 1), (1, 5), (5, 2), (3, 3), (9, 1), (4, 2), (6, 3)]


@pytest.fixture(scope='module')
def hip():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from ctc_asr_amd import hip as hip_mod
    hip_mod.load()
    return hip_mod


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _f32(want):
    """An expectation as float32, which it has to be exactly."""
    out = np.asarray(want).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), want)
    return out


def _exact(got, want):
    got = _np(got)
    return got.shape == np.shape(want) and np.array_equal(got, _f32(want))


def _inside_nan(a, left=4, right=4, rows_around=2):
    """A float32 view [r, c] of the values ``a`` inside a NaN-filled buffer: NaN rows above and
    below, NaN columns on both sides (leading dimension and offset multiples of four floats, as
    the NT form of the split GEMM asks)."""
    a = np.asarray(a, dtype=np.float32)
    r, c = a.shape
    ld = left + c + right
    ld += -ld % 4
    buf = torch.full((r + 2 * rows_around, ld), float('nan'), device=DEV)
    view = buf[rows_around:rows_around + r, left:left + c]
    view.copy_(_t(a))
    return view


class Guarded:
    """An f32 output view [m, n] with a leading dimension of n + 8 in the middle of NaN words:
    PAD words in front and behind, three columns to the left, five to the right, two rows below."""

    def __init__(self, m, n):
        self.m, self.n, self.ld = m, n, n + 8
        self.buf = torch.full((2 * PAD + (m + 2) * self.ld,), NAN_WORD, dtype=torch.int32,
                              device=DEV)
        self.view = self._view(self.buf)

    def _view(self, buf):
        body = buf[PAD:PAD + (self.m + 2) * self.ld].view(torch.float32)
        return body.view(self.m + 2, self.ld)[:self.m, 3:3 + self.n]

    def outside_intact(self):
        copy = self.buf.clone()
        self._view(copy).view(torch.int32).fill_(NAN_WORD)
        return bool((copy == NAN_WORD).all())

    def all_nan_words(self):
        return bool((self.buf == NAN_WORD).all())


def _ints(shape, seed, top=50):
    return np.random.default_rng(seed).integers(-top, top + 1, size=shape).astype(np.float64)


# ================================================================================ split GEMM
def _split_gemm(hip, form, a, b, out, accumulate):
    """out (+)= a [M, K] @ b [K, N] through the NT form (b handed over as [N, K]) or the TN form
    (a handed over as [K, M]); both operands as views inside NaN-filled buffers."""
    if form == 'nt':
        return hip.gemm_split_nt(_inside_nan(a), _inside_nan(b.T), out=out, accumulate=accumulate)
    return hip.gemm_split_tn(_inside_nan(a.T), _inside_nan(b), out, accumulate=accumulate)


def _check_split_gemm(hip, form, a, b):
    m, n = a.shape[0], b.shape[1]
    want = ref.distinct(ref.exact_product(a, b))
    out = Guarded(m, n)
    _split_gemm(hip, form, a, b, out.view, False)              # onto NaN: the old out is not read
    assert _exact(out.view, want)
    assert out.outside_intact()
    have = _ints((m, n), m + n)
    out.view.copy_(_t(have))
    _split_gemm(hip, form, a, b, out.view, True)
    assert _exact(out.view, want + have)
    assert out.outside_intact()


SEAMS = [('nt', m, n, 16) for m, n in MN] + [('nt', 255, 257, k) for k in (32, 48, 80)] + \
        [('tn', m, n, 17) for m, n in MN] + [('tn', 255, 257, k) for k in (1, 15, 16, 31, 33, 47)]


@pytest.mark.parametrize('form,m,n,k', SEAMS)
def test_split_gemm_is_exact_at_the_seams(hip, form, m, n, k):
    """M, N one below, at and one above a tile and two tiles and a row; NT: 1, 2, 3 and 5 K steps
    (both loop tails, the clamped refills); TN: K below, at and above one and two steps, rows past
    K counting as zeros."""
    _check_split_gemm(hip, form, *ref.int_case(m, n, k, 0))


@pytest.mark.parametrize('form', ['nt', 'tn'])
@pytest.mark.parametrize('tm,tn', GRIDS)
def test_split_gemm_tile_grids(hip, form, tm, tn):
    """Tile grids at one K step, the last tile row and column one element wide: a full group of
    four tile rows followed by a partial one, grids padded to a multiple of 8 with up to seven
    idle workgroups."""
    _check_split_gemm(hip, form, *ref.int_case(256 * (tm - 1) + 1, 256 * (tn - 1) + 1, 16, tm + tn))


@pytest.mark.parametrize('form,m,n,k', [('nt', 257, 255, 48), ('nt', 33, 300, 80),
                                        ('tn', 257, 255, 17), ('tn', 300, 33, 33)])
def test_split_gemm_needs_each_of_its_six_piece_products(hip, form, m, n, k):
    """Three-piece values against powers of two both ways round and two-piece against two-piece:
    every output needs a1 b1, a2 b1, a3 b1, a1 b2, a1 b3 and a2 b2; the dropped products are zero."""
    _check_split_gemm(hip, form, *ref.bf16_piece_case(m, n, k, 0))


@pytest.mark.parametrize('form', ['nt', 'tn'])
@pytest.mark.parametrize('bad', [float('nan'), INF])
def test_split_gemm_non_finite_values_reach_their_row_or_column_only(hip, form, bad):
    """A NaN or an inf in A[i, k] makes row i non-finite, in B[k, j] column j; every other element
    keeps its bits - the last row / column included, which the clamped loads of the tiles' idle
    rows read again."""
    m, n, k = 257, 300, 32 if form == 'nt' else 33
    a, b = ref.int_case(m, n, k, 5)
    want = _f32(ref.exact_product(a, b))
    for i, kk in ((0, 0), (m - 1, k - 1), (130, 7)):
        a2 = a.copy()
        a2[i, kk] = bad
        got = _np(_split_gemm(hip, form, a2, b, torch.empty(m, n, device=DEV), False))
        assert not np.isfinite(got[i]).any()
        rest = np.arange(m) != i
        assert np.array_equal(got[rest], want[rest])
    for j, kk in ((0, 1), (n - 1, k - 1), (256, 9)):
        b2 = b.copy()
        b2[kk, j] = bad
        got = _np(_split_gemm(hip, form, a, b2, torch.empty(m, n, device=DEV), False))
        assert not np.isfinite(got[:, j]).any()
        rest = np.arange(n) != j
        assert np.array_equal(got[:, rest], want[:, rest])


# =============================================================================== wgrad16: pack
def _pack_input(rows, cols, seed):
    """Values whose scaled form (times 2^11) exercises the split: random floats, two-piece and
    one-piece forms, ties of the fp16 rounding, values at and past the +-60000 clamp, infinities."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(rows, cols)) * np.exp2(rng.integers(-12, 4, size=(rows, cols)))
    x[::3] = ref.f16_two_piece(rng, x[::3].shape) / 2048.0
    special = np.array([2049.0, -2049.0, 2051.0, 4098.0, -4102.0, 60000.0, -60000.0, 60000.5,
                        59999.0, 65504.0, -65520.0, 1e9, -1e9, 0.0, -0.0, 2.0 ** -24, 2.0 ** -26,
                        1.0 + 2.0 ** -11, INF, -INF]) / 2048.0
    flat = x.reshape(-1)
    where = rng.permutation(flat.size)[:min(flat.size, 3 * special.size)]
    flat[where] = np.resize(special, where.size)
    return x.astype(np.float32)


def _wgrad16_pack(hip, x, rows_total, row0, stages, scale, col_scale):
    """`hip.wgrad16_pack` of a view inside a NaN-filled buffer into a longer dirty buffer: the
    bytes, after checking that nothing behind them was written."""
    need = ref.wgrad16_packed_bytes(stages, x.shape[1])
    out = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    got = hip.wgrad16_pack(_inside_nan(x, left=3, right=2), rows_total, row0, stages, scale,
                           col_scale=None if col_scale is None else _t(col_scale), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((out[need:] == 0xAB).all())
    return _np(out[:need])


@pytest.mark.parametrize('cols', [1, 15, 16, 17, 63, 64, 65, 300])
def test_wgrad16_pack_bit_for_bit(hip, cols):
    """Column counts around one and four column tiles (the block covers 64 columns) with the zero
    columns up to the tile; row ranges that start before the matrix, inside it, cross its end and
    lie wholly outside (all zeros); `rows_total` below, at and above a multiple of 32; with and
    without column scales; x a column slice of a wider NaN-filled matrix."""
    for rows_total, row0, stages in ((31, 0, 1), (32, 0, 1), (33, 0, 2), (33, -7, 1), (70, -40, 2),
                                     (70, 17, 1), (70, 60, 2), (33, 33, 1), (31, 64, 1),
                                     (31, -32, 1), (95, -3, 4)):
        for scaled in (True, False):
            x = _pack_input(rows_total + 2, cols, cols + rows_total + row0)
            rng = np.random.default_rng(cols)
            col_scale = np.exp2(rng.integers(-3, 4, size=cols)).astype(np.float32) if scaled else None
            want = ref.wgrad16_pack_reference(x, rows_total, row0, stages, col_scale, W_SCALE)
            got = _wgrad16_pack(hip, x, rows_total, row0, stages, W_SCALE, col_scale)
            assert np.array_equal(got, want), (rows_total, row0, stages, scaled)
            if row0 >= rows_total or row0 + 32 * stages <= 0:
                assert not got.any()


def test_wgrad16_pack_keeps_nan_and_saturates(hip):
    """A NaN stays a NaN in h1 (and in h2); infinities and values past the clamp come out as
    +-60000; nothing else is non-finite."""
    x = np.zeros((40, 20), dtype=np.float32)
    x[3, 4], x[33, 19], x[5, 0], x[6, 1], x[7, 2], x[8, 3] = np.nan, np.nan, INF, -INF, 1e30, -40.0
    col_scale = np.ones(20, dtype=np.float32)
    for cs in (None, col_scale):
        got = _wgrad16_pack(hip, x, 40, 0, 2, W_SCALE, cs)
        assert np.array_equal(got, ref.wgrad16_pack_reference(x, 40, 0, 2, cs, W_SCALE))
        h1, h2 = ref.wgrad16_unpack(got, 2, 20)
        assert np.isnan(h1[3, 4]) and np.isnan(h1[33, 19]) and np.isnan(h2[3, 4])
        assert int(np.isnan(h1.astype(np.float32)).sum()) == 2
        assert h1[5, 0] == 60000.0 and h1[6, 1] == -60000.0 and h1[7, 2] == 60000.0
        assert h1[8, 3] == -60000.0
    # a NaN column scale makes its column NaN and no other
    col_scale[7] = np.nan
    x = np.ones((32, 20), dtype=np.float32)
    h1, _ = ref.wgrad16_unpack(_wgrad16_pack(hip, x, 32, 0, 1, 1.0, col_scale), 1, 20)
    assert np.isnan(h1[:, 7]).all() and int(np.isnan(h1.astype(np.float32)).sum()) == 32


# =============================================================================== wgrad16: gemm
def _shifted(y, shift):
    """Rows r + shift of y at row r, zeros outside."""
    out = np.zeros_like(y)
    rows = y.shape[0]
    lo, hi = max(0, -shift), min(rows, rows - shift)
    if hi > lo:
        out[lo:hi] = y[lo + shift:hi + shift]
    return out


@functools.lru_cache(maxsize=None)
def _wgrad_data(rows, m, nx, ny, shift, seed):
    """Pair data (scaled d, x, y), column scales of d and the exact dW_x, dW_y of the scaled
    operands (float64; to be divided by the scales).  Columns whose outputs repeat another's are
    drawn again until dW_x has no two equal rows or columns, and dW_y neither where at least 16
    rows of the shifted y meet d (below that the few values a piece form takes cannot tell 257
    rows apart; dW_x of the same launch can).  A single row: one-piece integers up to 2047
    without repetition instead (a two-piece form has 24 values)."""
    rng = np.random.default_rng(seed)
    if rows == 1:
        pool = np.concatenate([np.arange(-2047.0, 0.0), np.arange(1.0, 2048.0)])
        ds = rng.permutation(pool)[:m].reshape(1, m)
        both = rng.permutation(pool)[:nx + ny].reshape(1, nx + ny)
        product = lambda d, x: ref.exact_product(d.T, x)
    else:
        ds = ref.f16_pair_columns(rng, rows, m, 'd')
        both = ref.f16_pair_columns(rng, rows, nx + ny, 'x')
        product = ref.f16_pair_product
    check_y = ny and rows - abs(shift) >= 16
    for attempt in range(200):
        xs, ys = both[:, :nx], both[:, nx:]
        want_x = product(ds, xs)
        want_y = product(ds, _shifted(ys, shift)) if ny else None
        again_d, again_x = ref.repeated(want_x, 0), ref.repeated(want_x, 1)
        if check_y:
            again_d = np.union1d(again_d, ref.repeated(want_y, 0))
            again_x = np.union1d(again_x, nx + ref.repeated(want_y, 1))
        if not again_d.size and not again_x.size:
            break
        assert rows > 1
        ds[:, again_d] = ref.f16_pair_columns(rng, rows, again_d.size, 'd')
        both[:, again_x] = ref.f16_pair_columns(rng, rows, again_x.size, 'x')
    ref.distinct(want_x)
    if check_y:
        ref.distinct(want_y)
    col_scale = np.exp2(np.random.default_rng(seed).integers(6, 14, size=m))
    return ds, xs, ys, col_scale, want_x, want_y


def _sync_words_zero(hip):
    sync = hip.wgrad16_sync_words(DEV)
    return not hip.wgrad16_gave_up_waiting(DEV) and (sync is None or int(sync.abs().sum()) == 0)


def _check_wgrad(hip, rows, m, nx, ny, parts=1, shift=0, seed=0, x_stage0=0, y_stage0=0,
                 x_scale=2048.0, y_scale=32768.0, by_reference=False, onto_ints=False,
                 defer=False):
    """One exact weight-gradient launch: d with power-of-two column scales, x and the shifted y
    packed by the kernel (or by the reference's bytes) - the second operands for ``*_stage0``
    stages of NaN rows more than the range in front of it - into guarded outputs.  ``defer``:
    returns (launch, verify) instead of running them."""
    ds, xs, ys, col_scale, want_x, want_y = _wgrad_data(rows, m, nx, ny, shift, seed)
    stages = (rows + 31) // 32
    d = (ds / col_scale).astype(np.float32)
    inv = _t(1.0 / col_scale)

    def pack(values, rows_total, row0, n_stages, scale, cs):
        if by_reference:
            return _t(ref.wgrad16_pack_reference(values, rows_total, row0, n_stages, cs, scale),
                      torch.uint8)
        return hip.wgrad16_pack(_inside_nan(values, left=3, right=2), rows_total, row0, n_stages,
                                scale, col_scale=None if cs is None else _t(cs))

    def second(values, scale, stage0, row_shift):
        front = np.full((32 * stage0, values.shape[1]), np.nan, dtype=np.float32)
        whole = np.concatenate([front, (values / scale).astype(np.float32)])
        return pack(whole, whole.shape[0], row_shift, stage0 + stages, scale, None)

    d_pk = pack(d, rows, 0, stages, 1.0, col_scale.astype(np.float32))
    x_pk = second(xs, x_scale, x_stage0, 0)
    if x_stage0:
        # the stages in front of the range hold NaN: nothing of them may be read
        assert np.isnan(ref.wgrad16_unpack(_np(x_pk), x_stage0 + stages, nx)[0][:32 * x_stage0]
                        .astype(np.float32)).any()
    out_x, out_y = Guarded(m, nx), Guarded(m, max(ny, 1))
    def onto(shape, seed, scale):
        # integers - for a single row of 22-bit products two bits above the product, whose
        # granule leaves no room for more
        if not onto_ints:
            return np.zeros(shape)
        if rows == 1:
            return _ints(shape, seed, 3) * 2.0 ** 22 / col_scale[:, None] / scale
        return _ints(shape, seed)

    have_x, have_y = onto((m, nx), 3, x_scale), onto((m, max(ny, 1)), 4, y_scale)
    out_x.view.copy_(_t(have_x))
    out_y.view.copy_(_t(have_y))
    y_pk = None
    if ny:
        # y is packed with its rows shifted: rows 32 * y_stage0 + r + shift of the buffer
        front = np.full((32 * y_stage0, ny), np.nan, dtype=np.float32)
        whole = np.concatenate([front, (ys / y_scale).astype(np.float32)])
        if y_stage0:
            # (pack in two goes, so that the NaN rows in front do not enter through the shift)
            y_pk = torch.empty(ref.wgrad16_packed_bytes(y_stage0 + stages, ny), dtype=torch.uint8,
                               device=DEV)
            cut = ref.wgrad16_packed_bytes(y_stage0, ny)
            y_pk[:cut] = pack(whole, 32 * y_stage0, 0, y_stage0, y_scale, None)
            y_pk[cut:] = pack((ys / y_scale).astype(np.float32), rows, shift, stages, y_scale, None)
        else:
            y_pk = pack(whole, rows, shift, stages, y_scale, None)
    def launch():
        hip.wgrad16_gemm(d_pk, m, stages, inv, x_pk, x_stage0, x_scale, out_x.view,
                         y_packed=y_pk, y_stage0=y_stage0, y_scale=y_scale,
                         dw_y=out_y.view if ny else None, parts=parts)

    def verify():
        assert _exact(out_x.view, want_x / col_scale[:, None] / x_scale + have_x)
        assert out_x.outside_intact()
        if ny:
            assert _exact(out_y.view, want_y / col_scale[:, None] / y_scale + have_y)
            assert out_y.outside_intact()
    if defer:
        return launch, verify
    launch()
    verify()
    if parts > 1:
        assert _sync_words_zero(hip)


TRIPLES = [(1, 1, 1), (15, 17, 16), (16, 16, 15), (17, 15, 17), (255, 257, 256), (256, 256, 255),
           (257, 255, 257), (513, 1, 16), (1, 513, 255), (257, 513, 1), (16, 256, 513),
           (255, 16, 0)]


@pytest.mark.parametrize('m,nx,ny', TRIPLES)
def test_wgrad16_gemm_is_exact_at_the_seams(hip, m, nx, ny):
    """Output rows and columns of both second operands below, at and above one MFMA tile, one and
    two workgroup tiles; one triple without the second output.  33 rows: a second stage of one
    row.  Every output needs d1 x1, d1 x2 and d2 x1."""
    _check_wgrad(hip, 33, m, nx, ny, seed=1)


@pytest.mark.parametrize('rows', [1, 31, 32, 33, 64, 95])
def test_wgrad16_gemm_rows_parts_and_shifts(hip, rows):
    """1 to 3 stages, the last one partly or wholly filled, cut into 1, 2 and 3 parts and into
    more parts than stages; y shifted by +-2 and +-32 rows across both ends and wholly outside;
    accumulation onto integers; operands packed by the reference's bytes."""
    for parts, shift in ((1, -2), (2, 2), (3, -32), (8, 32), (2, -96), (1, 0)):
        _check_wgrad(hip, rows, 257, 255, 17, parts=parts, shift=shift, seed=rows,
                     onto_ints=parts == 2)
    _check_wgrad(hip, rows, 257, 255, 17, parts=2, shift=-2, seed=rows, by_reference=True)
    if rows >= 64:
        # a shifted dW_y of one and of two tiles, no two rows or columns of it equal
        for ny, shift in ((255, -2), (257, 32)):
            assert rows - abs(shift) >= 16
            _check_wgrad(hip, rows, 257, 17, ny, parts=2, shift=shift, seed=rows + ny)


@pytest.mark.parametrize('x_stage0,y_stage0', [(2, 0), (0, 2), (2, 2)])
def test_wgrad16_gemm_stage_offsets_into_longer_operands(hip, x_stage0, y_stage0):
    """Second operands packed for two stages more than the range, those stages full of NaN: the
    kernel starts at `*_stage0` and reads nothing in front of it; with partial tiles and parts."""
    for rows, parts in ((33, 1), (64, 2), (95, 3)):
        _check_wgrad(hip, rows, 257, 300, 255, parts=parts, shift=2, seed=7, x_stage0=x_stage0,
                     y_stage0=y_stage0)


@pytest.mark.parametrize('m,nx,ny', [(1024, 1024, 1024), (769, 1000, 300), (1024, 512, 1024),
                                     (1024, 256, 1024), (2048, 1024, 0)])
def test_wgrad16_gemm_tile_orders(hip, m, nx, ny):
    """Both tile orders per operand at 64 rows: both operands in 4 x 4 blocks per XCD; operand 0
    blocked and operand 1 row-major; the other way round; operand 0's tile count forbidding the
    blocked order for an operand 1 that would qualify; two block rows without a second operand."""
    t256 = lambda v: (v + 255) // 256
    order = ref.wgrad16_tile_order(t256(m), t256(nx), t256(ny))
    want = {(1024, 1024, 1024): (True, True), (769, 1000, 300): (True, False),
            (1024, 512, 1024): (False, True), (1024, 256, 1024): (False, False),
            (2048, 1024, 0): (True, False)}[(m, nx, ny)]
    assert tuple(any(t[0] == w and t[3] for t in order) for w in (0, 1)) == want
    for parts in (1, 2):
        _check_wgrad(hip, 64, m, nx, ny, parts=parts, seed=2)


def test_wgrad16_gemm_launches_of_two_streams_take_turns(hip):
    """Launches with two parts each on streams of their own into different outputs share the
    tiles' turn words: first two, then four (16 workgroups in all: every part is resident), each
    set queued behind one busy kernel so that its launches start together.  All exact - a part 1
    released by ANOTHER launch's part 0 would add beside its own part 0 and lose an update - and
    the words back at zero."""
    _check_wgrad(hip, 33, 16, 16, 0, parts=2, seed=10)      # (the device's words exist and are zero)
    for seeds in ((11, 12), (13, 14, 15, 16)):
        pending = [_check_wgrad(hip, 64, 256, 256, 256, parts=2, seed=seed, defer=True)
                   for seed in seeds]
        streams = [torch.cuda.Stream() for _ in seeds]
        torch.cuda.synchronize()
        hip.occupy_cus(1, 2000)
        for (launch, _), stream in zip(pending, streams):
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                launch()
        torch.cuda.synchronize()
        for _, verify in pending:
            verify()
        assert _sync_words_zero(hip)


@pytest.mark.parametrize('parts', [1, 2])
def test_wgrad16_gemm_nan_reaches_its_row_or_column_only(hip, parts):
    """A NaN in d[r, m] makes exactly row m of both outputs NaN, a NaN in x[r, n] exactly column
    n of dW_x: through the pack (which keeps it) and the kernel; every other element keeps its
    bits."""
    rows, m, nx, ny = 64, 257, 300, 33
    ds, xs, ys, col_scale, want_x, want_y = _wgrad_data(rows, m, nx, ny, 0, 21)
    inv = _t(1.0 / col_scale)
    want_x = _f32(want_x / col_scale[:, None] / 2048.0)
    want_y = _f32(want_y / col_scale[:, None] / 2048.0)

    def run(d, x):
        d_pk = hip.wgrad16_pack(_t(d), rows, 0, 2, 1.0, col_scale=_t(col_scale))
        x_pk = hip.wgrad16_pack(_t(x), rows, 0, 2, 2048.0)
        y_pk = hip.wgrad16_pack(_t(ys / 2048.0), rows, 0, 2, 2048.0)
        dw_x, dw_y = torch.zeros(m, nx, device=DEV), torch.zeros(m, ny, device=DEV)
        hip.wgrad16_gemm(d_pk, m, 2, inv, x_pk, 0, 2048.0, dw_x, y_packed=y_pk, y_scale=2048.0,
                         dw_y=dw_y, parts=parts)
        return _np(dw_x), _np(dw_y)

    d, x = ds / col_scale, xs / 2048.0
    for r, mm in ((0, 0), (63, 256), (40, 100)):
        bad = d.copy()
        bad[r, mm] = np.nan
        got_x, got_y = run(bad, x)
        rest = np.arange(m) != mm
        assert np.isnan(got_x[mm]).all() and np.isnan(got_y[mm]).all()
        assert np.array_equal(got_x[rest], want_x[rest]) and np.array_equal(got_y[rest], want_y[rest])
    for r, nn in ((0, 0), (63, 299), (33, 256)):
        bad = x.copy()
        bad[r, nn] = np.nan
        got_x, got_y = run(d, bad)
        rest = np.arange(nx) != nn
        assert np.isnan(got_x[:, nn]).all()
        assert np.array_equal(got_x[:, rest], want_x[:, rest]) and np.array_equal(got_y, want_y)
    assert _sync_words_zero(hip)


# ====================================================================== dgrad16: pack and kernel
@pytest.mark.parametrize('n', [1, 15, 16, 17, 255, 257, 300])
def test_dgrad16_pack_weights_bit_for_bit(hip, n):
    """Column counts around one tile, around the four tiles a block covers and around a kernel
    tile; W a column slice of a wider NaN-filled matrix; ties, the clamp, infinities; NaN kept."""
    w = _pack_input(8 * H, n, n)
    w[8 * H - 1, n - 1], w[4 * H, 0] = np.nan, np.nan
    need = ref.dgrad16_packed_bytes(n)
    assert hip.dgrad16_packed_bytes(n) == need
    out = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    hip.dgrad16_pack_weights(_inside_nan(w, left=3, right=2), H, W_SCALE, out=out)
    assert bool((out[need:] == 0xAB).all())
    got = _np(out[:need])
    assert np.array_equal(got, ref.dgrad16_pack_reference(w, W_SCALE))
    h1, h2 = ref.dgrad16_unpack(got, n)
    nan = np.isnan(h1.astype(np.float32))
    assert nan[8 * H - 1, n - 1] and nan[4 * H, 0] and int(nan.sum()) == 2
    finite = h1.astype(np.float32)[~nan]
    assert np.abs(finite).max() == 60000.0 and np.isfinite(h2.astype(np.float32)[~nan]).all()


def _dgrad_dense(steps, batch, n, seed):
    """One-piece data over all of K = 8192: dxw = c 2^e with |c| <= 7 and a block exponent e in
    -2 .. 2 per (t, b, dir, P) - the published block scales then differ by up to 2^+-2 - against
    integer weights |w| <= 3."""
    rng = np.random.default_rng(seed)
    dxw = ref._nonzero_ints(rng, (steps, batch, 2, 4, H), 7)
    dxw *= np.repeat(np.exp2(rng.integers(-2, 3, size=(steps, batch, 2, 1, H // 16))), 16, axis=-1)
    w = ref._nonzero_ints(rng, (8 * H, n), 3)
    return dxw.reshape(steps, batch, 2, 4 * H), w, 0.25, 1.0


def _dgrad_pieces(steps, batch, n, seed):
    """Sparse K that needs each of d1 w1, d2 w1 and d1 w2: 8 units in the first two and the last
    producers, both halves m, all gates, both directions; on even units dxw is two-piece
    (a 2^11 + b) and W an integer, on odd units dxw is c 2^11 and W two-piece ((a 2^11 + b) /
    2^11).  One block scale everywhere (the bits the pieces take leave no room for more)."""
    rng = np.random.default_rng(seed)
    units = np.array([0, 1, 8, 9, 16, 17, 1014, 1023])
    dxw = np.zeros((steps, batch, 2, 4, H))
    w = np.zeros((2, 4, H, n))
    even, odd = units[units % 2 == 0], units[units % 2 == 1]
    dxw[..., even] = ref.f16_two_piece(rng, dxw[..., even].shape)
    w[:, :, even] = ref._nonzero_ints(rng, w[:, :, even].shape, 3)
    dxw[..., odd] = ref.f16_one_piece(rng, dxw[..., odd].shape, 7)
    w[:, :, odd] = ref.f16_two_piece(rng, w[:, :, odd].shape) / 2048.0
    ga = np.ones((2, 4, H))
    ga[:, :, odd] = 2048.0
    gb = np.ones((2, 4, H))
    gb[:, :, odd] = 1.0 / 2048.0
    return dxw.reshape(steps, batch, 2, 4 * H), w.reshape(8 * H, n), ga.reshape(-1), gb.reshape(-1)


def _dgrad_ids(steps, batch, n, seed):
    """For a single output column, where a row of the product is one number: two k carry the row's
    number (row % 128 + 1 and (row // 128 + 1) 128 against weights of 1), a random 32nd of K holds
    c 2^12 (|c| <= 3) against integer weights |w| <= 3, which fills the bits above."""
    rng = np.random.default_rng(seed)
    rows = steps * batch
    dxw = ref._nonzero_ints(rng, (rows, 8 * H), 3) * 4096.0 * (rng.random((rows, 8 * H)) < 1 / 32)
    w = ref._nonzero_ints(rng, (8 * H, n), 3)
    k_a, k_b = 5, 4 * H + 3 * H + 1020
    dxw[:, k_a], dxw[:, k_b] = np.arange(rows) % 128 + 1, (np.arange(rows) // 128 + 1) * 128
    w[k_a], w[k_b] = 1, 1
    return dxw.reshape(steps, batch, 2, 4 * H), w, 1.0, 1.0


@functools.lru_cache(maxsize=None)
def _dgrad_case(kind, steps, batch, n, seed=0):
    make = {'dense': _dgrad_dense, 'pieces': _dgrad_pieces, 'ids': _dgrad_ids}[kind]
    dxw, w, ga, gb = make(steps, batch, n, seed)
    flat = dxw.reshape(steps * batch, 8 * H)
    want = ref.distinct(ref.exact_product(flat, w, ga, gb))
    halves = [ref.exact_product(flat[:, 4 * H * d:4 * H * (d + 1)], w[4 * H * d:4 * H * (d + 1)],
                                np.broadcast_to(ga, (8 * H,))[4 * H * d:4 * H * (d + 1)],
                                np.broadcast_to(gb, (8 * H,))[4 * H * d:4 * H * (d + 1)])
              for d in (0, 1)]
    return dxw, w, want, halves


def _publish_poisoned(hip, dxw, t_lo=0, t_hi=None):
    """`publish` into a workspace whose exchange blocks of the steps outside [t_lo, t_hi) and
    whose inverse scales of the rows past B (and of those steps) hold NaN."""
    steps, batch = dxw.shape[:2]
    t_hi = steps if t_hi is None else t_hi
    ws = ref.publish(hip, _t(dxw))
    x_off, s_off = hip.dgrad16_published_offsets(steps, batch, H)
    block = 2 * batch * 4 * H * 4
    halves = ws[x_off + block:x_off + block * (steps + 1)].view(torch.int16).view(steps, 2, -1)
    scales = ws[s_off:s_off + steps * 2 * 64 * 32 * 4].view(torch.float32).view(steps, 2, 64, 32)
    scales[..., batch:] = float('nan')
    for t in list(range(t_lo)) + list(range(t_hi, steps)):
        for d, s in ((0, t), (1, steps - 1 - t)):
            halves[s, d] = NAN_HALF
            scales[s, d] = float('nan')
    return ws


DGRAD_SHAPES = [(1, 1, 1), (1, 16, 16), (2, 17, 257), (3, 32, 255), (16, 15, 300), (17, 16, 256),
                (9, 32, 513), (33, 32, 1), (65, 16, 257)]


@pytest.mark.parametrize('steps,batch,n', DGRAD_SHAPES)
def test_dgrad16_blockscaled_is_exact_at_the_seams(hip, steps, batch, n):
    """One row, one unit, a unit and a row, two units; a second row tile of one step; column tiles
    a column short and a column over; 5 row tiles; 5 x 2 tiles in a grid padded to 16.  Block
    scales differ per (t, b, dir, P); inverse scales of the rows past B are NaN.  Whole, into a
    guarded view with `ld_dx > n`; then one direction and the other added to it, both ways
    round; then everything added onto integers.  (A single output column takes `_dgrad_ids`.)"""
    dxw, w, want, halves = _dgrad_case('ids' if n == 1 and steps * batch > 1 else 'dense',
                                       steps, batch, n)
    ws = _publish_poisoned(hip, dxw)
    packed = hip.dgrad16_pack_weights(_t(w), H, W_SCALE)
    out = Guarded(steps * batch, n)
    hip.dgrad16_blockscaled(ws, steps, batch, H, packed, W_SCALE, n, out=out.view)
    assert _exact(out.view, want)
    assert out.outside_intact()
    for first in (0, 1):
        out = Guarded(steps * batch, n)
        hip.dgrad16_blockscaled(ws, steps, batch, H, packed, W_SCALE, n, out=out.view,
                                dirs=(first, first + 1))
        assert _exact(out.view, halves[first])
        hip.dgrad16_blockscaled(ws, steps, batch, H, packed, W_SCALE, n, out=out.view,
                                dirs=(1 - first, 2 - first), accumulate=True)
        assert _exact(out.view, want)
        assert out.outside_intact()
    have = _ints((steps * batch, n), n)
    out.view.copy_(_t(have))
    hip.dgrad16_blockscaled(ws, steps, batch, H, packed, W_SCALE, n, out=out.view, dirs=(0, 2),
                            accumulate=True)
    assert _exact(out.view, want + have)
    assert out.outside_intact()


@pytest.mark.parametrize('steps,batch,n,ranges', [
    (3, 32, 255, [(0, 1), (1, 3), (2, 3)]), (17, 16, 256, [(0, 16), (16, 17), (5, 17), (3, 4)]),
    (9, 32, 513, [(1, 9), (0, 8), (4, 5)]), (20, 17, 17, [(0, 9), (7, 20), (19, 20)])])
def test_dgrad16_blockscaled_step_ranges(hip, steps, batch, n, ranges):
    """Step ranges that end inside a tile (a tile is 16 units: 16 steps of B <= 16, 8 of more):
    the rows of the range are exact, every other row stays untouched as words, and the exchange
    blocks and inverse scales of the steps outside the range hold NaN - nothing unpublished
    reaches dx."""
    dxw, w, want, _ = _dgrad_case('dense', steps, batch, n)
    packed = hip.dgrad16_pack_weights(_t(w), H, W_SCALE)
    want = _f32(want)
    for t_lo, t_hi in ranges:
        ws = _publish_poisoned(hip, dxw, t_lo, t_hi)
        out = Guarded(steps * batch, n)
        hip.dgrad16_blockscaled(ws, steps, batch, H, packed, W_SCALE, n, out=out.view,
                                steps=(t_lo, t_hi))
        rows = slice(t_lo * batch, t_hi * batch)
        assert np.array_equal(_np(out.view[rows]), want[rows]), (t_lo, t_hi)
        out.view[rows].view(torch.int32).fill_(NAN_WORD)
        assert out.all_nan_words(), (t_lo, t_hi)


@pytest.mark.parametrize('steps,batch,n', [(2, 17, 257), (17, 16, 33)])
def test_dgrad16_blockscaled_needs_each_of_its_three_piece_products(hip, steps, batch, n):
    """Two-piece dxw against one-piece weights and the other way round, over both stage parities,
    both directions, the first and the last producer: d1 w1, d2 w1 and d1 w2 are all needed,
    d2 w2 - which the kernel drops - is zero."""
    dxw, w, want, halves = _dgrad_case('pieces', steps, batch, n)
    ws = _publish_poisoned(hip, dxw)
    # the reference's bytes for the weights here, the kernel's own pack elsewhere
    packed = _t(ref.dgrad16_pack_reference(w.astype(np.float32), W_SCALE), torch.uint8)
    assert torch.equal(packed, hip.dgrad16_pack_weights(_t(w), H, W_SCALE))
    h1, h2 = ref.dgrad16_unpack(_np(packed), n)
    assert h2.astype(np.float32).any()
    out = Guarded(steps * batch, n)
    hip.dgrad16_blockscaled(ws, steps, batch, H, packed, W_SCALE, n, out=out.view)
    assert _exact(out.view, want)
    assert out.outside_intact()


def test_dgrad16_blockscaled_nan_reaches_its_row_or_column_only(hip):
    """A NaN piece in the published row (t, b) makes exactly row t B + b of dx NaN - for either
    piece, either direction and the last row of the batch, which the clamped loads of a unit's
    idle rows read again; a NaN weight in column n exactly that column."""
    steps, batch, n = 3, 17, 257
    dxw, w, want, _ = _dgrad_case('dense', steps, batch, n)
    want = _f32(want)
    packed = hip.dgrad16_pack_weights(_t(w), H, W_SCALE)
    clean = ref.publish(hip, _t(dxw))
    x_off, _ = hip.dgrad16_published_offsets(steps, batch, H)
    block = 2 * batch * 4 * H * 4
    for t, b, d, p, half, piece, q, e in ((0, 0, 0, 0, 0, 0, 0, 0), (2, 16, 1, 63, 1, 1, 3, 7),
                                          (1, 15, 0, 31, 1, 0, 2, 5), (1, 16, 1, 5, 0, 1, 1, 2)):
        ws = clean.clone()
        view = ws[x_off + block:x_off + block * (steps + 1)].view(torch.int16).view(
            steps, 2, 64, 2, 2, 4, batch, 8)
        view[t if d == 0 else steps - 1 - t, d, p, half, piece, q, b, e] = NAN_HALF
        got = _np(hip.dgrad16_blockscaled(ws, steps, batch, H, packed, W_SCALE, n))
        row = t * batch + b
        rest = np.arange(steps * batch) != row
        assert np.isnan(got[row]).all(), (t, b, d)
        assert np.array_equal(got[rest], want[rest]), (t, b, d)
    for k, col in ((0, 0), (8 * H - 1, 256), (5000, 17)):
        bad = w.copy()
        bad[k, col] = np.nan
        got = _np(hip.dgrad16_blockscaled(clean, steps, batch, H,
                                          hip.dgrad16_pack_weights(_t(bad), H, W_SCALE), W_SCALE, n))
        rest = np.arange(n) != col
        assert np.isnan(got[:, col]).all()
        assert np.array_equal(got[:, rest], want[:, rest])


# =========================================================================== wrapper refusals
def test_wrappers_refuse_short_buffers_before_any_launch(hip):
    """Sizes go to the kernels as they are: a short buffer would be an out-of-bounds DMA.  The
    wrappers raise `CtcAsrError` instead; the outputs stay as they were."""
    err = hip.CtcAsrError
    x = torch.ones(40, 20, device=DEV)
    with pytest.raises(err):
        hip.wgrad16_pack(x, 41, 0, 2, 1.0)                            # rows_total > rows of x
    with pytest.raises(err):
        hip.wgrad16_pack(x[:, :17], 40, 0, 2, 1.0, col_scale=torch.ones(16, device=DEV))
    with pytest.raises(err):
        hip.wgrad16_pack(x, 40, 0, 2, 1.0, col_scale=torch.ones(21, device=DEV))
    with pytest.raises(err):
        hip.wgrad16_pack(x, 40, 0, 2, 1.0, col_scale=torch.ones(20))   # another device
    with pytest.raises(err):
        hip.wgrad16_pack(x, 40, 0, 2, 1.0, out=torch.empty(2 * 2 * 2048 - 1, dtype=torch.uint8,
                                                            device=DEV))
    m, nx, ny, stages = 20, 20, 17, 2
    d_pk = hip.wgrad16_pack(x, 40, 0, stages, 1.0)
    x_pk = hip.wgrad16_pack(x, 40, 0, stages, 1.0)
    y_pk = hip.wgrad16_pack(x[:, :ny], 40, 0, stages, 1.0)
    inv = torch.ones(m, device=DEV)
    dw_x = torch.full((m, nx), 5.0, device=DEV)
    dw_y = torch.full((m, ny), 6.0, device=DEV)

    def gemm(d=d_pk, xp=x_pk, yp=y_pk, scales=inv, x0=0, y0=0, out_x=dw_x, out_y=dw_y, parts=1):
        hip.wgrad16_gemm(d, m, stages, scales, xp, x0, 1.0, out_x, y_packed=yp, y_stage0=y0,
                         y_scale=1.0, dw_y=out_y, parts=parts)

    for bad in (dict(d=d_pk[:-1]), dict(xp=x_pk[:-1]), dict(yp=y_pk[:-1]), dict(x0=1), dict(y0=1),
                dict(x0=-1), dict(y0=-1), dict(scales=inv[:-1]), dict(yp=None), dict(out_y=None),
                dict(out_x=dw_x.cpu()), dict(out_y=dw_y.cpu()), dict(scales=inv.cpu()),
                dict(d=d_pk.cpu()), dict(xp=x_pk.cpu()), dict(yp=y_pk.cpu()),
                dict(d=d_pk[:-1], parts=2)):
        with pytest.raises(err):
            gemm(**bad)
    assert bool((dw_x == 5.0).all()) and bool((dw_y == 6.0).all())
    gemm()                                                              # (and the full call runs)
    assert float(dw_x[0, 0]) == 45.0 and float(dw_y[19, 16]) == 46.0
    # the data gradient
    steps, batch, n = 2, 3, 17
    ws = hip.rnn_workspace('lstm', steps, batch, H, DEV)
    packed = torch.zeros(hip.dgrad16_packed_bytes(n), dtype=torch.uint8, device=DEV)
    dx = torch.full((steps * batch, n), 7.0, device=DEV)
    x_off, s_off = hip.dgrad16_published_offsets(steps, batch, H)
    end = max(x_off + 3 * 2 * batch * 4 * H * 4, s_off + steps * 2 * 64 * 32 * 4)
    assert ws.numel() >= end
    for bad in (dict(packed=packed[:-1]), dict(workspace=ws[:end - 1]), dict(steps=(1, 1)),
                dict(steps=(2, 1)), dict(steps=(0, 3)), dict(steps=(-1, 1)), dict(dirs=(1, 1)),
                dict(dirs=(2, 0)), dict(dirs=(0, 3)), dict(packed=packed.cpu())):
        args = dict(workspace=ws, packed=packed, steps=None, dirs=(0, 2))
        args.update(bad)
        with pytest.raises(err):
            hip.dgrad16_blockscaled(args['workspace'], steps, batch, H, args['packed'], W_SCALE, n,
                                    out=dx, steps=args['steps'], dirs=args['dirs'])
    assert bool((dx == 7.0).all())
    hip.dgrad16_blockscaled(ws[:end], steps, batch, H, packed, W_SCALE, n, out=dx)
    assert bool((dx == 0.0).all())
    # the NT split GEMM wants 16-byte aligned operands and leading dimensions of whole float4s
    a = torch.ones(8, 36, device=DEV)
    b = torch.ones(8, 36, device=DEV)
    hip.gemm_split_nt(a[:, :32], b[:, 4:36])
    with pytest.raises(err):
        hip.gemm_split_nt(a[:, 1:33], b[:, :32])                        # misaligned a
    with pytest.raises(err):
        hip.gemm_split_nt(a[:, :32], b[:, 2:34])                        # misaligned b
    a = torch.ones(8, 34, device=DEV)
    with pytest.raises(err):
        hip.gemm_split_nt(a[:, :32], b[:, :32])                         # lda % 4
    with pytest.raises(err):
        hip.gemm_split_nt(b[:, :32], a[:, :32])                         # ldb % 4
