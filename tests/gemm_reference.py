"""Host references for the own MFMA GEMM kernels (csrc/split_gemm.hip, csrc/wgrad16.hip,
csrc/dgrad16.hip): plain numpy (torch only for `publish`, the restatement of what the backward
recurrence leaves in its workspace), nothing from the package under test.

Three things live here:

* the LAYOUTS of the packed operands, written from the layout comments of the kernels, with their
  inverses: `wgrad16_pack_reference` / `wgrad16_unpack`, `dgrad16_pack_reference` /
  `dgrad16_unpack`, `publish_blocks` / `publish`;
* an emulation of one 16 x 16 x 32 MFMA from two fragments (`mfma_16x16x32`) and the two products
  built from it the way the kernels walk their packed operands (`wgrad16_emulated`,
  `dgrad16_emulated`): they pin the layout restatement without a GPU;
* DATA ON WHICH THE KERNELS ARE EXACT.  Every operand value is an integer multiple of a power of
  two (its granule) with so few significant bits that each fp16 / bf16 piece holds it exactly,
  every dropped piece product is exactly zero, and `exact_product` hands out the float64 product
  only after it has checked that sum_k |a_k| |b_k|, in units of the product's granule, stays
  below 2^24 for every output: every partial sum in any order of addition is then an fp32 number,
  and a kernel has to give the float64 product bit for bit.  `distinct` asserts that no two rows
  and no two columns of an expectation are equal, so that a misplaced tile, row or column cannot
  pass.

The fp16 two-piece form: a scaled value +-(a * 2^11 + b) with a in 4 .. 7 and b in 1 .. 3 lies
in [2^13, 2^14), where fp16 steps by 8: h1 = +-a * 2^11 and h2 = +-b.  The bf16 forms:
+-(h * 2^8 + l) (h in 4 .. 7, l in 1 .. 3: two pieces) and +-(h * 2^17 + m * 2^8 + l) (m in
4 .. 7 too: three)."""

import numpy as np
import torch

from tests import elementwise_reference as ew

H = 1024                                    # hidden units of the block-scaled data gradient
PACK_BOUND = 60000.0                        # the packs clamp scaled values to +-60000
LIMIT = float(2 ** 24)


class InexactData(AssertionError):
    """The operands do not meet the precondition under which fp32 accumulation is exact."""


# ------------------------------------------------------------------------------- arithmetic
def clamp_keep_nan(v, bound=PACK_BOUND):
    """min(max(v, -bound), bound): infinities saturate, a NaN stays a NaN (numpy's minimum and
    maximum propagate it)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return np.minimum(np.maximum(v, np.float32(-bound)), np.float32(bound))


def f16_split2(v):
    """(h1, h2) float16: h1 = rne(v), h2 = rne(v - h1) of float32 values."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        h1 = v.astype(np.float16)
        h2 = (v - h1.astype(np.float32)).astype(np.float16)
    return h1, h2


def exact_product(a, b, ga=1.0, gb=1.0):
    """float64 a [M, K] @ b [K, N] of operands on which fp32 accumulation in any order is exact,
    or `InexactData`.  ``ga`` / ``gb`` (scalars or [K]): column k of a holds integer multiples of
    ga[k], row k of b of gb[k]; the product's granule is the smallest ga[k] gb[k] of a k that is
    used.  Precondition: for every output sum_k |a_k| |b_k| < 2^24 granules."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    k = a.shape[1]
    ga = np.broadcast_to(np.asarray(ga, dtype=np.float64), (k,))
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), (k,))
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise InexactData('non-finite operand')
    if not (np.array_equal(a / ga, np.rint(a / ga)) and
            np.array_equal(b / gb[:, None], np.rint(b / gb[:, None]))):
        raise InexactData('an operand is no integer multiple of its granule')
    used = (np.abs(a).max(axis=0) > 0) & (np.abs(b).max(axis=1) > 0)
    if not used.any():
        return a @ b
    granule = float((ga * gb)[used].min())
    bound = float((np.abs(a) @ np.abs(b)).max())
    if not bound < LIMIT * granule:
        raise InexactData('sum |a| |b| reaches {:.4g} granules, 2^24 allowed'
                          .format(bound / granule))
    return a @ b


def distinct(ref):
    """Assert that no two rows and no two columns of an expectation are equal; returns it."""
    ref = np.asarray(ref)
    assert len(np.unique(ref, axis=0)) == ref.shape[0], 'two equal rows in the expectation'
    assert len(np.unique(ref, axis=1).T) == ref.shape[1], 'two equal columns in the expectation'
    return ref


# ------------------------------------------------------------------------------- generators
def _nonzero_ints(rng, shape, top):
    """Integers in [-top, top] without 0."""
    v = rng.integers(1, top + 1, size=shape)
    return (v * rng.choice([-1, 1], size=shape)).astype(np.float64)


def f16_two_piece(rng, shape):
    """Scaled values a * 2^11 + b, |a| in 4 .. 7, 1 <= |b| <= 3 with a's sign (the magnitude
    stays inside [2^13, 2^14)): h1 = a * 2^11, h2 = b != 0."""
    sign = rng.choice([-1.0, 1.0], size=shape)
    return sign * (rng.integers(4, 8, size=shape) * 2048.0 + rng.integers(1, 4, size=shape))


def f16_one_piece(rng, shape, top=3):
    """Scaled values j * 2^11, 1 <= |j| <= top: one piece, h2 = 0."""
    return _nonzero_ints(rng, shape, top) * 2048.0


def f16_pair_columns(rng, rows, count, kind):
    """[rows, count] scaled columns of the first (``kind`` 'd') or of a second operand ('x') of
    the fp16 two-piece kernels: on even rows d is two-piece and x one-piece (|j| <= 3), on odd
    rows d is one-piece (|j| <= 7) and x two-piece."""
    out = np.empty((rows, count))
    two, one = (out[0::2], out[1::2]) if kind == 'd' else (out[1::2], out[0::2])
    two[...] = f16_two_piece(rng, two.shape)
    one[...] = f16_one_piece(rng, one.shape, 7 if kind == 'd' else 3)
    return out


def f16_pair_case(rows, m, n, seed):
    """Scaled operands (ds [rows, m], xs [rows, n]) of the fp16 two-piece kernels that need each of
    the three products d1 x1, d1 x2 and d2 x1 for EVERY output (of two rows or more) and make the
    dropped d2 x2 exactly zero: `f16_pair_columns`.  Both are integers; the product's granule is
    2^11."""
    rng = np.random.default_rng(seed)
    return f16_pair_columns(rng, rows, m, 'd'), f16_pair_columns(rng, rows, n, 'x')


def repeated(ref, axis):
    """Indices along ``axis`` of the rows (0) / columns (1) that repeat an earlier one."""
    ref = np.asarray(ref)
    _, first = np.unique(ref, axis=axis, return_index=True)
    return np.setdiff1d(np.arange(ref.shape[axis]), first)


def f16_pair_granules(rows):
    """(granules of ds, granules of xs) per row of `f16_pair_case`, for `exact_product`."""
    even = np.arange(rows) % 2 == 0
    return np.where(even, 1.0, 2048.0), np.where(even, 2048.0, 1.0)


def f16_pair_product(ds, xs):
    """Checked float64 ds^T xs of an `f16_pair_case` (any rows of it may have been zeroed)."""
    return exact_product(ds.T, xs, *f16_pair_granules(ds.shape[0]))


def bf16_one_piece(rng, shape, top=127):
    """Non-zero integers of at most 7 bits: one bf16 piece."""
    return _nonzero_ints(rng, shape, top)


def bf16_two_piece(rng, shape):
    """+-(h * 2^8 + l), h in 4 .. 7, l in 1 .. 3: p1 = +-h * 2^8, p2 = +-l, p3 = 0."""
    sign = rng.choice([-1.0, 1.0], size=shape)
    return sign * (rng.integers(4, 8, size=shape) * 256.0 + rng.integers(1, 4, size=shape))


def bf16_three_piece(rng, shape):
    """+-(h * 2^17 + m * 2^8 + l), h, m in 4 .. 7, l in 1 .. 3: three non-zero pieces."""
    sign = rng.choice([-1.0, 1.0], size=shape)
    return sign * (rng.integers(4, 8, size=shape) * 131072.0 +
                   rng.integers(4, 8, size=shape) * 256.0 + rng.integers(1, 4, size=shape))


def bf16_pieces(v):
    """float64 (p1, p2, p3) of float32 values, by `elementwise_reference.bf16_split3`."""
    return tuple(ew.bf16_value(bits) for bits in ew.bf16_split3(np.asarray(v, dtype=np.float32)))


def bf16_piece_case(m, n, k, seed):
    """(a [M, K], b [K, N]) that need each of the six products the bf16 kernel forms
    (a1 b1, a1 b2, a2 b1, a1 b3, a2 b2, a3 b1) and make every dropped one exactly zero.  Five k
    are used, spread over the K steps (the rest of K is zero): two with a three-piece a against a
    power of two in b, two the other way round, one with two-piece values on both sides."""
    rng = np.random.default_rng(seed)
    a, b = np.zeros((m, k)), np.zeros((k, n))
    ks = sorted(set(int(round(f * (k - 1))) for f in (0.0, 0.3, 0.5, 0.8, 1.0)))
    assert len(ks) == 5, 'K too small for the five piece pairings'
    pow2 = lambda shape: rng.choice([-2.0, -1.0, 1.0, 2.0], size=shape)
    for which, kk in zip((0, 1, 2, 0, 1), ks):
        if which == 0:
            a[:, kk], b[kk] = bf16_three_piece(rng, m), pow2(n)
        elif which == 1:
            a[:, kk], b[kk] = pow2(m), bf16_three_piece(rng, n)
        else:
            a[:, kk], b[kk] = bf16_two_piece(rng, m), bf16_two_piece(rng, n)
    # the pieces are what the construction says, and the dropped products vanish
    pa, pb = bf16_pieces(a), bf16_pieces(b)
    for i, j in ((1, 2), (2, 1), (2, 2)):
        assert not (np.abs(pa[i]) @ np.abs(pb[j])).any()
    for i, j in ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)):
        assert (np.abs(pa[i]) @ np.abs(pb[j])).all(), (i, j)
    return a, b


def int_case(m, n, k, seed):
    """Non-zero integer operands (a [M, K], b [K, N]) of one bf16 piece each whose product has
    no two equal rows or columns by construction.  K >= 4: four k carry f(i) + g(j) (a[i] = (i %
    128 + 1, i // 128 + 1, 1, 128) against b[:, j] = (1, 128, j % 128 + 1, j // 128 + 1): f(i) =
    i + 129, below 2^13 for up to 32640 rows), the other k hold random a in +-1 .. 7 against
    random +-1 .. 3 times 2^13, which fill the bits above.  K < 4: random, k = 0 without
    repetition (at most 510 rows / columns)."""
    rng = np.random.default_rng(seed)
    if k < 4:
        assert max(m, n) <= 510
        a, b = _nonzero_ints(rng, (m, k), 255), _nonzero_ints(rng, (k, n), 255)
        pool = np.concatenate([np.arange(-255.0, 0.0), np.arange(1.0, 256.0)])
        a[:, 0], b[0] = rng.permutation(pool)[:m], rng.permutation(pool)[:n]
        return a, b
    assert max(m, n) <= 32640
    a, b = _nonzero_ints(rng, (m, k), 7), _nonzero_ints(rng, (k, n), 3) * 8192.0
    i, j = np.arange(m), np.arange(n)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = i % 128 + 1, i // 128 + 1, 1, 128
    b[0], b[1], b[2], b[3] = 1, 128, j % 128 + 1, j // 128 + 1
    return a, b


def tile_order_maps(tiles_m, tiles_n):
    """The tile each workgroup of `split_gemm_kernel` / `dgrad16_bs_kernel` takes, restated:
    list of (tm, tn) or None (idle) by blockIdx, grid padded to a multiple of 8."""
    tiles = tiles_m * tiles_n
    per_xcd = (tiles + 7) // 8
    out = []
    for block in range(8 * per_xcd):
        v = (block & 7) * per_xcd + (block >> 3)
        if v >= tiles:
            out.append(None)
            continue
        group, within = divmod(v, 4 * tiles_n)
        rows_here = min(4, tiles_m - group * 4)
        out.append((group * 4 + within % rows_here, within // rows_here))
    return out


def wgrad16_tile_order(tiles_m, tiles_n0, tiles_n1):
    """`wgrad16_kernel`'s tile list restated: [(which, tm, tn, blocked)] by tile id."""
    out = []
    for which, tiles_n in ((0, tiles_n0), (1, tiles_n1)):
        count = tiles_m * tiles_n
        blocked = (tiles_m % 4 == 0 and tiles_n % 4 == 0 and count % 8 == 0 and
                   (tiles_m * tiles_n0) % 8 == 0) and count > 0
        for v in range(count):
            if blocked:
                pos = (v % 8) * (count // 8) + v // 8
                block, in_block = divmod(pos, 16)
                blocks_n = tiles_n // 4
                out.append((which, (block // blocks_n) * 4 + in_block // 4,
                            (block % blocks_n) * 4 + in_block % 4, True))
            else:
                out.append((which, v // tiles_n, v % tiles_n, False))
    return out


# --------------------------------------------------------------------- wgrad16: packed layout
def wgrad16_packed_bytes(stages, cols):
    return stages * ((cols + 15) // 16) * 2048


def wgrad16_scaled(x, rows_total, row0, stages, col_scale, scale):
    """float32 [32 * stages, 16 * col_tiles]: what `wgrad16_pack` splits - rows [row0, row0 + 32
    stages) of x (zeros outside [0, rows_total)), x * (col_scale[c] * scale), zero columns up to
    the column tile, clamped to +-60000 (NaN kept)."""
    x = np.asarray(x, dtype=np.float32)
    cols = x.shape[1]
    col_tiles = (cols + 15) // 16
    cs = np.ones(cols, dtype=np.float32) if col_scale is None \
        else np.asarray(col_scale, dtype=np.float32)
    cs = cs * np.float32(scale)
    v = np.zeros((32 * stages, 16 * col_tiles), dtype=np.float32)
    lo, hi = max(row0, 0), min(row0 + 32 * stages, rows_total)
    if hi > lo:
        with np.errstate(over='ignore', invalid='ignore'):
            v[lo - row0:hi - row0, :cols] = x[lo:hi] * cs
    return clamp_keep_nan(v)


def wgrad16_layout(h1, h2):
    """Pieces float16 [32 * stages, 16 * col_tiles] -> packed uint8
    [stage][column tile][piece][lane][16 B], lane l = (rows 8 (l >> 4) .. + 7, column l & 15)."""
    rows, cols = h1.shape
    stages, col_tiles = rows // 32, cols // 16
    both = np.stack([h1, h2]).view(np.uint16).reshape(2, stages, 4, 8, col_tiles, 16)
    # (piece, stage, k group, e, column tile, column) -> (stage, column tile, piece, k group, column, e)
    return np.ascontiguousarray(both.transpose(1, 4, 0, 2, 5, 3)).reshape(-1).view(np.uint8)


def wgrad16_pack_reference(x, rows_total, row0, stages, col_scale, scale):
    """The bytes `ctcasr_wgrad16_pack` writes."""
    return wgrad16_layout(*f16_split2(wgrad16_scaled(x, rows_total, row0, stages, col_scale, scale)))


def wgrad16_unpack(packed, stages, cols):
    """Packed bytes -> (h1, h2) float16 [32 * stages, 16 * col_tiles]."""
    col_tiles = (cols + 15) // 16
    both = np.asarray(packed).view(np.uint16).reshape(stages, col_tiles, 2, 4, 16, 8)
    both = np.ascontiguousarray(both.transpose(2, 0, 3, 5, 1, 4)).reshape(
        2, 32 * stages, 16 * col_tiles)
    return both[0].view(np.float16), both[1].view(np.float16)


# --------------------------------------------------------------------- dgrad16: packed weights
DG_STAGES = 2 * (H // 16) * 2               # (dir, producer P, half m)


def dgrad16_packed_bytes(n):
    return DG_STAGES * ((n + 15) // 16) * 2048


def dgrad16_layout(h1, h2):
    """Pieces float16 [2 * 4H, 16 * column tiles] (row = dir * 4H + gate * H + unit) -> packed
    uint8 [stage = (dir, P, m)][column tile][piece][lane = (q, column)][e]: unit 16 P + 8 m + 2 q
    + (e >> 2), gate e & 3."""
    nt = h1.shape[1] // 16
    both = np.stack([h1, h2]).view(np.uint16).reshape(2, 2, 4, H // 16, 2, 4, 2, nt, 16)
    # (piece, dir, gate, P, m, q, u1, tile, col) -> (dir, P, m, tile, piece, q, col, u1, gate)
    return np.ascontiguousarray(both.transpose(1, 3, 4, 7, 0, 5, 8, 6, 2)).reshape(-1).view(np.uint8)


def dgrad16_scaled(w, scale):
    w = np.asarray(w, dtype=np.float32)
    n = w.shape[1]
    v = np.zeros((8 * H, 16 * ((n + 15) // 16)), dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        v[:, :n] = w * np.float32(scale)
    return clamp_keep_nan(v)


def dgrad16_pack_reference(w, scale):
    """The bytes `ctcasr_dgrad16_pack_weights` writes for w [2 * 4H, n]."""
    return dgrad16_layout(*f16_split2(dgrad16_scaled(w, scale)))


def dgrad16_unpack(packed, n):
    """Packed bytes -> (h1, h2) float16 [2 * 4H, 16 * column tiles]."""
    nt = (n + 15) // 16
    both = np.asarray(packed).view(np.uint16).reshape(2, H // 16, 2, nt, 2, 4, 16, 2, 4)
    both = np.ascontiguousarray(both.transpose(4, 0, 8, 1, 2, 5, 7, 3, 6)).reshape(2, 8 * H, 16 * nt)
    return both[0].view(np.float16), both[1].view(np.float16)


# ------------------------------------------------------------------ dgrad16: published operand
def publish_blocks(dxw):
    """dxw [T, B, 2, 4H] (torch, any device) the way prnn_bwd16_kernel publishes its dgates
    (rnn_persistent.hip): per (step, dir, producer = 16 units x 4 gates) and row the power of two
    that puts the row's largest of the 64 values into [2^13, 2^14), two fp16 pieces,
    [step][dir][P][half m][piece][k group q][b][e = 4 (unit & 1) + gate]; inverse scales
    [step][dir][P][32 rows] (zero for the rows past B).  Step s = time s (dir 0) / T - 1 - s
    (dir 1).  Returns (pieces fp16 [T, 2, 64, 2, 2, 4, B, 2, 4], inverse scales f32 [T, 2, 64, 32])."""
    steps, batch = dxw.shape[:2]
    # (t, b, dir, gate, P, m, q, u1): unit = 16 P + 8 m + 2 q + u1
    d = dxw.view(steps, batch, 2, 4, 64, 2, 4, 2)
    top = d.abs().amax(dim=(3, 5, 6, 7))                          # (t, b, dir, P)
    expo = (torch.frexp(top)[1] - 1).float()                     # floor(log2(top)), exactly
    expo = torch.where(top > 0, (13 - expo).clamp(-100, 100), torch.zeros_like(expo))
    scale = torch.exp2(expo)
    scaled = d * scale.view(steps, batch, 2, 1, 64, 1, 1, 1)
    h1 = scaled.half()
    h2 = (scaled - h1.float()).half()
    pieces = torch.stack([h1, h2], dim=0)                         # (piece, t, b, dir, gate, P, m, q, u1)
    # -> (t, dir, P, m, piece, q, b, u1, gate)
    pieces = pieces.permute(1, 3, 5, 6, 0, 7, 2, 8, 4).contiguous()
    pieces[:, 1] = pieces[:, 1].flip(0)                           # dir 1: step s = T - 1 - t
    inv = torch.zeros(steps, 2, 64, 32, device=dxw.device)
    inv[..., :batch] = (1.0 / scale).permute(0, 2, 3, 1)
    inv[:, 1] = inv[:, 1].flip(0)
    return pieces, inv


def publish(hip, dxw, workspace=None):
    """`publish_blocks` of dxw written into a recurrence workspace (a fresh one by default) at the
    offsets the library reports."""
    steps, batch = dxw.shape[:2]
    if workspace is None:
        workspace = hip.rnn_workspace('lstm', steps, batch, H, dxw.device)
    x_off, s_off = hip.dgrad16_published_offsets(steps, batch, H)
    pieces, inv = publish_blocks(dxw)
    block = 2 * batch * 4 * H * 4                                 # bytes per step
    workspace[x_off + block:x_off + block * (steps + 1)] = pieces.view(torch.uint8).view(-1)
    workspace[s_off:s_off + inv.numel() * 4] = inv.view(torch.uint8).view(-1)
    return workspace


# ----------------------------------------------------------------------------- MFMA emulation
def mfma_16x16x32(a_frag, b_frag):
    """float64 D [16, 16] of v_mfma_f32_16x16x32_f16 from its operand registers: lane l of A
    holds row l & 15, k = 8 (l >> 4) .. + 7; lane l of B column l & 15, the same k.  ``a_frag``,
    ``b_frag``: [64 lanes, 8 halves]."""
    a = np.asarray(a_frag, dtype=np.float64).reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)
    b = np.asarray(b_frag, dtype=np.float64).reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)
    return a @ b.T


def _three_products(a1, a2, b1, b2):
    return mfma_16x16x32(a1, b1) + mfma_16x16x32(a1, b2) + mfma_16x16x32(a2, b1)


def wgrad16_emulated(d_packed, m, stages, inv_scale, x_packed, x_stage0, n, x_scale):
    """float64 dW [m, n] as `wgrad16_kernel` forms it: per stage, row tile and column tile the
    1 KB chunks of both packed buffers as MFMA fragments, three piece products, times
    inv_scale[m] / x_scale."""
    frag = lambda buf: np.asarray(buf).view(np.float16).reshape(-1, 2, 64, 8)
    mt, nt = (m + 15) // 16, (n + 15) // 16
    d, x = frag(d_packed), frag(x_packed)
    out = np.zeros((16 * mt, 16 * nt))
    for s in range(stages):
        for i in range(mt):
            dc = d[s * mt + i]
            for j in range(nt):
                xc = x[(x_stage0 + s) * nt + j]
                out[16 * i:16 * i + 16, 16 * j:16 * j + 16] += _three_products(dc[0], dc[1],
                                                                               xc[0], xc[1])
    return out[:m, :n] * np.asarray(inv_scale, dtype=np.float64)[:, None] / x_scale


def dgrad16_emulated(pieces, inv, w_packed, n, scale):
    """float64 dx [T * B, n] as `dgrad16_bs_kernel` forms it from `publish_blocks`' output and
    packed weights: per (step, dir, P, m) and 16-row unit a fresh 16 x 16 x 32 product that enters
    the total times the row's inverse scale."""
    pieces = pieces.cpu().numpy().astype(np.float64)      # [T, 2, 64, 2, piece, q, B, 2, 4]
    inv = inv.cpu().numpy().astype(np.float64)            # [T, 2, 64, 32]
    steps, batch = pieces.shape[0], pieces.shape[6]
    nt = (n + 15) // 16
    w = np.asarray(w_packed).view(np.float16).reshape(2, 64, 2, nt, 2, 64, 8)
    out = np.zeros((steps, batch, 16 * nt))
    for t in range(steps):
        for d in range(2):
            s = t if d == 0 else steps - 1 - t
            for p in range(64):
                if not pieces[s, d, p].any():
                    continue
                for half in range(2):
                    for b0 in range(0, batch, 16):
                        rows = min(16, batch - b0)
                        a = np.zeros((2, 4, 16, 8))
                        a[:, :, :rows] = pieces[s, d, p, half, :, :, b0:b0 + rows].reshape(
                            2, 4, rows, 8)
                        a = a.reshape(2, 64, 8)
                        for j in range(nt):
                            wc = w[d, p, half, j]
                            fresh = _three_products(a[0], a[1], wc[0], wc[1])
                            out[t, b0:b0 + rows, 16 * j:16 * j + 16] += \
                                fresh[:rows] * inv[s, d, p, b0:b0 + rows, None]
    return out.reshape(steps * batch, 16 * nt)[:, :n] / scale
