"""`ctcasr_grad_norm` where it can go wrong first: lengths around the float4 and the chunk seams,
empty segments in every place, a last segment that is no multiple of 4, the segment limit, a
vector long enough for the grid to stride, values whose squares leave float32 on either side,
NaN and inf, the clip factor on both sides of the threshold, the guard word, and the invariances
the pinned summation order promises.

Tolerances: none measured.  Every finite norm is within ONE float32 ulp of
float32(grad_scale * sqrt(fsum(x^2))) - the float64 sum is off by orders less, the ulp allows for
the double rounding - and equals, bit for bit, the host reference that adds in the pinned order
(tests/gradnorm_reference.py).  The clip factor equals numpy's float32 division of the norm the
kernel returned, bit for bit."""

import numpy as np
import pytest
import torch

from tests import gradnorm_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CHUNK = ref.CHUNK
BIG = (1 << 24) + 5         # 2049 chunks: more than the 2048 workgroups of the reading launch


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _offsets(table):
    return torch.tensor(table, dtype=torch.int64, device=DEV)


def _run(hip, x, table, scale=1.0, max_norm=0.0, skip=None):
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    norms, factor = hip.grad_norm(x, _offsets(table), scale, max_norm, skip=skip)
    assert norms.numel() == len(table) and factor.numel() == 1
    return norms.cpu().numpy(), factor.cpu().numpy()[0]


def _check(hip, x, table, scale=1.0):
    """Run, and compare with both yardsticks; returns the norms."""
    got, factor = _run(hip, x, table, scale)
    want = ref.exact_norms(x, table, scale)
    assert np.isfinite(got).all()
    assert ref.ulps32(got, want).max() <= 1, (table, got, want)
    pinned, _ = ref.grad_norm(x, table, scale)
    assert np.array_equal(_bits(got), _bits(pinned)), (table, got, pinned)
    assert _bits(factor) == _bits(1.0)
    return got


def _mixed(rng, n):
    x = rng.normal(size=n).astype(np.float32)
    x[1::5] = 0.0
    x[2::97] = 1e-30
    x[rng.integers(0, n, size=min(3, n))] = 3e19
    return x


def _tables(n):
    """One segment, two, and the limit - the last with empty segments first, in the middle and
    last, and (small n) all but one empty; the final segment keeps whatever n % 4 leaves."""
    half = (n // 2) & ~3
    rng = np.random.default_rng(n)
    inner = np.sort(rng.integers(0, n // 4 + 1, size=ref.MAX_SEGMENTS - 1)) * 4
    inner[:2], inner[30:33], inner[-2:] = 0, inner[30], inner[-3]
    full = [0] + [int(v) for v in np.sort(inner)] + [n]
    return [[0, n], [0, half, n], full]


SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]


@pytest.mark.parametrize('n', SIZES)
def test_norms_at_the_seams(hip, n):
    rng = np.random.default_rng(100 + n)
    x = rng.normal(size=n).astype(np.float32)
    for table in _tables(n):
        assert len(table) - 1 in (1, 2, hip.GRAD_NORM_MAX_SEGMENTS)
        got = _check(hip, x, table)
        for s, (a, b) in enumerate(zip(table[:-1], table[1:])):
            assert a != b or got[s] == 0.0
    _check(hip, _mixed(rng, n), [0, (n // 2) & ~3, n], 1.0 / 8)


def test_empty_segments_everywhere(hip):
    n = CHUNK + 7
    x = np.random.default_rng(2).normal(size=n).astype(np.float32)
    m = CHUNK + 4       # an empty LAST segment starts at the end: an interior offset, so 4 | m
    for table in ([0, 0, 0, n], [0, 8, 8, 8, n], [0, 8, m, m, m], [0, 0, m, m], [0, 0, 0, 0, 0, n],
                  [0, CHUNK, CHUNK, n], [0, n - 3, n]):
        got = _check(hip, x[:table[-1]], table)
        empty = [a == b for a, b in zip(table[:-1], table[1:])]
        assert all(got[s] == 0.0 for s, e in enumerate(empty) if e)
        assert all(got[s] > 0.0 for s, e in enumerate(empty) if not e)
    # nothing at all
    norms, factor = _run(hip, torch.empty(0, device=DEV), [0, 0, 0], max_norm=1.0)
    assert not norms.any() and _bits(factor) == _bits(1.0)


@pytest.fixture(scope='module')
def big():
    """2^24 + 5 values and their exactly rounded norms, computed once: (host values, device
    values, table, exact norms)."""
    x = _mixed(np.random.default_rng(24), BIG)
    table = [0, 4 * 1000003, 700 * CHUNK + 4, BIG]
    return x, torch.from_numpy(x).to(DEV), table, ref.exact_norms(x, table)


def test_the_grid_strides_and_its_size_does_not_matter(hip, big):
    x, dev, table, want = big
    assert -(-BIG // CHUNK) > 2048
    try:
        for layout in (table, [0, BIG]):
            runs = []
            for blocks in (0, 1, 3, 65536):
                hip.set_option('grad_norm_blocks', blocks)
                runs.append(_run(hip, dev, layout, max_norm=1.0))
            got, factor = runs[0]
            exact = want if layout is table else want[-1:].repeat(2)
            assert np.isfinite(got).all() and ref.ulps32(got, exact).max() <= 1, (got, exact)
            assert _bits(factor) == _bits(np.float32(1.0) / got[-1])
            for other, other_factor in runs[1:]:
                assert np.array_equal(_bits(other), _bits(got))
                assert _bits(other_factor) == _bits(factor)
            assert np.array_equal(_bits(got), _bits(ref.grad_norm(x, layout)[0]))
    finally:
        hip.set_option('grad_norm_blocks', 0)
    with pytest.raises(hip.CtcAsrError):
        hip.set_option('grad_norm_blocks', -1)


def test_zeros_small_and_huge_values(hip):
    n = 2 * CHUNK + 3
    norms, factor = _run(hip, np.zeros(n, dtype=np.float32), [0, 8, n], max_norm=1.0)
    assert np.array_equal(_bits(norms), _bits(np.zeros(3))) and _bits(factor) == _bits(1.0)
    rng = np.random.default_rng(5)
    x = _mixed(rng, n)
    x[5] = 3e19
    x[CHUNK:CHUNK + 64] = 0.0
    x[CHUNK:CHUNK + 64:4] = 1e-30                    # a segment of nothing but 1e-30 and zeros
    got = _check(hip, x, [0, CHUNK, CHUNK + 64, n])
    assert got[1] == np.float32(4e-30)              # 16 x 1e-60 in float64; float32 squares are 0
    assert got[3] > 3e19                            # 9e38 does not fit a float32 square


@pytest.mark.parametrize('poison', [float('nan'), float('inf'), float('-inf')])
def test_a_non_finite_value_poisons_its_segment_and_the_total_only(hip, poison):
    n = 2 * CHUNK + 3
    table = [0, 64, CHUNK + 64, n]
    x = np.random.default_rng(6).normal(size=n).astype(np.float32)
    clean, _ = _run(hip, x, table)
    x[64 + 4097] = poison
    skip = torch.tensor([0, 7], dtype=torch.int32, device=DEV)
    for max_norm in (0.0, 1.0):
        got, factor = _run(hip, x, table, max_norm=max_norm, skip=skip)
        assert np.array_equal(_bits(got[[0, 2]]), _bits(clean[[0, 2]]))
        if poison != poison:
            assert np.isnan(got[1]) and np.isnan(got[3])
        else:
            assert np.isposinf(got[1]) and np.isposinf(got[3])
        assert _bits(factor) == _bits(0.0)
        assert skip.tolist() == [1, 7]
    got, factor = _run(hip, x, table, max_norm=1.0, skip=None)       # no guard word: accepted
    assert _bits(factor) == _bits(0.0)


def test_a_finite_norm_leaves_the_guard_word_alone(hip):
    x = np.random.default_rng(8).normal(size=300).astype(np.float32)
    for words in ([0, 5], [1, 5], [-3, 0]):
        skip = torch.tensor(words, dtype=torch.int32, device=DEV)
        _, factor = _run(hip, x, [0, 300], max_norm=1.0, skip=skip)
        assert skip.tolist() == words and 0.0 < factor < 1.0
    # a norm that overflows float32 is not finite either
    skip = torch.zeros(2, dtype=torch.int32, device=DEV)
    norms, factor = _run(hip, np.full(1024, 3e38, dtype=np.float32), [0, 1024], skip=skip)
    assert np.isposinf(norms).all() and factor == 0.0 and skip.tolist() == [1, 0]


def test_the_clip_factor_on_both_sides_of_the_threshold(hip):
    x = np.random.default_rng(9).normal(size=CHUNK + 5).astype(np.float32)
    table = [0, 1024, CHUNK + 5]
    norms, factor = _run(hip, x, table)
    g = np.float32(norms[-1])
    assert _bits(factor) == _bits(1.0)
    one = _bits(1.0)
    for max_norm in (float(g), float(np.nextafter(g, np.float32(np.inf))), 0.0, -1.0, 1e30):
        again, factor = _run(hip, x, table, max_norm=max_norm)
        assert _bits(factor) == one, max_norm
        assert np.array_equal(_bits(again), _bits(norms))
    below = np.nextafter(g, np.float32(0))
    for max_norm in (below, np.float32(0.37) * g, np.float32(0.5) * g, np.float32(1e-20)):
        _, factor = _run(hip, x, table, max_norm=float(max_norm))
        assert _bits(factor) == _bits(np.float32(max_norm) / g), max_norm
        assert factor < 1.0
        assert _bits(factor) == _bits(ref.clip_factor(g, max_norm))
    assert _run(hip, x, table, max_norm=float(np.float32(0.5) * g))[1] == 0.5
    # with a scale: the factor divides by the SCALED norm
    scaled, factor = _run(hip, x, table, scale=0.25, max_norm=1.0)
    assert _bits(factor) == _bits(np.float32(1.0) / scaled[-1])


def test_reproducible_position_independent_and_scaled_exactly(hip):
    rng = np.random.default_rng(10)
    seg = _mixed(rng, 2 * CHUNK + 8)
    tail = rng.normal(size=CHUNK + 3).astype(np.float32)
    x = np.concatenate([rng.normal(size=12).astype(np.float32), seg,
                        rng.normal(size=CHUNK + 4).astype(np.float32), tail])
    a, b = 12, 12 + seg.size
    table = [0, a, a, b, x.size - tail.size, x.size]
    first = _run(hip, x, table, max_norm=1.0)
    second = _run(hip, x, table, max_norm=1.0)
    assert np.array_equal(_bits(first[0]), _bits(second[0]))
    assert _bits(first[1]) == _bits(second[1])
    _check(hip, x, table)
    alone = _run(hip, seg, [0, seg.size])[0]
    assert _bits(alone[0]) == _bits(first[0][2]) == _bits(alone[1])
    alone = _run(hip, tail, [0, tail.size])[0]
    assert _bits(alone[0]) == _bits(first[0][4])
    # the same segment among the limit of segments, behind empty ones
    many = [0] * (hip.GRAD_NORM_MAX_SEGMENTS - 2) + [a, b, x.size]
    assert _bits(_run(hip, x, many)[0][-3]) == _bits(first[0][2])
    eighth = _run(hip, x, table, scale=1.0 / 8)[0]
    assert np.array_equal(_bits(eighth), _bits(first[0] * np.float32(0.125)))


def test_out_and_workspace_are_the_callers(hip):
    x = torch.randn(CHUNK + 5, device=DEV)
    table = _offsets([0, 8, CHUNK + 5])
    need = hip.grad_norm_workspace_bytes(x.numel(), 2)
    assert need == (x.numel() // CHUNK + 2) * 8
    out = torch.full((4,), -1.0, device=DEV)
    workspace = torch.empty(need, dtype=torch.uint8, device=DEV)
    norms, factor = hip.grad_norm(x, table, max_norm=1.0, out=out, workspace=workspace)
    assert norms.data_ptr() == out.data_ptr() and factor.data_ptr() == out[3:].data_ptr()
    fresh = hip.grad_norm(x, table, max_norm=1.0)
    assert torch.equal(out[:3], fresh[0]) and torch.equal(out[3:], fresh[1])
    with pytest.raises(hip.CtcAsrError, match='out holds'):
        hip.grad_norm(x, table, out=torch.empty(3, device=DEV))
    with pytest.raises(hip.CtcAsrError, match='workspace holds'):
        hip.grad_norm(x, table, workspace=workspace[:need - 1])


def test_refusals(hip):
    lib = hip.load()
    n = 64
    buf = torch.zeros(n + 4, device=DEV)
    x = buf[:n]
    table = _offsets([0, 32, n])
    out = torch.full((4,), -1.0, device=DEV)
    need = hip.grad_norm_workspace_bytes(n, 2)
    workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)

    def call(grad=x.data_ptr(), count=n, offsets=table.data_ptr(), segments=2,
             norms=out.data_ptr(), factor=out.data_ptr() + 12, ws=workspace.data_ptr(),
             ws_bytes=need):
        return lib.ctcasr_grad_norm(grad, count, offsets, segments, 1.0, 0.0, norms, factor, None,
                                    ws, ws_bytes, None)

    assert call(ws_bytes=need - 1) == -3 and call(ws=None) == -3
    assert call(grad=buf[1:1 + n].data_ptr()) == -1              # a view offset by one float
    assert call(count=-1) == -1 and call(segments=0) == -1 and call(segments=-2) == -1
    assert call(grad=None) == -1 and call(offsets=None) == -1
    assert call(norms=None) == -1 and call(factor=None) == -1
    limit = hip.GRAD_NORM_MAX_SEGMENTS
    assert limit >= 64 and call(segments=limit + 1, ws_bytes=1 << 20) == -2
    assert lib.ctcasr_grad_norm_workspace_bytes(-1, 2) == 0
    assert lib.ctcasr_grad_norm_workspace_bytes(n, 0) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [-1.0] * 4                            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0.0, 0.0, 0.0, 1.0]
    # the wrapper: device, dtype, lengths
    long_table = _offsets([0] * (limit + 1) + [n])
    for bad in (lambda: hip.grad_norm(x.cpu(), table),
                lambda: hip.grad_norm(x, table.cpu()),
                lambda: hip.grad_norm(x, table.to(torch.int32)),
                lambda: hip.grad_norm(x.double(), table),
                lambda: hip.grad_norm(x.half(), table),
                lambda: hip.grad_norm(x, table[:1]),
                lambda: hip.grad_norm(x, long_table),
                lambda: hip.grad_norm(buf[1:1 + n], table),
                lambda: hip.grad_norm(x, table, skip=torch.zeros(2, device=DEV)),
                lambda: hip.grad_norm(x, table, skip=torch.zeros(2, dtype=torch.int32)),
                lambda: hip.grad_norm(x, table, skip=torch.zeros(0, dtype=torch.int32,
                                                                 device=DEV)),
                lambda: hip.grad_norm(x, table, out=torch.zeros(4)),
                lambda: hip.grad_norm(x, table, workspace=torch.zeros(256, device=DEV))):
        with pytest.raises(hip.CtcAsrError):
            bad()


def test_a_table_that_breaks_the_rules_is_clamped_into_the_vector(hip):
    """The kernels never use an offset as it comes: every entry is clamped into [0, n], the table
    made ascending and every entry but the last rounded down to a multiple of 4 before the first
    address is formed, so a descending, misaligned or overshooting table is the same call as its
    clamped form - which is what this compares, bit for bit.  (The values sit in the middle of a
    larger buffer of NaN: a read outside [0, n) would show in a norm.)"""
    n = CHUNK + 50
    buf = torch.full((n + 2 * CHUNK,), float('nan'), device=DEV)
    x = buf[CHUNK:CHUNK + n]
    assert x.data_ptr() % 16 == 0
    x.copy_(torch.from_numpy(np.random.default_rng(11).normal(size=n).astype(np.float32)))
    host = x.cpu().numpy()
    for table in ([0, 100, 40, n], [0, n, 8, 4], [-5, 10 ** 12, 7, n + 100], [3, 7, n],
                  [n, 0], [5 * n, 5 * n, 5 * n], [-(1 << 62), 1 << 62]):
        clamped = ref.sanitize_offsets(table, n)
        assert all(0 <= a <= b <= n for a, b in zip(clamped[:-1], clamped[1:]))
        assert all(v % 4 == 0 for v in clamped[:-1])
        got, _ = _run(hip, x, table)
        same, _ = _run(hip, x, clamped)
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(got), _bits(same)), table
        assert np.array_equal(_bits(got), _bits(ref.grad_norm(host, table)[0])), table
