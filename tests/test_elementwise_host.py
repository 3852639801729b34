"""The host references of tests/elementwise_reference.py, checked on their own (no GPU): what
test_gpu_elementwise_edges.py and test_gpu_split_edges.py hold the kernels against has to be
right first."""

import math

import numpy as np
import pytest

from oracle import nn as onn
from tests import elementwise_reference as ref


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- generator
@pytest.mark.parametrize('seed,rate,n', [(77, 0.25, 100000), (1234, 0.1, 1 << 17),
                                         (0, 0.5, 1 << 22), ((1 << 64) - 1, 0.9, 1 << 22)])
def test_mask_keeps_one_minus_rate(seed, rate, n):
    kept = int(ref.dropout_mask(seed, n, rate).sum())
    sigma = math.sqrt(n * rate * (1.0 - rate))
    deviation = abs(kept - n * (1.0 - rate)) / sigma
    print('seed {} rate {} n {}: {:.2f} binomial standard deviations'.format(
        seed, rate, n, deviation))
    assert deviation < 5.0


def test_uniform01_stays_in_the_half_open_interval():
    for seed in (0, 1, (1 << 64) - 1, 0x9E3779B97F4A7C15):
        u = ref.uniform01(seed, np.arange(1 << 18))
        assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    # indices beyond 2^32 are their own draws, not a wrap of the low word
    lo = ref.uniform01(5, np.arange(64))
    hi = ref.uniform01(5, np.arange(64) + (1 << 32))
    assert not np.array_equal(lo, hi)
    # python integers and arrays agree; the seed is taken modulo 2^64
    assert ref.uniform01(5, 7) == ref.uniform01(5 + (1 << 64), np.array([7]))[0]
    # one value by hand: splitmix64 from state 0 gives 0xE220A8397B1DCDAF first
    assert ref.uniform01(0, 0) == np.float32((0xE220A8397B1DCDAF >> 40) / 16777216.0)


def test_mask_start_offset_is_the_flat_index():
    full = ref.dropout_mask(9, 1000, 0.3)
    assert np.array_equal(ref.dropout_mask(9, 400, 0.3, start=600), full[600:])


# ---------------------------------------------------------------------------- epilogue
def test_epilogue_float32_and_float64_forms_agree():
    rng = np.random.default_rng(0)
    y = (rng.normal(size=(37, 29)) * 8).astype(np.float32)
    bias = rng.normal(size=29).astype(np.float32)
    for rate in (0.0, 0.1, 0.5):
        out, mask = ref.bias_act_fwd_f32(y, bias, 20.0, rate, seed=3)
        wide = ref.bias_act_fwd_f64(y, bias, 20.0, rate, seed=3)
        assert out.dtype == np.float32 and np.abs(out - wide).max() <= 2.0 ** -22 * 40.0
        assert (mask is None) == (rate == 0.0)
        if mask is not None:
            assert np.array_equal(out != 0, mask & (out != 0)) and not out[~mask].any()
        dy = rng.normal(size=y.shape).astype(np.float32)
        dz = ref.bias_act_bwd_f32(out, dy, 20.0, rate)
        wide = ref.bias_act_bwd_f64(out, dy, 20.0, rate)
        assert np.array_equal(dz != 0, wide != 0)
        assert np.abs(dz - wide).max() <= 2.0 ** -23 * np.abs(wide).max()
    # add only: no clip, no dropout, whatever the rate says
    out, mask = ref.bias_act_fwd_f32(y, bias, 0.0, 0.5, seed=3)
    assert mask is None and np.array_equal(out, y + bias)


def test_epilogue_edges():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    y = np.array([[0.0, -0.0, 20.0, np.nextafter(np.float32(20), inf), inf, -inf, nan, -3.0]],
                 dtype=np.float32)
    out, _ = ref.bias_act_fwd_f32(y, None, 20.0)
    assert np.array_equal(out[0, :6], np.array([0, 0, 20, 20, 20, 0], dtype=np.float32))
    assert np.isnan(out[0, 6]) and out[0, 7] == 0
    assert np.isnan(ref.bias_act_fwd_f64(y, None, 20.0)[0, 6])
    assert np.isnan(onn.relu_clip(np.array([np.nan]))[0])          # the project's float64 oracle
    # backward: the window is open on both sides
    upper = np.float32(20.0) * ref.inv_keep_f32(0.5)
    y = np.array([[0.0, np.nextafter(np.float32(0), inf), np.nextafter(upper, -inf), upper]],
                 dtype=np.float32)
    dz = ref.bias_act_bwd_f32(y, np.ones_like(y), 20.0, 0.5)
    assert dz.tolist() == [[0.0, 2.0, 2.0, 0.0]]


# ---------------------------------------------------------------------------- bf16 pieces
def _tie_patterns():
    """float32 bit patterns whose low half decides the rounding of the first bfloat16 piece."""
    out = []
    for sign in (0, 0x80000000):
        for top in (0x3F80, 0x3F81, 0x4049, 0x0080, 0x7F00):       # bit 16 clear / set, edges
            for low in (0x8000, 0x8001, 0x7FFF):
                out.append(sign | (top << 16) | low)
    return np.array(out, dtype=np.uint32)


def test_bf16_split3_rounds_ties_to_even():
    bits = _tie_patterns()
    b1, b2, b3 = ref.bf16_split3(_f32(bits))
    for u, got in zip(bits.tolist(), b1.tolist()):
        top, low = u >> 16, u & 0xFFFF
        if low == 0x8000:
            want = top + (top & 1)              # the tie: up only when that makes bit 16 even
        elif low == 0x8001:
            want = top + 1
        else:
            want = top                          # 0x7FFF: below the half
        assert got == want, (hex(u), hex(got), hex(want))
    # 0x8000 with bit 16 clear rounds down, with it set rounds up: both signs are in the list
    assert ref.bf16_split3(_f32([0x3F808000]))[0][0] == 0x3F80
    assert ref.bf16_split3(_f32([0x3F818000]))[0][0] == 0x3F82
    assert ref.bf16_split3(_f32([0xBF808000]))[0][0] == 0xBF80
    assert ref.bf16_split3(_f32([0xBF818000]))[0][0] == 0xBF82


def test_bf16_split3_pieces_sum_back_exactly():
    rng = np.random.default_rng(1)
    x = (rng.normal(size=4096) * np.logspace(-30, 30, 4096)).astype(np.float32)
    x = np.concatenate([x, _f32(_tie_patterns()), np.array([1.0, -1.0, 65504.0, 3.0e38],
                                                           dtype=np.float32)])
    # (pieces below 2^-133 do not exist in bfloat16: the remainders of the smallest normals are
    # lost, so the claim is for magnitudes well inside the normal range)
    x = x[np.abs(x) > 1e-30]
    b1, b2, b3 = ref.bf16_split3(x)
    total = ref.bf16_value(b1) + ref.bf16_value(b2) + ref.bf16_value(b3)
    assert np.array_equal(total, x.astype(np.float64))
    # a value that is a bfloat16 already has empty second and third pieces
    b1, b2, b3 = ref.bf16_split3(np.array([1.5, -0.0], dtype=np.float32))
    assert b1.tolist() == [0x3FC0, 0x8000] and not (b2 & 0x7FFF).any() and not (b3 & 0x7FFF).any()


# ---------------------------------------------------------------------------- fp16 pieces
def test_f16_split2_ties_and_saturation():
    for k in (-10, 0, 3):
        for sign in (1.0, -1.0):
            x = np.array([2049.0, 2051.0], dtype=np.float32) * np.float32(sign * 2.0 ** k)
            h1, h2 = ref.f16_split2(x, 1.0)
            v1 = h1.view(np.float16).astype(np.float64)
            v2 = h2.view(np.float16).astype(np.float64)
            # 2049 = 2048 + 1 is a tie between 2048 and 2050: even mantissa -> 2048;
            # 2051 is a tie between 2050 and 2052 -> 2052
            assert (v1 / (sign * 2.0 ** k)).tolist() == [2048.0, 2052.0]
            assert (v2 / (sign * 2.0 ** k)).tolist() == [1.0, -1.0]
    x = np.array([65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1e6], dtype=np.float32)
    h1, h2 = ref.f16_split2(x, 1.0, saturate=True)
    assert h1.view(np.float16).tolist() == [65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 65504.0]
    assert not (h2 & 0x7FFF).any()
    h1, _ = ref.f16_split2(x, 1.0)
    # without the clamp 65520 is the first value that rounds to infinity
    assert np.isinf(h1.view(np.float16)).tolist() == [False, False, False, True, True, True]
    # a column scale and a scale multiply in; powers of two are exact
    h1, h2 = ref.f16_split2(np.array([[3.0, 5.0]], dtype=np.float32), 4.0,
                            col_scale=np.array([0.5, 2.0], dtype=np.float32))
    assert h1.view(np.float16).tolist() == [[6.0, 40.0]] and not (h2 & 0x7FFF).any()


# ---------------------------------------------------------------------------- scales
def test_scale_for_max():
    assert ref.scale_for_max(0) == 1.0
    for e in (-126, -20, 0, 5, 13, 100, 127):
        at = _bits(np.float32(2.0 ** e))
        assert ref.scale_for_max(at) == np.float32(2.0 ** min(max(13 - e, -126), 127)), e
        if e < 127:
            below_next = _bits(np.float32(2.0 ** (e + 1))) - 1
            assert ref.scale_for_max(below_next) == ref.scale_for_max(at), e
            top = np.float64(_f32(below_next)) * np.float64(ref.scale_for_max(below_next))
            # (below 2^-114 the clamp at 2^127 binds and the maximum stays smaller)
            assert e < -114 or 2.0 ** 13 <= top < 2.0 ** 14
    assert ref.scale_for_max(1) == np.float32(2.0 ** 127)              # smallest denormal
    assert ref.scale_for_max(0x007FFFFF) == np.float32(2.0 ** 127)     # largest denormal
    assert ref.scale_for_max(0x7F7FFFFF) == np.float32(2.0 ** -114)    # largest finite
    assert np.isfinite(ref.scale_for_max(0x7F800000))                  # the pattern of inf
    got = ref.scale_for_max(np.array([0, 0x3F800000, 0x7F7FFFFF], dtype=np.int32))
    assert got.dtype == np.float32 and got.tolist() == [1.0, 8192.0, 2.0 ** -114]


# ---------------------------------------------------------------------------- Adam
def test_adam_f32_tracks_the_float64_oracle():
    rng = np.random.default_rng(2)
    n = 4099
    p = rng.normal(size=n).astype(np.float32)
    m = (rng.normal(size=n) * 1e-2).astype(np.float32)
    v = (rng.random(size=n) * 1e-3).astype(np.float32)
    g = rng.normal(size=n).astype(np.float32)
    g[::7], g[1::7], g[2::7] = 0.0, 1e-20, 1e10
    b1, b2, eps, lr = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8, 1e-3))
    for step in (1, 100000):
        for scale in (1.0, 1.0 / 16):
            got = ref.adam_f32(p, g, m, v, step, lr, b1, b2, eps, scale)
            want = onn.adam_step(p.astype(np.float64), g.astype(np.float64) * scale,
                                 m.astype(np.float64), v.astype(np.float64), step, lr, b1, b2, eps)
            # a handful of float32 operations: a few roundings of the terms that are added
            # (the result itself may be small where they cancel), 2^-149 where they underflow
            gs = g.astype(np.float64) * scale
            terms = {'m': np.abs(b1 * m) + np.abs((1.0 - b1) * gs),
                     'v': np.abs(b2 * v) + (1.0 - b2) * gs * gs,
                     'p': np.abs(p) + np.abs(want[0] - p)}
            for name, a, b in zip('pmv', got, want):
                assert a.dtype == np.float32
                err = np.abs(a.astype(np.float64) - b)
                assert (err <= 6 * 2.0 ** -24 * terms[name] + 2.0 ** -148).all(), \
                    (name, step, scale)
