"""Host references for the kernels of csrc/elementwise.hip and csrc/split.hip: plain numpy (torch
on the CPU only for the bfloat16 conversion), nothing from the package under test.

Everything here is defined operation by operation, so that a kernel can be compared bit for bit:

* the dropout generator is the counter-based splitmix64 finaliser over (seed, flat index) that
  elementwise.hip documents, evaluated on uint64 arrays with wrap-around;
* the float32 forms of the epilogue round once per operation in the kernel's order (add the bias,
  clip, multiply by ``float32(1) / (float32(1) - float32(rate))``); the float64 forms are the same
  expressions in double precision;
* the operand splits use round-to-nearest-even conversions and float32 remainders, which are
  exact (each remainder has fewer significant bits than its operand);
* `scale_for_max` is the rule "2^(13 - e), clamped to [2^-126, 2^127], 1 for zero" on the bit
  pattern of the maximum;
* `adam_f32` is the TensorFlow-form update with one float32 rounding per operation.  It is what
  separates "the kernel rounds differently" (FMA contraction, a float32 ``lr_t``) from "the kernel
  is wrong" in the bar of test_gpu_elementwise_edges.py; the float64 oracle stays
  `oracle.nn.adam_step`."""

import math

import numpy as np
import torch

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_MIX1 = np.uint64(0xBF58476D1CE4E5B9)
_MIX2 = np.uint64(0x94D049BB133111EB)
F16_MAX = 65504.0


def uniform01(seed, idx):
    """float32 uniform in [0, 1) for element ``idx`` (any integer array) under ``seed``: the top
    24 bits of splitmix64's finaliser over ``seed + golden * (idx + 1)``, all modulo 2^64."""
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    idx = np.asarray(idx).astype(np.uint64)
    with np.errstate(over='ignore'):
        z = seed + _GOLDEN * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * _MIX1
        z = (z ^ (z >> np.uint64(27))) * _MIX2
        z = z ^ (z >> np.uint64(31))
    # (z >> 40) < 2^24: exact in float32, and so is the product with 2^-24
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def dropout_mask(seed, n, rate, start=0):
    """bool[n]: element ``start + i`` is kept."""
    return uniform01(seed, np.arange(start, start + n, dtype=np.uint64)) >= np.float32(rate)


def inv_keep_f32(rate):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def _relu_clip(v, cutoff):
    # numpy's maximum / minimum propagate NaN, which is what the epilogue has to do
    return np.minimum(np.maximum(v, v.dtype.type(0.0)), v.dtype.type(cutoff))


def bias_act_fwd_f32(y, bias, cutoff, rate=0.0, seed=0):
    """dropout(min(max(y + bias, 0), cutoff)) in float32; ``cutoff <= 0``: the bias add only.
    Returns (out, mask) with mask None where no dropout applies."""
    v = np.asarray(y, dtype=np.float32)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float32)
    mask = None
    if cutoff > 0:
        v = _relu_clip(v, cutoff)
        if rate > 0:
            mask = dropout_mask(seed, v.size, rate).reshape(v.shape)
            v = np.where(mask, v * inv_keep_f32(rate), np.float32(0.0))
    return v.astype(np.float32), mask


def bias_act_bwd_f32(y, dy, cutoff, rate=0.0):
    """dz = dy / keep where 0 < y < cutoff / keep, else 0 (y: the forward's output)."""
    y = np.asarray(y, dtype=np.float32)
    dy = np.asarray(dy, dtype=np.float32)
    inv_keep = inv_keep_f32(rate)
    upper = np.float32(cutoff) * inv_keep
    live = (y > np.float32(0.0)) & (y < upper)
    return np.where(live, dy * inv_keep, np.float32(0.0)).astype(np.float32)


def bias_act_fwd_f64(y, bias, cutoff, rate=0.0, seed=0):
    v = np.asarray(y, dtype=np.float64)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)
    if cutoff > 0:
        v = _relu_clip(v, cutoff)
        if rate > 0:
            mask = dropout_mask(seed, v.size, rate).reshape(v.shape)
            v = np.where(mask, v / (1.0 - float(rate)), 0.0)
    return v


def bias_act_bwd_f64(y, dy, cutoff, rate=0.0):
    """float64 dz; the window is the kernel's (float32 ``cutoff / keep``), so that the two forms
    differ by rounding only, never by an element on the boundary."""
    y = np.asarray(y, dtype=np.float32)
    upper = np.float32(cutoff) * inv_keep_f32(rate)
    live = (y > np.float32(0.0)) & (y < upper)
    return np.where(live, np.asarray(dy, dtype=np.float64) / (1.0 - float(rate)), 0.0)


def _bf16_bits(x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy(), t.float().numpy()


def bf16_split3(x):
    """(b1, b2, b3): uint16 bit patterns of the three bfloat16 pieces x1 = rne(x),
    x2 = rne(x - x1), x3 = rne(x - x1 - x2)."""
    r = np.ascontiguousarray(x, dtype=np.float32)
    pieces = []
    for _ in range(3):
        bits, value = _bf16_bits(r)
        pieces.append(bits)
        r = r - value
    return tuple(pieces)


def bf16_value(bits):
    """float64 value of bfloat16 bit patterns."""
    return (np.asarray(bits, dtype=np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def f16_split2(x, scale, col_scale=None, saturate=False):
    """(h1, h2): uint16 bit patterns of the two fp16 pieces of ``x * col_scale * scale``
    (``saturate``: clamped to +-65504 first, as `split_f16` does)."""
    s = np.ascontiguousarray(x, dtype=np.float32)
    if col_scale is not None:
        s = s * np.asarray(col_scale, dtype=np.float32)
    s = s * np.float32(scale)
    if saturate:
        s = np.minimum(np.maximum(s, np.float32(-F16_MAX)), np.float32(F16_MAX))
    with np.errstate(over='ignore', invalid='ignore'):
        h1 = s.astype(np.float16)
        h2 = (s - h1.astype(np.float32)).astype(np.float16)
    return h1.view(np.uint16), h2.view(np.uint16)


def scale_for_max(bits):
    """float32 scale for the bit pattern(s) of a largest magnitude: 2^(13 - e) with e its
    exponent, clamped to [2^-126, 2^127]; 1 for zero."""
    bits = np.asarray(bits).astype(np.int64) & 0xFFFFFFFF
    e = ((bits >> 23) & 0xFF) - 127
    se = np.clip(13 - e, -126, 127)
    out = ((se + 127) << 23).astype(np.uint32).view(np.float32)
    return np.where(bits == 0, np.float32(1.0), out).astype(np.float32)


def adam_lr_t(step, lr, beta1, beta2):
    """The step size the library computes in double precision before it rounds it to float32."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return float(np.float32(lr)) * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)


def adam_f32(param, grad, m, v, step, lr=1e-5, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """TensorFlow-form Adam in float32, one rounding per operation; returns (param, m, v)."""
    f = np.float32
    p, g = np.asarray(param, dtype=f), np.asarray(grad, dtype=f)
    m, v = np.asarray(m, dtype=f), np.asarray(v, dtype=f)
    b1, b2, one = f(beta1), f(beta2), f(1.0)
    lr_t = f(adam_lr_t(step, lr, beta1, beta2))
    with np.errstate(over='ignore', under='ignore'):
        gr = g * f(grad_scale)
        m = b1 * m + (one - b1) * gr
        v = b2 * v + ((one - b2) * gr) * gr
        p = p - (lr_t * m) / (np.sqrt(v) + f(eps))
    return p, m, v
