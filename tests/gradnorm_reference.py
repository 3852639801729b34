"""Host reference of ``ctcasr_grad_norm`` (include/ctcasr.h, K14), in the arithmetic the header
pins: every square formed and added in float64, in the order that the layout alone fixes, one
rounding to float32 per norm, the clip factor by one float32 division.  numpy's float64 adds are
IEEE adds, so this reproduces the kernel's sums operation by operation.

`exact_norms` is the other yardstick: ``math.fsum`` over the same squares (exactly rounded), which
the float64 sums above can miss by some float64 ulps only - orders below one float32 ulp."""

import math

import numpy as np

CHUNK = 8192            # floats per chunk of a segment (hip.GRAD_NORM_CHUNK)
MAX_SEGMENTS = 64       # hip.GRAD_NORM_MAX_SEGMENTS
_LANES, _WAVE = 256, 64
_XOR = [np.arange(_WAVE) ^ off for off in (32, 16, 8, 4, 2, 1)]


def _butterfly(v):
    """v += v[lane ^ 32], ^ 16, ... ^ 1 over the last axis of 64; every lane ends with the sum."""
    for idx in _XOR:
        v = v + v[..., idx]
    return v


def chunk_sums(x):
    """float64 sums of squares of the chunks of one segment (float32 values, any length)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    chunks = -(-x.size // CHUNK)
    if chunks == 0:
        return np.zeros(0, dtype=np.float64)
    with np.errstate(all='ignore'):
        sq = np.zeros(chunks * CHUNK, dtype=np.float64)      # past the end: +0
        sq[:x.size] = x.astype(np.float64) ** 2              # exact
        sq = sq.reshape(chunks, CHUNK // 4 // _LANES, _LANES, 4)
        acc = np.zeros((chunks, _LANES), dtype=np.float64)
        for j in range(sq.shape[1]):                         # a lane's float4s in ascending order
            for e in range(4):                               # x, y, z, w
                acc = acc + sq[:, j, :, e]
        waves = _butterfly(acc.reshape(chunks, _LANES // _WAVE, _WAVE))[..., 0]
        return ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]


def segment_sum(x):
    """float64 sum of squares of one segment: lane l adds the chunk sums l, l + 64, ..."""
    part = chunk_sums(x)
    rows = -(-part.size // _WAVE)
    padded = np.zeros(max(rows, 1) * _WAVE, dtype=np.float64)
    padded[:part.size] = part
    lanes = np.zeros(_WAVE, dtype=np.float64)
    with np.errstate(all='ignore'):
        for row in padded.reshape(-1, _WAVE):
            lanes = lanes + row
        return float(_butterfly(lanes)[0])


def sanitize_offsets(offsets, n):
    """The table as the kernels use it: clamped into [0, n], ascending, every entry but the last
    rounded down to a multiple of 4.  A table that keeps the contract comes back unchanged."""
    out, prev = [], 0
    for i, o in enumerate(offsets):
        o = min(max(int(o), 0), n)
        if i < len(offsets) - 1:
            o &= ~3
        prev = max(prev, o)
        out.append(prev)
    return out


def _norm32(total, grad_scale):
    with np.errstate(all='ignore'):
        return np.float32(np.float64(np.float32(grad_scale)) * np.sqrt(np.float64(total)))


def clip_factor(global_norm, max_norm):
    """float32: max_norm / global by one float32 division where that clips, 0 for a norm that is
    not finite, else exactly 1."""
    g, m = np.float32(global_norm), np.float32(max_norm)
    if not np.isfinite(g):
        return np.float32(0.0)
    if m > 0 and g > m:
        return np.float32(m / g)
    return np.float32(1.0)


def grad_norm(x, offsets, grad_scale=1.0, max_norm=0.0):
    """(norms float32[segments + 1], clip factor float32) as the kernels compute them."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    table = sanitize_offsets(offsets, x.size)
    sums = [segment_sum(x[a:b]) for a, b in zip(table[:-1], table[1:])]
    total = np.float64(0.0)
    with np.errstate(all='ignore'):
        for s in sums:
            total = total + np.float64(s)
    norms = np.array([_norm32(s, grad_scale) for s in sums] + [_norm32(total, grad_scale)],
                     dtype=np.float32)
    return norms, clip_factor(norms[-1], max_norm)


def exact_norms(x, offsets, grad_scale=1.0):
    """float32(grad_scale * sqrt(fsum(x^2))) per segment and over everything: the squares exact in
    float64, their sum exactly rounded.  Finite values only."""
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    sq = x * x
    scale = float(np.float32(grad_scale))
    out = [np.float32(scale * math.sqrt(math.fsum(sq[a:b])))
           for a, b in zip(offsets[:-1], offsets[1:])]
    out.append(np.float32(scale * math.sqrt(math.fsum(sq[offsets[0]:offsets[-1]]))))
    return np.array(out, dtype=np.float32)


def ulps32(got, want):
    """Distance of two float32 arrays of finite values >= 0 in units in the last place."""
    got = np.asarray(got, dtype=np.float32).view(np.int32).astype(np.int64)
    want = np.asarray(want, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(got - want)
