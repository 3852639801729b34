"""Plain float64 reference of the three convolutions of the DS2 front end (csrc/conv.hip,
csrc/conv16.hip), for tests/test_gpu_conv_edges.py; pinned on the CPU by tests/test_conv_host.py.

    'conv0'   1 -> 32 channels, 11 x 41 taps, stride (2, 2), x [B, T, 80]
    's12_40'  32 -> 32 channels on 40 frequencies, 11 x 21 taps, stride (1, 2)
    's12_20'  32 -> 96 channels on 20 frequencies, 11 x 21 taps, stride (1, 2)

TensorFlow SAME padding (the odd element at the end), NHWC activations, kernels in the compute
layout [Cout, Cin, kt, kf].  The sums are `torch.nn.functional.conv2d` and the gradient
functions of `torch.nn.grad` in float64 on the CPU over an explicitly padded input; the clip is
numpy's minimum(maximum()), which keeps a NaN.  `time_major=True` takes / returns the OUTPUT-side
tensors (y, dz, act) as [T, B, F', C].

The integer generators at the end draw operands whose every product and partial sum is an integer
far below 2^24: a float32 kernel has to reproduce the float64 result exactly, whatever its
summation order (test_conv_host.py checks the magnitudes)."""

import collections

import numpy as np
import torch

Layer = collections.namedtuple('Layer', 'cin cout kt kf stride freq cutoff')
LAYERS = {
    'conv0': Layer(1, 32, 11, 41, (2, 2), 80, 64.0),
    's12_40': Layer(32, 32, 11, 21, (1, 2), 40, 256.0),
    's12_20': Layer(32, 96, 11, 21, (1, 2), 20, 256.0),
}


def same_padding(size, kernel, stride):
    """(outputs, pad before, pad after) of one axis."""
    out = (size + stride - 1) // stride
    total = max((out - 1) * stride + kernel - size, 0)
    return out, total // 2, total - total // 2


def out_shape(layer, batch, frames):
    lay = LAYERS[layer]
    return (batch, same_padding(frames, lay.kt, lay.stride[0])[0],
            same_padding(lay.freq, lay.kf, lay.stride[1])[0], lay.cout)


def relu_clip(v, cutoff):
    """min(max(v, 0), cutoff); NaN stays NaN, +inf -> cutoff, -inf -> 0."""
    return np.minimum(np.maximum(v, 0.0), cutoff)


def clip_mask(act, cutoff):
    """Where the gradient passes the clip: the STORED output lies strictly inside (0, cutoff)."""
    act = np.asarray(act)
    return (act > 0.0) & (act < cutoff)


def _nchw(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 3:                      # conv0's features [B, T, 80]: one input channel
        a = a[..., None]
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def _conv(layer, x_nchw, w):
    lay = LAYERS[layer]
    _, pt0, pt1 = same_padding(x_nchw.shape[2], lay.kt, lay.stride[0])
    _, pf0, pf1 = same_padding(x_nchw.shape[3], lay.kf, lay.stride[1])
    padded = torch.nn.functional.pad(x_nchw, (pf0, pf1, pt0, pt1))
    return torch.nn.functional.conv2d(padded, w, stride=lay.stride)


def _batch_major(a, time_major):
    a = np.asarray(a, dtype=np.float64)
    return a.transpose(1, 0, 2, 3) if time_major else a


def forward(layer, x, w, bias=None, cutoff=0.0, time_major=False):
    """x [B, T, F, Cin] ([B, T, 80] for 'conv0'), w [Cout, Cin, kt, kf] -> y [B, T', F', Cout]."""
    with torch.no_grad():
        y = _conv(layer, _nchw(x), torch.from_numpy(np.asarray(w, dtype=np.float64)))
    y = y.permute(0, 2, 3, 1).numpy()
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)
    if cutoff > 0.0:
        y = relu_clip(y, cutoff)
    return np.ascontiguousarray(y.transpose(1, 0, 2, 3) if time_major else y)


def masked(dz, act=None, cutoff=0.0, time_major=False):
    """The pre-activation gradient [B, T', F', Cout]: dz where the stored output `act` lies
    strictly inside (0, cutoff), 0 elsewhere (dz itself without `act`)."""
    dz = _batch_major(dz, time_major)
    if act is None:
        return dz
    return np.where(clip_mask(_batch_major(act, time_major), cutoff), dz, 0.0)


def _padded_size(layer, frames):
    lay = LAYERS[layer]
    _, pt0, pt1 = same_padding(frames, lay.kt, lay.stride[0])
    _, pf0, pf1 = same_padding(lay.freq, lay.kf, lay.stride[1])
    return (pt0, pt1, pf0, pf1), (frames + pt0 + pt1, lay.freq + pf0 + pf1)


def data_grad(layer, dz, w, frames, act=None, cutoff=0.0, time_major=False):
    """dx [B, T, F, Cin] of `forward` for the upstream gradient dz: the gradient with respect
    to the padded input, cropped."""
    lay = LAYERS[layer]
    g = masked(dz, act, cutoff, time_major)
    (pt0, _, pf0, _), (pt, pf) = _padded_size(layer, frames)
    dx = torch.nn.grad.conv2d_input((g.shape[0], lay.cin, pt, pf),
                                    torch.from_numpy(np.asarray(w, dtype=np.float64)), _nchw(g),
                                    stride=lay.stride)
    dx = dx[:, :, pt0:pt0 + frames, pf0:pf0 + lay.freq]
    return dx.permute(0, 2, 3, 1).contiguous().numpy()


def kernel_grad(layer, dz, x, act=None, cutoff=0.0, time_major=False):
    """(dw [Cout, Cin, kt, kf], dbias [Cout]) of `forward` for the upstream gradient dz."""
    lay = LAYERS[layer]
    g = masked(dz, act, cutoff, time_major)
    x_nchw = _nchw(x)
    (pt0, pt1, pf0, pf1), _ = _padded_size(layer, x_nchw.shape[2])
    padded = torch.nn.functional.pad(x_nchw, (pf0, pf1, pt0, pt1))
    dw = torch.nn.grad.conv2d_weight(padded, (lay.cout, lay.cin, lay.kt, lay.kf), _nchw(g),
                                     stride=lay.stride)
    return dw.numpy(), g.sum(axis=(0, 1, 2))


# ------------------------------------------------------------------------------------------
# which results a single poisoned operand element reaches (its receptive field, padding excluded):
# the same sums over indicators, with every other operand 1
# ------------------------------------------------------------------------------------------
def reach_of_x(layer, x_hit, time_major=False):
    lay = LAYERS[layer]
    ones = np.ones((lay.cout, lay.cin, lay.kt, lay.kf))
    return forward(layer, np.asarray(x_hit, dtype=np.float64), ones, time_major=time_major) > 0


def reach_of_w(layer, w_hit, batch, frames, time_major=False):
    lay = LAYERS[layer]
    ones = np.ones((batch, frames, lay.freq, lay.cin))
    return forward(layer, ones, np.asarray(w_hit, dtype=np.float64), time_major=time_major) > 0


def reach_of_dz_in_dx(layer, dz_hit, frames, time_major=False):
    lay = LAYERS[layer]
    ones = np.ones((lay.cout, lay.cin, lay.kt, lay.kf))
    return data_grad(layer, np.asarray(dz_hit, dtype=np.float64), ones, frames,
                     time_major=time_major) > 0


def reach_of_dz_in_dw(layer, dz_hit, frames, time_major=False):
    lay = LAYERS[layer]
    hit = _batch_major(dz_hit, time_major)
    shape = (hit.shape[0], frames, lay.freq) + ((lay.cin,) if lay.cin > 1 else ())
    return kernel_grad(layer, hit, np.ones(shape))[0] > 0


# ------------------------------------------------------------------------------------------
# integer operands
# ------------------------------------------------------------------------------------------
def int_inputs(rng, shape):
    """What sits behind a clipped ReLU: {0 .. 3}."""
    return rng.integers(0, 4, size=shape).astype(np.float32)


def int_features(rng, shape):
    """Features (conv0's input): {-3 .. 3}."""
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def int_weights(rng, layer):
    lay = LAYERS[layer]
    return rng.integers(-2, 3, size=(lay.cout, lay.cin, lay.kt, lay.kf)).astype(np.float32)


def int_bias(rng, layer):
    return rng.integers(-4, 5, size=LAYERS[layer].cout).astype(np.float32)


def int_dz(rng, shape):
    """{-3 .. 3} with about 10 % further zeros and some all-zero frames (axes 0 and 1 are batch
    and time in either order)."""
    dz = rng.integers(-3, 4, size=shape).astype(np.float32)
    dz[rng.random(shape) < 0.1] = 0.0
    dz[rng.random(shape[:2]) < 0.15] = 0.0
    return dz


def inside_share(act, cutoff):
    """Share of stored outputs strictly inside (0, cutoff)."""
    return float(clip_mask(act, cutoff).mean())


# ------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_conv_edges.py (here, so that test_conv_host.py can check on the CPU
# what the GPU tests assume about them)
# ------------------------------------------------------------------------------------------
S12_TT = {'s12_40': 32, 's12_20': 16}        # output frames per workgroup (Geometry::TT)


def s12_frames(layer):
    """Both sides of the 5-frame halo, of one workgroup's tile and of two."""
    tt = S12_TT[layer]
    return [1, 2, 5, 6, 10, 11, tt - 1, tt, tt + 1, tt + 5, tt + 6, 2 * tt, 2 * tt + 1]


# conv0: both parities of the front padding on either side of one and two 16-output-frame tiles
CONV0_FRAMES = [1, 2, 3, 10, 11, 12, 21, 22, 31, 32, 33, 34, 63, 64, 65, 66]
FORWARD_BATCHES = (1, 3)


def forward_frames(layer):
    return CONV0_FRAMES if layer == 'conv0' else s12_frames(layer)


def _seed(layer, batch, frames, salt):
    return [sorted(LAYERS).index(layer), batch, frames, salt]


def x_shape(layer, batch, frames):
    lay = LAYERS[layer]
    return (batch, frames, lay.freq) + ((lay.cin,) if lay.cin > 1 else ())


def forward_case(layer, batch, frames):
    """(x, w, bias) of a forward test: different content per utterance."""
    rng = np.random.default_rng(_seed(layer, batch, frames, 0))
    x = (int_features if layer == 'conv0' else int_inputs)(rng, x_shape(layer, batch, frames))
    return x, int_weights(rng, layer), int_bias(rng, layer)


def stored_outputs(rng, shape, cutoff):
    """What a clipped layer may have stored, for the backward mask: both ends of the clip (where
    the gradient stops) and values next to them (where it passes), 3 of 7 inside."""
    values = np.array([0.0, 0.0, 1.0, 7.0, cutoff - 1.0, cutoff, cutoff], dtype=np.float32)
    return values[rng.integers(0, len(values), size=shape)]


def backward_case(layer, batch, frames, time_major=False):
    """(dz, act, x, w) of a gradient test; dz and act [B, T', F', Cout] or time-major."""
    rng = np.random.default_rng(_seed(layer, batch, frames, 1))
    shape = out_shape(layer, batch, frames)
    if time_major:
        shape = (shape[1], shape[0]) + shape[2:]
    x = (int_features if layer == 'conv0' else int_inputs)(rng, x_shape(layer, batch, frames))
    return (int_dz(rng, shape), stored_outputs(rng, shape, LAYERS[layer].cutoff), x,
            int_weights(rng, layer))
