"""tests/conv_reference.py pinned on the CPU: against the numpy oracle's `conv2d_same` (a patch
loop that shares no code with torch's conv2d), its gradients against the adjoint identities, the
clip and its mask at their edges, and the two promises the exact GPU tests
(tests/test_gpu_conv_edges.py) rest on - integer results below 2^24, and a clip that is neither
always nor never active on that data."""

import numpy as np
import pytest

from oracle import nn as onn
from tests import conv_reference as ref

LAYER_NAMES = ('conv0', 's12_40', 's12_20')


_x_shape = ref.x_shape


def _x4(x):
    return x[..., None] if x.ndim == 3 else x


@pytest.mark.parametrize('layer', LAYER_NAMES)
@pytest.mark.parametrize('frames', [1, 2, 5, 8, 11, 12])
def test_forward_equals_the_numpy_oracle(layer, frames):
    lay = ref.LAYERS[layer]
    rng = np.random.default_rng(frames)
    x = rng.normal(size=_x_shape(layer, 2, frames))
    w = rng.normal(size=(lay.cout, lay.cin, lay.kt, lay.kf))
    bias = rng.normal(size=lay.cout)
    want = onn.conv2d_same(_x4(x), w.transpose(2, 3, 1, 0), bias, lay.stride)
    got = ref.forward(layer, x, w, bias)
    assert got.shape == want.shape == ref.out_shape(layer, 2, frames)
    assert np.abs(got - want).max() < 1e-11 * np.abs(want).max()
    cut = 0.3 * np.abs(want).max()
    assert np.array_equal(ref.forward(layer, x, w, bias, cutoff=cut),
                          onn.relu_clip(got, cut))
    assert np.array_equal(ref.forward(layer, x, w, bias, time_major=True),
                          got.transpose(1, 0, 2, 3))
    no_bias = ref.forward(layer, x, w)
    assert np.abs(no_bias + bias - got).max() < 1e-11 * np.abs(want).max()


def test_same_padding_puts_the_odd_element_at_the_end():
    for size in range(1, 40):
        for kernel, stride in ((11, 1), (11, 2), (21, 2), (41, 2)):
            assert ref.same_padding(size, kernel, stride) == onn.same_padding(size, kernel, stride)
    # the first layer's time axis: 5 frames in front for an odd T, 4 for an even one
    assert ref.same_padding(21, 11, 2)[1:] == (5, 5) and ref.same_padding(22, 11, 2)[1:] == (4, 5)


@pytest.mark.parametrize('layer', LAYER_NAMES)
@pytest.mark.parametrize('frames', [1, 4, 7, 12])
@pytest.mark.parametrize('time_major', [False, True])
def test_gradients_are_the_adjoints_of_the_forward_pass(layer, frames, time_major):
    """<conv(x, w), dz> = <x, dgrad(dz, w)> = <w, wgrad(dz, x)>, and the mask enters both
    gradients as a factor on dz."""
    lay = ref.LAYERS[layer]
    rng = np.random.default_rng(100 + frames)
    x = rng.normal(size=_x_shape(layer, 3, frames))
    w = rng.normal(size=(lay.cout, lay.cin, lay.kt, lay.kf))
    y = ref.forward(layer, x, w, time_major=time_major)
    dz = rng.normal(size=y.shape)
    lhs = float((y * dz).sum())
    dx = ref.data_grad(layer, dz, w, frames, time_major=time_major)
    dw, db = ref.kernel_grad(layer, dz, x, time_major=time_major)
    assert dx.shape == _x4(x).shape and dw.shape == w.shape and db.shape == (lay.cout,)
    scale = float(np.abs(y * dz).sum())
    assert abs(float((_x4(x) * dx).sum()) - lhs) < 1e-11 * scale
    assert abs(float((w * dw).sum()) - lhs) < 1e-11 * scale
    axes = (0, 1, 2)
    assert np.abs(db - dz.sum(axis=axes)).max() < 1e-12 * np.abs(dz).sum()
    # masked: the same as handing over dz * mask
    act = rng.uniform(-1.0, 3.0, size=y.shape)
    act[rng.random(y.shape) < 0.2] = 0.0
    act[rng.random(y.shape) < 0.2] = 2.0
    keep = (act > 0) & (act < 2.0)
    assert np.array_equal(ref.data_grad(layer, dz, w, frames, act, 2.0, time_major),
                          ref.data_grad(layer, dz * keep, w, frames, time_major=time_major))
    dw_m, db_m = ref.kernel_grad(layer, dz, x, act, 2.0, time_major)
    dw_k, db_k = ref.kernel_grad(layer, dz * keep, x, time_major=time_major)
    assert np.array_equal(dw_m, dw_k) and np.array_equal(db_m, db_k)
    assert np.abs(db_m - (dz * keep).sum(axis=axes)).max() < 1e-12 * np.abs(dz).sum()


def test_the_clip_keeps_nan_and_saturates_infinities():
    v = np.array([np.nan, -np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 3.0, 64.0, 65.0])
    got = ref.relu_clip(v, 64.0)
    assert np.isnan(got[:2]).all()
    assert got[2:].tolist() == [64.0, 0.0, 0.0, 0.0, 0.0, 3.0, 64.0, 64.0]
    assert np.array_equal(got, onn.relu_clip(v, 64.0), equal_nan=True)
    # through the fused epilogue of the reference: a NaN bias poisons its channel and no other
    rng = np.random.default_rng(0)
    x = ref.int_features(rng, (1, 4, 80))
    w = ref.int_weights(rng, 'conv0')
    bias = ref.int_bias(rng, 'conv0')
    bias[[3, 4, 5]] = np.nan, np.inf, -np.inf
    y = ref.forward('conv0', x, w, bias, cutoff=64.0)
    assert np.isnan(y[..., 3]).all() and (y[..., 4] == 64.0).all() and (y[..., 5] == 0.0).all()
    assert np.isfinite(np.delete(y, 3, axis=3)).all()


def test_the_mask_is_open_at_both_ends():
    eps = np.nextafter(np.float32(0), np.float32(1))
    below = np.nextafter(np.float32(256), np.float32(0))
    act = np.array([0.0, -0.0, eps, 1.0, below, 256.0, 257.0, -1.0, np.nan], dtype=np.float32)
    assert ref.clip_mask(act, 256.0).tolist() == [False, False, True, True, True, False, False,
                                                  False, False]
    dz = np.arange(1.0, 10.0)
    assert ref.masked(dz.reshape(1, 1, 1, 9), act.reshape(1, 1, 1, 9), 256.0).ravel().tolist() == \
        [0, 0, 3, 4, 5, 0, 0, 0, 0]


def test_reach_is_the_receptive_field_without_the_padding():
    hit = np.zeros((1, 12, 40, 32))
    hit[0, 0, 0, 7] = 1                                  # a corner of the input
    reach = ref.reach_of_x('s12_40', hit)
    want = np.zeros((1, 12, 20, 32), dtype=bool)
    want[0, :6, :5, :] = True                            # t - 5 <= 0, 2 fo - 9 <= 0 <= 2 fo + 11
    assert np.array_equal(reach, want)
    w_hit = np.zeros((32, 32, 11, 21))
    w_hit[3, 0, 0, 20] = 1                               # the last kf tap of the first kt row
    reach = ref.reach_of_w('s12_40', w_hit, 1, 12)
    want = np.zeros((1, 12, 20, 32), dtype=bool)
    want[0, 5:, :15, 3] = True                           # t - 5 >= 0, 2 fo + 11 <= 39
    assert np.array_equal(reach, want)
    dz_hit = np.zeros((1, 6, 40, 32))
    dz_hit[0, 5, 39, 2] = 1                              # conv0: 11 input frames -> 6 outputs
    assert ref.reach_of_dz_in_dw('conv0', dz_hit, 11)[2].any()
    assert not np.delete(ref.reach_of_dz_in_dw('conv0', dz_hit, 11), 2, axis=0).any()
    assert ref.reach_of_dz_in_dx('s12_20', np.ones((1, 3, 10, 96)), 3).all()


# ------------------------------------------------------------------------------------------
# the integer data of the exact GPU tests
# ------------------------------------------------------------------------------------------
def _is_small_integer(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.array_equal(a, np.rint(a)) and np.abs(a).max() < 2 ** 24)


@pytest.mark.parametrize('layer', LAYER_NAMES)
@pytest.mark.parametrize('batch,frames', [(1, 1), (3, 12), (2, 33)])
def test_integer_operands_give_integer_results_below_2_to_24(layer, batch, frames):
    lay = ref.LAYERS[layer]
    rng = np.random.default_rng(batch * 100 + frames)
    x = (ref.int_features if layer == 'conv0' else ref.int_inputs)(
        rng, _x_shape(layer, batch, frames))
    w, bias = ref.int_weights(rng, layer), ref.int_bias(rng, layer)
    assert set(np.unique(w)) <= {-2, -1, 0, 1, 2} and np.abs(bias).max() <= 4
    assert x.min() >= (-3 if layer == 'conv0' else 0) and x.max() <= 3
    y = ref.forward(layer, x, w, bias)
    dz = ref.int_dz(rng, y.shape)
    assert np.abs(dz).max() <= 3 and 0.1 < (dz == 0).mean() < 0.6
    dw, db = ref.kernel_grad(layer, dz, x)
    for result in (y, ref.data_grad(layer, dz, w, frames), dw, db):
        assert _is_small_integer(result)


def test_integer_results_stay_below_2_to_24_at_any_size_the_gpu_tests_use():
    """Bounds, not samples: |y| <= taps * 3 * 2 + 4; |dx| <= (taps per input element) * 3 * 2;
    |dw| <= 9 * output positions, |dbias| <= 3 * output positions - no case of the GPU file has
    more than 17 x 129 x 20 positions (11 x 21 layers) or 9 x 257 x 40 (first layer)."""
    for lay in ref.LAYERS.values():
        assert lay.cin * lay.kt * lay.kf * 6 + 4 < 2 ** 24
        assert lay.cout * lay.kt * lay.kf * 6 < 2 ** 24
    assert 9 * 17 * 129 * 20 < 2 ** 24 and 9 * 9 * 257 * 40 < 2 ** 24


@pytest.mark.parametrize('layer', LAYER_NAMES)
def test_the_clip_is_neither_always_nor_never_active_on_the_integer_data(layer):
    """The cutoffs of `LAYERS` (powers of two) against pre-activations of standard deviation
    ~230 (11 x 21 layers) / ~60 (first layer), smaller at the borders: between 5 % and 95 % of
    the stored outputs lie strictly inside (0, cutoff), for every forward case of the GPU file -
    and in what its gradient tests hand over as stored outputs."""
    lay = ref.LAYERS[layer]
    for frames in ref.forward_frames(layer):
        for batch in ref.FORWARD_BATCHES:
            x, w, bias = ref.forward_case(layer, batch, frames)
            y = ref.forward(layer, x, w, bias, cutoff=lay.cutoff)
            assert 0.05 < ref.inside_share(y, lay.cutoff) < 0.95, (batch, frames)
            assert (y == 0).any() and (frames < 17 or (y == lay.cutoff).any())
            if batch > 1:
                assert not np.array_equal(x[0], x[1])
    dz, act, _, _ = ref.backward_case(layer, 3, 7)
    assert 0.05 < ref.inside_share(act, lay.cutoff) < 0.95
    assert (act == 0).any() and (act == lay.cutoff).any() and dz.any()
