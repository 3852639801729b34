"""The convolution kernels of csrc/conv.hip and csrc/conv16.hip at their seams, compared exactly.

Operands are small integers (tests/conv_reference.py: inputs {0..3} or {-3..3}, weights {-2..2},
bias {-4..4}, power-of-two cutoffs), so every product and partial sum is an integer far below
2^24 and the float32-MFMA kernels have to reproduce the float64 reference at EVERY element in
any summation order: a tap dropped at a SAME-padding border, in the 5-frame halo between two
workgroups' tiles or in the last split of a kernel-gradient walk changes an integer, however
small it is next to the tensor's largest value.  The same holds for the fp16 two-piece kernels:
integers times their power-of-two scales are exact in fp16 (the second piece is 0), the MFMA sums
are multiples of one power of two with fewer than 24 significant bits, the scales come out by
powers of two.  Values are compared with `np.array_equal` (+0 == -0), the bias gradient too
(integer sums do not depend on the order of the atomics).

Shapes are the smallest that cross each seam: `Geometry::TT` (32 / 16 output frames per
workgroup, 5-frame halo), `WrwGeometry::TT` (4 / 8 frames per kernel-gradient tile) and the cap
of `wrw_splits` (read back from the workspace size), the 8-utterance blocks of `conv_s12_wrw16`,
conv0's 16-output-frame tiles with both parities of the front padding, its 16 reduce bands and
the 256-workgroup grid of `conv0_wrw16`.

Around that: every output sits inside a buffer of NaN words that must stay as they were, the
kernel gradients overwrite a dirty `dw` completely and give equal bits on dirty workspaces; a NaN
in x, w or bias reaches exactly the outputs whose receptive field holds it (clip on or off)
and a NaN or inf in dz every gradient it touches; a NaN conv weight or feature value drops the
training step; and the Python wrappers refuse arguments of the wrong size before anything is
launched."""

import functools

import numpy as np
import pytest
import torch

from tests import conv_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S12 = {'s12_40': (40, 32), 's12_20': (20, 96)}       # (input frequencies, output channels)
X_SCALE = 2.0 ** 11                                  # 3 x 2^11 is exact in fp16
NAN_WORD = 0x7FC0BEEF
PAD = 64                                             # guard words on either side of an output
INF = float('inf')


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _guarded(shape):
    """An output of this shape in the middle of a buffer of NaN words: (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), NAN_WORD, dtype=torch.int32, device=DEV)
    return buf, buf[PAD:PAD + n].view(torch.float32).view(*shape)


def _guards_intact(buf):
    return bool((buf[:PAD] == NAN_WORD).all()) and bool((buf[-PAD:] == NAN_WORD).all())


def _untouched(buf):
    return bool((buf == NAN_WORD).all())


def _exact(got, want):
    got, want = _np(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want.astype(np.float32))


def _bits(t):
    return _np(t).view(np.uint32)


def _dirty_allocator(nbytes):
    """Leave a freed block of 0xFF bytes (NaN words) for the wrapper's next workspace."""
    junk = torch.full((int(nbytes) + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    del junk


@functools.lru_cache(maxsize=None)
def _forward_reference(layer, batch, frames):
    x, w, bias = ref.forward_case(layer, batch, frames)
    return x, w, bias, ref.forward(layer, x, w, bias)


# ============================================================================ forward, 11 x 21
def _s12_forward(hip, layer, form, x, packs, bias, out, cutoff, time_major):
    cout = S12[layer][1]
    if form == 16:
        return hip.conv_s12_fwd16(x, X_SCALE, packs[16], cout, bias, out=out, relu_cutoff=cutoff,
                                  time_major=time_major)
    return hip.conv_s12_fwd(x, packs[32], cout, bias, out=out, relu_cutoff=cutoff,
                            time_major=time_major)


def _s12_packs(hip, w):
    w = _t(w)
    return {32: hip.conv_s12_pack_weights(w), 16: hip.conv_s12_pack_weights16(w)}


@pytest.mark.parametrize('layer', sorted(S12))
@pytest.mark.parametrize('step', range(13))
def test_conv_s12_forward_is_exact_at_the_tile_seams(hip, layer, step):
    """`conv_s12_fwd` and `conv_s12_fwd16` at T = 1, 2, 5, 6, 10, 11, TT-1, TT, TT+1, TT+5, TT+6,
    2 TT, 2 TT + 1: with and without bias, with the fused clip, batch-major and time-major."""
    frames = ref.s12_frames(layer)[step]
    cutoff = ref.LAYERS[layer].cutoff
    for batch in ref.FORWARD_BATCHES:
        x, w, bias, y = _forward_reference(layer, batch, frames)
        assert 0.05 < ref.inside_share(ref.relu_clip(y, cutoff), cutoff) < 0.95
        x_dev, bias_dev, packs = _t(x), _t(bias), _s12_packs(hip, w)
        for form in (32, 16):
            for with_bias in (True, False):
                for cut in (0.0, cutoff):
                    for time_major in (False, True):
                        want = y if with_bias else y - bias
                        want = ref.relu_clip(want, cut) if cut else want
                        want = want.transpose(1, 0, 2, 3) if time_major else want
                        buf, out = _guarded(want.shape)
                        got = _s12_forward(hip, layer, form, x_dev, packs,
                                           bias_dev if with_bias else None, out, cut, time_major)
                        what = (batch, frames, form, with_bias, cut, time_major)
                        assert got.data_ptr() == out.data_ptr(), what
                        assert _exact(got, want), what
                        assert _guards_intact(buf), what


# ============================================================================ data gradient
@pytest.mark.parametrize('layer', sorted(S12))
@pytest.mark.parametrize('step', range(13))
def test_conv_s12_data_gradient_is_exact_at_the_tile_seams(hip, layer, step):
    """`conv_s12_bwd_data` and `conv_s12_bwd_data16` at the frames of the forward test: dz with
    zero cells and all-zero frames, plain and with the clip's mask applied while dz is staged
    (stored outputs at exactly 0 and exactly the cutoff), batch-major and time-major - each
    against the reference, not against another call."""
    frames = ref.s12_frames(layer)[step]
    freq = S12[layer][0]
    cutoff = ref.LAYERS[layer].cutoff
    for batch in ref.FORWARD_BATCHES:
        for time_major in (False, True):
            dz, act, _, w = ref.backward_case(layer, batch, frames, time_major)
            assert 0.05 < ref.inside_share(act, cutoff) < 0.95
            packs = _s12_packs(hip, w)
            dz_dev, act_dev = _t(dz), _t(act)
            for use_mask in (False, True):
                want = ref.data_grad(layer, dz, w, frames, act if use_mask else None, cutoff,
                                     time_major)
                mask = dict(act=act_dev, relu_cutoff=cutoff) if use_mask else {}
                for form in (32, 16):
                    buf, out = _guarded((batch, frames, freq, 32))
                    if form == 16:
                        hip.conv_s12_bwd_data16(dz_dev, packs[16], out=out, time_major=time_major,
                                                **mask)
                    else:
                        hip.conv_s12_bwd_data(dz_dev, packs[32], out=out, time_major=time_major,
                                              **mask)
                    what = (batch, frames, form, use_mask, time_major)
                    assert _exact(out, want), what
                    assert _guards_intact(buf), what


# ============================================================================ kernel gradient
def _s12_wrw_splits(hip, batch, frames, layer):
    freq, cout = S12[layer]
    nbytes = hip.load().ctcasr_conv_s12_wrw_workspace_bytes(batch, frames, freq, cout)
    assert nbytes % (cout * 32 * 231 * 4) == 0
    return nbytes // (cout * 32 * 231 * 4)


def _s12_wrw16_splits(hip, batch, frames, layer):
    """The workspace of `conv_s12_wrw16` is 512 bytes of control words, both operands as fp16
    pieces in blocks of 8 utterances (1024 bytes per (frame, input frequency), 32 cout bytes per
    (frame, output frequency)) and one partial result per split."""
    freq, cout = S12[layer]
    blocks = (batch + 7) // 8
    nbytes = hip.load().ctcasr_conv_s12_wrw16_workspace_bytes(batch, frames, freq, cout)
    nbytes -= 512 + blocks * frames * freq * 1024 + blocks * frames * (freq // 2) * 32 * cout
    assert nbytes > 0 and nbytes % (cout * 32 * 231 * 4) == 0
    return nbytes // (cout * 32 * 231 * 4)


# (batch, frames, tiles relative to the cap of wrw_splits); tiles = B ceil(T / 4) on 40
# frequencies (cap 46 on this build), B ceil(T / 8) on 20 (cap 15)
WRW_CASES = {
    's12_40': [(1, 1, 'below'), (1, 5, 'below'), (3, 6, 'below'), (2, 90, 'equal'),
               (1, 186, 'one above'), (4, 90, 'twice'), (3, 122, 'twice and one')],
    's12_20': [(1, 1, 'below'), (1, 5, 'below'), (3, 11, 'below'), (3, 37, 'equal'),
               (2, 60, 'one above'), (3, 75, 'twice'), (1, 243, 'twice and one')],
}
# tiles = ceil(B / 8) T for the fp16 form: one frame of a block of 8 utterances
WRW16_CASES = {
    's12_40': [(1, 3, 'below'), (7, 46, 'equal'), (8, 47, 'one above'), (9, 46, 'twice'),
               (17, 31, 'twice and one')],
    's12_20': [(1, 5, 'below'), (7, 15, 'equal'), (9, 8, 'one above'), (17, 10, 'twice'),
               (8, 31, 'twice and one')],
}
RELATION = {'below': lambda tiles, cap: tiles < cap, 'equal': lambda tiles, cap: tiles == cap,
            'one above': lambda tiles, cap: tiles == cap + 1,
            'twice': lambda tiles, cap: tiles == 2 * cap,
            'twice and one': lambda tiles, cap: tiles == 2 * cap + 1}


def _check_kernel_gradient(call, layer, batch, frames, workspace_bytes):
    """`call(dz, x, out, time_major, act, relu_cutoff, dbias)` against the reference: plain and
    masked with the bias gradient, batch-major and time-major, into a dirty `dw` between guard
    words; twice on dirty workspaces with equal bits."""
    lay = ref.LAYERS[layer]
    dz, act, x, _ = ref.backward_case(layer, batch, frames)
    assert 0.05 < ref.inside_share(act, lay.cutoff) < 0.95
    want_plain, bias_plain = ref.kernel_grad(layer, dz, x)
    want_masked, bias_masked = ref.kernel_grad(layer, dz, x, act, lay.cutoff)
    x_dev = _t(x)
    layouts = (False, True) if layer != 'conv0' else (False,)
    for time_major in layouts:
        dz_dev = _t(dz.transpose(1, 0, 2, 3) if time_major else dz)
        act_dev = _t(act.transpose(1, 0, 2, 3) if time_major else act)
        for use_mask in (False, True):
            want, want_bias = (want_masked, bias_masked) if use_mask else (want_plain, bias_plain)
            seen = []
            for with_bias in (True, False):
                _dirty_allocator(workspace_bytes)
                buf, out = _guarded(want.shape)
                bias_buf, dbias = _guarded((lay.cout,))
                dbias.zero_()
                call(dz_dev, x_dev, out, time_major, act_dev if use_mask else None,
                     lay.cutoff if use_mask else 0.0, dbias if with_bias else None)
                what = (batch, frames, time_major, use_mask, with_bias)
                assert _exact(out, want), what
                assert _exact(dbias, want_bias if with_bias else np.zeros(lay.cout)), what
                assert _guards_intact(buf) and _guards_intact(bias_buf), what
                seen.append(_bits(out))
            assert np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize('layer,case', [(layer, case) for layer in sorted(WRW_CASES)
                                        for case in range(len(WRW_CASES[layer]))])
def test_conv_s12_kernel_gradient_is_exact_around_the_split_cap(hip, layer, case):
    """`conv_s12_wrw`: fewer tiles than splits allowed, as many, one more, twice as many, twice
    and one (the uneven walks of the split loop), T no multiple of the tile's frames, T <= 5."""
    batch, frames, relation = WRW_CASES[layer][case]
    freq = S12[layer][0]
    tile_frames = 80 // (freq // 2)
    tiles = batch * -(-frames // tile_frames)
    cap = _s12_wrw_splits(hip, 64, 64, layer)
    assert RELATION[relation](tiles, cap), (tiles, cap)
    assert _s12_wrw_splits(hip, batch, frames, layer) == min(tiles, cap)

    def call(dz, x, out, time_major, act, relu_cutoff, dbias):
        hip.conv_s12_wrw(dz, x, out=out, time_major=time_major, act=act, relu_cutoff=relu_cutoff,
                         dbias=dbias)
    _check_kernel_gradient(call, layer, batch, frames,
                           hip.load().ctcasr_conv_s12_wrw_workspace_bytes(
                               batch, frames, freq, S12[layer][1]))


@pytest.mark.parametrize('layer,case', [(layer, case) for layer in sorted(WRW16_CASES)
                                        for case in range(len(WRW16_CASES[layer]))])
def test_conv_s12_kernel_gradient_on_the_fp16_pipe_is_exact_around_the_split_cap(hip, layer,
                                                                                case):
    """`conv_s12_wrw16`: the same relations between tiles (a frame of a block of 8 utterances)
    and the split cap, with B = 1, 7, 8, 9, 17 - a lone utterance, a block one short, full, one
    over, two blocks and one."""
    batch, frames, relation = WRW16_CASES[layer][case]
    freq, cout = S12[layer]
    tiles = -(-batch // 8) * frames
    cap = _s12_wrw16_splits(hip, 64, 64, layer)
    assert RELATION[relation](tiles, cap), (tiles, cap)
    assert _s12_wrw16_splits(hip, batch, frames, layer) == min(tiles, cap)

    def call(dz, x, out, time_major, act, relu_cutoff, dbias):
        hip.conv_s12_wrw16(dz, x, X_SCALE, out=out, time_major=time_major, act=act,
                           relu_cutoff=relu_cutoff, dbias=dbias)
    _check_kernel_gradient(call, layer, batch, frames,
                           hip.load().ctcasr_conv_s12_wrw16_workspace_bytes(batch, frames, freq,
                                                                           cout))


def test_the_fp16_kernel_gradient_cases_cover_the_blocks_of_8_utterances():
    for cases in WRW16_CASES.values():
        assert {batch for batch, _, _ in cases} == {1, 7, 8, 9, 17}
    for layer, cases in WRW_CASES.items():
        tile_frames = 80 // (S12[layer][0] // 2)
        assert any(frames % tile_frames for _, frames, _ in cases)
        assert any(frames <= 5 for _, frames, _ in cases)


# ============================================================================ first layer
@pytest.mark.parametrize('frames', ref.CONV0_FRAMES)
def test_conv0_forward_is_exact_on_either_side_of_a_tile_for_both_paddings(hip, frames):
    """`conv0_fwd` and `conv0_fwd16`: an odd T puts 5 frames of padding in front, an even T 4;
    16 output frames = 31 or 32 input frames per workgroup."""
    cutoff = ref.LAYERS['conv0'].cutoff
    for batch in ref.FORWARD_BATCHES:
        x, w, bias, y = _forward_reference('conv0', batch, frames)
        assert 0.05 < ref.inside_share(ref.relu_clip(y, cutoff), cutoff) < 0.95
        x_dev, w_dev, bias_dev = _t(x), _t(w), _t(bias)
        packed16 = hip.conv0_pack_weights16(w_dev)
        for form in (32, 16):
            for with_bias in (True, False):
                for cut in (0.0, cutoff):
                    want = y if with_bias else y - bias
                    want = ref.relu_clip(want, cut) if cut else want
                    buf, out = _guarded(want.shape)
                    b = bias_dev if with_bias else None
                    if form == 16:
                        hip.conv0_fwd16(x_dev, packed16, b, out=out, relu_cutoff=cut)
                    else:
                        hip.conv0_fwd(x_dev, w_dev, b, out=out, relu_cutoff=cut)
                    what = (batch, frames, form, with_bias, cut)
                    assert _exact(out, want), what
                    assert _guards_intact(buf), what


# B x ceil(t_out / 16) workgroups' partial results against the 16 reduce bands: fewer parts than
# bands, as many, more (bands of 2 with an empty one; bands of 3)
CONV0_WRW_CASES = [(1, 2, 1), (5, 66, 15), (16, 3, 16), (17, 2, 17), (11, 65, 33)]


@pytest.mark.parametrize('batch,frames,parts', CONV0_WRW_CASES)
def test_conv0_kernel_gradient_is_exact_around_the_reduce_bands(hip, batch, frames, parts):
    t_out = (frames + 1) // 2
    assert batch * -(-t_out // 16) == parts
    nbytes = hip.load().ctcasr_conv0_wrw_workspace_bytes(batch, frames)
    assert nbytes == (parts + 16) * 32 * 11 * 41 * 4

    def call(dz, x, out, time_major, act, relu_cutoff, dbias):
        hip.conv0_wrw(dz, x, out=out, act=act, relu_cutoff=relu_cutoff, dbias=dbias)
    _check_kernel_gradient(call, 'conv0', batch, frames, nbytes)


# ceil(B / 8) x t_out tiles against the grid of 256 workgroups: one tile each but one, one each,
# one workgroup with two; and the smallest there is
CONV0_WRW16_CASES = [(1, 1, 1), (3, 509, 255), (9, 255, 256), (1, 514, 257), (9, 3, 4)]


@pytest.mark.parametrize('batch,frames,tiles', CONV0_WRW16_CASES)
def test_conv0_kernel_gradient_on_the_fp16_pipe_is_exact_around_its_grid(hip, batch, frames,
                                                                         tiles):
    """The workspace of `conv0_wrw16` is 512 bytes of control words, x as fp16 pieces in blocks
    of 8 utterances (2560 bytes per input frame), dz likewise (40 960 bytes per output frame) and
    one partial result per workgroup: the grid is read back from its size."""
    t_out, blocks = (frames + 1) // 2, (batch + 7) // 8
    assert blocks * t_out == tiles
    nbytes = hip.load().ctcasr_conv0_wrw16_workspace_bytes(batch, frames)
    grid_bytes = nbytes - 512 - blocks * frames * 2560 - blocks * t_out * 40960
    assert grid_bytes == min(tiles, 256) * 32 * 11 * 41 * 4

    def call(dz, x, out, time_major, act, relu_cutoff, dbias):
        hip.conv0_wrw16(dz, x, out=out, act=act, relu_cutoff=relu_cutoff, dbias=dbias)
    _check_kernel_gradient(call, 'conv0', batch, frames, nbytes)


# ============================================================================ NaN and inf
def _nan_like_clean(got, clean, reach, what, same_elsewhere=True):
    """NaN wherever the poisoned element reaches; the clean run's bits everywhere else."""
    got, clean = _np(got), _np(clean)
    assert np.isnan(got[reach]).all(), what
    if same_elsewhere:
        assert np.array_equal(got.view(np.uint32)[~reach], clean.view(np.uint32)[~reach]), what


def _forward_nan_cases(layer, batch, frames, seam):
    """(operand, index) of single NaNs: at a border, inside, and at a tile seam."""
    lay = ref.LAYERS[layer]
    if layer == 'conv0':
        xs = [(0, 0, 0), (batch - 1, seam // 2, 40), (0, seam - 1, 79), (batch - 1, seam, 3)]
    else:
        xs = [(0, 0, 0, 0), (batch - 1, seam // 2, lay.freq // 2 + 1, 17),
              (0, seam - 1, lay.freq - 1, 31), (batch - 1, seam, 2, 5)]
    ws = [(0, 0, 0, 0), (lay.cout // 2, lay.cin // 2, 5, lay.kf // 2),
          (lay.cout - 1, lay.cin - 1, lay.kt - 1, lay.kf - 1)]
    return [('x', i) for i in xs] + [('w', i) for i in ws] + [('bias', (0,)), ('bias', (19,))]


def _check_forward_nan(run, layer, batch, frames, seam):
    """`run(x, w, bias, cutoff)` -> y on the device, for every single-NaN case, clip on and off.
    A NaN weight meets the zeros of the padding too (0 x NaN): outputs of its channel outside
    the receptive field may be NaN or clean; every other channel keeps its bits."""
    lay = ref.LAYERS[layer]
    x, w, bias = ref.forward_case(layer, batch, frames)
    for cutoff in (0.0, lay.cutoff):
        clean = run(x, w, bias, cutoff)
        assert torch.isfinite(clean).all()
        for operand, index in _forward_nan_cases(layer, batch, frames, seam):
            bad = {'x': x.copy(), 'w': w.copy(), 'bias': bias.copy()}
            bad[operand][index] = np.nan
            got = run(bad['x'], bad['w'], bad['bias'], cutoff)
            what = (layer, operand, index, cutoff)
            hit = np.zeros(bad[operand].shape)
            hit[index] = 1
            if operand == 'x':
                _nan_like_clean(got, clean, ref.reach_of_x(layer, hit), what)
            elif operand == 'w':
                reach = ref.reach_of_w(layer, hit, batch, frames)
                assert reach.any() and not np.delete(reach, index[0], axis=3).any()
                got_np, clean_np = _np(got), _np(clean)
                assert np.isnan(got_np[reach]).all(), what
                others = np.ones(lay.cout, dtype=bool)
                others[index[0]] = False
                assert np.array_equal(got_np[..., others].view(np.uint32),
                                      clean_np[..., others].view(np.uint32)), what
                same = got_np[..., index[0]] == clean_np[..., index[0]]
                assert (same | np.isnan(got_np[..., index[0]])).all(), what
            else:
                reach = np.zeros(got.shape, dtype=bool)
                reach[..., index[0]] = True
                _nan_like_clean(got, clean, reach, what)
    # infinite pre-activations: +inf -> cutoff, -inf -> 0 through the clip, themselves without
    bias_inf = bias.copy()
    bias_inf[[2, 9]] = INF, -INF
    got = _np(run(x, w, bias_inf, lay.cutoff))
    assert (got[..., 2] == lay.cutoff).all() and (got[..., 9] == 0.0).all()
    got = _np(run(x, w, bias_inf, 0.0))
    assert (got[..., 2] == INF).all() and (got[..., 9] == -INF).all()
    assert np.isfinite(np.delete(got, [2, 9], axis=3)).all()


@pytest.mark.parametrize('layer', sorted(S12))
@pytest.mark.parametrize('form', [32, 16])
def test_a_nan_reaches_every_output_of_its_receptive_field_in_conv_s12(hip, layer, form):
    """A single NaN in x, in w or in bias - at a border, inside, and in the halo between two
    workgroups' tiles (T = TT + 6: frames TT - 1 and TT are read by both) - is a NaN in every
    output whose receptive field holds it, with the fused clip on and off (the epilogue's
    fminf(fmaxf(v, 0), cutoff) used to turn it into 0, the saturating staging of
    `conv_s12_fwd16` into -65504 / x_scale); every other output keeps the clean run's bits."""
    tile = ref.S12_TT[layer]
    batch, frames = 2, tile + 6

    def run(x, w, bias, cutoff):
        return _s12_forward(hip, layer, form, _t(x), _s12_packs(hip, w), _t(bias), None, cutoff,
                            False)
    _check_forward_nan(run, layer, batch, frames, tile)
    if form == 16:
        # by design: a finite or infinite input beyond the bound saturates to a finite result
        x, w, bias = ref.forward_case(layer, batch, frames)
        x[0, 3, 3, 3], x[1, tile, 5, 5], x[1, 2, 2, 2] = INF, -INF, 1e30
        assert torch.isfinite(run(x, w, bias, 0.0)).all()


@pytest.mark.parametrize('form', [32, 16])
def test_a_nan_reaches_every_output_of_its_receptive_field_in_conv0(hip, form):
    """The same for the first layer at T = 34 (17 output frames, two workgroups; input frames 31
    and 32 are read by both).  `conv0_fwd16` scales each patch by its own largest magnitude,
    found with fmaxf, which ignores a NaN: the other outputs keep their bits there too."""
    batch, frames = 2, 34

    def run(x, w, bias, cutoff):
        if form == 16:
            return hip.conv0_fwd16(_t(x), hip.conv0_pack_weights16(_t(w)), _t(bias),
                                   relu_cutoff=cutoff)
        return hip.conv0_fwd(_t(x), _t(w), _t(bias), relu_cutoff=cutoff)
    _check_forward_nan(run, 'conv0', batch, frames, 32)


GRADIENTS = ['conv_s12_bwd_data', 'conv_s12_bwd_data16', 'conv_s12_wrw', 'conv_s12_wrw16',
             'conv0_wrw', 'conv0_wrw16']


@pytest.mark.parametrize('kernel', GRADIENTS)
@pytest.mark.parametrize('poison', [np.nan, INF, -INF])
def test_a_nan_or_inf_in_dz_reaches_every_gradient_it_touches(hip, kernel, poison):
    """Nothing finite comes out where a non-finite dz went in (the fp16 forms derive scales from
    dz: what an inf does to the REST of their result is not a contract).  For the fp32 data
    gradient a NaN leaves every other element's bits alone."""
    layers = ['conv0'] if kernel.startswith('conv0') else sorted(S12)
    for layer in layers:
        batch, frames = 2, (ref.S12_TT[layer] + 6 if 'bwd_data' in kernel else 7)
        dz, _, x, w = ref.backward_case(layer, batch, frames)
        spots = [(0, 0, 0, 0), (1, dz.shape[1] - 1, dz.shape[2] - 1, dz.shape[3] - 1),
                 (1, dz.shape[1] // 2, 3, 7)]
        if 'bwd_data' in kernel:
            spots.append((0, ref.S12_TT[layer], 4, 20))
            packs = _s12_packs(hip, w)

        def run(dz_np):
            if kernel == 'conv_s12_bwd_data':
                return hip.conv_s12_bwd_data(_t(dz_np), packs[32])
            if kernel == 'conv_s12_bwd_data16':
                return hip.conv_s12_bwd_data16(_t(dz_np), packs[16])
            if kernel == 'conv_s12_wrw':
                return hip.conv_s12_wrw(_t(dz_np), _t(x))
            if kernel == 'conv_s12_wrw16':
                return hip.conv_s12_wrw16(_t(dz_np), _t(x), X_SCALE)
            return getattr(hip, kernel)(_t(dz_np), _t(x))
        clean = run(dz)
        assert torch.isfinite(clean).all()
        for spot in spots:
            bad = dz.copy()
            bad[spot] = poison
            hit = np.zeros(dz.shape)
            hit[spot] = 1
            if 'bwd_data' in kernel:
                reach = ref.reach_of_dz_in_dx(layer, hit, frames)
            else:
                reach = ref.reach_of_dz_in_dw(layer, hit, frames)
            assert reach.any()
            got = run(bad)
            assert not np.isfinite(_np(got)[reach]).any(), (layer, spot)
            if kernel == 'conv_s12_bwd_data' and poison != poison:
                _nan_like_clean(got, clean, reach, (layer, spot))


@pytest.mark.parametrize('conv_f16', ['1', '0'])
@pytest.mark.parametrize('poison', ['conv1/kernel', 'conv0/bias', 'feature'])
def test_a_nan_in_the_conv_stack_drops_the_step(hip, monkeypatch, conv_f16, poison):
    """A NaN in a conv kernel, a conv bias or one feature value reaches the loss on both
    arithmetic paths of the own conv kernels (the conv epilogues used to turn the NaN
    pre-activations into zeros, the fp16 staging a NaN input into a finite one): the step guard
    is set, parameters and moments stay as they were, the deferred check raises."""
    monkeypatch.setenv('CTCASR_CONV_F16', conv_f16)
    from ctc_asr_amd.engine import NanLossDuringTrainingError, Trainer
    from ctc_asr_amd.model import ModelConfig
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32, 96), num_units_dense=32,
                      num_layers_rnn=1, num_units_rnn=64, rnn_cell='lstm', cudnn=True,
                      dense_dropout_rate=0.0)
    trainer = Trainer(cfg, device=DEV, seed=3)
    assert trainer.model.conv_f16 == (conv_f16 == '1')
    rng = np.random.default_rng(5)
    feats = torch.tensor(rng.normal(size=(2, 21, 80)).astype(np.float32))
    flen = torch.tensor([21, 21], dtype=torch.int32)
    labels = [[1, 2, 3], [4, 5]]
    loss = trainer.train_step(feats, flen, labels)
    trainer.drain_checks()
    assert np.isfinite(float(loss)) and trainer.model.step_guard().tolist() == [0, 0]
    arena = trainer.model.arena
    if poison == 'feature':
        feats[1, 10, 40] = float('nan')
    else:
        arena.p[poison][(3, 2, 5, 10) if poison.endswith('kernel') else (7,)] = float('nan')
        arena.touch()
    before = [t.clone().view(torch.int32) for t in (arena.param, arena.m, arena.v)]
    loss = trainer.train_step(feats, flen, labels)
    torch.cuda.synchronize()
    assert not np.isfinite(float(loss))
    assert int(trainer.model.step_guard()[0]) == 1
    for was, now in zip(before, (arena.param, arena.m, arena.v)):
        assert torch.equal(was, now.view(torch.int32))
    with pytest.raises(NanLossDuringTrainingError):
        trainer.drain_checks()


# ============================================================================ refusals
def _refusal_cases(hip):
    """(name, call, sentinel-filled outputs): one wrong argument each; B = 1, T = 2."""
    lib = hip.load()
    rng = np.random.default_rng(1)
    cases = []
    for layer in sorted(S12):
        freq, cout = S12[layer]
        x = _t(ref.int_inputs(rng, (1, 2, freq, 32)))
        dz = _t(ref.int_dz(rng, (1, 2, freq // 2, cout)))
        act = torch.ones_like(dz)
        w = _t(ref.int_weights(rng, layer))
        bias = _t(ref.int_bias(rng, layer))
        packed, packed16 = hip.conv_s12_pack_weights(w), hip.conv_s12_pack_weights16(w)
        assert packed.numel() == hip.conv_s12_packed_floats(cout)
        assert packed16.numel() == lib.ctcasr_conv_s12_pack16_bytes(cout)
        y_n, dx_n, dw_n = dz.numel(), x.numel(), w.numel()

        def add(name, fn, good, outs=('out',), **wrong):
            """`fn(**good)` with `wrong` replacing some arguments; the arguments named in
            `outs` are replaced by guarded buffers (of the right size unless `wrong` says
            otherwise)."""
            cases.append(('{} {} {}'.format(fn.__name__, layer, name), fn, dict(good), outs,
                          wrong))
        fwd = dict(x=x, packed=packed, cout=cout, bias=bias, out=y_n)
        fwd16 = dict(x=x, x_scale=X_SCALE, packed16=packed16, cout=cout, bias=bias, out=y_n)
        for fn, good, pack in ((hip.conv_s12_fwd, fwd, 'packed'),
                               (hip.conv_s12_fwd16, fwd16, 'packed16')):
            add('out one short', fn, good, out=y_n - 1)
            add('out one long', fn, good, out=y_n + 1)
            add('bias', fn, good, bias=bias[:-1])
            add('bias of the other layer', fn, good, bias=torch.zeros(128 - cout, device=DEV))
            add(pack + ' short', fn, good, **{pack: good[pack][:-4]})
            add('x with 3 dimensions', fn, good, x=x.view(2, freq, 32))
            add('x with 5 dimensions', fn, good, x=x.view(1, 1, 2, freq, 32))
            add('x with 31 channels', fn, good, x=x[..., :31].contiguous())
            add('unsupported pair', fn, good, cout=128 - cout)
            add('unsupported frequencies', fn, good, x=x[:, :, :freq - 2].contiguous())
        for scale in (0.0, -2048.0, float('nan'), INF):
            add('x_scale {}'.format(scale), hip.conv_s12_fwd16, fwd16, x_scale=scale)
        bwd = dict(dz=dz, packed=packed, out=dx_n)
        bwd16 = dict(dz=dz, packed16=packed16, out=dx_n)
        for fn, good, pack in ((hip.conv_s12_bwd_data, bwd, 'packed'),
                               (hip.conv_s12_bwd_data16, bwd16, 'packed16')):
            add('out one short', fn, good, out=dx_n - 1)
            add('out one long', fn, good, out=dx_n + 1)
            add(pack + ' long', fn, good,
                **{pack: torch.cat([good[pack], good[pack][:4]])})
            add('act of another shape', fn, good, act=act[:, :1].contiguous(), relu_cutoff=256.0)
            add('act flattened', fn, good, act=act.view(-1), relu_cutoff=256.0)
            add('act without a cutoff', fn, good, act=act)
            add('act with a negative cutoff', fn, good, act=act, relu_cutoff=-1.0)
            add('dz with 3 dimensions', fn, good, dz=dz.view(2, freq // 2, cout))
            add('unsupported pair', fn, good, dz=dz[..., :cout - 16].contiguous())
        wrw = dict(dz=dz, x=x, out=dw_n, dbias=cout)
        wrw16 = dict(dz=dz, x=x, x_scale=X_SCALE, out=dw_n, dbias=cout)
        for fn, good in ((hip.conv_s12_wrw, wrw), (hip.conv_s12_wrw16, wrw16)):
            outs = ('out', 'dbias')
            add('out one short', fn, good, outs, out=dw_n - 1)
            add('out one long', fn, good, outs, out=dw_n + 1)
            add('dbias one short', fn, good, outs, dbias=cout - 1)
            add('dbias one long', fn, good, outs, dbias=cout + 1)
            add('act of another shape', fn, good, outs, act=act[:, :1].contiguous(),
                relu_cutoff=256.0)
            add('act without a cutoff', fn, good, outs, act=act)
            add('dz with 3 dimensions', fn, good, outs, dz=dz.view(2, freq // 2, cout))
            add('x of another length', fn, good, outs, x=x[:, :1].contiguous())
        for scale in (0.0, -1.0, float('nan')):
            add('x_scale {}'.format(scale), hip.conv_s12_wrw16, wrw16, ('out', 'dbias'),
                x_scale=scale)
        add('packed short', hip.conv_s12_pack_weights, dict(weight=w, packed=packed.numel()),
            ('packed',), packed=packed.numel() - 1)
    layer = 'conv0'
    x = _t(ref.int_features(rng, (1, 2, 80)))
    dz = _t(ref.int_dz(rng, (1, 1, 40, 32)))
    act = torch.ones_like(dz)
    w = _t(ref.int_weights(rng, layer))
    bias = _t(ref.int_bias(rng, layer))
    packed16 = hip.conv0_pack_weights16(w)
    assert packed16.numel() == lib.ctcasr_conv0_pack16_bytes()

    def add0(name, fn, good, outs=('out',), **wrong):
        cases.append(('{} {}'.format(fn.__name__, name), fn, dict(good), outs, wrong))
    fwd = dict(x=x, weight=w, bias=bias, out=dz.numel())
    fwd16 = dict(x=x, packed16=packed16, bias=bias, out=dz.numel())
    for fn, good in ((hip.conv0_fwd, fwd), (hip.conv0_fwd16, fwd16)):
        add0('out one short', fn, good, out=dz.numel() - 1)
        add0('out one long', fn, good, out=dz.numel() + 1)
        add0('bias', fn, good, bias=bias[:31])
        add0('x with 2 dimensions', fn, good, x=x.view(2, 80))
        add0('x with 4 dimensions', fn, good, x=x.view(1, 2, 80, 1))
        add0('x with 40 frequencies', fn, good, x=x[..., :40].contiguous())
    add0('packed16 short', hip.conv0_fwd16, fwd16, packed16=packed16[:-16])
    add0('packed16 long', hip.conv0_fwd16, fwd16, packed16=torch.cat([packed16, packed16[:16]]))
    add0('out short', hip.conv0_pack_weights16, dict(weight=w, out=packed16.numel()),
         out=packed16.numel() - 16)
    wrw = dict(dz=dz, x=x, out=w.numel(), dbias=32)
    for fn in (hip.conv0_wrw, hip.conv0_wrw16):
        outs = ('out', 'dbias')
        add0('out one short', fn, wrw, outs, out=w.numel() - 1)
        add0('out one long', fn, wrw, outs, out=w.numel() + 1)
        add0('dbias one short', fn, wrw, outs, dbias=31)
        add0('dbias one long', fn, wrw, outs, dbias=33)
        add0('act of another shape', fn, wrw, outs, act=act[..., :16].contiguous(),
             relu_cutoff=64.0)
        add0('act without a cutoff', fn, wrw, outs, act=act)
        add0('x with 2 dimensions', fn, wrw, outs, x=x.view(2, 80))
        add0('dz of another length', fn, wrw, outs, dz=torch.cat([dz, dz], dim=1))
    return cases


def test_the_conv_wrappers_refuse_arguments_of_the_wrong_size(hip):
    """An `out`, `bias`, `dbias`, `act`, `packed` or `packed16` of the wrong size, x or dz with
    the wrong number of dimensions, a scale or cutoff that is not positive, an unsupported layer:
    `CtcAsrError` before anything is launched - the outputs keep their NaN words.  The same
    arguments without the wrong one run (so it is the wrong one that is refused)."""
    cases = _refusal_cases(hip)
    assert len(cases) > 100
    ran = set()
    for name, fn, good, outs, wrong in cases:
        def materialise(args):
            bufs = []
            for key in outs:
                size = args[key]
                dtype_words = size if fn.__name__ != 'conv0_pack_weights16' else size // 4
                buf, view = _guarded((dtype_words,))
                args[key] = view.view(torch.uint8) if dtype_words != size else view
                bufs.append(buf)
            return bufs
        if fn.__name__ not in ran:              # the good call, once per wrapper
            args = dict(good)
            bufs = materialise(args)
            fn(**args)
            assert all(_guards_intact(buf) for buf in bufs) and not _untouched(bufs[0]), name
            ran.add(fn.__name__)
        args = dict(good)
        args.update(wrong)
        bufs = materialise(args)
        with pytest.raises(hip.CtcAsrError):
            fn(**args)
        torch.cuda.synchronize()
        assert all(_untouched(buf) for buf in bufs), name
    assert len(ran) == 12


def test_conv0_forward_refuses_a_batch_beyond_the_grid(hip):
    """B = 65536 at T = 1 does not fit the launch grid's second axis: CTCASR_ERR_UNSUPPORTED
    from the library, nothing written."""
    x = torch.zeros(65536, 1, 80, device=DEV)
    w = _t(ref.int_weights(np.random.default_rng(0), 'conv0'))
    for form in (32, 16):
        buf, out = _guarded((65536, 1, 40, 32))
        with pytest.raises(hip.CtcAsrError):
            if form == 16:
                hip.conv0_fwd16(x, hip.conv0_pack_weights16(w), out=out)
            else:
                hip.conv0_fwd(x, w, out=out)
        torch.cuda.synchronize()
        assert _untouched(buf)
    # the largest batch that does fit runs, and is exact
    x = _t(ref.int_features(np.random.default_rng(2), (65535, 1, 80)))
    got = hip.conv0_fwd(x, w)
    want = ref.forward('conv0', _np(x)[-3:], _np(w))
    assert _exact(got[-3:], want) and _exact(got[:3], ref.forward('conv0', _np(x)[:3], _np(w)))
