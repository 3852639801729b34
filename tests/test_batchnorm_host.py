"""What of the sequence-wise batch normalisation (include/ctcasr.h K20, --rnn_batch_norm) can be
checked without a GPU: the numpy restatement (tests/batchnorm_reference.py) against
``torch.nn.functional.batch_norm`` and autograd in float64, the parameter layout with the flag off
and on, the flags, the checkpoints of either kind, the refused TensorFlow checkpoints, and the
new exports with their argument checks through the host side of the cross-compiled library."""

import os
import types

import numpy as np
import pytest
import torch

from ctc_asr_amd import params, storage
from ctc_asr_amd.model import GATES, ModelConfig, ParamArena, init_params, param_spec, \
    predicted_input_bounds
from ctc_asr_amd.params import FLAGS
from tests import batchnorm_reference as ref


@pytest.fixture(autouse=True)
def _fresh_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    return hip.load()


# ---- 1. the yardstick against an independent implementation ------------------------------------
@pytest.mark.parametrize('lengths', [None, [7, 7, 7], [7, 0, 4], [9, 3, 1]])
def test_restatement_against_torch_batch_norm(lengths):
    """float64 throughout (``pinned=False``): y, dx, dgamma, dbeta and the running update on the
    counted rows agree with F.batch_norm + autograd to 1e-12; uncounted rows are zero."""
    rng = np.random.default_rng(5)
    steps, batch, channels = 7, 3, 8
    x = rng.normal(size=(steps, batch, channels)) * 2.0 + 3.0
    dy = rng.normal(size=x.shape)
    gamma, beta = rng.normal(size=channels) + 1.5, rng.normal(size=channels)
    run_mean, run_var = rng.normal(size=channels), rng.uniform(0.5, 2.0, size=channels)
    fwd = ref.forward(x, lengths, gamma, beta, run_mean, run_var, 0.9, rows_per_chunk=4,
                      pinned=False)
    bwd = ref.backward(dy, x, lengths, fwd['mean'], fwd['rstd'], gamma, rows_per_chunk=4,
                       pinned=False)
    mask = ref.counted(steps, batch, lengths)
    assert fwd['n'] == int(mask.sum()) == (21 if lengths is None else
                                          int(np.clip(lengths, 0, steps).sum()))

    tx = torch.tensor(x[mask], requires_grad=True)                    # [N, C]
    tg, tb = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    t_mean, t_var = torch.tensor(run_mean), torch.tensor(run_var)
    ty = torch.nn.functional.batch_norm(tx, t_mean, t_var, tg, tb, training=True,
                                        momentum=1.0 - 0.9, eps=ref.EPS)
    (ty * torch.tensor(dy[mask])).sum().backward()
    assert np.abs(fwd['y'][mask] - ty.detach().numpy()).max() < 1e-12
    assert np.abs(bwd['dx'][mask] - tx.grad.numpy()).max() < 1e-12
    assert np.abs(bwd['dgamma'] - tg.grad.numpy()).max() < 1e-12
    assert np.abs(bwd['dbeta'] - tb.grad.numpy()).max() < 1e-12
    assert (fwd['y'][~mask] == 0).all() and (bwd['dx'][~mask] == 0).all()
    assert np.abs(fwd['running_mean'] - t_mean.numpy()).max() < 1e-12
    # (torch moves the running variance by the UNBIASED batch variance, TensorFlow - and this
    # package - by the population variance)
    n = fwd['n']
    assert np.abs(fwd['running_var'] -
                  (0.9 * run_var + 0.1 * (t_var.numpy() - 0.9 * run_var) / 0.1 * (n - 1) / n)) \
        .max() < 1e-12
    # running-statistics mode
    y_run, _ = ref.infer(x, lengths, gamma, beta, run_mean, run_var, pinned=False)
    ty = torch.nn.functional.batch_norm(torch.tensor(x[mask]), torch.tensor(run_mean),
                                        torch.tensor(run_var), tg, tb, training=False, eps=ref.EPS)
    assert np.abs(y_run[mask] - ty.detach().numpy()).max() < 1e-12


def test_the_pinned_roundings_stay_inside_their_own_bounds():
    """The fp32 roundings the contract names move the restatement by less than the bounds it
    hands to the kernel tests; the chunk length moves the float64 sums by rounding only."""
    rng = np.random.default_rng(6)
    x = (rng.normal(size=(9, 4, 8)) + 1000.0).astype(np.float32)
    dy = rng.normal(size=x.shape).astype(np.float32)
    gamma = (rng.normal(size=8) + 1.5).astype(np.float32)
    beta = rng.normal(size=8).astype(np.float32)
    lengths = [9, 5, 0, 12]
    exact = ref.forward(x, lengths, gamma, beta, np.zeros(8), np.ones(8), 0.99, pinned=False)
    for rows in (1, 5, 64):
        got = ref.forward(x, lengths, gamma, beta, np.zeros(8), np.ones(8), 0.99,
                          rows_per_chunk=rows)
        assert (np.abs(got['mean'] - exact['mean']) <= ref.ulp32(exact['mean'])).all()
        assert (np.abs(got['rstd'] - exact['rstd']) <= ref.ulp32(exact['rstd'])).all()
        assert (np.abs(got['y'] - exact['y']) <= got['y_bound']).all()
        assert got['n'] == 23         # 9 + 5 + 0 + min(12, 9)
    # (backward: on data around zero - at 1000 the fp32 rounding of the saved mean alone moves
    # xhat by 2^-14 of a standard deviation, which is the contract's price, not a rounding of the
    # backward pass)
    x = (x - 1000.0).astype(np.float32)
    exact = ref.forward(x, lengths, gamma, beta, np.zeros(8), np.ones(8), 0.99, pinned=False)
    got = ref.forward(x, lengths, gamma, beta, np.zeros(8), np.ones(8), 0.99)
    bwd_exact = ref.backward(dy, x, lengths, exact['mean'], exact['rstd'], gamma, pinned=False)
    bwd = ref.backward(dy, x, lengths, got['mean'], got['rstd'], gamma)
    assert (np.abs(bwd['dgamma'] - bwd_exact['dgamma']) <= 2 * bwd['dgamma_bound']).all()
    assert (np.abs(bwd['dbeta'] - bwd_exact['dbeta']) <= ref.ulp32(bwd_exact['dbeta'])).all()
    # N == 0 and N == 1 as pinned
    none = ref.forward(x, [0, 0, 0, 0], gamma, beta, np.zeros(8), np.ones(8), 0.99)
    assert none['n'] == 0 and (none['y'] == 0).all() and (none['mean'] == 0).all()
    assert (none['rstd'] == 0).all() and (none['running_var'] == 1).all()
    one = ref.forward(x, [0, 1, 0, 0], gamma, beta, np.zeros(8), np.ones(8), 0.99)
    assert one['n'] == 1 and (one['var64'] == 0).all()
    assert (one['y'][0, 1] == beta).all() and (one['mean'] == x[0, 1]).all()


# ---- 2. the parameter layout --------------------------------------------------------------------
def _small(**kwargs):
    return ModelConfig(used_model='ds2', conv_filters=(4, 6), num_units_dense=10,
                       num_layers_rnn=3, num_units_rnn=5, rnn_cell='lstm', cudnn=True,
                       num_classes_=29, **kwargs)


def _todays_spec(cfg):
    """The layout of a model without the flag, written out independently of `param_spec`."""
    gh, hidden = GATES[cfg.cell] * cfg.num_units_rnn, cfg.num_units_rnn
    spec = [('conv0/kernel', (11, 41, 1, 4)), ('conv0/bias', (4,)),
            ('conv1/kernel', (11, 21, 4, 6)), ('conv1/bias', (6,))]
    in_size = 20 * 6                # 80 features halved twice, 6 channels
    for i in range(3):
        spec += [('rnn{}/w_ih'.format(i), (2, gh, in_size)), ('rnn{}/w_hh'.format(i), (2, gh, hidden)),
                 ('rnn{}/b_ih'.format(i), (2, gh)), ('rnn{}/b_hh'.format(i), (2, gh))]
        in_size = 2 * hidden
    return spec + [('dense4/kernel', (10, 10)), ('dense4/bias', (10,)),
                   ('logits/kernel', (10, 29)), ('logits/bias', (29,))]


def _offsets(spec):
    out, cursor = {}, 0
    for name, shape in spec:
        out[name] = cursor
        cursor += (int(np.prod(shape)) + 3) // 4 * 4
    return out, cursor


def test_the_layout_with_the_flag_off_is_todays():
    for cfg in (_small(), _small(rnn_batch_norm=False, rnn_bn_decay=0.5)):
        want = _todays_spec(cfg)
        assert param_spec(cfg) == want
        arena = ParamArena(cfg, 'cpu')
        offsets, size = _offsets(want)
        assert arena.offsets == offsets and arena.size == size
        assert list(arena.offsets) == [name for name, _ in want]
        assert [name for name, _, _ in arena.layer_slices] == \
            ['conv0', 'conv1', 'rnn0', 'rnn1', 'rnn2', 'dense4', 'logits']
        assert not any('bn_' in name for name in init_params(cfg, 0))
    assert ModelConfig().rnn_batch_norm is False and ModelConfig().rnn_bn_decay == 0.99


def test_the_layout_with_the_flag_on():
    cfg = _small(rnn_batch_norm=True)
    spec = param_spec(cfg)
    names = [name for name, _ in spec]
    want = []
    for name, shape in _todays_spec(cfg):
        layer = name.split('/')[0]
        if name.endswith('w_ih') and layer != 'rnn0':
            want += [(layer + '/bn_gamma', (10,)), (layer + '/bn_beta', (10,))]
        want.append((name, shape))
    assert spec == want
    assert 'rnn0/bn_gamma' not in names and 'rnn0/bn_beta' not in names
    arena = ParamArena(cfg, 'cpu')
    slices = {name: (start, stop) for name, start, stop in arena.layer_slices}
    assert list(slices) == ['conv0', 'conv1', 'rnn0', 'rnn1', 'rnn2', 'dense4', 'logits']
    for layer in ('rnn1', 'rnn2'):
        start, stop = slices[layer]
        assert arena.offsets[layer + '/bn_gamma'] == start          # in front of the weights
        assert arena.offsets[layer + '/bn_beta'] == start + 12      # (10 floats, 16-byte slots)
        assert arena.offsets[layer + '/w_ih'] == start + 24
        assert start < arena.offsets[layer + '/b_hh'] < stop
        assert arena.offsets[layer + '/bn_gamma'] % 4 == 0
    flat = init_params(cfg, 0)
    assert (flat['rnn1/bn_gamma'] == 1).all() and (flat['rnn2/bn_beta'] == 0).all()
    assert flat['rnn1/bn_gamma'].dtype == np.float32 and flat['rnn1/bn_gamma'].shape == (10,)
    # every other tensor is drawn as without the flag
    plain = init_params(_small(), 0)
    assert all((flat[name] == plain[name]).all() for name in plain)
    # a normalised input has no bound: the projection takes the row-scaled fp16 form or bf16x6
    assert predicted_input_bounds(cfg, True) == [20.0, None, None, 1.0]
    assert predicted_input_bounds(_small(), True) == [20.0, 1.0, 1.0, 1.0]


# ---- 3. flags -----------------------------------------------------------------------------------
def test_flags_and_refusals():
    defaults = FLAGS.defaults_dict()
    assert (defaults['rnn_batch_norm'], defaults['rnn_bn_decay']) == (False, 0.99)
    for argv in (['--rnn_bn_decay=0'], ['--rnn_bn_decay=1'], ['--rnn_bn_decay=1.5'],
                 ['--rnn_bn_decay=-0.1'], ['--rnn_bn_decay=nan'], ['--rnn_bn_decay=much']):
        FLAGS.reset()
        with pytest.raises(ValueError):
            FLAGS.parse(argv)
    FLAGS.reset()
    cfg = ModelConfig.from_flags(FLAGS)
    assert cfg.rnn_batch_norm is False and cfg.rnn_bn_decay == 0.99
    assert 'BatchNorm' not in params.get_parameters()
    assert FLAGS.parse(['--rnn_batch_norm', '--rnn_bn_decay=0.9']) == []
    cfg = ModelConfig.from_flags(FLAGS)
    assert cfg.rnn_batch_norm is True and cfg.rnn_bn_decay == 0.9
    assert '\tBatchNorm (rnn_batch_norm=True, rnn_bn_decay=0.9);' in \
        params.get_parameters().split('\n')
    with pytest.raises(ValueError, match='rnn_bn_decay'):
        ModelConfig(rnn_batch_norm=True, rnn_bn_decay=1.0)
    # flags objects written before the flag existed still build a model
    old = types.SimpleNamespace(**{k: v for k, v in FLAGS.defaults_dict().items()
                                   if not k.startswith('rnn_b')})
    assert ModelConfig.from_flags(old).rnn_batch_norm is False


# ---- 4. checkpoints -----------------------------------------------------------------------------
def _model(cfg, seed):
    arena = ParamArena(cfg, 'cpu')
    gen = torch.Generator().manual_seed(seed)
    for tensor in (arena.param, arena.m, arena.v):
        tensor.copy_(torch.randn(arena.size, generator=gen))
    bn_state = None
    if cfg.rnn_batch_norm:
        bn_state = torch.rand((cfg.num_layers_rnn - 1, 2, 2 * cfg.num_units_rnn), generator=gen)
    return types.SimpleNamespace(arena=arena, step_count=3 + seed, dropout_seed=9 + seed,
                                 bn_state=bn_state, cfg=cfg)


def test_checkpoints_carry_the_running_statistics_and_refuse_the_other_kind(tmp_path):
    on, off = _small(rnn_batch_norm=True), _small()
    src = _model(on, 1)
    path = storage.save_checkpoint(str(tmp_path / 'on'), src, epoch=2)
    assert torch.equal(torch.load(path, weights_only=False)['bn_state'], src.bn_state)
    dst = _model(on, 2)
    assert storage.restore_checkpoint(path, dst) == 2
    assert torch.equal(dst.bn_state, src.bn_state) and torch.equal(dst.arena.param, src.arena.param)
    with pytest.raises(ValueError, match='different network layout'):
        storage.restore_checkpoint(path, _model(off, 3))
    plain = _model(off, 4)
    path_off = storage.save_checkpoint(str(tmp_path / 'off'), plain, epoch=1)
    assert 'bn_state' not in torch.load(path_off, weights_only=False)
    with pytest.raises(ValueError, match='different network layout'):
        storage.restore_checkpoint(path_off, _model(on, 5))
    assert storage.restore_checkpoint(path_off, _model(off, 6)) == 1


def test_tensorflow_checkpoints_are_refused_with_the_flag_on(tmp_path):
    cfg = _small(rnn_batch_norm=True)
    arena = ParamArena(cfg, 'cpu')
    with pytest.raises(ValueError, match='rnn_batch_norm'):
        storage.export_tf_checkpoint(str(tmp_path), arena, cfg, 1)
    with pytest.raises(ValueError, match='rnn_batch_norm'):
        storage.import_tf_checkpoint(str(tmp_path), arena, cfg)
    assert list(tmp_path.iterdir()) == []


# ---- 5. the exports -----------------------------------------------------------------------------
def test_the_library_exports_the_entry_points(lib):
    from ctc_asr_amd import hip
    for name in ('ctcasr_seq_bn_workspace_bytes', 'ctcasr_seq_bn_fwd', 'ctcasr_seq_bn_infer',
                 'ctcasr_seq_bn_bwd'):
        assert name in hip.SIGNATURES and getattr(lib, name) is not None
    assert lib.ctcasr_abi_version() == 8
    rows = hip.SEQ_BN_ROWS
    assert 32 <= rows <= 64
    header = open(os.path.join(os.path.dirname(os.path.dirname(hip.LIB_PATH)), 'include',
                               'ctcasr.h')).read()
    assert '#define CTCASR_SEQ_BN_ROWS {}\n'.format(rows) in header
    # chunk sums [chunks][2][C] float64, then two floats per channel
    for n, channels in ((1, 4), (rows, 4), (rows + 1, 4), (3 * rows + 5, 4100), (16000, 2048)):
        chunks = -(-n // rows)
        assert hip.seq_bn_workspace_bytes(n, channels) == chunks * 2 * channels * 8 + 8 * channels
    for n, channels in ((0, 4), (-1, 4), (2 ** 31, 4), (8, 0), (8, 2), (8, 6), (8, -4)):
        assert hip.seq_bn_workspace_bytes(n, channels) == 0
    assert lib.ctcasr_set_option(b'seq_bn_blocks', 7) == 0
    assert lib.ctcasr_set_option(b'seq_bn_blocks', 0) == 0
    assert lib.ctcasr_set_option(b'seq_bn_blocks', -1) == -1
    assert lib.ctcasr_set_option(b'seq_bn_blocks', 65537) == -1


def test_the_abi_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every call below has to return before it touches the device.  The pointers
    are made-up addresses."""
    x, y, ws, vec = 0x10000, 0x20000, 0x30000, 0x40000
    need = lib.ctcasr_seq_bn_workspace_bytes(6, 8)
    good = dict(x=x, lengths=None, T=3, B=2, C=8, gamma=vec, beta=vec + 64, rm=vec + 128,
                rv=vec + 192, decay=0.99, eps=1e-5, y=y, mean=vec + 256, rstd=vec + 320, ws=ws,
                ws_bytes=need, dy=0x50000, dgamma=vec + 384, dbeta=vec + 448)

    def fwd(**change):
        v = dict(good, **change)
        return lib.ctcasr_seq_bn_fwd(v['x'], v['lengths'], v['T'], v['B'], v['C'], v['gamma'],
                                     v['beta'], v['rm'], v['rv'], v['decay'], v['eps'], v['y'],
                                     v['mean'], v['rstd'], v['ws'], v['ws_bytes'], None)

    def infer(**change):
        v = dict(good, **change)
        return lib.ctcasr_seq_bn_infer(v['x'], v['lengths'], v['T'], v['B'], v['C'], v['gamma'],
                                       v['beta'], v['rm'], v['rv'], v['eps'], v['y'], None)

    def bwd(**change):
        v = dict(good, **change)
        return lib.ctcasr_seq_bn_bwd(v['dy'], v['x'], v['lengths'], v['T'], v['B'], v['C'],
                                     v['mean'], v['rstd'], v['gamma'], v['dgamma'], v['dbeta'],
                                     v['y'], v['ws'], v['ws_bytes'], None)

    shapes = (dict(C=0), dict(C=2), dict(C=6), dict(C=-8), dict(T=0), dict(B=0), dict(T=-1),
              dict(T=65536, B=32768))
    for call, pointers in ((fwd, ('x', 'gamma', 'beta', 'rm', 'rv', 'y', 'mean', 'rstd')),
                           (infer, ('x', 'gamma', 'beta', 'rm', 'rv', 'y')),
                           (bwd, ('dy', 'x', 'mean', 'rstd', 'gamma', 'dgamma', 'dbeta', 'y'))):
        for name in pointers:
            assert call(**{name: None}) == -1, (call.__name__, name)
        for change in shapes + (dict(x=x + 4), dict(x=x + 8), dict(y=y + 4)):
            assert call(**change) == -1, (call.__name__, change)
    assert bwd(dy=0x50000 + 4) == -1
    for change in (dict(decay=-0.1), dict(decay=1.5), dict(decay=float('nan')), dict(eps=0.0),
                   dict(eps=-1e-5), dict(eps=float('inf')), dict(eps=float('nan'))):
        assert fwd(**change) == -1, change
    for change in (dict(eps=0.0), dict(eps=float('nan'))):
        assert infer(**change) == -1, change
    for call in (fwd, bwd):
        for change in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=ws + 4)):
            assert call(**change) == -3, (call.__name__, change)


def test_the_wrappers_refuse_before_the_device(lib):
    from ctc_asr_amd import hip
    vec = torch.zeros(8)
    with pytest.raises(hip.CtcAsrError, match='dimensions'):
        hip.seq_bn_infer(torch.zeros(6, 8), None, vec, vec, vec, vec, 1e-5)
    with pytest.raises(hip.CtcAsrError, match='multiple of 4'):
        hip.seq_bn_infer(torch.zeros(3, 2, 6), None, vec, vec, vec, vec, 1e-5)
    with pytest.raises(hip.CtcAsrError, match='empty'):
        hip.seq_bn_infer(torch.zeros(0, 2, 8), None, vec, vec, vec, vec, 1e-5)
    with pytest.raises(hip.CtcAsrError, match='gamma holds 4 elements'):
        hip.seq_bn_infer(torch.zeros(3, 2, 8), None, vec[:4], vec, vec, vec, 1e-5)
    with pytest.raises(hip.CtcAsrError, match='lengths holds 3 elements'):
        hip.seq_bn_infer(torch.zeros(3, 2, 8), torch.zeros(3, dtype=torch.int32), vec, vec, vec,
                         vec, 1e-5)
    with pytest.raises(hip.CtcAsrError, match='dy has shape'):
        hip.seq_bn_bwd(torch.zeros(3, 2, 4), torch.zeros(3, 2, 8), None, vec, vec, vec, vec, vec)
    with pytest.raises(hip.CtcAsrError, match='CPU tensor'):
        hip.seq_bn_infer(torch.zeros(3, 2, 8), None, vec, vec, vec, vec, 1e-5)
