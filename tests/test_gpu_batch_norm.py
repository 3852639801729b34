"""The sequence-wise batch normalisation kernels (include/ctcasr.h K20, csrc/seq_bn.hip) against
the numpy float64 restatement (tests/batchnorm_reference.py) at the smallest shapes that can go
wrong: one lane group (C = 4), the channel-tile seam (a workgroup covers 1024 channels: C = 1028
puts one lane into the second tile), a ragged last tile (4100), and 1, 2, ROWS - 1, ROWS, ROWS + 1
and 3 ROWS + 5 rows over several (T, B) factorizations, B = 1 and T = 1 among them.

Tolerances are derived, not tuned (the restatement computes every bound from the inputs and its
own values): mean, rstd, the running values and dbeta are fp64 results rounded once - one fp32 ulp;
y within 2^-22 (|a| (|x| + |mean|) + |beta|); dx within 2^-22 (|a| (|dy| + |m1| + |xhat m2|) +
|dx|); dgamma within 2^-22 sum |dy xhat|.

Where the one-pass variance ends.  var64 = S2 / N - mean64^2 loses mean^2 / var of its 2^53: its
relative error is about 2^-52 mean^2 / var, and rstd carries half of that.  rstd stays within one
fp32 ulp (2^-24) while mean^2 / var stays well below 2^29; the data `1000 + N(0, 1)` puts the
ratio at 10^6 (2^20), where the error is 2^-33 - tested below against a two-pass variance.  At
mean = 10^6 and unit variance (2^40) rstd would be off by 2^-13: inputs of a recurrent layer
(|h| <= 1, or a ReLU cell's activations) are nowhere near."""

import numpy as np
import pytest
import torch

from tests import batchnorm_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DECAY = 0.9


def _rows():
    from ctc_asr_amd import hip
    return hip.SEQ_BN_ROWS


def _shapes():
    """(T, B) factorizations of 1, 2, ROWS - 1, ROWS, ROWS + 1 and 3 ROWS + 5 rows."""
    rows = _rows()
    out = [(1, 1), (2, 1), (1, 2)]
    for n in (rows - 1, rows, rows + 1, 3 * rows + 5):
        out += [(n, 1), (1, n)]
        out += [(n // d, d) for d in (3, 5, 7, 8) if n % d == 0][:1]
    return out


def _lengths(kind, steps, batch, rng):
    if kind == 'none':
        return None
    if kind == 'full':
        return np.full(batch, steps, dtype=np.int32)
    if kind == 'zero':
        return np.zeros(batch, dtype=np.int32)
    out = rng.integers(0, steps + 1, size=batch).astype(np.int32)       # 'mixed'
    out[0] = steps + 3                  # above T: clamped
    if batch > 1:
        out[-1] = 0
    if batch > 2:
        out[1] = -2                     # below 0: clamped
    return out


def _dev(array, dtype=torch.float32):
    return None if array is None else torch.tensor(np.asarray(array), dtype=dtype, device=DEV)


def _f64(tensor):
    return tensor.detach().cpu().numpy().astype(np.float64)


def _is_plus_zero(tensor, mask):
    """Every element of the uncounted rows is +0.0 bit for bit."""
    bits = tensor.detach().cpu().numpy().view(np.int32)
    return bool((bits[~mask] == 0).all())


def _within_ulp(got, want):
    got = _f64(got) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    return bool((np.abs(got - want) <= ref.ulp32(want)).all())


def _data(rng, steps, batch, channels, offset):
    x = (rng.normal(size=(steps, batch, channels)) + offset).astype(np.float32)
    dy = rng.normal(size=x.shape).astype(np.float32)
    gamma = (rng.normal(size=channels) * 0.5 + 1.5).astype(np.float32)
    beta = rng.normal(size=channels).astype(np.float32)
    run_mean = rng.normal(size=channels).astype(np.float32)
    run_var = rng.uniform(0.5, 2.0, size=channels).astype(np.float32)
    return x, dy, gamma, beta, run_mean, run_var


def _check(hip, x, dy, lengths, gamma, beta, run_mean, run_var, what):
    """One forward, one inference and one backward call against the restatement."""
    rows = hip.SEQ_BN_ROWS
    want = ref.forward(x, lengths, gamma, beta, run_mean, run_var, DECAY, rows_per_chunk=rows)
    mask = want['mask']
    d_len = _dev(lengths, torch.int32)
    d_x, d_gamma, d_beta = _dev(x), _dev(gamma), _dev(beta)
    d_mean, d_var = _dev(run_mean), _dev(run_var)
    y, mean, rstd = hip.seq_bn_fwd(d_x, d_len, d_gamma, d_beta, d_mean, d_var, DECAY, ref.EPS)
    assert torch.equal(d_x.view(torch.int32), _dev(x).view(torch.int32)), what   # only read
    assert _within_ulp(mean, want['mean']) and _within_ulp(rstd, want['rstd']), what
    assert _within_ulp(d_mean, want['running_mean']), what
    assert _within_ulp(d_var, want['running_var']), what
    err = np.abs(_f64(y) - want['y'])
    print('{}: N = {}, max y error / bound {:.3f}'.format(
        what, want['n'], float((err / np.maximum(want['y_bound'], 1e-300))[mask].max())
        if want['n'] else 0.0))
    assert (err <= want['y_bound']).all(), what
    assert _is_plus_zero(y, mask), what

    y_run, run_bound = ref.infer(x, lengths, gamma, beta, run_mean, run_var)
    got = hip.seq_bn_infer(d_x, d_len, d_gamma, d_beta, _dev(run_mean), _dev(run_var), ref.EPS)
    assert (np.abs(_f64(got) - y_run) <= run_bound).all(), what
    assert _is_plus_zero(got, mask), what

    # backward from the restatement's saved statistics: the pass on its own
    back = ref.backward(dy, x, lengths, want['mean'], want['rstd'], gamma, rows_per_chunk=rows)
    dgamma = torch.zeros(x.shape[2], dtype=torch.float32, device=DEV)
    dbeta = torch.zeros_like(dgamma)
    dx = hip.seq_bn_bwd(_dev(dy), d_x, d_len, _dev(want['mean']), _dev(want['rstd']), d_gamma,
                        dgamma, dbeta)
    assert _within_ulp(dbeta, back['dbeta']), what
    assert (np.abs(_f64(dgamma) - back['dgamma']) <= back['dgamma_bound']).all(), what
    err = np.abs(_f64(dx) - back['dx'])
    assert (err <= back['dx_bound']).all(), what
    assert _is_plus_zero(dx, mask), what
    return want, back


@pytest.mark.parametrize('offset', [0.0, 1000.0])
@pytest.mark.parametrize('channels', [4, 128, 1028, 2048, 4100])
def test_kernels_against_the_restatement(hip, channels, offset):
    rng = np.random.default_rng(channels + int(offset))
    for steps, batch in _shapes():
        data = _data(rng, steps, batch, channels, offset)
        for kind in ('none', 'full', 'mixed', 'zero'):
            lengths = _lengths(kind, steps, batch, rng)
            _check(hip, data[0], data[1], lengths, *data[2:],
                   what='C={} T={} B={} lengths={} offset={}'.format(channels, steps, batch, kind,
                                                                     offset))


def test_one_pass_variance_against_two_passes_at_a_ratio_of_a_million(hip):
    """mean^2 / var = 10^6: the saved rstd is within one fp32 ulp of the two-pass float64 value."""
    rng = np.random.default_rng(11)
    steps, batch, channels = 3 * _rows() + 5, 1, 128
    x, _, gamma, beta, run_mean, run_var = _data(rng, steps, batch, channels, 1000.0)
    _, mean, rstd = hip.seq_bn_fwd(_dev(x), None, _dev(gamma), _dev(beta), _dev(run_mean),
                                   _dev(run_var), DECAY, ref.EPS)
    flat = x.astype(np.float64).reshape(-1, channels)
    two_pass = 1.0 / np.sqrt(flat.var(axis=0) + ref.EPS)
    ratio = flat.mean(axis=0) ** 2 / flat.var(axis=0)
    assert 5e5 < ratio.min() and ratio.max() < 2e6
    assert _within_ulp(rstd, ref.f32(two_pass)) and _within_ulp(mean, ref.f32(flat.mean(axis=0)))


def test_nan_outside_the_counted_rows_and_inside_one_channel(hip):
    rng = np.random.default_rng(12)
    steps, batch, channels = _rows() + 1, 3, 1028
    x, dy, gamma, beta, run_mean, run_var = _data(rng, steps, batch, channels, 0.0)
    lengths = np.array([steps, 5, 0], dtype=np.int32)
    mask = ref.counted(steps, batch, lengths)
    clean = _check(hip, x, dy, lengths, gamma, beta, run_mean, run_var, 'clean')
    # NaN (and inf) where nothing is counted: the outputs there are +0.0, everything else as before
    x_bad, dy_bad = x.copy(), dy.copy()
    x_bad[~mask] = np.nan
    dy_bad[~mask] = np.inf
    x_bad[7, 1, :] = np.nan
    dirty = _check(hip, x_bad, dy_bad, lengths, gamma, beta, run_mean, run_var, 'NaN outside')
    for key in ('mean', 'rstd', 'running_mean', 'running_var'):
        assert (clean[0][key] == dirty[0][key]).all(), key
    # one NaN in a counted element of channel 1025 (the second channel tile)
    x_nan = x.copy()
    x_nan[2, 1, 1025] = np.nan
    d_mean, d_var = _dev(run_mean), _dev(run_var)
    y, mean, rstd = hip.seq_bn_fwd(_dev(x_nan), _dev(lengths, torch.int32), _dev(gamma),
                                   _dev(beta), d_mean, d_var, DECAY, ref.EPS)
    y = y.cpu().numpy()
    assert np.isnan(y[:, :, 1025][mask]).all() and (y[:, :, 1025][~mask] == 0).all()
    assert np.isnan(mean.cpu().numpy()[1025])
    others = np.arange(channels) != 1025
    assert np.isfinite(y[:, :, others]).all()
    y_clean, _, _ = hip.seq_bn_fwd(_dev(x), _dev(lengths, torch.int32), _dev(gamma), _dev(beta),
                                   _dev(run_mean), _dev(run_var), DECAY, ref.EPS)
    assert (y[:, :, others] == y_clean.cpu().numpy()[:, :, others]).all()
    # its running values are left alone, every other channel's move
    assert d_mean.cpu().numpy()[1025] == run_mean[1025]
    assert d_var.cpu().numpy()[1025] == run_var[1025]
    assert (d_mean.cpu().numpy()[others] != run_mean[others]).all()
    assert _within_ulp(_f64(d_mean)[others], clean[0]['running_mean'][others])
    assert _within_ulp(_f64(d_var)[others], clean[0]['running_var'][others])


def test_gradients_are_added_to_what_the_arena_holds(hip):
    rng = np.random.default_rng(13)
    steps, batch, channels = 9, 4, 132
    x, dy, gamma, beta, run_mean, run_var = _data(rng, steps, batch, channels, 0.0)
    lengths = _dev(np.array([9, 4, 0, 7]), torch.int32)
    _, mean, rstd = hip.seq_bn_fwd(_dev(x), lengths, _dev(gamma), _dev(beta), _dev(run_mean),
                                   _dev(run_var), DECAY, ref.EPS)
    zero_g = torch.zeros(channels, dtype=torch.float32, device=DEV)
    zero_b = torch.zeros_like(zero_g)
    dx0 = hip.seq_bn_bwd(_dev(dy), _dev(x), lengths, mean, rstd, _dev(gamma), zero_g, zero_b)
    prior_g = _dev(rng.normal(size=channels) * 3.0)
    prior_b = _dev(rng.normal(size=channels) * 3.0)
    dgamma, dbeta = prior_g.clone(), prior_b.clone()
    dx1 = hip.seq_bn_bwd(_dev(dy), _dev(x), lengths, mean, rstd, _dev(gamma), dgamma, dbeta)
    # one fp32 addition of the rounded sum to the prior content
    assert torch.equal(dgamma, prior_g + zero_g) and torch.equal(dbeta, prior_b + zero_b)
    assert zero_g.abs().max() > 0 and zero_b.abs().max() > 0
    assert torch.equal(dx0.view(torch.int32), dx1.view(torch.int32))


def test_equal_bits_from_call_to_call_and_from_grid_to_grid(hip):
    rng = np.random.default_rng(14)
    steps, batch, channels = 3 * _rows() + 5, 3, 2052
    x, dy, gamma, beta, run_mean, run_var = _data(rng, steps, batch, channels, 1000.0)
    lengths = _dev(np.array([steps, steps // 2, 1]), torch.int32)

    def run():
        d_mean, d_var = _dev(run_mean), _dev(run_var)
        y, mean, rstd = hip.seq_bn_fwd(_dev(x), lengths, _dev(gamma), _dev(beta), d_mean, d_var,
                                       DECAY, ref.EPS)
        y_run = hip.seq_bn_infer(_dev(x), lengths, _dev(gamma), _dev(beta), _dev(run_mean),
                                 _dev(run_var), ref.EPS)
        dgamma = torch.zeros(channels, dtype=torch.float32, device=DEV)
        dbeta = torch.zeros_like(dgamma)
        dx = hip.seq_bn_bwd(_dev(dy), _dev(x), lengths, mean, rstd, _dev(gamma), dgamma, dbeta)
        return [t.view(torch.int32).clone() for t in (y, mean, rstd, d_mean, d_var, y_run, dx,
                                                      dgamma, dbeta)]

    first = run()
    assert all(torch.equal(a, b) for a, b in zip(first, run()))
    try:
        for blocks in (1, 3, 7, 65536):
            hip.set_option('seq_bn_blocks', blocks)
            assert all(torch.equal(a, b) for a, b in zip(first, run())), blocks
    finally:
        hip.set_option('seq_bn_blocks', 0)


def test_no_counted_row_and_one_counted_row(hip):
    rng = np.random.default_rng(15)
    steps, batch, channels = 5, 3, 8
    x, dy, gamma, beta, run_mean, run_var = _data(rng, steps, batch, channels, 0.0)
    # N == 0: y all zeros, mean = rstd = 0, the running values untouched; dx zeros, nothing added
    lengths = _dev(np.zeros(batch), torch.int32)
    d_mean, d_var = _dev(run_mean), _dev(run_var)
    y, mean, rstd = hip.seq_bn_fwd(_dev(x), lengths, _dev(gamma), _dev(beta), d_mean, d_var,
                                   DECAY, ref.EPS)
    everything = np.zeros((steps, batch), dtype=bool)
    assert _is_plus_zero(y, everything) and _is_plus_zero(mean, np.zeros(channels, dtype=bool))
    assert _is_plus_zero(rstd, np.zeros(channels, dtype=bool))
    assert torch.equal(d_mean, _dev(run_mean)) and torch.equal(d_var, _dev(run_var))
    dgamma, dbeta = _dev(gamma).clone(), _dev(beta).clone()
    dx = hip.seq_bn_bwd(_dev(dy), _dev(x), lengths, mean, rstd, _dev(gamma), dgamma, dbeta)
    assert _is_plus_zero(dx, everything)
    assert torch.equal(dgamma, _dev(gamma)) and torch.equal(dbeta, _dev(beta))
    # N == 1: mean is the row itself, the variance 0, y = beta there; the gradient of a constant
    lengths = _dev(np.array([0, 1, 0]), torch.int32)
    y, mean, rstd = hip.seq_bn_fwd(_dev(x), lengths, _dev(gamma), _dev(beta), d_mean, d_var,
                                   DECAY, ref.EPS)
    assert torch.equal(mean, _dev(x[0, 1])) and torch.equal(y[0, 1], _dev(beta))
    assert _within_ulp(rstd, ref.f32(np.full(channels, 1.0 / np.sqrt(ref.EPS))))
    one = np.zeros((steps, batch), dtype=bool)
    one[0, 1] = True
    assert _is_plus_zero(y, one)
    assert _within_ulp(d_var, ref.f32(DECAY * run_var.astype(np.float64)))
    dgamma = torch.zeros(channels, dtype=torch.float32, device=DEV)
    dbeta = torch.zeros_like(dgamma)
    dx = hip.seq_bn_bwd(_dev(dy), _dev(x), lengths, mean, rstd, _dev(gamma), dgamma, dbeta)
    assert torch.equal(dbeta, _dev(dy[0, 1])) and _is_plus_zero(dgamma, np.zeros(channels, bool))
    assert (dx == 0).all() and _is_plus_zero(dx, one)         # dy - m1 = 0 and xhat = 0


def test_bad_arguments_return_their_codes_without_a_launch(hip):
    lib = hip.load()
    steps, batch, channels = 3, 2, 8
    x = torch.randn((steps, batch, channels), device=DEV)
    vec = [torch.full((channels,), 7.0, device=DEV) for _ in range(6)]
    y = torch.full_like(x, 7.0)
    need = hip.seq_bn_workspace_bytes(steps * batch, channels)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    ptr = [v.data_ptr() for v in vec]

    def fwd(x_ptr=x.data_ptr(), c=channels, t=steps, ws_ptr=ws.data_ptr(), ws_bytes=need,
            decay=DECAY, gamma=ptr[0]):
        return lib.ctcasr_seq_bn_fwd(x_ptr, None, t, batch, c, gamma, ptr[1], ptr[2], ptr[3],
                                     decay, ref.EPS, y.data_ptr(), ptr[4], ptr[5], ws_ptr,
                                     ws_bytes, None)

    def bwd(c=channels, ws_ptr=ws.data_ptr(), ws_bytes=need, dy_ptr=x.data_ptr()):
        return lib.ctcasr_seq_bn_bwd(dy_ptr, x.data_ptr(), None, steps, batch, c, ptr[4],
                                     ptr[5], ptr[0], ptr[2], ptr[3], y.data_ptr(), ws_ptr,
                                     ws_bytes, None)

    assert fwd(c=6) == fwd(c=0) == fwd(t=0) == fwd(x_ptr=None) == fwd(gamma=None) == -1
    assert fwd(x_ptr=x.data_ptr() + 4) == fwd(decay=1.5) == -1
    assert fwd(ws_ptr=None) == fwd(ws_bytes=need - 1) == fwd(ws_ptr=ws.data_ptr() + 4) == -3
    assert bwd(c=6) == bwd(dy_ptr=None) == bwd(dy_ptr=x.data_ptr() + 8) == -1
    assert bwd(ws_ptr=None) == bwd(ws_bytes=need - 1) == -3
    assert lib.ctcasr_seq_bn_infer(x.data_ptr(), None, steps, batch, 6, ptr[0], ptr[1], ptr[2],
                                   ptr[3], ref.EPS, y.data_ptr(), None) == -1
    assert lib.ctcasr_seq_bn_infer(x.data_ptr(), None, steps, batch, channels, ptr[0], ptr[1],
                                   ptr[2], ptr[3], 0.0, y.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (y == 7.0).all() and all((v == 7.0).all() for v in vec) and (ws == 0).all()
    for call in (lambda: hip.seq_bn_fwd(x, None, vec[0], vec[1], vec[2], vec[3], DECAY, ref.EPS,
                                        workspace=ws[:need - 8]),
                 lambda: hip.seq_bn_infer(x[:, :, :6].contiguous(), None, *vec[:4], ref.EPS),
                 lambda: hip.seq_bn_infer(x.double(), None, *vec[:4], ref.EPS),
                 lambda: hip.seq_bn_bwd(x, x, torch.zeros(3, dtype=torch.int32, device=DEV),
                                        *vec[:5])):
        with pytest.raises(hip.CtcAsrError):
            call()
