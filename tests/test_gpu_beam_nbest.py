"""N-best lists from both beam searches (csrc/beam.hip, `hip.ctc_beam_decode_nbest`).

Rank 0 is the existing kernels' answer bit for bit, and the top-1 entry points are undisturbed by
an n-best launch on the same workspace.  The lower ranks are checked against
`tests/nbest_reference.py` at N <= W / 2; near-ties among them are the normal case (the
reference's smallest gap among the first N + 1 totals is ~2e-3 at N = 8 and 1e-4 .. 3e-4 at
N = 16, the size of the existing logp tolerance), so the assertion is not rank-for-rank path
equality but: logp[k] within the bar of the reference's k-th total, path k somewhere in the
reference's full list with a total within the bar of logp[k], no path twice, logp sorted.  At
N = W (the bottom of the beam, where a near-tie at the eviction boundary may legitimately
differ) only the structure is checked.  One group does not go through TensorFlow-style code: an
unpruned search must list every labelling of `brute_force_posteriors`."""

import numpy as np
import pytest
import torch

from ctc_asr_amd import lm
from oracle import ctc as octc
from tests import nbest_reference as ref
from tests.beam_helpers import _logits, _random_scorer, _same_bits, _t, _tables, raw_beam

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORMS = ['max', 'log_softmax']
MAX_WIDTH = 1024


def _close(a, b):
    """The existing logp bar: rtol 1e-5, atol 1e-3."""
    return bool(np.isclose(np.float64(a), np.float64(b), rtol=1e-5, atol=1e-3))


def _nbest(hip, logits, seq_len, width, top_paths, scorer=None, blank=None, norm='max'):
    got = hip.ctc_beam_decode_nbest(_t(logits), _t(np.asarray(seq_len), torch.int32), width,
                                    top_paths, scorer=scorer, blank=blank, normalization=norm)
    return tuple(x.cpu().numpy() for x in got)


def _top1(hip, logits, seq_len, width, scorer=None, blank=None, norm='max'):
    lg, sl = _t(logits), _t(np.asarray(seq_len), torch.int32)
    if scorer is None:
        got = hip.ctc_beam_decode(lg, sl, width, blank=blank, normalization=norm)
    else:
        got = hip.ctc_beam_decode_lm(lg, sl, width, scorer, blank=blank, normalization=norm)
    return tuple(x.cpu().numpy() for x in got)


def _paths(out, out_len, b, count):
    return [tuple(out[b, k, :out_len[b, k]].tolist()) for k in range(count)]


def _check_structure(out, out_len, logp, n_paths, top_paths, classes, blank):
    """What holds for every n-best result: shapes, rows zero beyond their length, labels in
    range, distinct paths, logp non-increasing, the tail empty."""
    batch = n_paths.shape[0]
    assert out.shape[:2] == (batch, top_paths) and out_len.shape == logp.shape == (batch, top_paths)
    for b in range(batch):
        n = int(n_paths[b])
        assert 1 <= n <= top_paths, (b, n)
        paths = _paths(out, out_len, b, n)
        assert len(set(paths)) == n, (b, paths)
        for k in range(n):
            row, length = out[b, k], int(out_len[b, k])
            assert (row[length:] == 0).all(), (b, k)
            assert ((row[:length] >= 0) & (row[:length] < classes) & (row[:length] != blank)).all()
        assert (np.diff(logp[b, :n]) <= 0).all(), (b, logp[b, :n])
        assert (out_len[b, n:] == 0).all() and (out[b, n:] == 0).all(), b
        assert np.isneginf(logp[b, n:]).all(), b


# ------------------------------------------------------------------------------------------------
# 1. Rank 0 is the existing kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('fused', [False, True], ids=['plain', 'fused'])
@pytest.mark.parametrize('num_steps', [1, 2, 37])
def test_rank_0_is_the_top_1_search_bit_for_bit(hip, num_steps, fused, norm):
    rng = np.random.default_rng(100 + num_steps)
    logits = _logits(rng, num_steps, 3, 29, 28)
    seq_len = np.array([num_steps, 0, max(1, num_steps - 5)], dtype=np.int32)
    scorer = _random_scorer(rng, 5, 29, forbidden=0.05) if fused else None
    for width in (1, 8, 64, MAX_WIDTH):
        want = _top1(hip, logits, seq_len, width, scorer, 28, norm)
        for top_paths in sorted({1, min(2, width), width}):
            out, out_len, logp, n_paths = _nbest(hip, logits, seq_len, width, top_paths, scorer,
                                                 28, norm)
            assert _same_bits((out[:, 0], out_len[:, 0], logp[:, 0]), want), (width, top_paths)
            _check_structure(out, out_len, logp, n_paths, top_paths, 29, 28)
            assert n_paths[1] == 1 and out_len[1, 0] == 0      # seq_len 0: the root alone


@pytest.mark.parametrize('fused', [False, True], ids=['plain', 'fused'])
def test_top_1_entry_points_are_undisturbed_by_an_nbest_launch(hip, fused):
    """Top-1, n-best, top-1 on the same bytes: the two top-1 results are identical bits and
    rank 0 of the n-best launch is theirs."""
    rng = np.random.default_rng(7)
    logits = _logits(rng, 30, 4, 29, 28)
    seq_len = np.array([30, 22, 0, 5], dtype=np.int32)
    scorer = _random_scorer(rng, 6, 29, forbidden=0.1) if fused else None
    need = hip.ctc_beam_nbest_workspace_bytes(30, 4, 29, 32)
    assert need == hip.ctc_beam_workspace_bytes(30, 4, 29, 32)
    workspace = torch.full((need,), 0xff, dtype=torch.uint8, device=DEV)
    lg, sl = _t(logits), _t(seq_len, torch.int32)
    status, before = raw_beam(hip, lg, sl, 32, scorer, workspace)
    assert status == 0
    status, (out, out_len, logp, n_paths) = raw_beam(hip, lg, sl, 32, scorer, workspace, 8)
    assert status == 0
    status, after = raw_beam(hip, lg, sl, 32, scorer, workspace)
    assert status == 0
    assert _same_bits(before[:3], after[:3])
    assert _same_bits((out[:, 0], out_len[:, 0], logp[:, 0]), before[:3])
    _check_structure(out, out_len, logp, n_paths, 8, 29, 28)


# ------------------------------------------------------------------------------------------------
# 2. Parity with the reference at N <= W / 2; structure at N = W
# ------------------------------------------------------------------------------------------------
PARITY_SHAPES = [(12, 8, 4), (30, 16, 8), (40, 32, 8), (60, 32, 16)]     # (T, W, N)


def _parity_case(shape, classes, blank, scale, fused):
    num_steps, width, top_paths = shape
    rng = np.random.default_rng(1000 * num_steps + 10 * classes + int(scale) + 5 * fused)
    logits = _logits(rng, num_steps, 2, classes, blank, scale=float(scale))
    seq_len = np.array([num_steps, num_steps - 3], dtype=np.int32)
    scorer = None
    if fused:
        labels = [c for c in range(classes) if c != blank]
        rows = [[labels[int(i)] for i in rng.integers(0, min(len(labels), 6),
                                                      size=int(rng.integers(1, 12)))]
                for _ in range(40)]
        scorer = lm.build_char_ngram(rows, 3, classes, blank=blank).scaled(0.7, 0.3)
    return logits, seq_len, scorer


@pytest.mark.parametrize('fused', [False, True], ids=['plain', 'n-gram'])
@pytest.mark.parametrize('scale', [1, 3])
@pytest.mark.parametrize('classes,blank', [(29, 28), (5, 2)])
@pytest.mark.parametrize('shape', PARITY_SHAPES, ids=lambda s: 'T{}-W{}-N{}'.format(*s))
def test_parity_with_the_reference(hip, shape, classes, blank, scale, fused):
    num_steps, width, top_paths = shape
    logits, seq_len, scorer = _parity_case(shape, classes, blank, scale, fused)
    for norm in NORMS:
        _parity(hip, shape, classes, blank, scale, fused, norm, logits, seq_len, scorer)


def _parity(hip, shape, classes, blank, scale, fused, norm, logits, seq_len, scorer):
    num_steps, width, top_paths = shape
    want = ref.nbest(logits, seq_len, width, *_tables(scorer), blank=blank, normalization=norm)
    out, out_len, logp, n_paths = _nbest(hip, logits, seq_len, width, top_paths, scorer, blank,
                                         norm)
    _check_structure(out, out_len, logp, n_paths, top_paths, classes, blank)
    worst = 0.0
    for b in range(2):
        leaves = want[b]
        assert n_paths[b] == min(top_paths, len(leaves)), (b, n_paths[b], len(leaves))
        totals = {tuple(path): total for path, total in leaves}
        assert len(totals) == len(leaves)
        for k, path in enumerate(_paths(out, out_len, b, int(n_paths[b]))):
            worst = max(worst, abs(float(logp[b, k]) - float(leaves[k][1])))
            assert _close(logp[b, k], leaves[k][1]), (b, k, logp[b, k], leaves[k][1])
            assert path in totals, (b, k, path)
            assert _close(totals[path], logp[b, k]), (b, k, totals[path], logp[b, k])
    print('{} C {} x{} {} {}: max |logp[k] - reference total k| {:.3g}'.format(
        shape, classes, scale, 'fused' if fused else 'plain', norm, worst))

    # N = W: the bottom of the beam - structure only, and rank 0 as above
    out, out_len, logp, n_paths = _nbest(hip, logits, seq_len, width, width, scorer, blank, norm)
    _check_structure(out, out_len, logp, n_paths, width, classes, blank)
    assert n_paths.tolist() == [len(leaves) for leaves in want]
    top = _top1(hip, logits, seq_len, width, scorer, blank, norm)
    assert _same_bits((out[:, 0], out_len[:, 0], logp[:, 0]), top)


# ------------------------------------------------------------------------------------------------
# 3. Truth, not through TensorFlow-style code
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('forbid', [None, 0], ids=['free', 'label 0 forbidden'])
def test_unpruned_list_is_every_labelling_with_its_posterior(hip, forbid):
    """C = 3, T = 5: at most 63 labellings, width 1024 prunes nothing, and with `log_softmax`
    every total is the exact ln p(labelling | x).  With a scorer that forbids one label the
    labellings that hold it are absent and the others keep their posteriors."""
    classes, num_steps, blank, batch = 3, 5, 2, 4
    rng = np.random.default_rng(35)
    logits = (rng.normal(size=(num_steps, batch, classes)) * 2).astype(np.float32)
    scorer = None
    if forbid is not None:
        score = np.zeros((1, classes), dtype=np.float32)
        score[0, forbid] = -np.inf
        scorer = lm.LmScorer(np.zeros((1, classes), dtype=np.int32), score)
    out, out_len, logp, n_paths = _nbest(hip, logits, [num_steps] * batch, MAX_WIDTH, 63, scorer,
                                         blank, 'log_softmax')
    _check_structure(out, out_len, logp, n_paths, 63, classes, blank)
    for b in range(batch):
        post = octc.brute_force_posteriors(logits[:, b].astype(np.float64), blank)
        full = len(post)
        if forbid is not None:
            post = {label: p for label, p in post.items() if forbid not in label}
        assert len(post) <= 63 and (forbid is None or len(post) < full)
        assert n_paths[b] == len(post), (b, n_paths[b], len(post))
        paths = _paths(out, out_len, b, int(n_paths[b]))
        assert set(paths) == set(post)
        got = np.exp(logp[b, :n_paths[b]].astype(np.float64))
        want = np.array([post[path] for path in paths])
        assert np.abs(got - want).max() <= 1e-5, (b, np.abs(got - want).max())
        assert (np.diff(got) <= 0).all()


# ------------------------------------------------------------------------------------------------
# 4. Fewer leaves than N, garbage in the output buffers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('classes', [5, 29])
def test_fewer_leaves_than_top_paths(hip, classes):
    """T = 1: the root and one child per label, C leaves in all."""
    rng = np.random.default_rng(classes)
    logits = _logits(rng, 1, 3, classes, classes - 1)
    lg, sl = _t(logits), _t(np.array([1, 0, 1]), torch.int32)
    workspace = torch.empty(hip.ctc_beam_nbest_workspace_bytes(1, 3, classes, 8),
                            dtype=torch.uint8, device=DEV)
    status, (out, out_len, logp, n_paths) = raw_beam(hip, lg, sl, 8, None, workspace, 8,
                                                     blank=classes - 1)
    assert status == 0
    assert n_paths.tolist() == [min(8, classes), 1, min(8, classes)]
    _check_structure(out, out_len, logp, n_paths, 8, classes, classes - 1)


# ------------------------------------------------------------------------------------------------
# 5. Refusals and the exhausted pool
# ------------------------------------------------------------------------------------------------
def test_bad_top_paths_is_a_bad_argument(hip):
    logits = _t(np.zeros((6, 2, 29), dtype=np.float32))
    seq_len = _t(np.array([6, 6]), torch.int32)
    workspace = torch.empty(hip.ctc_beam_nbest_workspace_bytes(6, 2, 29, 8), dtype=torch.uint8,
                            device=DEV)
    for top_paths in (0, 9, -1):
        status, _ = raw_beam(hip, logits, seq_len, 8, None, workspace, top_paths)
        assert status == -1, top_paths
        with pytest.raises(hip.CtcAsrError):
            hip.ctc_beam_decode_nbest(logits, seq_len, 8, top_paths)
    status, _ = raw_beam(hip, logits, seq_len, 8, None, workspace, 8)
    assert status == 0
    with pytest.raises(hip.CtcAsrError, match='1 lengths for a batch of 2'):
        hip.ctc_beam_decode_nbest(logits, seq_len[:1], 8, 2)
    for args in ((0, 4, 29, 8), (30, 4, 29, 0)):
        assert hip.load().ctcasr_ctc_beam_nbest_workspace_bytes(*args) == 0


@pytest.mark.timeout(160)
def test_pool_exhaustion_is_reported_as_n_paths_minus_1(hip):
    """The inputs of test_gpu_beam_edges.py's exhaustion case, through the C ABI: a workspace one
    byte short is refused first, then the row reports n_paths = -1 and every out_len -1 (what
    the wrapper raises on), and the next launch is sound."""
    classes, blank, num_steps = 64, 63, 3200
    rng = np.random.default_rng(8)
    logits = _t(_logits(rng, num_steps, 1, classes, blank, scale=0.3, blank_bias=0.0))
    seq_len = _t(np.array([num_steps]), torch.int32)
    need = hip.ctc_beam_nbest_workspace_bytes(num_steps, 1, classes, MAX_WIDTH)
    workspace = torch.empty(need, dtype=torch.uint8, device=DEV)
    status, _ = raw_beam(hip, logits, seq_len, MAX_WIDTH, None, workspace, 4, blank,
                         nbytes=need - 1)
    assert status == -3
    status, (out, out_len, logp, n_paths) = raw_beam(hip, logits, seq_len, MAX_WIDTH, None,
                                                     workspace, 4, blank)
    assert status == 0
    assert n_paths.tolist() == [-1] and (out_len == -1).all()
    small = _logits(rng, 30, 3, 29, 28)
    got = _nbest(hip, small, [30, 12, 0], 32, 4)
    assert _same_bits((got[0][:, 0], got[1][:, 0], got[2][:, 0]),
                      _top1(hip, small, [30, 12, 0], 32))


# ------------------------------------------------------------------------------------------------
# 6. Independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [False, True], ids=['plain', 'fused'])
def test_a_row_in_a_batch_of_64_is_the_row_alone(hip, fused):
    rng = np.random.default_rng(64)
    logits = _logits(rng, 50, 64, 29, 28)
    seq_len = rng.integers(0, 51, size=64).astype(np.int32)
    seq_len[[0, 63]] = 50
    scorer = _random_scorer(rng, 7, 29, forbidden=0.03) if fused else None
    for width in (16, 100):
        joint = _nbest(hip, logits, seq_len, width, 8, scorer, 28)
        _check_structure(*joint, 8, 29, 28)
        for b in (0, 17, 40, 63):
            one = _nbest(hip, logits[:, b:b + 1], seq_len[b:b + 1], width, 8, scorer, 28)
            assert _same_bits(one, tuple(x[b:b + 1] for x in joint)), (width, b)
