"""Pins the CTC oracle: recalled TensorFlow known-answer vectors, brute-force path enumeration,
torch.nn.functional.ctc_loss, and the C restatement against the numpy one."""

import json
import os

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as st

from oracle import cref
from oracle import ctc as octc

KAT = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'ctc_kat.json')))


def test_tensorflow_known_answers_loss_and_gradient():
    for case in KAT['loss_cases']:
        logits = np.log(np.array(case['probs']))
        loss, grad = octc.ctc_loss_single(logits, case['targets'])
        assert loss == pytest.approx(case['loss'], abs=2e-5)
        assert np.abs(grad - np.array(case['grad'])).max() < 2e-6
        c_loss, c_grad, status = cref.ctc_loss(logits[:, None, :], [case['targets']],
                                               [logits.shape[0]])
        assert status[0] == 0 and c_loss[0] == pytest.approx(case['loss'], abs=2e-5)
        assert np.abs(c_grad[:, 0] - np.array(case['grad'])).max() < 2e-6


def test_decode_known_answers():
    case = KAT['decode_case']
    logits = np.log(np.array(case['probs']))
    assert octc.greedy_decode(logits[:, None, :], [5])[0] == case['greedy']
    assert octc.beam_search_decode_single(logits, 64)[0] == case['beam_wide']
    assert octc.beam_search_decode_single(logits, 2)[0] == case['beam_width_2']   # TF's own test
    post = octc.brute_force_posteriors(logits)
    ranked = sorted(post.items(), key=lambda kv: -kv[1])[:5]
    for (labels, prob), (ref_labels, ref_prob) in zip(ranked, case['top5']):
        assert list(labels) == ref_labels and prob == pytest.approx(ref_prob, rel=2e-3)


@settings(max_examples=25, deadline=None)
@given(st.integers(2, 4), st.integers(1, 5), st.integers(0, 2 ** 31 - 1))
def test_loss_equals_brute_force(classes, steps, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(steps, classes)) * 2
    post = octc.brute_force_posteriors(logits)
    assert sum(post.values()) == pytest.approx(1.0)
    for label, prob in post.items():
        loss, _ = octc.ctc_loss_single(logits, list(label))
        assert loss == pytest.approx(-np.log(prob), abs=1e-9)
    # an infeasible label raises like TensorFlow
    with pytest.raises(octc.InfeasibleAlignment):
        octc.ctc_loss_single(logits, [0] * (steps + 1))


@settings(max_examples=25, deadline=None)
@given(st.integers(2, 4), st.integers(1, 5), st.integers(0, 2 ** 31 - 1))
def test_unpruned_beam_search_finds_the_most_probable_labelling(classes, steps, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(steps, classes)) * 2
    post = octc.brute_force_posteriors(logits)
    best_label, best_prob = max(post.items(), key=lambda kv: kv[1])
    for norm in ('max', 'log_softmax'):
        path, logp = octc.beam_search_decode_single(logits, 10 ** 6, normalization=norm)
        assert post[tuple(path)] == pytest.approx(best_prob, rel=1e-5)
        if norm == 'log_softmax':
            assert np.exp(logp) == pytest.approx(best_prob, rel=1e-4)
    assert tuple(octc.greedy_decode(logits[:, None, :], [steps])[0]) in post


def test_gradient_matches_torch_and_is_zero_beyond_seq_len():
    rng = np.random.default_rng(7)
    steps, batch, classes = 30, 4, 29
    logits = rng.normal(size=(steps, batch, classes))
    labels = [[1, 1, 2], [3], [], list(rng.integers(0, 28, size=10))]
    seq_len = [30, 12, 7, 25]
    loss, grad = octc.ctc_loss(logits, labels, seq_len)
    x = torch.tensor(logits, requires_grad=True)
    ref = torch.nn.functional.ctc_loss(
        torch.log_softmax(x, -1), torch.tensor([v for r in labels for v in r]),
        torch.tensor(seq_len), torch.tensor([len(r) for r in labels]), blank=classes - 1,
        reduction='none')
    ref.sum().backward()
    assert np.abs(loss - ref.detach().numpy()).max() < 1e-9
    assert np.abs(grad - x.grad.numpy()).max() < 1e-9
    for b, length in enumerate(seq_len):
        assert np.abs(grad[length:, b]).max(initial=0.0) == 0.0
    # C restatement agrees, including status codes
    c_loss, c_grad, status = cref.ctc_loss(logits, labels, seq_len)
    assert (status == 0).all() and np.abs(c_loss - loss).max() < 1e-4   # float32 input
    assert np.abs(c_grad - grad).max() < 1e-5
    _, _, status = cref.ctc_loss(logits[:4], [[0, 0, 0], [1], [28], [2]], [4, 4, 4, 4])
    assert status.tolist() == [1, 0, 2, 0]


def test_c_beam_search_equals_numpy_beam_search():
    rng = np.random.default_rng(11)
    logits = (rng.normal(size=(25, 5, 7)) * 2).astype(np.float32)
    seq_len = [25, 9, 17, 1, 25]
    for width in (1, 2, 3, 8, 50):
        for norm in ('max', 'log_softmax'):
            p1, s1 = octc.beam_search_decode(logits, seq_len, width, normalization=norm)
            p2, s2 = cref.beam_search_decode(logits, seq_len, width, normalization=norm)
            assert p1 == p2 and np.allclose(s1, s2, atol=1e-5)


def _edge_inputs():
    """(logits [T, B, C], seq_len, blank) of the input classes the GPU beam search is held to in
    test_gpu_beam_edges.py: rows of length 0 and 1, T = 1, the blank at 0 and mid, C = 2 with
    either blank, C = 64, and -inf entries (a class for all frames, on alternate frames, the
    blank on some frames)."""
    rng = np.random.default_rng(12)
    cases = []
    for steps, classes, blank in ((12, 7, 0), (12, 7, 3), (1, 7, 6), (10, 2, 0), (10, 2, 1),
                                  (12, 64, 63), (12, 64, 0)):
        logits = (rng.normal(size=(steps, 4, classes)) * 2).astype(np.float32)
        cases.append((logits, [steps, 0, 1, max(1, steps - 3)], blank))
    for kind in range(3):
        logits = (rng.normal(size=(14, 3, 7)) * 2).astype(np.float32)
        if kind == 0:
            logits[:, :, 2] = -np.inf
        elif kind == 1:
            logits[0::2, :, 2] = -np.inf
            logits[1::2, :, 2] += 4.0
        else:
            logits[0::3, 0, 6] = -np.inf
            logits[2::3, 1:, 6] = -np.inf
        cases.append((logits, [14, 14, 9], 6))
    return cases


def test_c_beam_search_equals_numpy_beam_search_at_the_edge_inputs():
    for logits, seq_len, blank in _edge_inputs():
        for width in (1, 8, 100):
            for norm in ('max', 'log_softmax'):
                p1, s1 = octc.beam_search_decode(logits, seq_len, width, blank, norm)
                p2, s2 = cref.beam_search_decode(logits, seq_len, width, blank, norm)
                assert p1 == p2 and np.allclose(s1, s2, atol=1e-5), (logits.shape, blank, width)
                for b, length in enumerate(seq_len):
                    assert length > 0 or (p2[b] == [] and s2[b] == 0.0)


def test_c_beam_search_counts_the_prefixes_that_entered_the_beam():
    """`return_nodes`: with a beam wider than the prefix tree every labelling that fits into the
    frames enters the beam once, and those are the keys of the exhaustive enumeration; a
    masked class takes its labellings out; width 1 admits one new prefix per frame at most; the
    paths and scores are those of the plain entry point."""
    rng = np.random.default_rng(13)
    logits = (rng.normal(size=(5, 4, 4)) * 2).astype(np.float32)
    logits[:, 3, 0] = -np.inf
    seq_len = [5, 0, 3, 5]
    for blank in (3, 1):
        for norm in ('max', 'log_softmax'):
            paths, logp, nodes = cref.beam_search_decode(logits, seq_len, 1024, blank, norm,
                                                         return_nodes=True)
            want = [len([k for k, p in octc.brute_force_posteriors(logits[:n, b], blank).items()
                         if p > 0]) for b, n in enumerate(seq_len)]
            assert nodes.tolist() == want and nodes[1] == 1
            plain = cref.beam_search_decode(logits, seq_len, 1024, blank, norm)
            assert plain[0] == paths and np.array_equal(plain[1], logp)
            _, _, narrow = cref.beam_search_decode(logits, seq_len, 1, blank, norm,
                                                   return_nodes=True)
            assert (narrow <= 1 + np.array(seq_len)).all() and (narrow >= 1).all()


def test_dense_to_label_lists_drops_padding_zeros():
    assert octc.dense_to_label_lists(np.array([[3, 4, 0, 0], [0, 0, 0, 0], [1, 0, 2, 0]])) == \
        [[3, 4], [], [1, 2]]


def _torch_ctc(logits, labels, seq_len, blank):
    """torch.nn.functional.ctc_loss in float64 on the same (float32) logits: loss per row and the
    gradient w.r.t. the logits through autograd."""
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    ref = torch.nn.functional.ctc_loss(
        torch.log_softmax(x, -1), torch.tensor([v for r in labels for v in r], dtype=torch.long),
        torch.tensor(seq_len), torch.tensor([len(r) for r in labels]), blank=blank,
        reduction='none')
    ref.sum().backward()
    return ref.detach().numpy(), x.grad.numpy()


def _edge_case(name):
    """(logits f32[T, B, C], labels, seq_len, blank) of the edge shapes test_gpu_ctc_edges.py
    runs the kernel at."""
    rng = np.random.default_rng(sum(map(ord, name)))

    def labels_of(lengths, classes, blank):
        ids = np.array([c for c in range(classes) if c != blank])
        return [rng.choice(ids, size=n).tolist() for n in lengths]

    if name == 'T=1':
        classes, blank, labels, seq_len = 5, 4, [[], [2], [0]], [1, 1, 1]
    elif name == 'T=1 blank=0':
        classes, blank, labels, seq_len = 5, 0, [[], [3]], [1, 1]
    elif name == 'T=3 len=0':
        classes, blank, labels, seq_len = 6, 5, [[], [1, 1], [], [2]], [0, 3, 2, 1]
    elif name == 'C=64 blank=0':
        classes, blank = 64, 0
        labels, seq_len = labels_of([63, 20, 0], classes, blank), [140, 90, 70]
    elif name == 'C=64 blank=32':
        classes, blank = 64, 32
        labels, seq_len = labels_of([63, 20, 1], classes, blank), [140, 140, 3]
    elif name == 'L=575 blank=0':
        classes, blank = 64, 0
        labels, seq_len = labels_of([575, 300], classes, blank), [1200, 1100]
    elif name == 'L=575 blank=32':
        classes, blank = 64, 32
        labels, seq_len = labels_of([575, 575], classes, blank), [1200, 1200]
    num_steps = max(seq_len + [1])
    logits = (rng.normal(size=(num_steps, len(labels), classes)) * 2).astype(np.float32)
    return logits, labels, seq_len, blank


@pytest.mark.parametrize('name', ['T=1', 'T=1 blank=0', 'T=3 len=0', 'C=64 blank=0',
                                  'C=64 blank=32', 'L=575 blank=0', 'L=575 blank=32'])
def test_c_oracle_matches_torch_at_the_edge_shapes(name):
    """The C oracle that test_gpu_ctc_edges.py measures the kernel against, pinned at the same
    edges: T = 1, len = 0 with L = 0 (loss exactly 0, no gradient), L = 575 (the kernel's label
    ceiling), C = 64 and a blank of 0 or C // 2."""
    logits, labels, seq_len, blank = _edge_case(name)
    loss, grad, status = cref.ctc_loss(logits, labels, seq_len, blank)
    ref_loss, ref_grad = _torch_ctc(logits, labels, seq_len, blank)
    assert (status == 0).all()
    assert (np.abs(loss - ref_loss) <= 1e-9 * np.maximum(1.0, np.abs(ref_loss))).all()
    assert np.abs(grad - ref_grad).max() < 1e-9
    for b, length in enumerate(seq_len):
        assert (grad[length:, b] == 0).all()
        if length == 0:
            assert loss[b] == 0.0


@pytest.mark.parametrize('classes', [2, 3, 4])
@pytest.mark.parametrize('num_steps', [1, 2, 3, 4])
def test_c_oracle_equals_path_enumeration(num_steps, classes):
    """Every labelling that has probability at T <= 4, C <= 4, with the blank at C - 1, 0 and
    C // 2: the C oracle's loss is minus the log of the summed probability of its paths, and a
    labelling that needs more frames than there are is refused with status 1."""
    rng = np.random.default_rng(10 * num_steps + classes)
    logits = (rng.normal(size=(num_steps, classes)) * 2).astype(np.float32)
    for blank in sorted({classes - 1, 0, classes // 2}):
        post = octc.brute_force_posteriors(logits.astype(np.float64), blank)
        labels = [list(label) for label in post]
        batch = np.repeat(logits[:, None, :], len(labels), axis=1)
        loss, _, status = cref.ctc_loss(batch, labels, [num_steps] * len(labels), blank)
        assert (status == 0).all()
        want = -np.log([post[tuple(label)] for label in labels])
        assert np.abs(loss - want).max() < 1e-9
        symbol = 0 if blank else 1
        _, _, status = cref.ctc_loss(logits[:, None, :], [[symbol] * num_steps + [symbol]],
                                     [num_steps], blank)
        assert status[0] == 1
