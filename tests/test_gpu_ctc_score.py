"""`ctcasr_ctc_score` (csrc/ctc_score.hip, `hip.ctc_score`): the forward-only CTC log-likelihood
of many label sequences, one wavefront per hypothesis with the lattice in registers.

Reference: `oracle.ctc.ctc_loss_single` (float64).  Bar: that of test_gpu_ctc_edges.py's losses,
restated here - 1e-3 absolute up to a loss of 1000, relative 1e-6 above (a float32 score of 2e4
alone rounds by up to 1e-3, and every frame's table entry carries a relative error ~6e-8).

Label lengths sit on the seams of the kernel: S = 2L + 1 against the 64 lanes and against the
states-per-lane counts it is compiled for (1, 2, 3, 6, 18: S <= 64, 128, 192, 384, 1152, that is
L <= 31, 63, 95, 191, 575).  The references are computed once per module and shared."""

import numpy as np
import pytest
import torch

from oracle import ctc as octc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CLASSES, BLANK = 29, 28
STEPS = 130                       # of the main bank; the long rows have a bank of their own
SEAM_LENGTHS = [0, 1, 31, 32, 63, 64, 95, 96]
UNSUPPORTED = -2


def _bar(ref_loss):
    return np.maximum(1e-3, 1e-6 * np.abs(ref_loss))


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _pack(labels):
    offsets = np.zeros(len(labels) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(row) for row in labels])
    flat = np.array([v for row in labels for v in row] or [0], dtype=np.int32)
    return flat, offsets


def _score(hip, logits, seq_len, hyps, blank=BLANK, max_label_len=None, offsets=None):
    """`hip.ctc_score` on host data; ``hyps`` is a list of (utt, label list).  Returns host
    (score f32[H], status i32[H])."""
    flat, packed = _pack([label for _, label in hyps])
    offsets = packed if offsets is None else offsets
    lg = logits if torch.is_tensor(logits) else _t(logits)
    score, status = hip.ctc_score(lg, _t(np.asarray(seq_len), torch.int32), _t(flat, torch.int32),
                                  _t(offsets, torch.int32),
                                  _t(np.array([u for u, _ in hyps]), torch.int32),
                                  max_label_len=max_label_len, blank=blank)
    return score.cpu().numpy(), status.cpu().numpy()


def _reference(logits, seq_len, hyps, blank=BLANK):
    """ln p of each hypothesis in float64; -inf where no alignment exists."""
    want = np.zeros(len(hyps))
    for h, (utt, label) in enumerate(hyps):
        frames = int(seq_len[utt])
        if frames == 0 and not label:
            continue
        try:
            want[h] = -octc.ctc_loss_single(logits[:frames, utt].astype(np.float64), label,
                                            blank)[0]
        except octc.InfeasibleAlignment:
            want[h] = -np.inf
    return want


def _random_label(rng, length, classes=CLASSES, blank=BLANK):
    ids = [c for c in range(classes) if c != blank]
    return [ids[int(i)] for i in rng.integers(0, len(ids), size=length)]


def _assert_close(score, want, factor=1.0, what=''):
    finite = np.isfinite(want)
    assert np.array_equal(np.isneginf(score), np.isneginf(want)), what
    err = np.abs(score[finite].astype(np.float64) - want[finite])
    bar = factor * _bar(want[finite])
    print('{}: max |score - reference| {:.3g} (bar {:.3g})'.format(
        what, err.max() if err.size else 0.0, bar.min() if bar.size else 0.0))
    assert (err <= bar).all(), (what, err.max())


@pytest.fixture(scope='module')
def bank():
    """T = 130, four utterances (one shorter, one of no use to anybody), and hypotheses at every
    seam: random labels at each L, all-equal and strictly alternating ones where T allows."""
    rng = np.random.default_rng(2024)
    logits = (rng.normal(size=(STEPS, 4, CLASSES)) * 2).astype(np.float32)
    seq_len = np.array([STEPS, STEPS, 101, STEPS], dtype=np.int32)
    hyps = []
    for i, length in enumerate(SEAM_LENGTHS):
        hyps.append((i % 3, _random_label(rng, length)))
    for length in (1, 31, 32, 63, 64):
        hyps.append((0, [5] * length))                         # every skip forbidden
        hyps.append((1, [3 + (k & 1) for k in range(length)]))  # every skip allowed
    hyps.append((2, [7] * 51))                                 # exactly 101 frames: one path
    hyps.append((2, [7] * 52))                                 # one frame short
    want = _reference(logits, seq_len, hyps)
    assert np.isneginf(want[-1]) and np.isfinite(want[:-1]).all()
    return logits, seq_len, hyps, want


# ------------------------------------------------------------------------------------------------
def test_seams_against_the_float64_oracle(hip, bank):
    logits, seq_len, hyps, want = bank
    score, status = _score(hip, logits, seq_len, hyps)
    assert status.tolist() == [0] * (len(hyps) - 1) + [1]
    _assert_close(score, want, what='seams, H {}'.format(len(hyps)))


@pytest.mark.parametrize('count', [1, 5, 257])
def test_any_number_of_hypotheses(hip, bank, count):
    """H = 1, 5, 257 (no multiple of the waves of a workgroup): the bank's hypotheses, repeated;
    each equals its bits in the bank's own call, whatever max_label_len selects the kernel."""
    logits, seq_len, hyps, want = bank
    base, _ = _score(hip, logits, seq_len, hyps)
    picks = [(3 * i + 1) % len(hyps) for i in range(count)]
    score, status = _score(hip, logits, seq_len, [hyps[i] for i in picks])
    assert np.array_equal(_bits(score), _bits(base[picks]))
    _assert_close(score, want[picks], what='H {}'.format(count))
    assert status.tolist() == [int(np.isneginf(want[i])) for i in picks]


def test_the_arrangement_of_utt_does_not_matter(hip, bank):
    """Sorted by utterance, shuffled, and the hypotheses of one utterance alone: the same bits.
    Utterance 3 has no hypothesis at all."""
    logits, seq_len, hyps, want = bank
    rng = np.random.default_rng(3)
    base, base_status = _score(hip, logits, seq_len, hyps, max_label_len=96)
    by_utt = sorted(range(len(hyps)), key=lambda i: hyps[i][0])
    shuffled = rng.permutation(len(hyps)).tolist()
    only_1 = [i for i in range(len(hyps)) if hyps[i][0] == 1]
    assert not any(utt == 3 for utt, _ in hyps) and len(only_1) >= 5
    for order in (by_utt, shuffled, only_1, only_1[::-1]):
        score, status = _score(hip, logits, seq_len, [hyps[i] for i in order], max_label_len=96)
        assert np.array_equal(_bits(score), _bits(base[order]))
        assert np.array_equal(status, base_status[order])
    # ... and the same hypotheses all on utterance 3 are that utterance's scores
    moved = [(3, label) for utt, label in hyps if utt == 1]
    score, _ = _score(hip, logits, seq_len, moved)
    _assert_close(score, _reference(logits, seq_len, moved), what='all on one utterance')


def test_few_frames_the_one_feasible_path_and_one_frame_fewer(hip):
    rng = np.random.default_rng(11)
    logits = (rng.normal(size=(9, 7, CLASSES)) * 2).astype(np.float32)
    seq_len = np.array([1, 2, 3, 7, 6, 0, 9], dtype=np.int32)
    tight = [4, 4, 9, 9, 2]                                    # L 5 + 2 repeats = 7 frames
    hyps = [(0, []), (0, [3]), (0, [3, 4]), (1, []), (1, [3]), (1, [3, 3]), (1, [3, 4]),
            (2, [3, 3]), (2, [3, 4, 5]), (2, [1, 2, 1, 2]), (3, tight), (4, tight), (5, []),
            (5, [3]), (6, tight), (6, [])]
    want = _reference(logits, seq_len, hyps)
    score, status = _score(hip, logits, seq_len, hyps)
    assert status.tolist() == [int(np.isneginf(w)) for w in want]
    assert status.tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0]
    _assert_close(score, want, what='T 1, 2, 3, tight')
    assert score[12] == 0.0                                    # seq_len 0, empty label
    # the empty label: the blank's log-softmax summed over the frames
    blank_sum = octc.log_softmax(logits[:, 6].astype(np.float64))[:, BLANK].sum()
    assert abs(score[15] - blank_sum) <= 1e-3


def test_long_rows_and_the_largest_legal_one(hip):
    """L = 191 / 192 (the seam between 6 and 18 states per lane) at T = 230, and L = 575, the
    largest legal row; L = 576 is CTCASR_ERR_UNSUPPORTED as the call's return."""
    rng = np.random.default_rng(575)
    logits = (rng.normal(size=(580, 2, CLASSES)) * 2).astype(np.float32)
    seq_len = np.array([230, 580], dtype=np.int32)
    # (a strictly alternating row has no repeats: L = 575 fits 580 frames)
    hyps = [(0, _random_label(rng, 191)), (0, [3 + (k & 1) for k in range(192)]),
            (1, [3 + (k % 3) for k in range(575)])]
    want = _reference(logits, seq_len, hyps)
    score, status = _score(hip, logits, seq_len, hyps)
    assert status.tolist() == [0, 0, 0]
    _assert_close(score, want, what='L 191, 192, 575')
    alone, _ = _score(hip, logits, seq_len, hyps[:1])          # 6 states per lane, not 18
    assert _bits(alone)[0] == _bits(score)[0]
    lib = hip.load()
    lg, sl = _t(logits), _t(seq_len, torch.int32)
    flat, offsets = _pack([[3] * 576])
    fl, of, ut = _t(flat, torch.int32), _t(offsets, torch.int32), _t(np.zeros(1), torch.int32)
    out, st = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    workspace = torch.empty(hip.ctc_score_workspace_bytes(580, 2, CLASSES, 1, 575),
                            dtype=torch.uint8, device=DEV)
    for max_len, expect in ((576, UNSUPPORTED), (575, 0)):
        assert lib.ctcasr_ctc_score(lg.data_ptr(), sl.data_ptr(), 580, 2, CLASSES, BLANK,
                                    fl.data_ptr(), of.data_ptr(), ut.data_ptr(), 1, max_len,
                                    out.data_ptr(), st.data_ptr(), workspace.data_ptr(),
                                    workspace.numel(), None) == expect
    torch.cuda.synchronize()
    assert st.item() == 2 and np.isneginf(out.item())          # longer than max_label_len
    with pytest.raises(hip.CtcAsrError):
        _score(hip, logits, seq_len, [(1, [3] * 576)])


def test_equals_the_loss_kernel_on_replicated_rows(hip, bank):
    """The only route there was: one [T, C] slab of logits per hypothesis through
    `ctc_loss_fwd_bwd`.  Twice the bar: each side carries its own error."""
    logits, seq_len, hyps, want = bank
    hyps = hyps[:-1]                                           # (the infeasible row: status 1)
    score, _ = _score(hip, logits, seq_len, hyps)
    utt = [u for u, _ in hyps]
    flat, offsets = _pack([label for _, label in hyps])
    loss, _, status = hip.ctc_loss_fwd_bwd(_t(logits[:, utt]), _t(flat, torch.int32),
                                           _t(offsets, torch.int32),
                                           _t(seq_len[utt], torch.int32), 96, blank=BLANK)
    assert status.cpu().tolist() == [0] * len(hyps)
    loss = loss.cpu().numpy().astype(np.float64)
    err = np.abs(score.astype(np.float64) + loss)
    print('against the loss kernel: max |score + loss| {:.3g}'.format(err.max()))
    assert (err <= 2 * _bar(loss)).all(), err.max()


def test_status_2_rows_do_not_disturb_their_neighbours(hip, bank):
    logits, seq_len, hyps, _ = bank
    good = hyps[:9]
    base, _ = _score(hip, logits, seq_len, good, max_label_len=96)

    def run(bad_hyp, lengths=seq_len, max_label_len=96):
        score, status = _score(hip, logits, lengths, good[:4] + [bad_hyp] + good[4:],
                               max_label_len=max_label_len)
        return score, status

    for bad in ((0, [3, BLANK, 4]), (0, [3, CLASSES]), (0, [3, -1]), (-1, [3, 4]), (4, [3, 4]),
                (1, [3] * 97)):
        score, status = run(bad)
        assert status[4] == 2 and np.isneginf(score[4]), bad
        keep = [0, 1, 2, 3, 5, 6, 7, 8, 9]
        assert status[keep].tolist() == [0] * 9
        assert np.array_equal(_bits(score[keep]), _bits(base)), bad
    # seq_len = T + 1 and a negative one: every hypothesis of that utterance, nobody else
    for length in (STEPS + 1, -1):
        lengths = seq_len.copy()
        lengths[3] = length
        score, status = run((3, [3, 4]), lengths)
        assert status[4] == 2 and np.isneginf(score[4])
        assert np.array_equal(_bits(np.delete(score, 4)), _bits(base))
    # decreasing offsets: a row of negative length
    flat, offsets = _pack([label for _, label in good])
    offsets = offsets.copy()
    offsets[3] = offsets[4] + 2
    score, status = _score(hip, logits, seq_len, good, max_label_len=96, offsets=offsets)
    assert status[3] == 2 and np.isneginf(score[3])
    assert np.array_equal(_bits(score[4:]), _bits(base[4:]))


@pytest.mark.parametrize('poison', [np.nan, np.inf], ids=['nan', '+inf'])
def test_non_finite_logits(hip, bank, poison):
    """Inside the counted frames: NaN, as the loss gives.  Outside: no effect, bit for bit."""
    logits, seq_len, hyps, _ = bank
    hyps = hyps[:9]
    base, base_status = _score(hip, logits, seq_len, hyps)
    outside = logits.copy()
    outside[101:, 2, :] = poison                               # utterance 2 counts 101 frames
    score, status = _score(hip, outside, seq_len, hyps)
    assert np.array_equal(_bits(score), _bits(base)) and np.array_equal(status, base_status)
    inside = logits.copy()
    inside[100, 2, 7] = poison
    score, status = _score(hip, inside, seq_len, hyps)
    on_2 = np.array([utt == 2 for utt, _ in hyps])
    assert on_2.any() and np.isnan(score[on_2]).all() and (status == 0).all()
    assert np.array_equal(_bits(score[~on_2]), _bits(base[~on_2]))
    utt = [u for u, _ in hyps]
    flat, offsets = _pack([label for _, label in hyps])
    loss, _, _ = hip.ctc_loss_fwd_bwd(_t(inside[:, utt]), _t(flat, torch.int32),
                                      _t(offsets, torch.int32), _t(seq_len[utt], torch.int32),
                                      96, blank=BLANK)
    assert np.array_equal(np.isnan(loss.cpu().numpy()), on_2)


def test_per_frame_shifts_move_no_score(hip, bank):
    """Every frame shifted by an amount of its own in [-50, 50]: log-softmax takes it out."""
    logits, seq_len, hyps, want = bank
    rng = np.random.default_rng(50)
    shift = rng.uniform(-50, 50, size=(STEPS, 4, 1)).astype(np.float32)
    shift[::7] = 50.0
    shift[3::7] = -50.0
    score, _ = _score(hip, logits + shift, seq_len, hyps)
    _assert_close(score, want, factor=2.0, what='shifted by +-50')


# ------------------------------------------------------------------------------------------------
# With the beam: a pruned beam sums a subset of the alignments
# ------------------------------------------------------------------------------------------------
def _nbest_hyps(hip, logits, seq_len, width, top_paths, blank):
    out, out_len, logp, n_paths = hip.ctc_beam_decode_nbest(
        _t(logits), _t(seq_len, torch.int32), width, top_paths, blank=blank,
        normalization='log_softmax')
    out, out_len, logp, n_paths = (x.cpu().numpy() for x in (out, out_len, logp, n_paths))
    hyps, beam = [], []
    for b in range(logits.shape[1]):
        for k in range(int(n_paths[b])):
            hyps.append((b, out[b, k, :out_len[b, k]].tolist()))
            beam.append(logp[b, k])
    return hyps, np.array(beam, dtype=np.float64)


@pytest.mark.parametrize('classes,blank', [(29, 28), (5, 2)])
@pytest.mark.parametrize('shape', [(12, 8, 4), (30, 16, 8), (40, 32, 8), (60, 32, 16)],
                         ids=lambda s: 'T{}-W{}-N{}'.format(*s))
def test_exact_score_is_no_less_than_the_pruned_beams_total(hip, shape, classes, blank):
    num_steps, width, top_paths = shape
    for scale in (1.0, 3.0):
        rng = np.random.default_rng(num_steps + classes + int(scale))
        logits = (rng.normal(size=(num_steps, 3, classes)) * scale).astype(np.float32)
        seq_len = np.array([num_steps, num_steps - 3, num_steps], dtype=np.int32)
        hyps, beam = _nbest_hyps(hip, logits, seq_len, width, top_paths, blank)
        score, status = _score(hip, logits, seq_len, hyps, blank=blank)
        assert (status == 0).all()
        assert (score >= beam - 1e-3).all(), (score - beam).min()
        print('{} C {} x{}: exact - beam total in [{:.3g}, {:.3g}]'.format(
            shape, classes, scale, (score - beam).min(), (score - beam).max()))


def test_exact_score_equals_the_unpruned_beams_total(hip):
    """C = 3, T = 5, width 1024: nothing is pruned, so the totals are the exact scores."""
    rng = np.random.default_rng(35)
    logits = (rng.normal(size=(5, 4, 3)) * 2).astype(np.float32)
    seq_len = np.full(4, 5, dtype=np.int32)
    hyps, beam = _nbest_hyps(hip, logits, seq_len, 1024, 63, 2)
    score, status = _score(hip, logits, seq_len, hyps, blank=2)
    assert (status == 0).all() and len(hyps) > 4 * 20
    assert np.abs(score - beam).max() <= 1e-3
    for (utt, label), got in zip(hyps, score):
        post = octc.brute_force_posteriors(logits[:, utt].astype(np.float64), 2)
        assert abs(np.exp(float(got)) - post[tuple(label)]) <= 1e-5
