"""The CTC beam search (csrc/beam.hip, `hip.ctc_beam_decode`, `CTCModel.decode_fn` /
`decode_many`) at the shapes where it goes wrong first: the blank anywhere in [0, C), C = 2 and
C = 63 / 64 (label 63: the top bit of the 6-bit label field and of the 64-bit children mask),
widths 1023 / 1024 (slot 2047: the last value of the 11-bit slot field, all 16 key registers
of `beam_expand<16>` in use) and widths far above the number of prefixes that exist, utterances
of 0-3 frames, lengths outside [0, T], batches on both sides of 64 and 256, `-inf` logits (a
masked class), a NaN or +inf in a neighbouring row, the report of an exhausted prefix-tree pool,
and the refusals (C = 1 / 65, width 0 / 1025, a blank outside [0, C), logits that are not
[T, B, C], a `seq_len` that does not hold one length per utterance).

Parity is against the C oracle (`cref.beam_search_decode`, pinned against the numpy oracle on
these input classes in test_oracle_ctc.py) at the bars of test_gpu_kernels.py: path and length
equal, logp rtol 1e-5 / atol 1e-3 (atol 1e-2 from T = 500).  One group does not go through the
project's TensorFlow-style oracles at all: an unpruned search must return the most probable
labelling of `brute_force_posteriors` (all C^T paths, float64) and the log of its posterior.
Inputs are continuous random logits: exact ties in a total are not a parity case (beam.hip's
header)."""

import math
import time

import numpy as np
import pytest
import torch

from oracle import cref
from oracle import ctc as octc
from tests.beam_helpers import _logits, _same_bits, _t

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORMS = ['max', 'log_softmax']

MAX_WIDTH, MAX_CLASSES = 1024, 64                   # BEAM_MAX_WIDTH, BEAM_MAX_CLASSES
NODE_ID_CAP = 1 << 21                               # nodes_per_utt's ceiling (the key's id field)

# what whoever runs the module reads to report it (the asserts do not depend on it):
# {group: largest |logp - reference|}, and the wall time of the pool-exhaustion launch
MEASURED = {}


def _run(hip, logits, seq_len, width, blank=None, norm='max'):
    """The wrapper on host arrays.  Returns host (out i32[B, T], out_len i32[B], logp f32[B])."""
    out, out_len, logp = hip.ctc_beam_decode(_t(logits), _t(np.asarray(seq_len), torch.int32),
                                             width, blank=blank, normalization=norm)
    return out.cpu().numpy(), out_len.cpu().numpy(), logp.cpu().numpy()


def _check(hip, logits, seq_len, width, blank, norm, group='parity'):
    """One call against the C oracle, every row: out_len and path equal; the row zero beyond
    out_len (the wrapper allocates `out` uninitialised, so this holds the kernel's own zeroing);
    every label in [0, C) and never the blank; logp within rtol 1e-5 / atol 1e-3 (1e-2 from
    T = 500), the bars of test_gpu_kernels.py.  The oracle is given the lengths clipped to
    [0, T] (see `test_beam_lengths_outside_0_T_are_clamped`).  Returns (out, out_len, logp,
    oracle paths)."""
    num_steps, batch, classes = logits.shape
    seq_len = np.asarray(seq_len, dtype=np.int32)
    out, out_len, logp = _run(hip, logits, seq_len, width, blank, norm)
    clipped = np.clip(seq_len, 0, num_steps)
    ref_paths, ref_logp = cref.beam_search_decode(logits, clipped, width, blank, norm)
    assert out.shape == (batch, num_steps) and out_len.shape == (batch,)
    for b in range(batch):
        n = int(out_len[b])
        assert n == len(ref_paths[b]), (b, n, len(ref_paths[b]))
        assert 0 <= n <= clipped[b], (b, n)
        assert out[b, :n].tolist() == ref_paths[b], (b, width, norm)
        assert (out[b, n:] == 0).all(), b
        assert ((out[b, :n] >= 0) & (out[b, :n] < classes) & (out[b, :n] != blank)).all(), b
    err = np.abs(np.where(logp == ref_logp, 0.0, logp.astype(np.float64) - ref_logp))
    MEASURED[group] = max(MEASURED.get(group, 0.0), float(err.max()))
    print('{}: T {} B {} C {} blank {} W {} {}: max |logp - oracle| {:.3g}'.format(
        group, num_steps, batch, classes, blank, width, norm, err.max()))
    assert np.allclose(logp, ref_logp, rtol=1e-5, atol=1e-2 if num_steps >= 500 else 1e-3), \
        (logp, ref_logp)
    return out, out_len, logp, ref_paths


def _row_alone(hip, logits, seq_len, width, blank, norm, got, rows):
    """Each listed row of a batch is bit-identical (out, out_len, logp) to that utterance
    decoded alone at B = 1 with the same T."""
    out, out_len, logp = got[:3]
    for b in rows:
        one = _run(hip, logits[:, b:b + 1], seq_len[b:b + 1], width, blank, norm)
        assert _same_bits(one, (out[b:b + 1], out_len[b:b + 1], logp[b:b + 1])), b


# ------------------------------------------------------------------------------------------------
# 1. Classes and blank
# ------------------------------------------------------------------------------------------------
CLASS_CASES = [(2, 0), (2, 1), (3, 1), (29, 0), (29, 13), (29, 28), (63, 62), (64, 0), (64, 31),
               (64, 63)]


def _class_case_inputs(classes, blank):
    """T = 30, B = 6, ragged: four rows of peaked logits, two of flat ones (scale 0.3, where
    most of the beam is replaced in every frame).  For C = 64, rows 0 and 1 lean towards the
    label whose bit sits at the top of the packed fields - 63, or 62 when 63 is the blank - on
    every fourth frame, row 1 also towards the label below it; the flat rows lean towards a
    pair of labels 32 apart, which a label field cut to 5 bits would confuse.  Returns (logits,
    seq_len, that top label or None)."""
    rng = np.random.default_rng(1000 * classes + blank)
    logits = _logits(rng, 30, 6, classes, blank)
    logits[:, 4:] = _logits(rng, 30, 2, classes, blank, scale=0.3, blank_bias=0.0)
    seq_len = np.array([30, 17, 1, 23, 30, 26], dtype=np.int32)
    top = None
    if classes == MAX_CLASSES:
        top = 62 if blank == 63 else 63
        logits[1::4, 0, top] += 7.0
        logits[2::4, 1, top] += 7.0
        logits[0::4, 1, top - 1] += 7.0
        low = 30 if blank in (31, 63) else 31
        logits[:, 4:, [low, low + 32]] += 1.5
    return logits, seq_len, top


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('classes,blank', CLASS_CASES)
def test_beam_classes_and_blank(hip, classes, blank, norm):
    """The blank at 0, mid and C - 1, from C = 2 (one label) to C = 64 (every bit of the
    children mask), at widths 1, 8 and 100.  The kernel reads `blank` in three places (the
    blank's frame value, the children it proposes, the repeated-label compare); a `C - 1`
    hard-wired into any of them fails here.  For C = 64 the oracle's own paths must hold label
    63 (with blank = 63: label 62), so the case cannot silently stop covering the top bit."""
    logits, seq_len, top = _class_case_inputs(classes, blank)
    for width in (1, 8, 100):
        _, _, _, ref_paths = _check(hip, logits, seq_len, width, blank, norm, 'classes and blank')
        if top is not None:
            assert top in ref_paths[0] and top in ref_paths[1], (top, width, ref_paths[:2])


@pytest.mark.parametrize('classes,blank', [(65, 64), (65, 0), (1, 0), (29, 29), (29, -1), (2, 2),
                                           (64, 64)])
def test_beam_class_count_and_blank_refused(hip, classes, blank):
    logits = np.zeros((4, 2, classes), dtype=np.float32)
    with pytest.raises(hip.CtcAsrError):
        _run(hip, logits, [4, 4], 8, blank=blank)


# ------------------------------------------------------------------------------------------------
# 2. Width seams at full size
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('width', [1023, 1024])
@pytest.mark.parametrize('classes,blank', [(29, 28), (64, 63), (64, 20)])
def test_beam_width_ceiling(hip, classes, blank, width, norm):
    """T = 120, B = 2, flat logits (scale 0.3: every frame replaces most of the beam, the churn
    worst case), so the beam is full from the third frame on and every one of the 2 * W slots
    is handed out: at width 1024 that includes slot 2047, the last value of the 11-bit slot
    field of the heap and sort keys, and position 1023, register 15 of lane 63.

    A thousand float32 totals a few units apart lie a few ulp from each other, so on such
    inputs one eviction can hang on the last bit of an exp or a log.  The inputs here (seed
    1000 + C + W) are ones whose answer the oracle keeps, all twelve cases, when its ties go to
    the younger node, to a hashed order or to the node that entered the beam first, and when
    half of its exp / log results are moved by one ulp (24 random streams each).  Seed C + W
    was not: for (29, 28, 1023, log_softmax) the oracle itself gave a second answer from frame
    86 on under 6 of 40 such streams - the answer the kernel gave; that input was dropped as a
    near-tie, no assertion changed.  (At T = 60 the kernel equals the oracle at its own width
    and at neither neighbouring width on 480 rows each of widths 1022 / 1023 / 1024.)"""
    rng = np.random.default_rng(1000 + classes + width)
    logits = _logits(rng, 120, 2, classes, blank, scale=0.3, blank_bias=0.0)
    _check(hip, logits, [120, 97], width, blank, norm, 'width ceiling')


@pytest.mark.parametrize('width', [1025, 2048, 0, -3])
def test_beam_width_refused(hip, width):
    logits = np.zeros((4, 2, 29), dtype=np.float32)
    with pytest.raises(hip.CtcAsrError):
        _run(hip, logits, [4, 4], width)


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('width', [64, 1024])
@pytest.mark.parametrize('blank', [0, 2])
def test_beam_wider_than_the_prefix_tree(hip, blank, width, norm):
    """C = 3, T = 4: 15 labellings fit into four frames (a repeated label needs a blank in
    between) and the oracle's count of prefixes that entered the beam says that all of them did,
    so the beam is never full (`nheap < W` for the whole search) and nothing is ever evicted."""
    rng = np.random.default_rng(40 + blank)
    logits = _logits(rng, 4, 3, 3, blank)
    seq_len = np.array([4, 2, 3], dtype=np.int32)
    _, _, nodes = cref.beam_search_decode(logits, seq_len, width, blank, norm, return_nodes=True)
    assert nodes.tolist() == [15, 5, 9] == [
        len(octc.brute_force_posteriors(logits[:n, b], blank)) for b, n in enumerate(seq_len)]
    _check(hip, logits, seq_len, width, blank, norm, 'width >> prefixes')


# ------------------------------------------------------------------------------------------------
# 3. Lengths
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('batch', [1, 5])
@pytest.mark.parametrize('num_steps', [1, 2, 3])
def test_beam_one_to_three_frames(hip, num_steps, batch, norm):
    rng = np.random.default_rng(10 * num_steps + batch)
    for classes, blank in ((29, 28), (5, 0)):
        logits = _logits(rng, num_steps, batch, classes, blank)
        seq_len = np.array([num_steps, 1, 0, num_steps, max(1, num_steps - 1)][:batch],
                           dtype=np.int32)
        for width in (1, 8, 1024):
            _check(hip, logits, seq_len, width, blank, norm, 'T = 1-3')


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('lengths', [[0, 12, 1, 0], [0, 0, 0, 0], [0]])
def test_beam_rows_of_length_zero(hip, lengths, norm):
    """A row of length 0 decodes to nothing: out_len 0, logp exactly 0 (the empty prefix with
    probability 1), a row of zeros - and the oracle says the same."""
    rng = np.random.default_rng(len(lengths))
    logits = _logits(rng, 12, len(lengths), 29, 28)
    for width in (1, 64):
        out, out_len, logp, _ = _check(hip, logits, lengths, width, 28, norm, 'length 0')
        for b, length in enumerate(lengths):
            if length == 0:
                assert out_len[b] == 0 and logp[b] == 0.0 and (out[b] == 0).all()


@pytest.mark.parametrize('norm', NORMS)
def test_beam_lengths_outside_0_T_are_clamped(hip, norm):
    """seq_len > T decodes T frames, seq_len < 0 decodes none: the beam search CLAMPS, like
    `ctc_greedy_decode` (test_gpu_ctc_edges.py::test_greedy_decode_ties_and_lengths) - the
    decoders have no per-row status to report through, unlike `ctc_loss_fwd_bwd`, which marks
    such a row with status 2.  Bit for bit the result of the clamped lengths, and the oracle's
    for them."""
    num_steps = 20
    rng = np.random.default_rng(33)
    logits = _logits(rng, num_steps, 5, 29, 28)
    wild = np.array([num_steps + 7, -2, num_steps, 3, 2 ** 31 - 1], dtype=np.int32)
    tame = np.array([num_steps, 0, num_steps, 3, num_steps], dtype=np.int32)
    for width in (8, 100):
        got = _check(hip, logits, wild, width, 28, norm, 'clamped lengths')
        assert got[1][1] == 0 and got[2][1] == 0.0
        assert _same_bits(got[:3], _run(hip, logits, tame, width, 28, norm))


@pytest.mark.parametrize('norm', NORMS)
def test_beam_frames_past_the_length_are_never_read(hip, norm):
    """`decode_many` pads short batches inside a joint tensor and relies on this: NaN in the
    frames t >= seq_len[b] gives bit for bit the result of zeros there."""
    num_steps = 24
    rng = np.random.default_rng(34)
    logits = _logits(rng, num_steps, 4, 29, 28)
    seq_len = np.array([num_steps, 9, 0, 1], dtype=np.int32)
    zeros, nans = logits.copy(), logits.copy()
    for b, length in enumerate(seq_len):
        zeros[length:, b] = 0.0
        nans[length:, b] = np.nan
    for width in (8, 100):
        want = _check(hip, zeros, seq_len, width, 28, norm, 'frames past len')
        assert _same_bits(_run(hip, nans, seq_len, width, 28, norm), want[:3])


# ------------------------------------------------------------------------------------------------
# 4. Batch
# ------------------------------------------------------------------------------------------------
def _ragged(rng, batch, num_steps):
    seq_len = rng.integers(0, num_steps + 1, size=batch).astype(np.int32)
    seq_len[0], seq_len[1], seq_len[batch // 2], seq_len[-1] = num_steps, 0, 1, num_steps
    return seq_len


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('batch', [63, 64, 65, 256, 300])
def test_beam_batch_sizes(hip, batch, norm):
    """One workgroup per utterance, on both sides of 64 and of the 256 CUs (and of the 256
    utterances `decode_many` launches at most): width 64, T = 50, ragged lengths with 0 and 1;
    every row against the oracle, and rows from the start, the middle and the end decoded
    alone must come out bit-identical - a search does not depend on its neighbours."""
    rng = np.random.default_rng(batch)
    seq_len = _ragged(rng, batch, 50)
    logits = _logits(rng, 50, batch, 29, 28)
    got = _check(hip, logits, seq_len, 64, 28, norm, 'batch')
    _row_alone(hip, logits, seq_len, 64, 28, norm, got, (0, 1, batch // 2, batch - 2, batch - 1))


@pytest.mark.parametrize('norm', NORMS)
def test_beam_batch_256_at_full_width(hip, norm):
    """B = 256 at width 1024, T = 20: every CU holds a full-size beam (~120 KB of LDS) and the
    pool is 4 W T + 64 K nodes per row."""
    batch, num_steps, classes = 256, 20, 29
    need = hip.ctc_beam_workspace_bytes(num_steps, batch, classes, MAX_WIDTH)
    nodes = 4 * MAX_WIDTH * num_steps + 65536
    assert need == batch * nodes * (3 + classes) * 4 + 256           # 4.8 GB
    if need > 48 << 30:
        pytest.skip('workspace {} B exceeds the 48 GB budget of decode_group_size'.format(need))
    rng = np.random.default_rng(256)
    seq_len = _ragged(rng, batch, num_steps)
    logits = _logits(rng, num_steps, batch, classes, 28, scale=1.0)
    got = _check(hip, logits, seq_len, MAX_WIDTH, 28, norm, 'batch 256, width 1024')
    _row_alone(hip, logits, seq_len, MAX_WIDTH, 28, norm, got, (0, 131, 255))


# ------------------------------------------------------------------------------------------------
# 5. Independent truth
# ------------------------------------------------------------------------------------------------
TRUTH_SEEDS = 10
TRUTH_CASES = [(2, 10), (3, 9), (4, 5), (5, 4)]


def _truth_inputs(classes, num_steps, blank):
    """TRUTH_SEEDS utterances as one batch, and per utterance the two most probable labellings
    of the exhaustive enumeration: (label, p), (runner-up, p)."""
    rng = np.random.default_rng(10000 * classes + 100 * num_steps + blank)
    logits = (rng.normal(size=(num_steps, TRUTH_SEEDS, classes)) * 2).astype(np.float32)
    ranked = []
    for b in range(TRUTH_SEEDS):
        post = octc.brute_force_posteriors(logits[:, b].astype(np.float64), blank)
        assert abs(sum(post.values()) - 1.0) < 1e-12
        ranked.append(sorted(post.items(), key=lambda kv: -kv[1])[:2])
    return logits, ranked


@pytest.mark.parametrize('classes,num_steps', TRUTH_CASES)
def test_beam_unpruned_search_finds_the_most_probable_labelling(hip, classes, num_steps):
    """Not through the TensorFlow-style oracles: at most 1023 prefixes exist for these (C, T),
    so width 1024 prunes nothing and, with `log_softmax`, the winner's total is the exact CTC
    posterior of its labelling.  The GPU path must be the argmax of `brute_force_posteriors`
    (float64, all C^T paths) and logp its logarithm within rtol 1e-5 (no absolute term).  A
    seed whose two best posteriors are closer than 1e-4 relative is a near-tie and is skipped;
    the inputs are fixed so that at most 1 seed in 10 is, asserted below."""
    assert sum((classes - 1) ** k for k in range(num_steps + 1)) <= 1023
    for blank in sorted({0, classes // 2, classes - 1}):
        logits, ranked = _truth_inputs(classes, num_steps, blank)
        out, out_len, logp = _run(hip, logits, [num_steps] * TRUTH_SEEDS, MAX_WIDTH, blank,
                                  'log_softmax')
        skipped, worst = 0, 0.0
        for b, ((best, p_best), (_, p_next)) in enumerate(ranked):
            if p_best - p_next < 1e-4 * p_best:
                skipped += 1
                continue
            assert tuple(out[b, :out_len[b]].tolist()) == best, (blank, b)
            rel = abs(float(logp[b]) - math.log(p_best)) / abs(math.log(p_best))
            worst = max(worst, rel)
            assert rel <= 1e-5, (blank, b, float(logp[b]), math.log(p_best))
            assert math.exp(float(logp[b])) == pytest.approx(p_best, rel=1e-5 * abs(
                math.log(p_best)) + 1e-7)
        print('truth C {} T {} blank {}: skipped {} of {}, max rel |logp - ln p| {:.3g}'.format(
            classes, num_steps, blank, skipped, TRUTH_SEEDS, worst))
        MEASURED['truth rel'] = max(MEASURED.get('truth rel', 0.0), worst)
        assert skipped * 10 <= TRUTH_SEEDS, skipped


# ------------------------------------------------------------------------------------------------
# 6. Masked classes
# ------------------------------------------------------------------------------------------------
def _masked_inputs(kind, blank, classes=29):
    rng = np.random.default_rng(60 + blank)
    logits = _logits(rng, 30, 3, classes, blank)
    label = 5
    if kind == 'class, every frame':
        logits[:, :, label] = -np.inf
    elif kind == 'class, alternate frames':
        logits[0::2, 0, label] = -np.inf
        logits[1::2, 1:, label] = -np.inf
        logits[1::2, 0, label] += 4.0        # ... and likely where it is allowed
        logits[0::2, 1:, label] += 4.0
    else:
        logits[0::3, 0, blank] = -np.inf     # the first frame too: the empty prefix dies at once
        logits[2::3, 1:, blank] = -np.inf
    return logits, np.array([30, 30, 19], dtype=np.int32)


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('blank', [28, 0])
@pytest.mark.parametrize('kind', ['class, every frame', 'class, alternate frames',
                                  'blank, some frames'])
def test_beam_masked_classes(hip, kind, blank, norm):
    """A class at -inf (probability 0): for every frame, on alternate frames, and the blank on
    every third frame.  `lse2f` must pass -inf through (hi + log1p(exp(lo - hi)) is NaN for two
    -inf), a child through a masked class must not enter, and a leaf whose total falls to -inf
    must neither expand nor win."""
    logits, seq_len = _masked_inputs(kind, blank)
    for width in (1, 8, 100):
        out, out_len, logp, _ = _check(hip, logits, seq_len, width, blank, norm, 'masked')
        assert np.isfinite(logp).all()
        if kind == 'class, every frame':
            assert all(5 not in out[b, :out_len[b]] for b in range(3))


# ------------------------------------------------------------------------------------------------
# 7. Non-finite poison does not spread
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('poison', [np.nan, np.inf])
def test_beam_non_finite_row_does_not_spread(hip, poison, norm):
    """A NaN or +inf in one frame of one row - what a half-trained model can emit.  That row has
    no defined answer; it must still come back in range (0 <= out_len <= len, labels in [0, C),
    zero beyond out_len), and the three other rows bit for bit as without the poison.  (Every
    loop of the kernel is bounded by the heap size, C, the slot count or the acyclic parent
    chain, none by a float compare, so the row cannot hold its workgroup up.)"""
    rng = np.random.default_rng(70)
    clean = _logits(rng, 30, 4, 29, 28)
    seq_len = np.array([30, 26, 30, 11], dtype=np.int32)
    dirty = clean.copy()
    dirty[7, 1, 3] = poison
    for width in (8, 100):
        want = _check(hip, clean, seq_len, width, 28, norm, 'poison (clean batch)')
        out, out_len, logp = _run(hip, dirty, seq_len, width, 28, norm)
        others = [0, 2, 3]
        assert _same_bits((out[others], out_len[others], logp[others]),
                          (want[0][others], want[1][others], want[2][others]))
        n = int(out_len[1])
        assert 0 <= n <= seq_len[1]
        assert ((out[1, :n] >= 0) & (out[1, :n] < 28)).all() and (out[1, n:] == 0).all()


# ------------------------------------------------------------------------------------------------
# 8. Pool exhausted is reported
# ------------------------------------------------------------------------------------------------
# Width 1024, C = 64, logits N(0, 0.3): the oracle counts ~1040 new prefixes per frame
# (T = 1000: 0.99 M, 2000: 2.08 M, 3000: 3.13 M = 1.49 x 2^21; C = 29, T = 3000: 2.31 M), so
# T = 3200 (3.29 M = 1.57 x 2^21) clears 1.5 x 2^21 with a workspace of 2^21 nodes x 67 ints =
# 562 MB.  First run on the MI355X: 3.7 s for the launch, 8.1 s for the test.
EXHAUST_STEPS = 3200


@pytest.mark.timeout(160)          # 20 x the first run
def test_beam_pool_exhausted_is_reported(hip):
    """More prefixes than the pool can hold (2^21 nodes, the id field of the sort key): the
    kernel finishes its frames, reports out_len = -1 and the wrapper raises.  The oracle's count
    of prefixes that ever entered the beam - the nodes a create-on-entry tree makes - is at least
    1.5 x 2^21, so the case does not hang on the two implementations agreeing to the node.
    Nothing is sticky: a small batch decoded right after, on the same stream, matches the
    oracle, and so does the same width on the first frames of the same utterance."""
    classes, blank = 64, 63
    rng = np.random.default_rng(8)
    logits = _logits(rng, EXHAUST_STEPS, 1, classes, blank, scale=0.3, blank_bias=0.0)
    _, _, nodes = cref.beam_search_decode(logits, [EXHAUST_STEPS], MAX_WIDTH, blank,
                                          return_nodes=True)
    assert nodes[0] >= 1.5 * NODE_ID_CAP, nodes
    need = hip.ctc_beam_workspace_bytes(EXHAUST_STEPS, 1, classes, MAX_WIDTH)
    assert need == NODE_ID_CAP * (3 + classes) * 4 + 256 and need < 1 << 30
    start = time.perf_counter()
    with pytest.raises(hip.CtcAsrError, match='pool exhausted'):
        _run(hip, logits, [EXHAUST_STEPS], MAX_WIDTH, blank)
    MEASURED['pool exhausted: seconds'] = time.perf_counter() - start
    print('pool exhausted: oracle nodes {} ({:.2f} x 2^21), launch + sync {:.2f} s'.format(
        int(nodes[0]), nodes[0] / NODE_ID_CAP, MEASURED['pool exhausted: seconds']))
    small = _logits(rng, 30, 3, 29, 28)
    _check(hip, small, [30, 12, 0], 64, 28, 'max', 'after exhaustion')
    _check(hip, logits[:100], [100], MAX_WIDTH, blank, 'max', 'after exhaustion, same width')


# ------------------------------------------------------------------------------------------------
# 9. Model level
# ------------------------------------------------------------------------------------------------
def test_decode_many_pads_short_batches_and_keeps_empty_rows():
    """`decode_many` against `decode_fn` batch by batch where the joint tensor has to pad: T'
    of 7 next to 52, a batch of one utterance, rows of length 0 (and a whole batch of them), at
    the widths 8 and 1024 - and each batch against the oracle."""
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    cfg = ModelConfig(used_model='ds2', conv_filters=(4, 4), rnn_cell='lstm', cudnn=True,
                      num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0)
    model = CTCModel(cfg, 'cuda', params=init_params(cfg, 0))
    classes = cfg.num_classes
    rng = np.random.default_rng(90)
    batches, host = [], []
    for steps, lengths in ((7, [7, 0, 3]), (52, [52]), (21, [0, 21, 1, 0]), (3, [0, 0]),
                           (52, [40, 52, 0])):
        logits = _logits(rng, steps, len(lengths), classes, classes - 1, blank_bias=1.5)
        originals = np.array(['utt {}'.format(i).encode('utf-8') for i in range(len(lengths))],
                             dtype=object)
        host.append((logits, np.array(lengths, dtype=np.int32)))
        batches.append((_t(logits), _t(np.array(lengths), torch.int32), originals))
    for width in (8, MAX_WIDTH):
        joint = model.decode_many(batches, beam_width=width)
        assert len(joint) == len(batches)
        for (logits, seq_len, originals), (np_logits, np_len), got in zip(batches, host, joint):
            ref = model.decode_fn(logits, seq_len, originals, beam_width=width)
            assert got[0] == ref[0]
            assert list(got[1]) == list(ref[1])
            assert np.array_equal(got[2], ref[2])
            assert got[0] == cref.beam_search_decode(np_logits, np_len, width)[0]
            assert all(got[0][b] == [] for b in np.flatnonzero(np_len == 0))
    # one batch of one utterance through decode_many alone
    alone = model.decode_many(batches[1:2], beam_width=64)
    assert alone[0][0] == model.decode_fn(*batches[1], beam_width=64)[0]
    assert model.decode_many([]) == []


# ------------------------------------------------------------------------------------------------
# Arguments the wrappers refuse before anything is launched
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('decoder', ['beam', 'greedy'])
def test_decoders_refuse_mismatched_seq_len_and_logits_rank(hip, decoder):
    """`seq_len` shorter than the batch would have the kernel read lengths past the tensor; the
    wrappers compare the two and name both numbers.  Logits must be [T, B, C]."""
    def call(logits, seq_len):
        if decoder == 'beam':
            return hip.ctc_beam_decode(logits, seq_len, 8)
        return hip.ctc_greedy_decode(logits, seq_len)

    logits = _t(np.zeros((6, 5, 29), dtype=np.float32))
    for count in (4, 6, 0, 1):
        with pytest.raises(hip.CtcAsrError, match='{} lengths for a batch of 5'.format(count)):
            call(logits, torch.full((count,), 6, dtype=torch.int32, device=DEV))
    for shape in ((30, 29), (870,), (6, 5, 29, 1)):
        with pytest.raises(hip.CtcAsrError, match='{} dimensions'.format(len(shape))):
            call(logits.reshape(shape), torch.full((5,), 6, dtype=torch.int32, device=DEV))
    out = call(logits, torch.full((5,), 6, dtype=torch.int32, device=DEV))
    assert out[1].shape == (5,)
