"""`ctcasr_ctc_search` (csrc/ctc_search.hip, `hip.ctc_search`, K22): CTC phrase spotting, one
wavefront per (utterance, phrase) pair with a Viterbi lattice - free start, free end - in
registers, the hits picked on the device.

Reference: tests/search_reference.py, the pinned arithmetic of include/ctcasr.h in numpy float64,
run on the table `hip.log_softmax_fwd` makes of the same logits.  From the table on, max, add and
subtract in IEEE fp64 have one answer, so EVERY comparison is exact equality - end_score,
end_start, hits, scores, counts, best and status - with no tolerance.

Phrase lengths sit on both sides of the seams of the kernel: S = 2L - 1 states against the
states-per-lane counts it is compiled for (1, 2, 3, 6, 18: S <= 64, 128, 192, 384, 1152, that is
L <= 32, 64, 96, 192, 576), and the number of pairs crosses the four a workgroup takes."""

import numpy as np
import pytest
import torch

from tests import search_reference as sref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CLASSES, BLANK = 29, 28
NEG = -np.inf
OUTPUTS = ('hits', 'hit_score', 'n_hits', 'best_score', 'best_span', 'end_score', 'end_start',
           'status')
BAD_ARGUMENT, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _pack(phrases):
    offsets = np.zeros(len(phrases) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(row) for row in phrases])
    flat = np.array([v for row in phrases for v in row] or [0], dtype=np.int32)
    return flat, offsets


def _run(hip, logits, seq_len, phrases, pairs, min_score, max_hits=4, blank=BLANK,
         max_label_len=None, per_frame=True, workspace=None):
    """`hip.ctc_search` on host data; ``pairs`` is a list of (utt, phrase).  Returns a dict of
    host arrays named as `OUTPUTS` (the per-frame ones None without ``per_frame``)."""
    flat, offsets = _pack(phrases)
    lg = logits if torch.is_tensor(logits) else _t(logits)
    out = hip.ctc_search(lg, _t(np.asarray(seq_len), torch.int32), _t(flat, torch.int32),
                         _t(offsets, torch.int32),
                         _t(np.array([u for u, _ in pairs]), torch.int32),
                         _t(np.array([p for _, p in pairs]), torch.int32),
                         _t(np.asarray(min_score, dtype=np.float64), torch.float64),
                         max_hits=max_hits, max_label_len=max_label_len, blank=blank,
                         per_frame=per_frame, workspace=workspace)
    return {name: None if value is None else value.cpu().numpy()
            for name, value in zip(OUTPUTS, out)}


def _want(hip, logits, seq_len, phrases, pairs, min_score, max_hits=4, blank=BLANK,
          max_label_len=None):
    lg = logits if torch.is_tensor(logits) else _t(logits)
    table = hip.log_softmax_fwd(lg).cpu().numpy()
    return sref.search(table, seq_len, blank, phrases, min_score, [u for u, _ in pairs],
                       [p for _, p in pairs], max_hits, max_label_len)


def _same(got, want, what='', names=OUTPUTS):
    """Exact equality, NaN equal to NaN, of every output (dtype and shape included)."""
    for name in names:
        a, b = got[name], want[name]
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert a.dtype == b.dtype, (what, name, a.dtype, b.dtype)
        if not np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'):
            where = np.argwhere(~((a == b) | ((a != a) & (b != b))))[:5]
            raise AssertionError('{} {}: differs at {} (got {}, want {})'.format(
                what, name, where.tolist(), [a[tuple(w)] for w in where],
                [b[tuple(w)] for w in where]))


def _check(hip, logits, seq_len, phrases, pairs, min_score, what='', **kwargs):
    got = _run(hip, logits, seq_len, phrases, pairs, min_score, **kwargs)
    kwargs.pop('per_frame', None)
    kwargs.pop('workspace', None)
    want = _want(hip, logits, seq_len, phrases, pairs, min_score, **kwargs)
    _same(got, want, what)
    return got, want


def _random_label(rng, length, classes=CLASSES, blank=BLANK):
    ids = [c for c in range(classes) if c != blank]
    return [ids[int(i)] for i in rng.integers(0, len(ids), size=length)]


def _peaked(rng, steps, label, blank=BLANK, classes=CLASSES, peak=6.0):
    """Random logits [steps, classes] with ``label`` raised along a legal path that fills the
    frames: one frame a label, a blank between equal neighbours, the rest on the last label."""
    logits = rng.normal(size=(steps, classes)).astype(np.float32)
    t = 2
    for i, c in enumerate(label):
        if i and label[i - 1] == c and t < steps:
            logits[t, blank] += peak
            t += 1
        if t < steps:
            logits[t, c] += peak
            t += 1
    return logits


def _plant(logits, b, lab, at, run, gap, blank=BLANK, peak=9.0):
    """Raise ``lab`` of utterance b on consecutive frames from ``at``: ``run`` frames a label,
    ``gap`` blanks between labels (one at least between equal ones).  The first label is pushed
    down in the frame before and the last in the frame after, so that the span of the greedy path
    is exactly the planted one.  Returns (first, last) frame."""
    logits[at - 1, b, lab[0]] -= 20.0
    t = at
    for i, c in enumerate(lab):
        if i:
            for _ in range(max(gap, 1 if lab[i - 1] == c else 0)):
                logits[t, b, blank] += peak
                t += 1
        for _ in range(run):
            logits[t, b, c] += peak
            t += 1
    logits[t, b, lab[-1]] -= 20.0
    return at, t - 1


# ---- tier seams ---------------------------------------------------------------------------------

SEAMS = [(32, 2), (33, 3), (64, 3), (65, 6), (96, 6), (97, 18), (192, 18), (193, None),
         (576, None)]


@pytest.mark.parametrize('length,next_tier', SEAMS)
def test_both_sides_of_every_tier_seam(hip, length, next_tier):
    """L on both sides of every seam, T = L + 8 frames, one utterance, random and peaked logits;
    the same pair through a call whose max_label_len forces the next tier up: identical bits."""
    rng = np.random.default_rng(100 + length)
    label = _random_label(rng, length)
    steps = length + 8 + sref.adjacent_repeats(label)
    logits = np.stack([rng.normal(size=(steps, CLASSES)).astype(np.float32),
                       _peaked(rng, steps, label)], axis=1)
    pairs = [(0, 0), (1, 0)]
    threshold = [-3.0 * length]
    got, want = _check(hip, logits, [steps, steps], [label], pairs, threshold,
                       what='L = {}'.format(length))
    assert got['status'].tolist() == [0, 0]
    assert np.isfinite(got['best_score']).all() and (got['n_hits'] >= 1).any()
    if next_tier is not None:
        # states per lane (2 * max_label_len - 1 + 63) // 64 == next_tier
        forced = (next_tier * 64 - 63) // 2 + 1
        assert (2 * forced - 1 + 63) // 64 == next_tier > (2 * length - 1 + 63) // 64
        again = _run(hip, logits, [steps, steps], [label], pairs, threshold,
                     max_label_len=forced)
        _same(again, got, 'L = {} under {} states per lane'.format(length, next_tier))


def test_the_ceiling_is_576_labels(hip):
    rng = np.random.default_rng(5)
    logits = rng.normal(size=(8, 1, CLASSES)).astype(np.float32)
    with pytest.raises(hip.CtcAsrError, match='unsupported|not supported|-2'):
        _run(hip, logits, [8], [_random_label(rng, 577)], [(0, 0)], [NEG])
    with pytest.raises(hip.CtcAsrError):
        _run(hip, logits, [8], [[1, 2]], [(0, 0)], [NEG], max_label_len=577)
    # 576 is served even where no utterance can hold it
    got = _run(hip, logits, [8], [_random_label(rng, 576)], [(0, 0)], [NEG])
    assert got['status'].tolist() == [1]


# ---- smallest cases -----------------------------------------------------------------------------

def test_smallest_phrases_and_shortest_utterances(hip):
    """L = 1 (one state: entry and exit in it), L = 2 with equal labels (no skip, the blank is
    needed), seq_len of 0, 1, L + repeats - 1 (status 1) and L + repeats."""
    rng = np.random.default_rng(7)
    steps = 9
    lens = [0, 1, 2, 3, 4, 9]
    logits = rng.normal(size=(steps, len(lens), CLASSES)).astype(np.float32)
    logits[:, 5, 5] -= 10.0           # never the greedy label there: no frame continues at 0.0
    phrases = [[5], [5, 5], [5, 6], [5, 5, 6]]
    pairs = [(b, p) for b in range(len(lens)) for p in range(len(phrases))]
    got, _ = _check(hip, logits, lens, phrases, pairs, [NEG] * 4, max_hits=3)
    need = [1, 3, 2, 4]
    assert got['status'].reshape(len(lens), 4).tolist() == \
        [[0 if n >= k else 1 for k in need] for n in lens]
    # one state: every frame is entered and left at once, the start is the frame itself
    single = got['end_start'].reshape(len(lens), 4, steps)[5, 0]
    assert single.tolist() == list(range(steps))
    # with exactly L + repeats frames the only span is the whole utterance
    exact = got['best_span'].reshape(len(lens), 4, 2)
    assert exact[3, 1].tolist() == [0, 2] and exact[2, 2].tolist() == [0, 1] and \
        exact[4, 3].tolist() == [0, 3]
    _check(hip, logits, lens, phrases, pairs, [0.0, -1.0, -2.5, -40.0], max_hits=2)


# ---- ties ---------------------------------------------------------------------------------------

def test_all_equal_logits_tie_every_path_at_zero(hip):
    logits = np.zeros((12, 1, CLASSES), dtype=np.float32)
    got, _ = _check(hip, logits, [12], [[1, 1, 2], [3]], [(0, 0), (0, 1)], [0.0, 0.0])
    assert got['end_score'][0].tolist() == [NEG] * 3 + [0.0] * 9
    assert got['end_start'][0].tolist() == [-1] * 3 + [0] * 9
    # one state: staying at 0.0 wins over entering at 0.0, so the start stays frame 0
    assert got['end_start'][1].tolist() == [0] * 12
    assert got['n_hits'].tolist() == [1, 1]
    assert got['hits'][:, 0].tolist() == [[0, 11], [0, 11]]
    assert got['hit_score'][:, 0].tolist() == [0.0, 0.0]
    assert (got['hits'][:, 1:] == -1).all() and np.isneginf(got['hit_score'][:, 1:]).all()
    assert got['best_score'].tolist() == [0.0, 0.0] and got['best_span'].tolist() == [[0, 3], [0, 0]]


@pytest.mark.parametrize('classes', [2, 29, 64])
def test_logits_on_a_grid_tie_often(hip, classes):
    """Logits on a grid of 0.25, T = 24, the blank at 0, in the middle and at C - 1."""
    rng = np.random.default_rng(classes)
    steps, batch = 24, 3
    logits = (rng.integers(-4, 5, size=(steps, batch, classes)) * 0.25).astype(np.float32)
    lg = _t(logits)
    for blank in (0, classes // 2, classes - 1):
        ids = [c for c in range(classes) if c != blank]
        phrases = [[ids[int(i)] for i in rng.integers(0, len(ids), size=n)]
                   for n in (1, 2, 3, 5, 8)]
        phrases.append([ids[0]] * 4)
        pairs = [(b, p) for b in range(batch) for p in range(len(phrases))]
        for threshold in (NEG, -1.0):
            _check(hip, lg, [24, 17, 9], phrases, pairs, [threshold * len(p) for p in phrases],
                   what='C = {}, blank {}'.format(classes, blank), blank=blank, max_hits=6)


# ---- pairs --------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def bank(hip):
    """Four utterances, five phrases (the third planted three times in utterance 1), and the
    reference of all 20 pairs, computed once."""
    rng = np.random.default_rng(11)
    steps, batch = 90, 4
    logits = rng.normal(size=(steps, batch, CLASSES)).astype(np.float32)
    phrases = [_random_label(rng, n) for n in (3, 7, 4, 12, 1)]
    phrases[2] = [4, 4, 9, 2]
    spans = [_plant(logits, 1, phrases[2], at, run, gap)
             for at, run, gap in ((5, 1, 0), (30, 2, 1), (60, 3, 0))]
    seq_len = [90, 85, 40, 61]
    lg = _t(logits)
    min_score = [-2.0 * len(p) for p in phrases]
    pairs = [(b, p) for b in range(batch) for p in range(len(phrases))]
    want = _want(hip, lg, seq_len, phrases, pairs, min_score)
    return lg, logits, seq_len, phrases, min_score, pairs, want, spans


def _rows(want, index):
    return {name: want[name][index] for name in OUTPUTS}


@pytest.mark.parametrize('count', [1, 3, 4, 5, 9])
def test_pair_counts_cross_the_pairs_per_workgroup(hip, bank, count):
    lg, _, seq_len, phrases, min_score, pairs, want, _ = bank
    chosen = [(7 * k + 3) % len(pairs) for k in range(count)]
    got = _run(hip, lg, seq_len, phrases, [pairs[k] for k in chosen], min_score)
    _same(got, _rows(want, chosen), 'H = {}'.format(count))


def test_permuted_and_duplicated_pair_lists_give_the_same_bits_per_pair(hip, bank):
    lg, _, seq_len, phrases, min_score, pairs, want, _ = bank
    got = _run(hip, lg, seq_len, phrases, pairs, min_score)
    _same(got, want, 'all pairs')
    order = np.random.default_rng(3).permutation(len(pairs)).tolist()
    _same(_run(hip, lg, seq_len, phrases, [pairs[k] for k in order], min_score),
          _rows(want, order), 'permuted')
    twice = [0, 7, 7, 7, 12, 0, 19, 7]
    _same(_run(hip, lg, seq_len, phrases, [pairs[k] for k in twice], min_score),
          _rows(want, twice), 'duplicated')
    # utterance 2 has no pair; phrase 2 is used by the three others
    some = [k for k, (b, p) in enumerate(pairs) if b != 2 and p == 2]
    assert len(some) == 3
    _same(_run(hip, lg, seq_len, phrases, [pairs[k] for k in some], min_score),
          _rows(want, some), 'an utterance without a pair')


# ---- hits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('max_hits', [0, 1, 2, 8])
def test_a_phrase_planted_three_times(hip, bank, max_hits):
    lg, _, seq_len, phrases, _, _, _, spans = bank
    got, _ = _check(hip, lg, seq_len, phrases, [(1, 2), (0, 2)], [-1.0] * 5, max_hits=max_hits)
    assert got['n_hits'][0] == 3 and got['status'].tolist() == [0, 0]
    assert got['hits'].shape == (2, max_hits, 2) and got['hit_score'].shape == (2, max_hits)
    kept = min(3, max_hits)
    assert got['hits'][0, :kept].tolist() == [list(span) for span in spans[:kept]]
    assert got['hit_score'][0, :kept].tolist() == [0.0] * kept
    assert (got['hits'][0, kept:] == -1).all() and np.isneginf(got['hit_score'][0, kept:]).all()
    assert got['best_score'][0] == 0.0 and got['best_span'][0].tolist() == list(spans[0])


def test_thresholds_of_zero_minus_infinity_and_above_every_score(hip, bank):
    lg, _, seq_len, phrases, _, pairs, want, _ = bank
    some = [pairs[k] for k in (0, 6, 7, 8, 13, 19)]
    for threshold in (0.0, NEG, np.nextafter(0.0, 1.0), np.nan):
        got, _ = _check(hip, lg, seq_len, phrases, some, [threshold] * 5, max_hits=8,
                        what='threshold {}'.format(threshold))
        if threshold != threshold or threshold > 0:
            assert (got['n_hits'] == 0).all()
        # the threshold touches nothing but the hits
        for name in ('best_score', 'best_span', 'end_score', 'end_start', 'status'):
            assert np.array_equal(got[name], want[name][[0, 6, 7, 8, 13, 19]])
    everything = _run(hip, lg, seq_len, phrases, some, [NEG] * 5, max_hits=64)
    for h in range(len(some)):
        n = int(everything['n_hits'][h])
        spans = everything['hits'][h, :n]
        assert n >= 1 and (spans[:, 0] <= spans[:, 1]).all()
        assert (spans[1:, 0] > spans[:-1, 1]).all()          # pairwise disjoint, ascending


# ---- non-finite ---------------------------------------------------------------------------------

def test_non_finite_logits(hip, bank):
    """NaN, +inf and a row of -inf inside seq_len give status 3, for that utterance's pairs
    only; the same values behind seq_len change nothing; a single -inf logit is legal."""
    lg, logits, seq_len, phrases, min_score, pairs, want, _ = bank
    assert seq_len[2] == 40 and seq_len[3] == 61
    for what, value, whole_row in (('NaN', np.nan, False), ('+inf', np.inf, False),
                                   ('a row of -inf', NEG, True)):
        behind = logits.copy()
        behind[70, 3, :] = value                      # behind utterance 3
        behind[40, 2, 5 if not whole_row else slice(None)] = value      # first frame behind 2
        _same(_run(hip, behind, seq_len, phrases, pairs, min_score), want, what + ' behind')
        inside = logits.copy()
        inside[39, 2, slice(None) if whole_row else 5] = value          # last frame of 2
        got = _run(hip, inside, seq_len, phrases, pairs, min_score)
        _same(got, _want(hip, inside, seq_len, phrases, pairs, min_score), what + ' inside')
        hit = [k for k, (b, _) in enumerate(pairs) if b == 2]
        clean = [k for k, (b, _) in enumerate(pairs) if b != 2]
        assert (got['status'][hit] == 3).all() and (got['status'][clean] == 0).all()
        assert np.isnan(got['best_score'][hit]).all() and np.isnan(got['end_score'][hit]).all()
        assert (got['n_hits'][hit] == 0).all() and (got['hits'][hit] == -1).all()
        assert np.isneginf(got['hit_score'][hit]).all() and (got['end_start'][hit] == -1).all()
        _same(_rows(got, clean), _rows(want, clean), what + ': the other utterances')
    single = logits.copy()
    single[10, 0, phrases[0][0]] = NEG
    single[11, 0, BLANK] = NEG
    got, _ = _check(hip, single, seq_len, phrases, pairs, min_score, what='one -inf logit')
    assert (got['status'] == 0).all()


# ---- bad input ----------------------------------------------------------------------------------

def test_bad_phrases_and_pairs_give_status_2(hip, bank):
    lg, _, seq_len, phrases, _, _, _, _ = bank
    bad = [phrases[0], [1, CLASSES], [-1, 2], [3, BLANK, 4], [], phrases[3]]
    pairs = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (4, 0), (-1, 0), (0, 6), (0, -1), (1, 0),
             (0, 5), (2, 0)]
    lens = list(seq_len)
    lens[1], lens[2] = 91, -1                          # seq_len > T, seq_len < 0
    got, _ = _check(hip, lg, lens, bad, pairs, [NEG] * 6, max_label_len=8)
    # (phrase 5 holds 12 labels: longer than max_label_len)
    assert got['status'].tolist() == [0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]
    rows = slice(1, None)
    assert (got['n_hits'][rows] == 0).all() and (got['best_span'][rows] == -1).all()
    assert np.isneginf(got['best_score'][rows]).all() and np.isneginf(got['end_score'][rows]).all()
    # a negative row: offsets that run backwards
    flat, offsets = _pack(bad)
    offsets = offsets.copy()
    offsets[1], offsets[2] = offsets[2], offsets[1]
    out = hip.ctc_search(lg, _t(np.asarray(seq_len), torch.int32), _t(flat, torch.int32),
                         _t(offsets, torch.int32), _t(np.array([0, 0]), torch.int32),
                         _t(np.array([1, 3]), torch.int32), _t(np.full(6, NEG), torch.float64),
                         max_hits=2, max_label_len=16)
    assert out[7].cpu().tolist() == [2, 2]


def test_each_c_level_error_code(hip):
    lib = hip.load()
    steps, batch, classes, pairs, phrases, max_hits = 6, 2, 5, 3, 2, 2
    logits = torch.zeros((steps, batch, classes), device=DEV)
    seq_len = torch.full((batch,), steps, dtype=torch.int32, device=DEV)
    labels = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)
    offsets = torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV)
    min_score = torch.zeros(phrases, dtype=torch.float64, device=DEV)
    utt = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    phrase = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    hits = torch.full((pairs, max_hits, 2), 7, dtype=torch.int32, device=DEV)
    hit_score = torch.zeros((pairs, max_hits), dtype=torch.float64, device=DEV)
    n_hits = torch.full((pairs,), 7, dtype=torch.int32, device=DEV)
    best = torch.zeros(pairs, dtype=torch.float64, device=DEV)
    span = torch.zeros((pairs, 2), dtype=torch.int32, device=DEV)
    status = torch.full((pairs,), 7, dtype=torch.int32, device=DEV)
    need = hip.ctc_search_workspace_bytes(steps, batch, classes)
    assert need >= steps * batch * (classes + 1) * 4
    assert hip.ctc_search_workspace_bytes(steps, batch, 0) == 0
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**change):
        args = dict(logits=logits.data_ptr(), seq_len=seq_len.data_ptr(), T=steps, B=batch,
                    C=classes, blank=classes - 1, labels=labels.data_ptr(),
                    offsets=offsets.data_ptr(), P=phrases, max_label_len=2,
                    min_score=min_score.data_ptr(), utt=utt.data_ptr(), phrase=phrase.data_ptr(),
                    H=pairs, max_hits=max_hits, hits=hits.data_ptr(),
                    hit_score=hit_score.data_ptr(), n_hits=n_hits.data_ptr(),
                    best=best.data_ptr(), span=span.data_ptr(), end_score=None, end_start=None,
                    status=status.data_ptr(), work=work.data_ptr(), work_bytes=need,
                    stream=stream)
        assert set(change) <= set(args)
        args.update(change)
        return lib.ctcasr_ctc_search(*args.values())

    for name in ('logits', 'seq_len', 'labels', 'offsets', 'min_score', 'utt', 'phrase', 'n_hits',
                 'best', 'span', 'status', 'hits', 'hit_score'):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    for change in (dict(T=-1), dict(B=-1), dict(P=-1), dict(H=-1), dict(max_label_len=-1),
                   dict(max_hits=-1), dict(C=1), dict(C=0), dict(blank=-1), dict(blank=classes)):
        assert call(**change) == BAD_ARGUMENT, change
    for change in (dict(C=65, blank=0), dict(max_label_len=577), dict(max_hits=1025)):
        assert call(**change) == UNSUPPORTED, change
    assert call(work_bytes=need - 1) == WORKSPACE and call(work=None) == WORKSPACE
    torch.cuda.synchronize()
    # nothing was launched by any of them
    assert status.cpu().tolist() == [7] * pairs and n_hits.cpu().tolist() == [7] * pairs
    assert call(H=0) == 0 and call(H=0, P=0) == 0
    assert call(H=0, utt=None, phrase=None, status=None, n_hits=None, best=None, span=None) == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [7] * pairs
    # no hit rows are needed where none is stored; the limits themselves are served
    assert call(max_hits=0, hits=None, hit_score=None) == 0
    assert call(max_label_len=576) == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * pairs and n_hits.cpu().tolist() == [1] * pairs
    with pytest.raises(hip.CtcAsrError, match='seq_len'):
        hip.ctc_search(logits, seq_len[:1], labels, offsets, utt, phrase, min_score)
    with pytest.raises(hip.CtcAsrError, match='pair_phrase'):
        hip.ctc_search(logits, seq_len, labels, offsets, utt, phrase[:2], min_score)
    with pytest.raises(hip.CtcAsrError, match='min_score'):
        hip.ctc_search(logits, seq_len, labels, offsets, utt, phrase, min_score[:1])
    with pytest.raises(hip.CtcAsrError, match='outside'):
        hip.ctc_search(logits, seq_len, labels[:2], offsets, utt, phrase, min_score)
    with pytest.raises(hip.CtcAsrError, match='min_score'):
        hip.ctc_search(logits, seq_len, labels, offsets, utt, phrase, min_score.float())
    with pytest.raises(hip.CtcAsrError, match='logits'):
        hip.ctc_search(logits[0], seq_len, labels, offsets, utt, phrase, min_score)
    empty = hip.ctc_search(logits, seq_len, labels, offsets, utt[:0], phrase[:0], min_score)
    assert [tuple(v.shape) for v in empty if v is not None] == \
        [(0, 16, 2), (0, 16), (0,), (0,), (0, 2), (0,)]


# ---- per-frame outputs, workspaces --------------------------------------------------------------

def test_without_the_per_frame_outputs_the_others_are_identical(hip, bank):
    lg, _, seq_len, phrases, min_score, pairs, want, _ = bank
    got = _run(hip, lg, seq_len, phrases, pairs, min_score, per_frame=False)
    assert got['end_score'] is None and got['end_start'] is None
    _same(got, want, 'per_frame=False',
          [name for name in OUTPUTS if name not in ('end_score', 'end_start')])


def test_a_reused_workspace_and_garbage_in_the_outputs_change_nothing(hip, bank):
    lg, logits, seq_len, phrases, min_score, pairs, want, _ = bank
    rng = np.random.default_rng(13)
    work = torch.randint(0, 255, (hip.ctc_search_workspace_bytes(*lg.shape) + 512,),
                         dtype=torch.uint8, device=DEV)
    _same(_run(hip, lg, seq_len, phrases, pairs, min_score, workspace=work), want, 'first use')
    # fewer frames, other data, the same workspace - against a fresh one
    for steps in (33, 90, 64):
        other = rng.normal(size=(steps, 4, CLASSES)).astype(np.float32)
        lens = [min(n, steps) for n in seq_len]
        # (the allocator hands freed blocks out again: the output tensors of the call below
        # start from whatever these leave behind)
        junk = [torch.full((len(pairs), steps), 7.5, dtype=torch.float64, device=DEV),
                torch.full((len(pairs), steps), 12345, dtype=torch.int32, device=DEV),
                torch.full((len(pairs), 4, 2), 12345, dtype=torch.int32, device=DEV),
                torch.full((len(pairs), 4), 7.5, dtype=torch.float64, device=DEV)]
        del junk
        reused = _run(hip, other, lens, phrases, pairs, min_score, workspace=work)
        fresh = _run(hip, other, lens, phrases, pairs, min_score)
        _same(reused, fresh, 'T = {}'.format(steps))
        if steps == 33:
            _same(reused, _want(hip, other, lens, phrases, pairs, min_score), 'T = 33')
    _same(_run(hip, lg, seq_len, phrases, pairs, min_score, workspace=work), want, 'last use')
    short = torch.empty(hip.ctc_search_workspace_bytes(*lg.shape) - 1, dtype=torch.uint8,
                        device=DEV)
    with pytest.raises(hip.CtcAsrError):
        _run(hip, lg, seq_len, phrases, pairs, min_score, workspace=short)
