"""Edit distance with error counts on the host: the tuple reference of ``ctcasr_edit_distance``
(tests/edit_reference.py) against `metrics.levenshtein` and brute-force enumeration, the host
helpers that turn integer counts into today's rates, and what the ABI entry refuses before it
touches a device."""

import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

from ctc_asr_amd import metrics
from tests import edit_reference as ref

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'reference_python.json')))


@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    return hip.load()


def _check_identities(counts, hyp, ref_seq):
    distance, subs, dels, ins = counts
    assert distance == subs + dels + ins
    assert dels - ins == len(ref_seq) - len(hyp)
    assert min(subs, dels, ins) >= 0


def test_reference_distance_is_levenshtein():
    for case in GOLD['levenshtein']:
        counts = ref.error_counts(case['a'], case['b'])
        assert counts[0] == case['distance'] == metrics.levenshtein(case['a'], case['b'])
        _check_identities(counts, case['a'], case['b'])
    rng = np.random.default_rng(13)
    for index in range(300):
        alphabet = (2, 4, 28)[index % 3]
        hyp = rng.integers(0, alphabet, size=int(rng.integers(0, 40))).tolist()
        ref_seq = rng.integers(0, alphabet, size=int(rng.integers(0, 40))).tolist()
        counts = ref.error_counts(hyp, ref_seq)
        assert counts[0] == metrics.levenshtein(hyp, ref_seq)
        _check_identities(counts, hyp, ref_seq)


def test_reference_takes_the_fewest_substitutions_among_the_shortest_alignments():
    for hyp_len, ref_len in itertools.product(range(5), repeat=2):
        for hyp in itertools.product((0, 1), repeat=hyp_len):
            for ref_seq in itertools.product((0, 1), repeat=ref_len):
                counts = ref.error_counts(hyp, ref_seq)
                assert counts == ref.brute_force(hyp, ref_seq), (hyp, ref_seq)
    # a pair where the rule decides: 'ab' -> 'ba' is two substitutions or one deletion plus one
    # insertion, both of distance 2
    assert ref.error_counts([1, 0], [0, 1]) == (2, 0, 1, 1)
    assert ref.error_counts([], []) == (0, 0, 0, 0)
    assert ref.error_counts([5, 6, 7], []) == (3, 0, 0, 3)
    assert ref.error_counts([], [5, 6]) == (2, 0, 2, 0)


def _symbols(rng, alphabet, size):
    if alphabet == 'wide':       # ids of 2^31 scale, both signs
        pool = rng.integers(-2 ** 31, 2 ** 31, size=24)
        return pool[rng.integers(0, len(pool), size=size)].tolist()
    return rng.integers(0, alphabet, size=size).tolist()


def test_fast_reference_equals_the_tuple_reference():
    rng = np.random.default_rng(61)
    lengths = [(0, 0), (0, 60), (60, 0), (1, 1), (60, 60)] + \
        [tuple(rng.integers(0, 61, size=2).tolist()) for _ in range(75)]
    for alphabet in (2, 3, 28, 'wide'):
        for hyp_len, ref_len in lengths:
            hyp, ref_seq = _symbols(rng, alphabet, hyp_len), _symbols(rng, alphabet, ref_len)
            counts = ref.error_counts_fast(hyp, ref_seq)
            assert counts == ref.error_counts(hyp, ref_seq), (alphabet, hyp, ref_seq)
            assert all(type(v) is int for v in counts)
    assert ref.error_counts_fast([1, 0], [0, 1]) == (2, 0, 1, 1)
    # symbols of any comparable kind, as `error_counts` takes them
    assert ref.error_counts_fast('a dog sat'.split(), 'the dog'.split()) == \
        ref.error_counts('a dog sat'.split(), 'the dog'.split())


def test_fast_reference_equals_brute_force_on_tiny_pairs():
    for hyp_len, ref_len in itertools.product(range(5), repeat=2):
        for hyp in itertools.product((0, 1), repeat=hyp_len):
            for ref_seq in itertools.product((0, 1), repeat=ref_len):
                assert ref.error_counts_fast(hyp, ref_seq) == ref.brute_force(hyp, ref_seq), \
                    (hyp, ref_seq)
    rng = np.random.default_rng(67)
    for _ in range(60):
        hyp = rng.integers(0, 3, size=int(rng.integers(0, 6))).tolist()
        ref_seq = rng.integers(0, 3, size=int(rng.integers(0, 6))).tolist()
        assert ref.error_counts_fast(hyp, ref_seq) == ref.brute_force(hyp, ref_seq), (hyp, ref_seq)


@pytest.mark.parametrize('ref_len,subs,dels,ins', [
    (1, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 0, 1), (7, 1, 1, 1),   # densest: 3 apart
    (300, 100, 0, 0), (300, 0, 100, 0), (300, 0, 0, 100), (300, 34, 33, 33),
    (2000, 0, 0, 0), (2000, 200, 0, 0), (2000, 0, 200, 0), (2000, 0, 0, 200),
    (2000, 60, 60, 60), (2000, 1, 300, 2), (1999, 222, 222, 222)])
def test_known_edits_are_what_the_fast_reference_finds(ref_len, subs, dels, ins):
    rng = np.random.default_rng(ref_len + 3 * subs + 5 * dels + 7 * ins)
    hyp, ref_seq, counts = ref.known_edits(rng, ref_len, subs, dels, ins)
    assert counts == (subs + dels + ins, subs, dels, ins)
    assert len(ref_seq) == ref_len == len(set(ref_seq)) and len(hyp) == ref_len - dels + ins
    assert min(ref_seq) < 0 < max(ref_seq) or ref_len < 8
    assert all(-2 ** 31 <= v < 2 ** 31 for v in hyp + ref_seq)
    assert len(set(hyp) - set(ref_seq)) == subs + ins
    # every edit is at least two untouched symbols away from the next
    kept = set(ref_seq) & set(hyp)
    touched = [i for i, v in enumerate(hyp) if v not in kept]
    assert all(b - a >= 3 for a, b in zip(touched, touched[1:]))
    assert ref.error_counts_fast(hyp, ref_seq) == counts
    if ref_len <= 300:
        assert ref.error_counts(hyp, ref_seq) == counts


def test_known_edits_refuses_more_edits_than_fit():
    with pytest.raises(AssertionError, match='no room'):
        ref.known_edits(np.random.default_rng(0), 6, 1, 1, 1)


def test_word_ids_split_as_wer_does():
    originals = ['the cat  sat', b'caf\xc3\xa9 au lait', '', ' a\tb\nc ']
    results = [b'the cat sat on', 'cafe au  lait', 'x', 'a b']
    original_ids, result_ids = metrics.word_ids(originals, results)
    for original, result, o_ids, r_ids in zip(originals, results, original_ids, result_ids):
        original = original.decode('utf-8') if isinstance(original, bytes) else original
        result = result.decode('utf-8') if isinstance(result, bytes) else result
        assert len(o_ids) == len(original.split()) and len(r_ids) == len(result.split())
        assert all(isinstance(v, int) for v in o_ids + r_ids)
        assert metrics.levenshtein(o_ids, r_ids) == \
            metrics.levenshtein(original.split(), result.split())
    # one dictionary per call: equal words share an id across utterances and sides
    table = {}
    for text, ids in zip(originals + results, original_ids + result_ids):
        text = text.decode('utf-8') if isinstance(text, bytes) else text
        for word, idx in zip(text.split(), ids):
            assert table.setdefault(word, idx) == idx
    assert len(set(table.values())) == len(table)


def _bits(array):
    return np.asarray(array, dtype=np.float32).view(np.uint32).tolist()


def test_rates_from_counts_are_the_host_rates_bit_for_bit():
    batch = GOLD['wer_batch']
    original_ids, result_ids = metrics.word_ids(batch['originals'], batch['results'])
    distances = [ref.error_counts(r, o)[0] for o, r in zip(original_ids, result_ids)]
    rates, mean = metrics.wer_batch_from_counts(distances, [len(o) for o in original_ids])
    want_rates, want_mean = metrics.wer_batch(batch['originals'], batch['results'])
    assert rates.dtype == want_rates.dtype and mean.dtype == want_mean.dtype
    assert rates.shape == want_rates.shape and mean.shape == want_mean.shape
    assert _bits(rates) == _bits(want_rates) and _bits(mean) == _bits(want_mean)
    with pytest.raises(ZeroDivisionError):
        metrics.wer_batch_from_counts([1], [0])
    with pytest.raises(ZeroDivisionError):
        metrics.wer_batch(['   '], ['a'])
    with pytest.raises(AssertionError):
        metrics.wer_batch_from_counts([1, 2], [3])

    rng = np.random.default_rng(5)
    hyps = [rng.integers(1, 29, size=int(n)).tolist() for n in (0, 3, 0, 7, 40, 1)]
    truths = [rng.integers(1, 29, size=int(n)).tolist() for n in (0, 0, 4, 9, 37, 1)]
    distances = np.array([ref.error_counts(h, t)[0] for h, t in zip(hyps, truths)],
                         dtype=np.int32)
    lengths = np.array([len(t) for t in truths])
    for normalize in (True, False):
        got, got_mean = metrics.edit_distance_batch_from_counts(distances, lengths, normalize)
        want, want_mean = metrics.edit_distance_batch(hyps, truths, normalize)
        assert got.dtype == want.dtype and got_mean.dtype == want_mean.dtype
        assert _bits(got) == _bits(want) and _bits(got_mean) == _bits(want_mean)
    got, _ = metrics.edit_distance_batch_from_counts(distances, lengths)
    assert got[0] == 0.0 and np.isinf(got[1])       # empty truth: 0 for an empty hypothesis
    empty, empty_mean = metrics.edit_distance_batch_from_counts([], [])
    want, want_mean = metrics.edit_distance_batch([], [])
    assert empty.shape == want.shape and _bits(empty_mean) == _bits(want_mean)
    with pytest.raises(ValueError):
        metrics.edit_distance_batch_from_counts([1], [1, 2])


def test_abi_refuses_bad_arguments_without_a_device(lib):
    p = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before launch
    null = ctypes.c_void_p(0)

    def call(hyp=p, hyp_off=p, hyp_len=p, ref_=p, ref_off=p, ref_len=p, batch=4, max_hyp=10,
             max_ref=10, distance=p, status=p, workspace=null, workspace_bytes=0):
        return lib.ctcasr_edit_distance(hyp, hyp_off, hyp_len, ref_, ref_off, ref_len, batch,
                                        max_hyp, max_ref, distance, null, null, null, status,
                                        workspace, workspace_bytes, null)

    for name in ('hyp', 'hyp_off', 'hyp_len', 'ref_', 'ref_off', 'ref_len', 'distance',
                 'status'):
        assert call(**{name: null}) == -1, name
    assert call(batch=0) == -1
    assert call(batch=-3) == -1
    assert call(max_hyp=-1) == -1
    assert call(max_hyp=32768) == -2
    assert call(max_ref=32768) == -2
    # a reference side too long for the carry columns to stay in LDS needs the workspace
    need = lib.ctcasr_edit_distance_workspace_bytes(4, 10, 20000)
    assert need > 0
    assert call(max_ref=20000) == -3
    assert call(max_ref=20000, workspace=p, workspace_bytes=need - 1) == -3


def test_workspace_query_is_host_arithmetic_and_monotone(lib):
    query = lib.ctcasr_edit_distance_workspace_bytes
    assert query(0, 10, 10) == 0
    assert query(176, 200, 200) == 0          # an evaluation group: everything in LDS
    lengths = (0, 1, 64, 1000, 4000, 5000, 9000, 10000, 20000, 32767)
    for batch in (1, 7, 600):
        for max_hyp in lengths:
            sizes = [query(batch, max_hyp, max_ref) for max_ref in lengths]
            assert sizes == sorted(sizes)
            assert sizes[-1] >= batch * 32767 * 4
        for max_ref in lengths:
            assert len({query(batch, max_hyp, max_ref) for max_hyp in lengths}) == 1
            assert query(batch, 10, max_ref) <= query(batch + 1, 10, max_ref)


def test_wrapper_refuses_mismatched_lengths_and_cpu_tensors():
    from ctc_asr_amd import hip
    symbols = torch.zeros(12, dtype=torch.int32)
    offsets = torch.tensor([0, 4, 8], dtype=torch.int32)
    lengths = torch.tensor([4, 4, 4], dtype=torch.int32)
    with pytest.raises(hip.CtcAsrError, match='batch of 3'):
        hip.edit_distance(symbols, offsets, lengths, symbols, offsets, lengths[:2])
    with pytest.raises(hip.CtcAsrError, match='batch of 3'):
        hip.edit_distance(symbols, offsets[:1], lengths, symbols, offsets, lengths)
    with pytest.raises(hip.CtcAsrError, match='CPU tensor'):
        hip.edit_distance(symbols, offsets, lengths, symbols, offsets, lengths)
    with pytest.raises(hip.CtcAsrError, match='empty'):
        hip.edit_distance(symbols, offsets[:0], lengths[:0], symbols, offsets[:0], lengths[:0])
    with pytest.raises(ValueError):
        metrics.error_counts([[1]], [[1], [2]], 'cpu')
