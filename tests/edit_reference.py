"""Edit distance with error counts for the tests of ``ctcasr_edit_distance``.

The rule the kernel documents (include/ctcasr.h, K13): unit costs, and among all alignments of
minimum distance the one with the fewest substitutions - the lexicographic minimum of
(distance, substitutions).  Here that is a full-matrix dynamic programme over tuples with
Python's tuple ``min``; `brute_force` enumerates every alignment instead.

For rows of thousands of symbols `error_counts_fast` runs the same rule a matrix row at a time
in numpy, and `known_edits` builds pairs whose four counts are known by construction, for rows
too long for any dynamic programme on the host.
"""

import numpy as np

_STEP = 65536      # a packed cell is distance * 65536 + substitutions; both stay below 32768


def error_counts(hyp, ref):
    """(distance, substitutions, deletions, insertions) of turning ``ref`` into ``hyp``: a
    deletion leaves a reference symbol unmatched, an insertion adds a hypothesis symbol."""
    hyp, ref = list(hyp), list(ref)
    # cell[i][j]: (distance, substitutions) of ref[:i] against hyp[:j]
    cell = [[(j, 0) for j in range(len(hyp) + 1)]]
    for i in range(1, len(ref) + 1):
        row = [(i, 0)]
        above = cell[i - 1]
        for j in range(1, len(hyp) + 1):
            if ref[i - 1] == hyp[j - 1]:
                diagonal = above[j - 1]
            else:
                diagonal = (above[j - 1][0] + 1, above[j - 1][1] + 1)
            row.append(min(diagonal, (above[j][0] + 1, above[j][1]),
                           (row[j - 1][0] + 1, row[j - 1][1])))
        cell.append(row)
    distance, subs = cell[len(ref)][len(hyp)]
    return _with_counts(distance, subs, len(hyp), len(ref))


def _with_counts(distance, subs, hyp_len, ref_len):
    # D + I = distance - S and D - I = ref_len - hyp_len
    dels = (distance - subs + ref_len - hyp_len) // 2
    return distance, subs, dels, distance - subs - dels


def error_counts_fast(hyp, ref):
    """`error_counts` for long rows: the cells of one hypothesis symbol against every prefix of
    ``ref`` are one int64 vector of packed values, so the loop is over the hypothesis alone."""
    hyp, ref = np.asarray(list(hyp)), np.asarray(list(ref))
    assert len(hyp) < 32768 and len(ref) < 32768      # the substitutions stay inside their field
    ramp = np.arange(len(ref) + 1, dtype=np.int64) * _STEP
    cells = ramp.copy()                               # no hypothesis symbol yet: all deletions
    for j, symbol in enumerate(hyp, 1):
        # without the move along the reference (a deletion after the cell above it) ...
        open_ = np.empty_like(cells)
        open_[0] = j * _STEP
        open_[1:] = np.minimum(cells[1:] + _STEP,
                               cells[:-1] + np.where(ref == symbol, 0, _STEP + 1))
        # ... which is a chain: cells[i] = min over k <= i of open_[k] + (i - k) * _STEP
        cells = np.minimum.accumulate(open_ - ramp) + ramp
    distance, subs = divmod(int(cells[-1]), _STEP)
    return _with_counts(distance, subs, len(hyp), len(ref))


def known_edits(rng, ref_len, subs, dels, ins):
    """(hyp, ref, counts): a reference of ``ref_len`` pairwise distinct int32 symbols of both
    signs and a hypothesis made from it by ``subs`` substitutions, ``dels`` deletions and ``ins``
    insertions, each edit at least two untouched symbols away from the next, the substituted and
    inserted symbols occurring nowhere else.  No alignment can share work between two such edits
    or trade one kind for another, so ``counts`` = (subs + dels + ins, subs, dels, ins)."""
    edits = subs + dels + ins
    assert ref_len >= 3 * (edits - 1) + 1, 'no room for that many isolated edits'
    fresh = ref_len + subs + ins
    pool = np.unique(rng.integers(-2 ** 31, 2 ** 31, size=fresh + fresh // 4 + 16))
    assert len(pool) >= fresh
    pool = rng.permutation(pool)[:fresh]
    ref, foreign = pool[:ref_len].tolist(), pool[ref_len:].tolist()
    # sites at least 3 apart: an insertion goes in front of its site and keeps the site's symbol
    sites = np.sort(rng.choice(ref_len - 2 * max(edits - 1, 0), size=edits, replace=False)) + \
        2 * np.arange(edits)
    kinds = rng.permutation(['s'] * subs + ['d'] * dels + ['i'] * ins)
    kind_at = dict(zip(sites.tolist(), kinds.tolist()))
    hyp = []
    for position, symbol in enumerate(ref):
        kind = kind_at.get(position)
        if kind == 'd':
            continue
        if kind == 'i':
            hyp.append(foreign.pop())
        hyp.append(foreign.pop() if kind == 's' else symbol)
    assert not foreign and len(hyp) == ref_len - dels + ins
    return hyp, ref, (edits, subs, dels, ins)


def brute_force(hyp, ref):
    """The same four numbers from the enumeration of every alignment (tiny inputs only)."""
    hyp, ref = list(hyp), list(ref)

    def walk(i, j):
        # every (substitutions, deletions, insertions) reachable from (i, j) to the end
        if i == len(ref) and j == len(hyp):
            yield (0, 0, 0)
            return
        if i < len(ref) and j < len(hyp):
            cost = 0 if ref[i] == hyp[j] else 1
            for s, d, n in walk(i + 1, j + 1):
                yield (s + cost, d, n)
        if i < len(ref):
            for s, d, n in walk(i + 1, j):
                yield (s, d + 1, n)
        if j < len(hyp):
            for s, d, n in walk(i, j + 1):
                yield (s, d, n + 1)

    best = min((s + d + n, s, d, n) for s, d, n in walk(0, 0))
    return best
