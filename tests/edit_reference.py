"""Edit distance with error counts for the tests of ``ctcasr_edit_distance``.

The rule the kernel documents (include/ctcasr.h, K13): unit costs, and among all alignments of
minimum distance the one with the fewest substitutions - the lexicographic minimum of
(distance, substitutions).  Here that is a full-matrix dynamic programme over tuples with
Python's tuple ``min``; `brute_force` enumerates every alignment instead.
"""


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
