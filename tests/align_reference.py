"""Float64 CTC forced alignment (Viterbi) for the tests of ``ctcasr_ctc_align``.

The rule the kernel documents (include/ctcasr.h, K11): delta_0(0) = lp_0(blank), delta_0(1) =
lp_0(l_1); delta_t(s) = lp_t(ext[s]) + max over s, s - 1 and s - 2 (s - 2 only when ext[s] is
not the blank and differs from ext[s - 2]); the path ends in S - 1 or, for L > 0, S - 2.  Ties:
strict > in the order s, s - 1, s - 2 (numpy's argmax keeps the first maximum), and S - 1 wins
over S - 2 at the end.
"""

import itertools

import numpy as np

from oracle.ctc import extended_labels, log_softmax

NEG_INF = -np.inf


def _skip_allowed(ext, blank):
    ext = np.asarray(ext)
    ok = np.zeros(len(ext), dtype=bool)
    ok[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return ok


def viterbi(logits, label, blank=None, logp=None):
    """One utterance: ``logits`` [T, C] raw values (or ``logp`` [T, C] given directly).  Returns
    (score, path of T states) or (-inf, None) when no alignment exists."""
    logp = log_softmax(logits) if logp is None else np.asarray(logp, dtype=np.float64)
    num_steps, classes = logp.shape
    blank = classes - 1 if blank is None else blank
    ext = np.asarray(extended_labels(label, blank))
    size = len(ext)
    if num_steps == 0:
        return (0.0, []) if size == 1 else (NEG_INF, None)
    skip = _skip_allowed(ext, blank)
    delta = np.full(size, NEG_INF)
    delta[0] = logp[0, blank]
    if size > 1:
        delta[1] = logp[0, ext[1]]
    moves = np.zeros((num_steps, size), dtype=np.int64)
    for t in range(1, num_steps):
        cand = np.full((3, size), NEG_INF)
        cand[0] = delta
        cand[1, 1:] = delta[:-1]
        cand[2, 2:] = np.where(skip[2:], delta[:-2], NEG_INF)
        moves[t] = np.argmax(cand, axis=0)
        delta = cand[moves[t], np.arange(size)] + logp[t, ext]
    end = size - 1
    if size > 1 and delta[size - 2] > delta[size - 1]:
        end = size - 2
    score = delta[end]
    if score == NEG_INF:
        return NEG_INF, None
    path = [end]
    for t in range(num_steps - 1, 0, -1):
        path.append(path[-1] - int(moves[t, path[-1]]))
    return float(score), path[::-1]


def margin(logits, label, path, blank=None, logp=None):
    """How much the best path beats every other alignment: best score minus the best score of a
    path through any (t, s) off ``path`` (max-sum forward + backward).  +inf when ``path`` is the
    only alignment."""
    logp = log_softmax(logits) if logp is None else np.asarray(logp, dtype=np.float64)
    num_steps, classes = logp.shape
    blank = classes - 1 if blank is None else blank
    ext = np.asarray(extended_labels(label, blank))
    size = len(ext)
    skip = _skip_allowed(ext, blank)
    fwd = np.full((num_steps, size), NEG_INF)
    fwd[0, 0] = logp[0, blank]
    if size > 1:
        fwd[0, 1] = logp[0, ext[1]]
    for t in range(1, num_steps):
        best = fwd[t - 1].copy()
        best[1:] = np.maximum(best[1:], fwd[t - 1, :-1])
        best[2:] = np.maximum(best[2:], np.where(skip[2:], fwd[t - 1, :-2], NEG_INF))
        fwd[t] = best + logp[t, ext]
    bwd = np.full((num_steps, size), NEG_INF)      # excludes the emission at t
    bwd[-1, size - 1] = 0.0
    if size > 1:
        bwd[-1, size - 2] = 0.0
    for t in range(num_steps - 2, -1, -1):
        nxt = bwd[t + 1] + logp[t + 1, ext]
        best = nxt.copy()
        best[:-1] = np.maximum(best[:-1], nxt[1:])
        best[:-2] = np.maximum(best[:-2], np.where(skip[2:], nxt[2:], NEG_INF))
        bwd[t] = best
    through = fwd + bwd
    top = max(through[-1, size - 1], through[-1, size - 2] if size > 1 else NEG_INF)
    on_path = np.zeros_like(through, dtype=bool)
    on_path[np.arange(num_steps), path] = True
    # a second path that differs only in its end state passes through the other end node
    rival = np.max(np.where(on_path, NEG_INF, through))
    return float(top - rival) if rival != NEG_INF else np.inf


def path_classes(path, label, blank):
    """The class each frame of a state path emits."""
    ext = extended_labels(label, blank)
    return [ext[s] for s in path]


def collapse(classes, blank):
    """Merge repeats, drop blanks: the label a frame path stands for."""
    out, prev = [], None
    for c in classes:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def brute_force(logits, label, blank=None):
    """(best score, best frame-class path) over all C^T frame paths that collapse to ``label``;
    (-inf, None) when none does."""
    logp = log_softmax(logits)
    num_steps, classes = logp.shape
    blank = classes - 1 if blank is None else blank
    best, best_path = NEG_INF, None
    for seq in itertools.product(range(classes), repeat=num_steps):
        if collapse(seq, blank) != list(label):
            continue
        score = float(sum(logp[t, c] for t, c in enumerate(seq)))
        if score > best:
            best, best_path = score, list(seq)
    return best, best_path


def is_valid_path(path, label, blank, length):
    """Monotone, legal moves only, starts in {0, 1}, ends in {S - 1, S - 2}, collapses to the
    label; returns a reason string for the first violation, or None."""
    ext = extended_labels(label, blank)
    size = len(ext)
    if len(path) != length:
        return 'length {} != {}'.format(len(path), length)
    if length == 0:
        return None if size == 1 else 'empty path for a non-empty label'
    if not all(0 <= s < size for s in path):
        return 'state out of range'
    if path[0] not in (0, 1):
        return 'starts in {}'.format(path[0])
    if path[-1] not in (size - 1, size - 2):
        return 'ends in {}'.format(path[-1])
    for t in range(1, length):
        move = path[t] - path[t - 1]
        if move not in (0, 1, 2):
            return 'move {} at t = {}'.format(move, t)
        s = path[t]
        if move == 2 and (ext[s] == blank or ext[s] == ext[s - 2]):
            return 'illegal skip into {} at t = {}'.format(s, t)
    if collapse(path_classes(path, label, blank), blank) != list(label):
        return 'does not collapse to the label'
    return None


def rescore(logits, label, path, blank=None):
    """Float64 log-probability of a state path."""
    logp = log_softmax(logits)
    blank = logp.shape[1] - 1 if blank is None else blank
    ext = extended_labels(label, blank)
    return float(sum(logp[t, ext[s]] for t, s in enumerate(path)))
