"""Host reference of ``ctcasr_ctc_mwer`` (include/ctcasr.h, K23) in numpy float64: the arithmetic
the header pins, restated.  The log-softmax table, the extended labels and the feasibility rule are
``oracle.ctc``'s; the lattices are ``oracle.ctc.ctc_loss_single``'s recursions with the loop over
the states vectorised (tests/test_mwer_host.py holds the two against each other), so that the
longest rows the kernel serves stay quick."""

import numpy as np

from oracle import ctc as octc


def lattices(logp, label, blank):
    """(alpha [T, S], beta [T, S], ln p(label | x)) of one utterance; ``logp`` [T, C] is the
    log-softmax table, T >= 1.  beta(t, u) excludes the emission at t, as in ``oracle.ctc``."""
    ext = np.array(octc.extended_labels(label, blank), dtype=np.int64)
    size, steps = len(ext), logp.shape[0]
    skip = np.zeros(size, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    emit = logp[:, ext]                                     # [T, S]
    neg = np.full(2, -np.inf)
    alpha = np.full((steps, size), -np.inf)
    alpha[0, :2] = emit[0, :2]
    beta = np.full((steps, size), -np.inf)
    beta[steps - 1, max(size - 2, 0):] = 0.0
    with np.errstate(invalid='ignore'):
        for t in range(1, steps):
            prev = np.concatenate([neg, alpha[t - 1]])
            acc = np.logaddexp(prev[2:], prev[1:-1])
            acc = np.logaddexp(acc, np.where(skip, prev[:-2], -np.inf))
            alpha[t] = np.where(np.isneginf(acc), -np.inf, acc + emit[t])
        # u -> u + 2 is allowed where u + 2 may be entered by a skip
        allowed = np.zeros(size, dtype=bool)
        allowed[:max(size - 2, 0)] = skip[2:]
        for t in range(steps - 2, -1, -1):
            nxt = np.concatenate([beta[t + 1] + emit[t + 1], neg])
            acc = np.logaddexp(nxt[:-2], nxt[1:-1])
            beta[t] = np.logaddexp(acc, np.where(allowed, nxt[2:], -np.inf))
        log_pyx = np.logaddexp(alpha[-1, -1], alpha[-1, -2] if size > 1 else -np.inf)
    return alpha, beta, float(log_pyx)


def occupancy(logp, label, blank):
    """(occ [T, C], ln p): occ[t, k] = sum over the states u with l'[u] = k of exp(alpha + beta -
    ln p); zero throughout when ln p is -inf."""
    steps, classes = logp.shape
    occ = np.zeros((steps, classes))
    if steps == 0:
        return occ, 0.0
    alpha, beta, log_pyx = lattices(logp, label, blank)
    if np.isneginf(log_pyx):
        return occ, log_pyx
    ext = octc.extended_labels(label, blank)
    with np.errstate(invalid='ignore'):
        joint = np.exp(alpha + beta - log_pyx)
    joint[np.isnan(joint)] = 0.0                            # (-inf) + (+-inf) pairs: no path
    for u, sym in enumerate(ext):
        occ[:, sym] += joint[:, u]
    return occ, log_pyx


def row_status(label, length, steps, classes, blank, max_label_len=None):
    """K14's status of one row (0, 1 or 2; the non-finite logits of 3 are the caller's)."""
    label = [int(v) for v in label]
    if max_label_len is not None and len(label) > max_label_len:
        return 2
    if any(v < 0 or v >= classes or v == blank for v in label) or length > steps or length < 0:
        return 2
    return 1 if length < octc.required_time(label) else 0


def weights(scores, risks, valid):
    """(P, R, c) of one utterance in float64: the softmax of the valid ``scores``, the expected
    risk and c_i = P_i (W_i - R); c is zero throughout with fewer than two valid rows."""
    scores = np.asarray(scores, dtype=np.float64)
    risks = np.asarray(risks, dtype=np.float64)
    valid = np.asarray(valid, dtype=bool)
    post = np.zeros(len(scores))
    coeff = np.zeros(len(scores))
    if not valid.any():
        return post, 0.0, coeff
    peak = scores[valid].max()
    with np.errstate(invalid='ignore'):
        raw = np.ones(len(scores)) if np.isneginf(peak) else np.exp(scores - peak)
    total = 0.0
    for i in np.flatnonzero(valid):                         # ascending rank
        total += raw[i]
    expected = 0.0
    for i in np.flatnonzero(valid):
        post[i] = raw[i] / total
        expected += post[i] * risks[i]
    if valid.sum() >= 2:
        for i in np.flatnonzero(valid):
            coeff[i] = post[i] * (risks[i] - expected)
    return post, float(expected), coeff


def mwer(logits, seq_len, hyps, risks, n_hyps=None, blank=None, scale=1.0, scores=None,
         max_label_len=None):
    """The whole call.  ``logits`` [T, B, C]; ``hyps[b]`` the N label lists of utterance b,
    ``risks[b]`` their N risks, ``n_hyps[b]`` how many of them are used (default: all).
    ``scores`` ([B, N], the kernel's own fp32 scores): the weights are taken from these instead
    of the reference's ln p.  Returns a dict of float64 / int arrays: ``grad`` [T, B, C],
    ``expected_risk`` [B], ``score`` / ``posterior`` / ``status`` / ``c`` [B, N]."""
    logits = np.asarray(logits, dtype=np.float64)
    steps, batch, classes = logits.shape
    blank = classes - 1 if blank is None else blank
    nbest = len(hyps[0])
    grad = np.zeros((steps, batch, classes))
    expected = np.zeros(batch)
    score = np.full((batch, nbest), -np.inf)
    post = np.zeros((batch, nbest))
    coeff = np.zeros((batch, nbest))
    status = np.full((batch, nbest), -1, dtype=np.int64)
    for b in range(batch):
        used = nbest if n_hyps is None else min(max(int(n_hyps[b]), 0), nbest)
        length = int(seq_len[b])
        live = length if 0 <= length <= steps else 0
        with np.errstate(invalid='ignore'):
            logp = octc.log_softmax(logits[:live, b]) if live else np.zeros((0, classes))
        # a NaN or +inf logit (or a row of -inf) makes its frame's whole table row NaN
        poisoned = bool(np.isnan(logp).any())
        occs = [None] * nbest
        for i in range(used):
            status[b, i] = row_status(hyps[b][i], length, steps, classes, blank, max_label_len)
            if status[b, i] == 0 and poisoned:
                status[b, i], score[b, i] = 3, np.nan
            elif status[b, i] == 0:
                occs[i], score[b, i] = occupancy(logp, hyps[b][i], blank)
        if (status[b] == 3).any():
            expected[b] = np.nan
            post[b, status[b] == 3] = np.nan
            grad[:live, b] = np.nan
            continue
        valid = status[b] == 0
        basis = score[b] if scores is None else np.asarray(scores, dtype=np.float64)[b]
        safe_risks = np.where(valid, np.asarray(risks[b], dtype=np.float64), 0.0)
        post[b], expected[b], coeff[b] = weights(basis, safe_risks, valid)
        for i in np.flatnonzero(valid):                     # ascending rank
            grad[:live, b] += coeff[b, i] * occs[i]
    return {'grad': scale * grad, 'expected_risk': expected, 'score': score, 'posterior': post,
            'status': status, 'c': coeff}


def expected_risk(logits, hyps, risks, blank=None):
    """R of ONE utterance ([T, C] logits, all hypotheses feasible): the function whose gradient
    `mwer` claims to be, for finite differences."""
    logits = np.asarray(logits, dtype=np.float64)
    blank = logits.shape[1] - 1 if blank is None else blank
    logp = octc.log_softmax(logits)
    scores = [lattices(logp, label, blank)[2] for label in hyps]
    return weights(scores, risks, np.ones(len(hyps), dtype=bool))[1]
