"""The pinned arithmetic of ``ctcasr_ctc_search`` (include/ctcasr.h, K22) in plain numpy float64:
loops over t and u, then the hit pass.  It runs on a log-softmax TABLE handed to it (the GPU tests
take `hip.log_softmax_fwd(logits)`): from there on max, add and subtract in IEEE fp64 have one
answer, so everything is compared for exact equality."""

import numpy as np

NEG = -np.inf


def table_of(logits):
    """A float32 log-softmax for the host tests (the GPU tests do not use it)."""
    x = np.asarray(logits, dtype=np.float32)
    mx = x.max(-1, keepdims=True)
    s = np.exp(x - mx).sum(-1, keepdims=True, dtype=np.float32)
    return (x - (mx + np.log(s))).astype(np.float32)


def fill_of(table):
    """fmaxf over the classes: a row of NaN stays NaN (a row is NaN throughout or nowhere)."""
    table = np.asarray(table, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(table).all(-1), np.float32(np.nan),
                        np.fmax.reduce(table, axis=-1)).astype(np.float32)


def adjacent_repeats(lab):
    return sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def lattice(table, lab, blank, seq_len):
    """(end_score f64[T], end_start i64[T]) of one phrase on one utterance's table [T, C]."""
    table = np.asarray(table, dtype=np.float32)
    num_steps = table.shape[0]
    states = 2 * len(lab) - 1
    ext = [lab[u // 2] if u % 2 == 0 else blank for u in range(states)]
    skip = [u >= 2 and u % 2 == 0 and lab[u // 2] != lab[u // 2 - 1] for u in range(states)]
    end_score = np.full(num_steps, NEG)
    end_start = np.full(num_steps, -1, dtype=np.int64)
    if seq_len == 0:
        return end_score, end_start
    fill = fill_of(table[:seq_len])
    # cost_t(u) = (double)table[t, ext(u)] - (double)fill[t], as Python floats (IEEE doubles)
    cost = (table[:seq_len][:, ext].astype(np.float64) -
            fill.astype(np.float64)[:, None]).tolist()
    d = [NEG] * states
    st = [-1] * states
    for t in range(seq_len):
        nd, ns = [NEG] * states, [-1] * states
        row = cost[t]
        for u in range(states):
            best, start = NEG, -1
            if t > 0:
                if d[u] > best:
                    best, start = d[u], st[u]
                if u >= 1 and d[u - 1] > best:
                    best, start = d[u - 1], st[u - 1]
                if skip[u] and d[u - 2] > best:
                    best, start = d[u - 2], st[u - 2]
            if u == 0 and 0.0 > best:
                best, start = 0.0, t
            value = best + row[u]
            nd[u], ns[u] = value, (-1 if value == NEG else start)
        d, st = nd, ns
        end_score[t], end_start[t] = d[states - 1], st[states - 1]
    return end_score, end_start


def best_of(end_score, end_start):
    """(score, (start, end)): the first t, by strict >, that reaches the largest end_score."""
    best, span = NEG, (-1, -1)
    for t in range(len(end_score)):
        if end_score[t] > best:
            best, span = float(end_score[t]), (int(end_start[t]), t)
    return best, span


def hit_pass(end_score, end_start, min_score):
    """Every flushed hit (score, start, end), in order."""
    hits = []
    pending = None
    flushed_end = -1
    for t in range(len(end_score)):
        score, start = float(end_score[t]), int(end_start[t])
        if not (score > NEG and score >= min_score):
            continue
        if start <= flushed_end:
            continue
        if pending is None:
            pending = (score, start, t)
        elif start <= pending[2]:
            if score > pending[0] or (score == pending[0] and start == pending[1]):
                pending = (score, start, t)
        else:
            hits.append(pending)
            flushed_end = pending[2]
            pending = (score, start, t)
    if pending is not None:
        hits.append(pending)
    return hits


def pack_hits(found, max_hits):
    """(hits i32[max_hits, 2], hit_score f64[max_hits], n_hits) as the kernel stores them."""
    hits = np.full((max_hits, 2), -1, dtype=np.int32)
    hit_score = np.full(max_hits, NEG)
    for k, (score, start, end) in enumerate(found[:max_hits]):
        hits[k] = (start, end)
        hit_score[k] = score
    return hits, hit_score, len(found)


def search(table, seq_len, blank, phrases, min_score, pair_utt, pair_phrase, max_hits,
           max_label_len=None):
    """Everything ``ctcasr_ctc_search`` returns, for table f32[T, B, C]: a dict of numpy arrays
    hits, hit_score, n_hits, best_score, best_span, end_score, end_start, status."""
    table = np.asarray(table, dtype=np.float32)
    num_steps, batch, classes = table.shape
    pairs = len(pair_utt)
    if max_label_len is None:
        max_label_len = max([len(p) for p in phrases] + [0])
    out = {'hits': np.full((pairs, max_hits, 2), -1, dtype=np.int32),
           'hit_score': np.full((pairs, max_hits), NEG),
           'n_hits': np.zeros(pairs, dtype=np.int32),
           'best_score': np.full(pairs, NEG),
           'best_span': np.full((pairs, 2), -1, dtype=np.int32),
           'end_score': np.full((pairs, num_steps), NEG),
           'end_start': np.full((pairs, num_steps), -1, dtype=np.int32),
           'status': np.zeros(pairs, dtype=np.int32)}
    for h in range(pairs):
        b, p = int(pair_utt[h]), int(pair_phrase[h])
        status = 0
        if not (0 <= b < batch and 0 <= p < len(phrases)):
            status = 2
        else:
            lab = [int(c) for c in phrases[p]]
            length = int(seq_len[b])
            if len(lab) == 0 or len(lab) > max_label_len or length > num_steps or length < 0 or \
                    any(c < 0 or c >= classes or c == blank for c in lab):
                status = 2
            elif length < len(lab) + adjacent_repeats(lab):
                status = 1
            elif np.isnan(fill_of(table[:length, b])).any():
                status = 3
        out['status'][h] = status
        if status == 3:
            out['best_score'][h] = np.nan
            out['end_score'][h] = np.nan
        if status != 0:
            continue
        end_score, end_start = lattice(table[:, b], lab, blank, length)
        out['end_score'][h], out['end_start'][h] = end_score, end_start
        out['best_score'][h], out['best_span'][h] = best_of(end_score, end_start)
        out['hits'][h], out['hit_score'][h], out['n_hits'][h] = pack_hits(
            hit_pass(end_score, end_start, float(min_score[p])), max_hits)
    return out
