"""What the GPU tests of the CTC beam searches share: inputs, bit comparison, random dense
scorers, and `raw_beam`, the C entry points of csrc/beam.hip on a workspace of the caller's."""

import ctypes

import numpy as np
import torch

from ctc_asr_amd import lm

DEV = 'cuda'


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _logits(rng, num_steps, batch, classes, blank, scale=2.0, blank_bias=1.0):
    logits = rng.normal(size=(num_steps, batch, classes)) * scale
    logits[:, :, blank] += blank_bias
    return logits.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _random_scorer(rng, states, classes, final=True, forbidden=0.0):
    score = rng.normal(size=(states, classes)).astype(np.float32)
    if forbidden:
        score[rng.random(size=score.shape) < forbidden] = -np.inf
    return lm.LmScorer(rng.integers(0, states, size=(states, classes)), score,
                       rng.normal(size=states).astype(np.float32) if final else None)


def _tables(scorer):
    return (None, None, None) if scorer is None else (scorer.next, scorer.score, scorer.final)


def raw_beam(hip, logits, seq_len, width, scorer, workspace, top_paths=None, blank=28, norm=0,
             nbytes=None, table='own', stats=None):
    """(status, (out, out_len, logp, n_paths)) of one C entry point on a workspace of the
    caller's, the outputs pre-filled with garbage (-7, NaN).  ``scorer`` None or an `lm.LmScorer`:
    the top-1 entry point of that model where ``top_paths`` is None (``n_paths`` stays garbage),
    else the n-best one.  An `lm.WordLmScorer`: the word entry point, the look-ahead one where the
    scorer carries a table (``table``: 'own', or None for a NULL pointer); ``stats`` as
    `hip.ctc_beam_decode_wordlm` takes it."""
    num_steps, batch, classes = logits.shape
    ptr = lambda t: None if t is None else t.data_ptr()                          # noqa: E731
    rows = (batch,) if top_paths is None else (batch, max(top_paths, 1))
    out = torch.full(rows + (num_steps,), -7, dtype=torch.int32, device=DEV)
    out_len = torch.full(rows, -7, dtype=torch.int32, device=DEV)
    logp = torch.full(rows, float('nan'), dtype=torch.float32, device=DEV)
    n_paths = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    lib = hip.load()
    head = (logits.data_ptr(), seq_len.data_ptr(), num_steps, batch, classes, blank, width, norm)
    top1 = (out.data_ptr(), out_len.data_ptr(), logp.data_ptr())
    tail = (workspace.data_ptr(), workspace.numel() if nbytes is None else nbytes,
            torch.cuda.current_stream().cuda_stream)
    if isinstance(scorer, lm.WordLmScorer):
        struct, keep = hip._wordlm_struct(scorer, logits.device, stats)
        head += (top_paths, ctypes.addressof(struct))
        if scorer.lookahead is None:
            status = lib.ctcasr_ctc_beam_decode_wordlm(*head, *top1, n_paths.data_ptr(), *tail)
        else:
            ahead = None if table is None else scorer.lookahead_to(logits.device)
            status = lib.ctcasr_ctc_beam_decode_wordlm_lookahead(
                *head, ptr(ahead), *top1, n_paths.data_ptr(), *tail)
    else:
        keep = (None, None, None) if scorer is None else \
            scorer.to(torch.device(DEV, torch.cuda.current_device()))
        model = tuple(ptr(t) for t in keep) + (0 if scorer is None else scorer.num_states,)
        if top_paths is not None:
            status = lib.ctcasr_ctc_beam_decode_nbest(*head, top_paths, *model, *top1,
                                                      n_paths.data_ptr(), *tail)
        elif scorer is None:
            status = lib.ctcasr_ctc_beam_decode(*head, *top1, *tail)
        else:
            status = lib.ctcasr_ctc_beam_decode_lm(*head, *model, *top1, *tail)
    torch.cuda.synchronize()
    del keep
    return status, tuple(x.cpu().numpy() for x in (out, out_len, logp, n_paths))
