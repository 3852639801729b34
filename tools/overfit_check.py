#!/usr/bin/env python
"""End-to-end learning check: the DS2 model (own convolutions, persistent BiLSTM-1024 kernels,
CTC, Adam) memorises a small batch of noise "utterances" with random transcripts - the loss
falls towards zero and the greedy / beam decodes become the transcripts.
    python tools/overfit_check.py [steps batch seconds] [--rnn_batch_norm] [--mwer_nbest N]
With --mwer_nbest N (2..64) the CTC stage is followed by MWER_STEPS steps of minimum word error
rate training on the same batch (word risk, beam width 64, the default CTC weight): the expected
word errors per utterance over the n-best list, and the word errors of the beam-64 decode, are
printed before and after - give it fewer CTC steps than it takes to memorise the batch (120, say)
so that there is an error left to lower."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd.engine import Trainer  # noqa: E402
from ctc_asr_amd import metrics  # noqa: E402
from ctc_asr_amd.labels import decode  # noqa: E402
from ctc_asr_amd.model import CTCModel, ModelConfig  # noqa: E402
from ctc_asr_amd.synth import synthetic_batch  # noqa: E402


class Flags:
    learning_rate, adam_beta1, adam_beta2, adam_epsilon = 3e-4, 0.9, 0.999, 1e-8


MWER_STEPS = 100


def word_errors(model, feats_d, len_d, texts):
    """Word errors of the beam-64 decode of the batch, summed (inference mode)."""
    logits, seq_len = model.inference_fn(feats_d, len_d, training=False)
    beam, _, _ = model.decode_fn(logits, seq_len, None, beam_width=64)
    ref_words, hyp_words = metrics.word_ids(texts, [decode(b) for b in beam])
    return int(metrics.error_counts(hyp_words, ref_words, model.device)[:, 0].sum())


def fine_tune(trainer, feats_d, len_d, packed, texts, nbest, verbose=True):
    """MWER_STEPS steps of MWER training on the batch; returns (expected risk per utterance at
    the first and after the last step, word errors of the beam-64 decode before and after)."""
    from ctc_asr_amd.params import MWER_DEFAULTS
    errors_before = word_errors(trainer.model, feats_d, len_d, texts)
    trainer.mwer = {'nbest': int(nbest), 'beam_width': MWER_DEFAULTS['mwer_beam_width'],
                    'ctc_weight': MWER_DEFAULTS['mwer_ctc_weight'],
                    'risk': MWER_DEFAULTS['mwer_risk']}
    risks = []
    for step in range(MWER_STEPS + 1):
        trainer.train_step(feats_d, len_d, packed, check=(step % 50 == 0), originals=texts)
        if step % 25 == 0:
            risks.append(float(trainer.last_expected_risk.mean()))
            if verbose:
                print('mwer step {:4d} expected word errors per utterance {:.4f}, lists of {:.1f}'
                      .format(step, risks[-1], float(trainer.last_mwer_paths.float().mean())))
    trainer.drain_checks()
    errors_after = word_errors(trainer.model, feats_d, len_d, texts)
    if verbose:
        print('mwer_nbest {}: expected word errors per utterance {:.4f} -> {:.4f} in {} steps; '
              'beam-64 word errors of the batch {} -> {}'.format(
                  nbest, risks[0], risks[-1], MWER_STEPS, errors_before, errors_after))
    return risks[0], risks[-1], errors_before, errors_after


def run(steps=300, batch=8, seconds=2.0, verbose=True, rnn_batch_norm=False, mwer_nbest=0):
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32), num_units_dense=512,
                      num_layers_rnn=2, num_units_rnn=1024, rnn_cell='lstm', cudnn=True,
                      dense_dropout_rate=0.0, rnn_batch_norm=rnn_batch_norm)
    trainer = Trainer(cfg, flags=Flags, device='cuda', seed=3)
    feats, lengths, labels, texts = synthetic_batch(batch, seconds, seed=5, chars_per_second=6.0)
    feats_d = torch.tensor(feats, device='cuda')
    len_d = torch.tensor(lengths, device='cuda')
    packed = CTCModel.pack_labels(labels, trainer.model.device)
    t0 = time.perf_counter()
    losses = []
    for step in range(steps):
        loss = trainer.train_step(feats_d, len_d, packed, check=(step % 50 == 0))
        if step % 25 == 0 or step == steps - 1:
            losses.append(float(loss))
            if verbose:
                print('step {:4d} loss {:.4f}'.format(step, losses[-1]))
    trainer.model.check_rnn_error()
    if mwer_nbest:
        fine_tune(trainer, feats_d, len_d, packed, texts, mwer_nbest, verbose)
    logits, seq_len = trainer.model.inference_fn(feats_d, len_d, training=False)
    greedy, _, _ = trainer.model.decode_fn(logits, seq_len, None, greedy=True)
    beam, _, _ = trainer.model.decode_fn(logits, seq_len, None, beam_width=64)
    hits_g = sum(decode(g) == t for g, t in zip(greedy, texts))
    hits_b = sum(decode(b) == t for b, t in zip(beam, texts))
    if verbose:
        print('{:.1f} s; greedy {}/{} exact, beam-64 {}/{} exact; e.g. "{}" vs "{}"'.format(
            time.perf_counter() - t0, hits_g, batch, hits_b, batch, decode(beam[0]), texts[0]))
    return losses, hits_g, hits_b, batch


if __name__ == '__main__':
    argv = sys.argv[1:]
    batch_norm = '--rnn_batch_norm' in argv
    nbest = 0
    if '--mwer_nbest' in argv:
        at = argv.index('--mwer_nbest')
        nbest = int(argv[at + 1])
        del argv[at:at + 2]
    args = [float(v) for v in argv if v != '--rnn_batch_norm'][:3]
    run(*(int(args[0]) if len(args) > 0 else 300, int(args[1]) if len(args) > 1 else 8,
          args[2] if len(args) > 2 else 2.0), rnn_batch_norm=batch_norm, mwer_nbest=nbest)
