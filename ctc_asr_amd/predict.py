"""Transcribe one WAV file: ``python -m ctc_asr_amd.predict --input file.wav``
(counterpart of ``asr/predict.py:44-67``; returns / prints {'decoded', 'plaintext'}).
``--timestamps`` adds ``'words'``: the decoded text aligned to the same logits
(`CTCModel.align_fn`), one ``{'word', 'start', 'end', 'confidence'}`` per word.  ``--lm_path``
decodes with that language model fused into the beam search (``--lm_weight``, ``--lm_bonus``);
the timestamps are then those of the text it decoded.  ``--nbest N`` adds ``'nbest'``, one
``{'plaintext', 'logp', 'ctc_logp', 'lm_logp', 'posterior'}`` per hypothesis of the final beam
in first-pass order (``logp``: the beam's total; ``ctc_logp``: the exact ln p(y | x)), and
``'confidence'``, the posterior of the printed hypothesis.  That is rank 0 - what is printed
without the flag - unless ``--rescore_lm_path`` re-ranks the list: then the selected hypothesis
is printed, and ``--timestamps`` aligns its text.  ``--resample_input`` takes a file of any
sampling rate, channel count and sample format (`input_functions.read_audio`)."""

import os
import sys

import numpy as np
import torch

from ctc_asr_amd import alignment, lm, storage
from ctc_asr_amd.input_functions import features_from_files
from ctc_asr_amd.model import CTCModel, ModelConfig
from ctc_asr_amd.params import FLAGS


def predict(model, wav_path, timestamps=False, scorer=None, nbest=0, rescorer=None):
    feats, lengths = features_from_files([wav_path], model.device)
    logits, seq_len = model.inference_fn(feats, lengths, training=False)
    model.check_rnn_error()
    if nbest:
        listed = model.nbest_fn(logits, seq_len, nbest, scorer=scorer, rescorer=rescorer)[0]
        hyps = listed['hypotheses']
        chosen = hyps[listed['selected'] if rescorer is not None else 0]
        decoded = [chosen['labels']]
        result = {'decoded': np.array(decoded[0], dtype=np.int32),
                  'plaintext': chosen['plaintext'], 'confidence': chosen['posterior'],
                  'nbest': [{'plaintext': h['plaintext'], 'logp': h['beam_logp'],
                             'ctc_logp': h['ctc_logp'], 'lm_logp': h['lm_logp'],
                             'posterior': h['posterior']} for h in hyps]}
    else:
        decoded, plaintext, _ = model.decode_fn(logits, seq_len, None, scorer=scorer)
        result = {'decoded': np.array(decoded[0], dtype=np.int32), 'plaintext': plaintext[0]}
    if timestamps:
        ids = [v for v in decoded[0] if v != 0]     # (id 0 renders as '' and is no label)
        path, _, frame_logp, _ = model.align_fn(logits, seq_len, [ids])
        # a decode the alignment cannot place (status != 0) leaves a path of -1: no words
        result['words'] = alignment.segments(
            path[0].cpu().numpy(), ids,
            alignment.frame_seconds(model.cfg, FLAGS.features_drop_every_second_frame),
            frame_logp[0].cpu().numpy())
    return result


def main(argv=None):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    if not os.path.isfile(FLAGS.input):
        raise ValueError('The input file "{}" does not exist.'.format(FLAGS.input))
    if not torch.cuda.is_available():
        raise SystemExit('ctc_asr_amd.predict needs an MI355X; no GPU is visible.')
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=FLAGS.random_seed or 1)
    latest = storage.latest_checkpoint(FLAGS.train_dir)
    if latest is None:
        raise SystemExit('No checkpoint found in {}.'.format(FLAGS.train_dir))
    storage.restore_checkpoint(latest, model, weights='ema' if FLAGS.eval_ema else 'param')
    print('Inputs: {}'.format(FLAGS.input))
    print(predict(model, FLAGS.input, FLAGS.timestamps, lm.from_flags(model.cfg.num_classes),
                  FLAGS.nbest, lm.rescorer_from_flags(model.cfg.num_classes)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
