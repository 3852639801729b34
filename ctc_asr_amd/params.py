"""Hyper-parameters, network layout and reporting options.

The flag *names and defaults* are the drop-in knob API of the reference
(``asr/params.py:15-134``; list in SURVEY.md section 8b).  The reference registers them with
``tf.flags``; here they live in a small self-contained registry (`FLAGS`) that parses the same
``--name=value`` / ``--name value`` / ``--[no]bool`` command lines, so scripts written against
``from asr.params import FLAGS`` keep working after changing the import.
"""

import math
import os
import sys

import numpy as np

from ctc_asr_amd.labels import num_classes

BASE_PATH = os.path.realpath(os.path.join(os.path.dirname(os.path.realpath(__file__)), '../'))


class _Flag:
    __slots__ = ('name', 'kind', 'default', 'value', 'help', 'check')

    def __init__(self, name, kind, default, help_text, check=None):
        self.name, self.kind, self.default, self.help = name, kind, default, help_text
        self.check = check
        self.value = list(default) if kind == 'multi_int' else default


class FlagValues:
    """Minimal absl-style flag container: attribute access, ``parse``, ``reset``."""

    def __init__(self):
        object.__setattr__(self, '_flags', {})
        object.__setattr__(self, '_validators', [])

    # -- definition -------------------------------------------------------------------------
    def define_validator(self, validator):
        """``validator(flags)``: raises ValueError for a COMBINATION of values that is refused; run
        after every `parse`, when all flags of the command line are known."""
        self._validators.append(validator)

    def define(self, kind, name, default, help_text='', check=None):
        """``check(value)``: raises ValueError for a value the flag refuses - when the command line
        is parsed or the flag is assigned, not when it is first used."""
        if name in self._flags:
            raise ValueError('Duplicate flag "{}".'.format(name))
        self._flags[name] = _Flag(name, kind, default, help_text, check)

    # -- access -----------------------------------------------------------------------------
    def __getattr__(self, name):
        flags = object.__getattribute__(self, '_flags')
        if name not in flags:
            raise AttributeError('Unknown flag "{}".'.format(name))
        return flags[name].value

    def __setattr__(self, name, value):
        if name not in self._flags:
            raise AttributeError('Unknown flag "{}".'.format(name))
        self._flags[name].value = self._convert(self._flags[name], value)

    def __contains__(self, name):
        return name in self._flags

    def flag_values_dict(self):
        return {k: f.value for k, f in self._flags.items()}

    def defaults_dict(self):
        return {k: f.default for k, f in self._flags.items()}

    def reset(self):
        for flag in self._flags.values():
            flag.value = list(flag.default) if flag.kind == 'multi_int' else flag.default

    def update(self, **kwargs):
        for key, value in kwargs.items():
            setattr(self, key, value)
        return self

    # -- parsing ----------------------------------------------------------------------------
    @classmethod
    def _convert(cls, flag, raw):
        value = cls._convert_kind(flag, raw)
        if flag.check is not None:
            flag.check(value)
        return value

    @staticmethod
    def _convert_kind(flag, raw):
        if flag.kind == 'string':
            return str(raw)
        if flag.kind == 'int':
            return int(raw)
        if flag.kind == 'float':
            return float(raw)
        if flag.kind == 'bool':
            if isinstance(raw, str):
                low = raw.lower()
                if low in ('1', 'true', 't', 'yes', 'y'):
                    return True
                if low in ('0', 'false', 'f', 'no', 'n'):
                    return False
                raise ValueError('Bad boolean "{}" for --{}.'.format(raw, flag.name))
            return bool(raw)
        if flag.kind == 'multi_int':
            if isinstance(raw, (list, tuple)):
                return [int(v) for v in raw]
            return [int(v) for v in str(raw).replace(',', ' ').split()]
        raise ValueError(flag.kind)

    def parse(self, argv=None):
        """Parse ``argv`` (without the program name); returns the unparsed remainder."""
        argv = list(sys.argv[1:] if argv is None else argv)
        rest, seen_multi = [], set()
        i = 0
        while i < len(argv):
            arg = argv[i]
            i += 1
            if arg == '--':
                continue
            if not arg.startswith('-'):
                rest.append(arg)
                continue
            body = arg.lstrip('-')
            name, eq, raw = body.partition('=')
            if name not in self._flags and name.startswith('no') and name[2:] in self._flags \
                    and self._flags[name[2:]].kind == 'bool':
                self._flags[name[2:]].value = False
                continue
            if name not in self._flags:
                raise ValueError('Unknown command line flag "{}".'.format(arg))
            flag = self._flags[name]
            if not eq:
                if flag.kind == 'bool':
                    flag.value = True
                    continue
                if i >= len(argv):
                    raise ValueError('Missing value for flag --{}.'.format(name))
                raw = argv[i]
                i += 1
            if flag.kind == 'multi_int':
                values = self._convert(flag, raw)
                if name in seen_multi:
                    flag.value = flag.value + values
                else:
                    flag.value = values
                    seen_multi.add(name)
            else:
                flag.value = self._convert(flag, raw)
        for validator in self._validators:
            validator(self)
        return rest


FLAGS = FlagValues()

# Directories (defaults are outside of the project directory, asr/params.py:13-27).
FLAGS.define('string', 'train_dir', os.path.join(BASE_PATH, '../ctc-asr-checkpoints/3c4r2d-rnn'),
             'Checkpoint / log directory (resume source unless --delete).')
_CORPUS_DIR = os.path.join(BASE_PATH, '../speech-corpus')
FLAGS.define('string', 'corpus_dir', os.path.join(_CORPUS_DIR, 'corpus'),
             'Root of the WAV corpus; CSV paths are relative to it.')
FLAGS.define('string', 'train_csv', os.path.join(_CORPUS_DIR, 'train.csv'), 'Training manifest (path;label;length).')
FLAGS.define('string', 'test_csv', os.path.join(_CORPUS_DIR, 'test.csv'), 'Test manifest.')
FLAGS.define('string', 'dev_csv', os.path.join(_CORPUS_DIR, 'dev.csv'), 'Validation manifest.')

# Layer and activation options (asr/params.py:29-50).
FLAGS.define('string', 'used_model', 'ds2', "Front-end: 'ds1' = 3 dense layers, 'ds2' = 2-D convolutions.")
FLAGS.define('int', 'num_units_dense', 2048, 'Width of every dense layer.')
FLAGS.define('float', 'relu_cutoff', 20.0, 'Upper clip applied after each ReLU.')
FLAGS.define('multi_int', 'conv_filters', [32, 32, 96],
             'Number of filters for each convolutional layer (3 = reference stack; 2 entries '
             'select the "2-conv" variant of BASELINE.json).')
FLAGS.define('int', 'num_layers_rnn', 4, 'Depth of the bidirectional recurrent stack.')
FLAGS.define('int', 'num_units_rnn', 2048, 'Hidden units per direction.')
FLAGS.define('string', 'rnn_cell', 'rnn_relu', "Recurrent cell: rnn_relu | rnn_tanh | lstm | gru.")

# Inputs (asr/params.py:52-61).
FLAGS.define('int', 'batch_size', 16, 'Utterances per minibatch (per GPU when data parallel).')
FLAGS.define('string', 'feature_type', 'mfcc', "'mel' = 80 log-mel bands, 'mfcc' = 40 cepstra + 40 deltas.")
FLAGS.define('string', 'feature_normalization', 'local', "Per-utterance normalisation: none | local | local_scalar.")
FLAGS.define('bool', 'features_drop_every_second_frame', False,
             'Keep only every second feature frame (Deep Speech 1 style).')

# Learning rate (asr/params.py:63-74; the three decay flags are inert in the reference - here
# --lr_schedule staircase makes them do what their help texts there say).
FLAGS.define('int', 'max_epochs', 15, 'Total epochs (the first one walks the CSV in order).')
FLAGS.define('float', 'learning_rate', 1e-5, 'Adam step size (the initial one under a schedule).')
FLAGS.define('float', 'learning_rate_decay_factor', 4 / 5,
             'Factor the learning rate is multiplied by at each decay (--lr_schedule staircase).')
FLAGS.define('int', 'steps_per_decay', 75000,
             'Updates between two decays of the learning rate (--lr_schedule staircase).')
FLAGS.define('float', 'minimum_lr', 1e-6,
             'Floor of the staircase schedule; where the cosine schedule ends.')

LR_SCHEDULES = ('constant', 'staircase', 'cosine')


def _one_of(name, choices):
    def check(value):
        if value not in choices:
            raise ValueError('--{}={} is none of {}.'.format(name, value, ', '.join(choices)))
    return check


def _int_range(name, low, high=None):
    def check(value):
        if value < low or (high is not None and value > high):
            raise ValueError('--{}={} is outside {}..{}.'.format(
                name, value, low, 'unbounded' if high is None else high))
    return check


def _ema_decay_check(value):
    if not 0.0 <= value < 1.0:          # (a NaN fails both comparisons)
        raise ValueError('--ema_decay={} is outside 0 <= d < 1.'.format(value))


# The rest of the training recipe (no counterpart in the reference; all off by default: a training
# step then launches what it always did).
FLAGS.define('string', 'lr_schedule', 'constant',
             'constant | staircase (learning_rate_decay_factor every steps_per_decay updates, '
             'down to minimum_lr) | cosine (half a cosine down to minimum_lr over '
             'lr_total_steps updates).', _one_of('lr_schedule', LR_SCHEDULES))
FLAGS.define('int', 'lr_warmup_steps', 0,
             'Updates over which any schedule ramps up linearly from zero (0: no warm-up).',
             _int_range('lr_warmup_steps', 0))
FLAGS.define('int', 'lr_total_steps', 0, 'Length of the cosine schedule in updates.')
FLAGS.define('int', 'grad_accum_steps', 1,
             'Micro-batches whose gradients are summed into one update (1..1024).',
             _int_range('grad_accum_steps', 1, 1024))
FLAGS.define('float', 'ema_decay', 0.0,
             'Decay of the exponential moving average of the parameters, kept in the Adam '
             'launch (0 <= d < 1; 0: off).', _ema_decay_check)
FLAGS.define('bool', 'eval_ema', False,
             'Evaluate, predict, align and export with the averaged parameters.')


def learning_rate_at(update, flags=FLAGS):
    """The learning rate of update number ``update`` (1-based), a pure function of the flags, in
    float64: 'constant' - ``learning_rate``; 'staircase' - ``max(minimum_lr, learning_rate *
    learning_rate_decay_factor ** ((update - 1) // steps_per_decay))``; 'cosine' - half a cosine
    from ``learning_rate`` down to ``minimum_lr`` over ``lr_total_steps`` updates, ``minimum_lr``
    after them; any of them times ``min(1, update / lr_warmup_steps)`` when that is positive.
    Under 'constant' without warm-up the result is ``learning_rate`` itself, the same float."""
    if update < 1:
        raise ValueError('learning_rate_at: updates count from 1 (got {}).'.format(update))
    base = flags.learning_rate
    schedule = getattr(flags, 'lr_schedule', 'constant')
    if schedule == 'constant':
        rate = base
    elif schedule == 'staircase':
        if flags.steps_per_decay < 1:
            raise ValueError('--lr_schedule staircase needs --steps_per_decay > 0.')
        rate = max(float(flags.minimum_lr), float(base) * float(flags.learning_rate_decay_factor)
                   ** ((int(update) - 1) // int(flags.steps_per_decay)))
    elif schedule == 'cosine':
        total = int(getattr(flags, 'lr_total_steps', 0))
        if total <= 0:
            raise ValueError('--lr_schedule cosine needs --lr_total_steps > 0.')
        low = float(flags.minimum_lr)
        if update >= total:
            rate = low
        else:
            rate = low + 0.5 * (float(base) - low) * (1.0 + np.cos(np.pi * (update - 1) /
                                                                   (total - 1)))
            rate = float(rate)
    else:
        raise ValueError('Unknown --lr_schedule "{}".'.format(schedule))
    warmup = int(getattr(flags, 'lr_warmup_steps', 0))
    if warmup > 0 and update < warmup:
        rate = float(rate) * (float(update) / warmup)
    return rate


def ema_decay_at(ema_decay, num_updates):
    """``min(ema_decay, (1 + k) / (10 + k))`` with k = ``num_updates``, the updates counted BEFORE
    this one: the decay ``tf.train.ExponentialMovingAverage(decay, num_updates)`` applies, so that
    a young average follows the parameters instead of its own starting point.  float64."""
    k = float(num_updates)
    if k < 0:
        raise ValueError('ema_decay_at: num_updates is negative.')
    return min(float(ema_decay), (1.0 + k) / (10.0 + k))


def ema_alpha_at(ema_decay, num_updates):
    """``1 - ema_decay_at(...)`` in float64: what `hip.adam_step(ema_alpha=...)` is handed (it
    rounds to float32 once, at the ABI)."""
    return 1.0 - ema_decay_at(ema_decay, num_updates)

# Adam (asr/params.py:76-82).
FLAGS.define('float', 'adam_beta1', 0.9, 'First-moment decay.')
FLAGS.define('float', 'adam_beta2', 0.999, 'Second-moment decay.')
FLAGS.define('float', 'adam_epsilon', 1e-8, 'Added to sqrt(v) (TensorFlow form).')

# Gradient clipping by global norm and the per-layer norms (no counterpart in the reference, which
# does not clip; both off: the training step launches what it always did).
FLAGS.define('float', 'max_grad_norm', 0.0,
             'Scale the gradients of a step so that their global L2 norm is at most this (0: off).')
FLAGS.define('bool', 'report_grad_norms', False,
             'Compute the global and per-layer gradient norms every step and log them.')


def _bn_decay_check(value):
    if not 0.0 < value < 1.0:           # (a NaN fails both comparisons)
        raise ValueError('--rnn_bn_decay={} is outside 0 < d < 1.'.format(value))


# Sequence-wise batch normalisation of the input of recurrent layers 2..L (no counterpart in the
# reference; off: the parameters, the checkpoints and every launch of a step are what they were).
FLAGS.define('bool', 'rnn_batch_norm', False,
             'Normalise the input of recurrent layers 2..L per channel over all frames of the '
             'batch; adds rnn{i}/bn_gamma and rnn{i}/bn_beta and running statistics.')
FLAGS.define('float', 'rnn_bn_decay', 0.99,
             'Decay of the running statistics of --rnn_batch_norm (0 < d < 1).', _bn_decay_check)

# Augmentation of training batches on the device (no counterpart in the reference, which does not
# augment; all off: a training batch launches what it always did).  Only the targets
# 'train_bucket' and 'train_batch' augment; evaluate / predict / align never do.
SPECAUG_MAX_MASKS = 16          # CTCASR_SPEC_AUGMENT_MAX_MASKS
SPEED_PERCENT_RANGE = (50, 200)


def parse_speed_perturb(text):
    """'90,100,110' -> [90, 100, 110]; '' -> []; ValueError for anything else."""
    percents = []
    for part in str(text).replace(',', ' ').split():
        try:
            percent = int(part)
        except ValueError:
            raise ValueError('--speed_perturb: "{}" is not a whole percent.'.format(part))
        if not SPEED_PERCENT_RANGE[0] <= percent <= SPEED_PERCENT_RANGE[1]:
            raise ValueError('--speed_perturb: {} is outside {}..{} percent.'.format(
                percent, *SPEED_PERCENT_RANGE))
        percents.append(percent)
    return percents


FLAGS.define('bool', 'spec_augment', False,
             'Mask the features of training batches (SpecAugment): masked cells are set to 0.0, '
             "the per-column mean under 'local' normalisation (zero is written under 'none' and "
             "'local_scalar' too).")
FLAGS.define('int', 'specaug_freq_masks', 2, 'Number of frequency masks (0..16).',
             _int_range('specaug_freq_masks', 0, SPECAUG_MAX_MASKS))
FLAGS.define('int', 'specaug_freq_width', 27, 'Largest frequency mask, in feature columns.',
             _int_range('specaug_freq_width', 0))
FLAGS.define('int', 'specaug_time_masks', 2, 'Number of time masks (0..16).',
             _int_range('specaug_time_masks', 0, SPECAUG_MAX_MASKS))
FLAGS.define('int', 'specaug_time_width', 100, 'Largest time mask, in frames.',
             _int_range('specaug_time_width', 0))
FLAGS.define('int', 'specaug_time_permille', 1000,
             'Cap on a time mask as a share of the utterance, in thousandths (0..1000).',
             _int_range('specaug_time_permille', 0, 1000))
FLAGS.define('string', 'speed_perturb', '',
             'Comma list of speeds in percent (50..200), for example 90,100,110: every training '
             'utterance is resampled to one of them, drawn uniformly; empty: off.',
             parse_speed_perturb)

# Additive noise on the device (no counterpart in the reference; off while --noise_csv is empty: a
# batch then launches what it always did).  Training batches draw whether, which clip, where in it
# and how many dB per row; 'dev' and 'test' batches mix only under --eval_noise_snr_db, every row at
# that one value.  predict / align never mix.
NOISE_SNR_DB_RANGE = (-20, 60)      # CTCASR_NOISE_MIX_MIN_SNR_DB, CTCASR_NOISE_MIX_MAX_SNR_DB


def _snr_db(flag, part):
    try:
        value = int(part)
    except ValueError:
        raise ValueError('--{}: "{}" is not a whole number of dB.'.format(flag, part))
    if not NOISE_SNR_DB_RANGE[0] <= value <= NOISE_SNR_DB_RANGE[1]:
        raise ValueError('--{}: {} is outside {}..{} dB.'.format(flag, value, *NOISE_SNR_DB_RANGE))
    return value


def parse_noise_snr_db(text):
    """'10,30' -> (10, 30); '15' -> (15, 15); ValueError for anything else."""
    parts = str(text).replace(',', ' ').split()
    if len(parts) not in (1, 2):
        raise ValueError('--noise_snr_db: "{}" is neither "lo,hi" nor one value.'.format(text))
    values = [_snr_db('noise_snr_db', part) for part in parts]
    if values[0] > values[-1]:
        raise ValueError('--noise_snr_db: {} is above {}.'.format(values[0], values[-1]))
    return values[0], values[-1]


def parse_eval_noise_snr_db(text):
    """'' -> None (off); '10' -> 10; ValueError for anything else."""
    parts = str(text).split()
    if not parts:
        return None
    if len(parts) != 1:
        raise ValueError('--eval_noise_snr_db: "{}" is not one value.'.format(text))
    return _snr_db('eval_noise_snr_db', parts[0])


def check_noise_flags(flags):
    if parse_eval_noise_snr_db(flags.eval_noise_snr_db) is not None and not flags.noise_csv:
        raise ValueError('--eval_noise_snr_db needs --noise_csv.')


FLAGS.define('string', 'noise_csv', '',
             'Manifest (path;label;length, labels ignored) of the noise recordings mixed into '
             'training batches; empty: off.')
FLAGS.define('string', 'noise_dir', '', 'Root of the noise WAVs; empty: corpus_dir.')
FLAGS.define('string', 'noise_snr_db', '10,30',
             'Speech-to-noise ratio of a mixed utterance in whole dB, "lo,hi" (drawn uniformly, '
             'both ends included) or one value; -20..60.', parse_noise_snr_db)
FLAGS.define('int', 'noise_permille', 500,
             'Share of the training utterances that get noise, in thousandths (0..1000).',
             _int_range('noise_permille', 0, 1000))
FLAGS.define('int', 'noise_max_seconds', 3600,
             'Noise kept in HBM: reading the manifest stops at this many seconds (at least 1).',
             _int_range('noise_max_seconds', 1))
FLAGS.define('string', 'eval_noise_snr_db', '',
             "Mix noise into every utterance of 'dev' / 'test' batches at this many dB (-20..60), "
             'the same draws at every evaluation; needs --noise_csv; empty: off.',
             parse_eval_noise_snr_db)
FLAGS.define_validator(check_noise_flags)

# Reverberation on the device (no counterpart in the reference; off while --rir_csv is empty: a
# batch then launches what it always did).  Training batches draw whether and with which room
# impulse response per row, after the speed perturbation and before the noise; 'dev' / 'test',
# evaluate / predict / align never reverberate.
RIR_TAPS_RANGE = (8, 8192)          # CTCASR_REVERB_TAP_ALIGN, CTCASR_REVERB_MAX_TAPS
FLAGS.define('string', 'rir_csv', '',
             'Manifest (path;label;length, labels ignored) of the room impulse responses that '
             'training batches are convolved with; empty: off.')
FLAGS.define('string', 'rir_dir', '', 'Root of the impulse response WAVs; empty: corpus_dir.')
FLAGS.define('int', 'rir_permille', 500,
             'Share of the training utterances that get reverberated, in thousandths (0..1000).',
             _int_range('rir_permille', 0, 1000))
FLAGS.define('int', 'rir_max_taps', 8192,
             'Cap on the length of an impulse response, in samples (8..8192).',
             _int_range('rir_max_taps', *RIR_TAPS_RANGE))

# CTC decoder (asr/params.py:84-86).
FLAGS.define('int', 'beam_width', 1024, 'Leaves kept by the CTC beam search (<= 1024).')

# Dropout (asr/params.py:88-94).
FLAGS.define('float', 'conv_dropout_rate', 0.0, 'Drop probability after each conv layer.')
FLAGS.define('float', 'rnn_dropout_rate', 0.0, 'Drop probability between recurrent layers.')
FLAGS.define('float', 'dense_dropout_rate', 0.1, 'Drop probability after each dense layer.')

# Corpus (asr/params.py:96-103).
FLAGS.define('int', 'num_buckets', 96, 'Upper bound on length buckets.')
FLAGS.define('int', 'num_classes', num_classes(), 'Alphabet size + unused id 0 + CTC blank.')
FLAGS.define('int', 'sampling_rate', 16000, 'Expected WAV sampling rate in Hz.')
# Any WAV for the tools that read single recordings (no counterpart in the reference, whose corpus
# is 16 kHz mono int16; off: every reader refuses anything else, as it always did).  predict,
# transcribe, align, the noise bank and the impulse-response bank then read through
# `input_functions.read_audio`: rate conversion and channel downmix on the device
# (ctcasr_resample).  The train / dev / test readers never convert.
FLAGS.define('bool', 'resample_input', False,
             'predict / transcribe / align / --noise_csv / --rir_csv: take WAV files of any '
             'sampling rate (4..192 kHz), 1..8 channels, 8 / 16 / 24 / 32-bit PCM or float32, '
             'converted to --sampling_rate mono int16 on the device.')

# Performance / GPU (asr/params.py:105-112).  `cudnn=True` selects the fused recurrent kernels
# with cuDNN semantics (no sequence lengths); False selects the length-aware tanh-RNN semantics of
# the TensorFlow BasicRNNCell path.  Both run on the MI355X HIP kernels.
FLAGS.define('bool', 'cudnn', True, 'cuDNN-semantics RNN stack (True) or TF BasicRNNCell (False).')
FLAGS.define('int', 'shuffle_buffer_size', 2 ** 14, 'Sliding shuffle window of the bucketed targets.')

# Logging (asr/params.py:114-125).
FLAGS.define('int', 'log_frequency', 200, 'Steps between loss / throughput log lines.')
FLAGS.define('int', 'num_samples_to_report', 4, 'Decoded examples printed per evaluation.')
FLAGS.define('int', 'gpu_hook_query_frequency', 5, 'Accepted for compatibility (NVML hook of the reference).')
FLAGS.define('int', 'gpu_hook_average_queries', 100, 'Accepted for compatibility. ')

# Miscellaneous (asr/params.py:127-137).
FLAGS.define('bool', 'delete', False, 'Wipe train_dir first instead of resuming.')
FLAGS.define('int', 'random_seed', 0, 'Seed for init / dropout / shuffling; 0 = wall clock.')
FLAGS.define('bool', 'log_device_placement', False, 'Accepted for compatibility (no effect).')
FLAGS.define('bool', 'allow_vram_growth', True, 'Accepted for compatibility (no effect).')

# Driver-specific flags of the reference: `dev` (asr/evaluate.py:10), `input` (asr/predict.py:13).
FLAGS.define('bool', 'dev', False, 'evaluate.py: score dev.csv instead of test.csv.')
FLAGS.define('string', 'input', '', 'predict.py: WAV file to decode.')

# Forced alignment (no counterpart in the reference): word timestamps in predict.py, and the
# corpus aligner `python -m ctc_asr_amd.align`.
FLAGS.define('bool', 'timestamps', False, "predict.py: add 'words' (start / end / confidence) "
             'by aligning the decoded text to the logits.')
FLAGS.define('string', 'align_csv', '', 'align.py: path;label;length manifest to align, in file '
             'order.')
FLAGS.define('string', 'align_output', '', 'align.py: JSON-lines output, one line per manifest row.')

# Language model fused into the beam search (no counterpart in the reference): evaluate.py and
# predict.py decode with the model of --lm_path; `python -m ctc_asr_amd.lm` builds one.
FLAGS.define('string', 'lm_path', '', 'Character or word n-gram (.npz of ctc_asr_amd.lm) the beam '
             'search scores with; empty: no language model.')
FLAGS.define('float', 'lm_weight', 1.0, 'Weight of the language model\'s log-probabilities.')
FLAGS.define('float', 'lm_bonus', 0.0, 'Added to the score of every emitted label.')
FLAGS.define('int', 'lm_order', 5, 'lm.py: order of the n-gram to build.')
FLAGS.define('string', 'lm_corpus_csv', '', 'lm.py: path;label;length manifest whose transcripts '
             'the n-gram is built from.')
# ... a word n-gram over a lexicon trie (--lm_unit word), looked up on the device when a hypothesis
# closes a word; --lm_path / --rescore_lm_path take either kind of file.
LM_UNITS = ('char', 'word')


def _lm_unit_check(value):
    if value not in LM_UNITS:
        raise ValueError('--lm_unit={} is none of {}.'.format(value, ', '.join(LM_UNITS)))


def _oov_score(name):
    def check(value):
        if np.isnan(value) or value == np.inf:
            raise ValueError('--{}={} is neither -inf nor finite.'.format(name, value))
    return check


FLAGS.define('string', 'lm_unit', 'char', 'lm.py: the unit of the n-gram to build, char or word.',
             _lm_unit_check)
FLAGS.define('int', 'lm_vocab_size', 0, 'lm.py, word models: keep the most frequent words only '
             '(0: all); every other word counts as <unk>.', _int_range('lm_vocab_size', 0))
FLAGS.define('string', 'lm_corpus_text', '', 'lm.py, word models: a plain text file, one transcript '
             'per line, normalised like a long transcript (digits are refused).')
FLAGS.define('float', 'lm_oov_score', float('-inf'), 'Word models: added once to a word outside '
             'the vocabulary, which then scores as <unk>; -inf (the default): closed vocabulary.',
             _oov_score('lm_oov_score'))
FLAGS.define('bool', 'lm_lookahead', False, 'Word models: look-ahead scores inside a word - '
             'entering a trie node charges the best unigram score of a word below it, the space '
             'settles the difference.  Complete hypotheses keep their scores; a narrower beam '
             'keeps the right word alive.  Needs --lm_path with a word model.')

# N-best lists and second-pass rescoring (no counterpart in the reference): evaluate.py and
# predict.py read the --nbest best hypotheses off the final beam, score each exactly
# (hip.ctc_score) and, with --rescore_lm_path, re-rank them under that model.
NBEST_RANGE = (0, 1024)


def _finite(name):
    def check(value):
        if not np.isfinite(value):
            raise ValueError('--{} must be finite (got {}).'.format(name, value))
    return check


FLAGS.define('int', 'nbest', 0, 'Hypotheses kept per utterance (0: off; at most --beam_width).',
             _int_range('nbest', *NBEST_RANGE))
FLAGS.define('string', 'rescore_lm_path', '', 'Character or word n-gram (.npz of ctc_asr_amd.lm) '
             'that re-ranks the n-best list; needs --nbest >= 2.  Empty: no rescoring.')
FLAGS.define('float', 'rescore_lm_weight', 1.0, 'Weight of the rescoring model.',
             _finite('rescore_lm_weight'))
FLAGS.define('float', 'rescore_lm_bonus', 0.0, 'Added per label by the rescoring model.',
             _finite('rescore_lm_bonus'))
FLAGS.define('float', 'rescore_lm_oov_score', float('-inf'), 'A rescoring word model\'s '
             '--lm_oov_score (-inf: closed vocabulary); the first pass keeps its own.',
             _oov_score('rescore_lm_oov_score'))


def _validate_nbest(flags):
    if flags.nbest > flags.beam_width:
        raise ValueError('--nbest {} is above --beam_width {}.'.format(flags.nbest,
                                                                       flags.beam_width))
    if flags.nbest < 2 and (flags.rescore_lm_path or flags.rescore_lm_weight != 1.0 or
                            flags.rescore_lm_bonus != 0.0):
        raise ValueError('--rescore_lm_path / _weight / _bonus need --nbest >= 2 (got {}).'
                         .format(flags.nbest))
    if flags.rescore_lm_path:
        from ctc_asr_amd import lm
        lm.check_file('--rescore_lm_path', flags.rescore_lm_path, flags.num_classes)


FLAGS.define_validator(_validate_nbest)


def _validate_lm_path(flags):
    """--lm_path names a model to decode with, unless a corpus flag says that `ctc_asr_amd.lm` is
    about to write it."""
    from ctc_asr_amd import lm
    if flags.lm_lookahead and not flags.lm_path:
        raise ValueError('--lm_lookahead needs --lm_path with a word model.')
    if not flags.lm_path or flags.lm_corpus_csv or flags.lm_corpus_text:
        return
    kind = lm.check_file('--lm_path', flags.lm_path, flags.num_classes)
    if flags.lm_lookahead and kind != lm.WORD_KIND:
        raise ValueError('--lm_lookahead needs a word model: --lm_path {} holds a character '
                         'model.'.format(flags.lm_path))


FLAGS.define_validator(_validate_lm_path)

# Minimum word error rate training (no counterpart in the reference; off while --mwer_nbest is 0:
# a step then launches what it always did).  A training step decodes the n-best list of its own
# logits, scores every hypothesis against the transcript and adds the gradient of the expected
# error count (hip.ctc_mwer) to --mwer_ctc_weight times the CTC gradient.  The usual last stage
# after CTC training; the search is the plain one (no language model) at its own, narrow width.
MWER_NBEST_RANGE = (2, 64)
MWER_BEAM_RANGE = (2, 1024)
MWER_RISKS = ('word', 'label')
MWER_DEFAULTS = {'mwer_beam_width': 64, 'mwer_ctc_weight': 0.01, 'mwer_risk': 'word'}


def _mwer_nbest_check(value):
    if value != 0 and not MWER_NBEST_RANGE[0] <= value <= MWER_NBEST_RANGE[1]:
        raise ValueError('--mwer_nbest={} is neither 0 (off) nor in {}..{}.'.format(
            value, *MWER_NBEST_RANGE))


def _mwer_ctc_weight_check(value):
    if not (np.isfinite(value) and value >= 0.0):
        raise ValueError('--mwer_ctc_weight={} is not a finite value >= 0.'.format(value))


def check_mwer_settings(nbest, beam_width, ctc_weight, risk):
    """ValueError for a value or combination that MWER training refuses (``nbest`` 0: off, and
    then nothing else is looked at); what the flags and `engine.Trainer` both go by."""
    nbest = int(nbest)
    if nbest == 0:
        return
    _mwer_nbest_check(nbest)
    if not nbest <= int(beam_width) <= MWER_BEAM_RANGE[1]:
        raise ValueError('--mwer_beam_width={} is outside --mwer_nbest ({})..{}.'.format(
            beam_width, nbest, MWER_BEAM_RANGE[1]))
    _mwer_ctc_weight_check(ctc_weight)
    _one_of('mwer_risk', MWER_RISKS)(risk)


FLAGS.define('int', 'mwer_nbest', 0,
             'Hypotheses per utterance of the expected-risk term of a training step (0: off; '
             '2..64).', _mwer_nbest_check)
FLAGS.define('int', 'mwer_beam_width', MWER_DEFAULTS['mwer_beam_width'],
             'Leaves kept by the beam search of a training step (--mwer_nbest..1024); '
             '--beam_width is not used there.', _int_range('mwer_beam_width', *MWER_BEAM_RANGE))
FLAGS.define('float', 'mwer_ctc_weight', MWER_DEFAULTS['mwer_ctc_weight'],
             'Weight of the CTC loss beside the expected risk (finite, >= 0; a choice, not a '
             'measured optimum).', _mwer_ctc_weight_check)
FLAGS.define('string', 'mwer_risk', MWER_DEFAULTS['mwer_risk'],
             "The error count whose expectation is minimised: 'word' or 'label'.",
             _one_of('mwer_risk', MWER_RISKS))


def _validate_mwer(flags):
    if flags.mwer_nbest == 0:
        changed = [name for name, default in MWER_DEFAULTS.items()
                   if getattr(flags, name) != default]
        if changed:
            raise ValueError('--{} needs --mwer_nbest >= 2.'.format(changed[0]))
        return
    check_mwer_settings(flags.mwer_nbest, flags.mwer_beam_width, flags.mwer_ctc_weight,
                        flags.mwer_risk)


FLAGS.define_validator(_validate_mwer)

# Long recordings (no counterpart in the reference): `python -m ctc_asr_amd.transcribe` cuts
# --input at its pauses (ctc_asr_amd/vad.py), batches the pieces and puts their texts back on one
# time axis.  Nothing else reads these flags.
FLAGS.define('int', 'vad_margin_db', 9,
             'Speech threshold, in whole dB above the noise floor of the recording (0..60).',
             _int_range('vad_margin_db', 0, 60))
FLAGS.define('int', 'vad_floor_permille', 100,
             'Percentile of the 10 ms energies taken as the noise floor, in thousandths (1..999).',
             _int_range('vad_floor_permille', 1, 999))
FLAGS.define('int', 'vad_min_rms', 16,
             'Absolute lower bound of the speech threshold, as an rms of 16-bit samples '
             '(0..32767).', _int_range('vad_min_rms', 0, 32767))
FLAGS.define('int', 'vad_rms', 0,
             'Fixed speech threshold as an rms (1..32767); 0: derived from the recording.',
             _int_range('vad_rms', 0, 32767))
FLAGS.define('int', 'vad_pad_ms', 200,
             'Padding around speech, and half the pause that is bridged, in ms (0..2000; whole '
             '10 ms steps, rounded down).', _int_range('vad_pad_ms', 0, 2000))
FLAGS.define('int', 'vad_min_speech_ms', 50,
             'Speech above the threshold a piece must hold, in ms (10..2000).',
             _int_range('vad_min_speech_ms', 10, 2000))
FLAGS.define('int', 'max_segment_seconds', 15,
             'Longest piece; longer speech is cut at its quietest 10 ms (1..30).',
             _int_range('max_segment_seconds', 1, 30))
FLAGS.define('string', 'transcribe_output', '',
             'transcribe.py: JSON-lines file, one line per piece; empty: print.')

# A long recording WITH its text (no counterpart in the reference): `python -m
# ctc_asr_amd.align_long` places --transcript on --input (one alignment over the whole recording,
# `hip.ctc_align_long`), writes the word times to --align_output and, with --corpus_out_dir /
# --corpus_out_csv, cuts the recording at the pauses between words into a training corpus.
# Nothing else reads these flags.
FLAGS.define('string', 'transcript', '', 'align_long.py: text file holding what --input says.')
FLAGS.define('string', 'corpus_out_dir', '', 'align_long.py: directory the cut WAV files go to.')
FLAGS.define('string', 'corpus_out_csv', '',
             'align_long.py: manifest (path;label;length) of the cut corpus; a JSON-lines report '
             'of every utterance is written next to it.')
FLAGS.define('int', 'cut_max_seconds', 15, 'Longest utterance that is cut, in seconds (1..17).',
             _int_range('cut_max_seconds', 1, 17))
FLAGS.define('int', 'cut_min_gap_ms', 200,
             'Shortest pause between two words at which a cut is made, in ms (0..5000).',
             _int_range('cut_min_gap_ms', 0, 5000))
FLAGS.define('int', 'cut_pad_ms', 100,
             'Audio kept before the first and after the last word of an utterance, in ms '
             '(0..1000).', _int_range('cut_pad_ms', 0, 1000))


def parse_cut_min_confidence(text):
    """--cut_min_confidence: '' (off) -> None, otherwise a finite float."""
    if text == '':
        return None
    try:
        value = float(text)
    except ValueError:
        value = float('nan')
    if not math.isfinite(value):
        raise ValueError('--cut_min_confidence={} is neither empty nor a finite number.'
                         .format(text))
    return value


FLAGS.define('string', 'cut_min_confidence', '',
             'Utterances whose mean log-probability over their label frames is below this are '
             'reported as low_confidence and not written; empty: off.', parse_cut_min_confidence)


def check_transcript_wildcard(token):
    """--transcript_wildcard: '' (off), or one token that no word of a transcript can be: no
    whitespace in it, and nothing of it survives `align_long.normalize_transcript`."""
    if token == '':
        return
    if token.split() != [token]:
        raise ValueError('--transcript_wildcard="{}" holds whitespace: it is one token of the '
                         'transcript.'.format(token))
    from ctc_asr_amd.align_long import normalize_transcript    # (imports this module)
    try:
        word = normalize_transcript(token)
    except ValueError as error:
        if 'digit' in str(error):
            raise ValueError('--transcript_wildcard="{}" holds a digit.'.format(token))
        return
    raise ValueError('--transcript_wildcard="{}" reads as the word "{}": choose a token without '
                     'letters, such as "[...]".'.format(token, word))


# A text that covers only PART of the recording (`hip.ctc_align_partial`): both off by default,
# and then `align_long` does what it did without them.
FLAGS.define('string', 'transcript_wildcard', '',
             'align_long.py: a whitespace-delimited token of the transcript that stands for '
             '"something is said here that the text does not hold"; empty: off.',
             check_transcript_wildcard)
FLAGS.define('bool', 'align_free_ends', False,
             'align_long.py: the same before the first word and after the last one of the '
             'transcript (a spoken preamble, a closing line).')

# Phrase spotting (no counterpart in the reference): `python -m ctc_asr_amd.search` looks for the
# phrases of --phrases in --input, scoring them against the logits (`hip.ctc_search`), not against
# the decoded text.  Nothing else reads these flags.
SEARCH_MAX_HITS = 1024     # hip.SEARCH_MAX_HITS: the most hits the kernel stores per pair


def _check_search_min_score(value):
    if not (math.isfinite(value) and value <= 0):
        raise ValueError('--search_min_score={} is not a finite number <= 0.'.format(value))


FLAGS.define('string', 'phrases', '',
             'search.py: text file, one phrase a line; blank lines are skipped.')
FLAGS.define('float', 'search_min_score', -1.0,
             'Lowest score PER LABEL of a hit: the log of (best path through the phrase) over '
             '(the greedy path on the same frames), divided by the number of labels; a finite '
             'float <= 0.  The default is a choice, not a measured value: calibrate it on the '
             'summary lines search.py prints for every phrase.', _check_search_min_score)
FLAGS.define('int', 'search_max_hits', 16,
             'Most hits kept per phrase and piece (1..{}).'.format(SEARCH_MAX_HITS),
             _int_range('search_max_hits', 1, SEARCH_MAX_HITS))
FLAGS.define('string', 'search_output', '',
             'search.py: JSON-lines file, one line per hit, then one per phrase; empty: print.')

# ####### Constants (asr/params.py:138-155). #########
NP_FLOAT = np.float32

MIN_EXAMPLE_LENGTH = 0.7
MAX_EXAMPLE_LENGTH = 17.0

WIN_LENGTH = 0.025  # Window length in seconds.
WIN_STEP = 0.010  # Step between successive windows in seconds.
NUM_FEATURES = 80  # Number of features to extract.

CSV_HEADER_PATH = 'path'
CSV_HEADER_LABEL = 'label'
CSV_HEADER_LENGTH = 'length'
CSV_FIELDNAMES = [CSV_HEADER_PATH, CSV_HEADER_LABEL, CSV_HEADER_LENGTH]
CSV_DELIMITER = ';'


def get_parameters():
    """Summary string of training and network parameters (``asr/params.py:160-184``)."""
    rows = [
        '',
        '\tLearning Rate (lr={}, steps_per_decay={:,d}, decay_factor={});'.format(
            FLAGS.learning_rate, FLAGS.steps_per_decay, FLAGS.learning_rate_decay_factor),
        '\tGPU-Options (cudnn={});'.format(FLAGS.cudnn),
        '\tModel (used_model={}, beam_width={:,d})'.format(FLAGS.used_model, FLAGS.beam_width),
        '\tConv (conv_filters={}); Dense (num_units={:,d});'.format(
            FLAGS.conv_filters, FLAGS.num_units_dense),
        '\tRNN (num_units={:,d}, num_layers={:,d});'.format(
            FLAGS.num_units_rnn, FLAGS.num_layers_rnn),
        '\tTraining (batch_size={:,d}, max_epochs={:,d}, log_frequency={:,d});'.format(
            FLAGS.batch_size, FLAGS.max_epochs, FLAGS.log_frequency),
        '\tFeatures (type={}, normalization={}, skip_every_2nd_frame={});'.format(
            FLAGS.feature_type, FLAGS.feature_normalization,
            FLAGS.features_drop_every_second_frame),
    ]
    if FLAGS.max_grad_norm > 0 or FLAGS.report_grad_norms:
        # (a row of its own, and only when switched on: the summary of a default run stays the
        # reference's, line for line)
        rows.append('\tGradients (max_grad_norm={}, report_grad_norms={});'.format(
            FLAGS.max_grad_norm, FLAGS.report_grad_norms))
    if FLAGS.rnn_batch_norm:
        rows.append('\tBatchNorm (rnn_batch_norm={}, rnn_bn_decay={});'.format(
            FLAGS.rnn_batch_norm, FLAGS.rnn_bn_decay))
    if FLAGS.spec_augment or FLAGS.speed_perturb:
        rows.append('\tAugmentation (spec_augment={}, freq_masks={} x {}, time_masks={} x {}, '
                    'time_permille={}, speed_perturb={});'.format(
                        FLAGS.spec_augment, FLAGS.specaug_freq_masks, FLAGS.specaug_freq_width,
                        FLAGS.specaug_time_masks, FLAGS.specaug_time_width,
                        FLAGS.specaug_time_permille, FLAGS.speed_perturb or 'off'))
    if FLAGS.noise_csv:
        rows.append('\tNoise (noise_csv={}, snr_db={}, permille={}, max_seconds={:,d}, '
                    'eval_snr_db={});'.format(
                        FLAGS.noise_csv, FLAGS.noise_snr_db, FLAGS.noise_permille,
                        FLAGS.noise_max_seconds, FLAGS.eval_noise_snr_db or 'off'))
    if FLAGS.rir_csv:
        rows.append('\tReverb (rir_csv={}, permille={}, max_taps={:,d});'.format(
            FLAGS.rir_csv, FLAGS.rir_permille, FLAGS.rir_max_taps))
    if FLAGS.lr_schedule != 'constant' or FLAGS.lr_warmup_steps > 0 or \
            FLAGS.grad_accum_steps > 1 or FLAGS.ema_decay > 0 or FLAGS.eval_ema:
        rows.append('\tSchedule (lr_schedule={}, minimum_lr={}, warmup_steps={:,d}, '
                    'total_steps={:,d}, grad_accum_steps={:,d}, ema_decay={}, eval_ema={});'
                    .format(FLAGS.lr_schedule, FLAGS.minimum_lr, FLAGS.lr_warmup_steps,
                            FLAGS.lr_total_steps, FLAGS.grad_accum_steps, FLAGS.ema_decay,
                            FLAGS.eval_ema))
    if FLAGS.mwer_nbest:
        rows.append('\tMWER (mwer_nbest={:,d}, mwer_beam_width={:,d}, mwer_ctc_weight={}, '
                    'mwer_risk={});'.format(FLAGS.mwer_nbest, FLAGS.mwer_beam_width,
                                            FLAGS.mwer_ctc_weight, FLAGS.mwer_risk))
    return '\n'.join(rows)
