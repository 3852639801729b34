"""ctypes binding of ``libctcasr.so`` (``include/ctcasr.h``) for torch tensors.

PyTorch only supplies device memory and the HIP stream here; every function below hands raw
device pointers to the C ABI.  There is no fallback: a missing library, a CPU tensor or a
non-zero status raises.
"""

import ctypes
import functools
import os

import numpy as np
import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, 'libctcasr.so')

ABI_VERSION = 8
BUILD_PROBE_WRONG_RESULTS, BUILD_NONDEFAULT_TUNING = 1, 2      # ctcasr_build_flags() bits
RNN_DEFAULT, RNN_HALF_CHIP, RNN_WHOLE_CHIP, RNN_ONE_BARRIER = 0, 1, 2, 4   # rnn_fwd/bwd `flags`
RNN_F16 = 16          # persistent LSTM / GRU kernels: the recurrent products as fp16x3 (ABI v5)
RNN_XCD_SPLIT = 32    # fp16-pipe kernels: one direction per half of the XCDs
RNN_STAGGER = 64      # fp16-pipe LSTM-1024 backward, 24 / 32 rows: tiles staggered by half a step
RNN_KPAIR = 128       # fp16-pipe LSTM-2048 backward: the K axis split over pairs of workgroups
RESIDENT_GATE_MAX_US = 100000   # ctcasr_rnn_resident_gate: the longest bound it takes
# ctcasr_grad_norm: floats per chunk of a segment, and the most segments a call takes
GRAD_NORM_CHUNK = 8192
GRAD_NORM_MAX_SEGMENTS = 64
SPEC_AUGMENT_MAX_MASKS = 16     # ctcasr_spec_augment: frequency masks, and time masks, per call
NOISE_MIX_CHUNK = 8192          # ctcasr_noise_mix: samples of a row per workgroup
NOISE_MIX_SNR_DB = (-20, 60)    # ... and the SNR range it takes
REVERB_CHUNK = 2048             # ctcasr_reverb: output samples of a row per workgroup,
REVERB_TAP_BLOCK = 32           # ... taps per round of its inner loop (a remainder 8 at a time),
REVERB_TAP_ALIGN = 8            # ... what a response's length and offset are multiples of,
REVERB_MAX_TAPS = 8192          # ... and the longest response it serves
VAD_HOP = 160                   # ctcasr_vad_energy: samples per hop (the feature step),
VAD_LEVELS = 160                # ... bins of its level histogram,
VAD_CHUNK = 40960               # ... and samples per workgroup
RESAMPLE_MAX_TABLE = 16640      # ctcasr_resample: the most weights (L * taps) of a served rate pair,
RESAMPLE_RATES = (4000, 192000)  # ... the rates it takes,
RESAMPLE_MAX_CHANNELS = 8       # ... and the most channels it mixes down
SEQ_BN_ROWS = 64                # ctcasr_seq_bn_*: consecutive rows per chunk of the pinned sums
ALIGN_LONG_TILE_STATES = 1024   # ctcasr_ctc_align_long: lattice states per tile,
ALIGN_LONG_TILE_FRAMES = 256    # ... frames per tile when the call passes 0,
ALIGN_LONG_MAX = (1 << 22, 1 << 20, 64)   # ... and the most frames, labels and classes it serves
ALIGN_WILDCARD = -1             # ctcasr_ctc_align_partial: the label that matches whatever is said
SEARCH_MAX_LABEL_LEN = 576      # ctcasr_ctc_search: the longest phrase (2L - 1 <= 1151 states),
SEARCH_MAX_HITS = 1024          # ... the most hits it stores per pair,
SEARCH_WAVES = 4                # ... and the pairs one workgroup takes
CELL_IDS = {'rnn_relu': 0, 'rnn_tanh': 1, 'lstm': 2, 'gru': 3}
CELL_GATES = {'rnn_relu': 1, 'rnn_tanh': 1, 'lstm': 4, 'gru': 3}

_c_int, _c_i64, _c_u64 = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
_c_f, _c_p, _c_sz = ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
_c_d = ctypes.c_double

# name -> (restype, argtypes); doubles as the list of symbols the ABI must export
SIGNATURES = {
    'ctcasr_abi_version': (_c_int, []),
    'ctcasr_build_flags': (ctypes.c_uint, []),
    'ctcasr_error_string': (ctypes.c_char_p, [_c_int]),
    'ctcasr_set_option': (_c_int, [ctypes.c_char_p, _c_int]),
    'ctcasr_rnn_kernel_events': (_c_int, [_c_p, _c_p]),
    'ctcasr_log_softmax_fwd': (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_p]),
    'ctcasr_log_softmax_bwd': (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_p]),
    'ctcasr_ctc_loss_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_ctc_loss_fwd_bwd': (_c_int, [_c_p] * 4 + [_c_int] * 5 + [_c_f] + [_c_p] * 4 +
                                [_c_sz, _c_p]),
    'ctcasr_ctc_greedy_decode': (_c_int, [_c_p, _c_p] + [_c_int] * 4 + [_c_p, _c_p, _c_p]),
    'ctcasr_ctc_beam_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_ctc_beam_decode': (_c_int, [_c_p, _c_p] + [_c_int] * 6 + [_c_p] * 4 + [_c_sz, _c_p]),
    'ctcasr_ctc_beam_lm_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_ctc_beam_decode_lm': (_c_int, [_c_p, _c_p] + [_c_int] * 6 + [_c_p] * 3 + [_c_int] +
                                  [_c_p] * 4 + [_c_sz, _c_p]),
    'ctcasr_ctc_beam_wordlm_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_ctc_beam_decode_wordlm': (_c_int, [_c_p, _c_p] + [_c_int] * 7 + [_c_p] * 6 +
                                      [_c_sz, _c_p]),
    'ctcasr_ctc_beam_decode_wordlm_lookahead': (_c_int, [_c_p, _c_p] + [_c_int] * 7 + [_c_p] * 7 +
                                                [_c_sz, _c_p]),
    'ctcasr_wordlm_lookup': (_c_int, [_c_p] * 3 + [_c_int] + [_c_p] * 3),
    'ctcasr_ctc_beam_nbest_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_ctc_beam_decode_nbest': (_c_int, [_c_p, _c_p] + [_c_int] * 7 + [_c_p] * 3 + [_c_int] +
                                     [_c_p] * 5 + [_c_sz, _c_p]),
    'ctcasr_ctc_score_workspace_bytes': (_c_sz, [_c_int] * 5),
    'ctcasr_ctc_score': (_c_int, [_c_p, _c_p] + [_c_int] * 4 + [_c_p] * 3 + [_c_int] * 2 +
                         [_c_p] * 3 + [_c_sz, _c_p]),
    'ctcasr_ctc_mwer_workspace_bytes': (_c_sz, [_c_int] * 5),
    'ctcasr_ctc_mwer': (_c_int, [_c_p, _c_p] + [_c_int] * 4 + [_c_p] * 4 + [_c_int, _c_int, _c_f,
                                                                              _c_int] +
                        [_c_p] * 6 + [_c_sz, _c_p]),
    'ctcasr_ctc_align_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_ctc_align': (_c_int, [_c_p] * 4 + [_c_int] * 5 + [_c_p] * 5 + [_c_sz, _c_p]),
    'ctcasr_ctc_align_long_workspace_bytes': (_c_sz, [_c_i64, _c_int, _c_i64, _c_int]),
    'ctcasr_ctc_align_long': (_c_int, [_c_p, _c_p, _c_i64, _c_int, _c_int, _c_i64, _c_int] +
                              [_c_p] * 6 + [_c_sz, _c_p]),
    'ctcasr_ctc_align_partial': (_c_int, [_c_p, _c_p, _c_i64, _c_int, _c_int, _c_i64, _c_int] +
                                 [_c_p] * 6 + [_c_sz, _c_p]),
    'ctcasr_ctc_search_workspace_bytes': (_c_sz, [_c_int] * 3),
    'ctcasr_ctc_search': (_c_int, [_c_p, _c_p] + [_c_int] * 4 + [_c_p, _c_p, _c_int, _c_int] +
                          [_c_p] * 3 + [_c_int, _c_int] + [_c_p] * 9 + [_c_sz, _c_p]),
    'ctcasr_edit_distance_workspace_bytes': (_c_sz, [_c_int] * 3),
    'ctcasr_edit_distance': (_c_int, [_c_p] * 6 + [_c_int] * 3 + [_c_p] * 6 + [_c_sz, _c_p]),
    'ctcasr_rnn_reserve_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_rnn_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_rnn_persistent_supported': (_c_int, [_c_int] * 4),
    'ctcasr_rnn_poll_error': (_c_int, [_c_p, _c_sz] + [_c_int] * 4 + [_c_p]),
    'ctcasr_rnn_resident_gate': (_c_int, [_c_p, _c_sz] + [_c_int] * 4 + [ctypes.c_uint, _c_int,
                                                                          _c_p]),
    'ctcasr_rnn_gru_drec_offset': (_c_sz, [_c_int] * 3),
    'ctcasr_rnn_fwd': (_c_int, [_c_int] + [_c_p] * 5 + [_c_int] * 3 + [_c_p] * 3 + [_c_sz, _c_p]),
    'ctcasr_rnn_bwd': (_c_int, [_c_int] + [_c_p] * 5 + [_c_int] * 3 + [_c_p] * 4 + [_c_sz, _c_p]),
    'ctcasr_rnn_fwd_steps': (_c_int, [_c_int] + [_c_p] * 5 + [_c_int] * 3 + [_c_p] * 4 +
                             [_c_sz, _c_int, _c_int, _c_int, _c_p]),
    'ctcasr_rnn_fwd_f16_supported': (_c_int, [_c_int] * 5),
    'ctcasr_rnn_bwd_steps': (_c_int, [_c_int] + [_c_p] * 5 + [_c_int] * 3 + [_c_p] * 5 +
                             [_c_sz, _c_int, _c_int, _c_int, _c_p]),
    'ctcasr_rnn_bwd_f16_supported': (_c_int, [_c_int] * 5),
    'ctcasr_bias_act_fwd': (_c_int, [_c_p, _c_p, _c_i64, _c_int, _c_f, _c_f, _c_u64, _c_p]),
    'ctcasr_bias_act_bwd': (_c_int, [_c_p] * 4 + [_c_i64, _c_int, _c_f, _c_f, _c_p]),
    'ctcasr_dropout': (_c_int, [_c_p, _c_p, _c_i64, _c_f, _c_u64, _c_p]),
    'ctcasr_colsum_accumulate': (_c_int, [_c_p, _c_p, _c_i64, _c_int, _c_p]),
    'ctcasr_conv_s12_supported': (_c_int, [_c_int, _c_int]),
    'ctcasr_conv_s12_pack_weights': (_c_int, [_c_p, _c_p, _c_int, _c_p]),
    'ctcasr_conv_s12_fwd': (_c_int, [_c_p, _c_p, _c_p, _c_p] + [_c_int] * 4 + [_c_f, _c_int, _c_p]),
    'ctcasr_conv_s12_pack16_bytes': (_c_sz, [_c_int]),
    'ctcasr_conv_s12_pack_weights16': (_c_int, [_c_p, _c_p, _c_int, _c_p]),
    'ctcasr_conv_s12_fwd16': (_c_int, [_c_p, _c_f, _c_p, _c_p, _c_p] + [_c_int] * 4 +
                              [_c_f, _c_int, _c_p]),
    'ctcasr_conv_s12_bwd_data16': (_c_int, [_c_p, _c_p, _c_p] + [_c_int] * 5 + [_c_p, _c_f, _c_p]),
    'ctcasr_conv0_pack16_bytes': (_c_sz, []),
    'ctcasr_conv0_pack_weights16': (_c_int, [_c_p, _c_p, _c_p]),
    'ctcasr_conv0_fwd16': (_c_int, [_c_p] * 4 + [_c_int, _c_int, _c_f, _c_p]),
    'ctcasr_conv0_wrw16_workspace_bytes': (_c_sz, [_c_int, _c_int]),
    'ctcasr_conv0_wrw16': (_c_int, [_c_p] * 3 + [_c_int, _c_int, _c_p, _c_f, _c_p, _c_p, _c_sz,
                                                 _c_p]),
    'ctcasr_conv_s12_wrw16_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_conv_s12_wrw16': (_c_int, [_c_p, _c_p, _c_f, _c_p] + [_c_int] * 5 +
                              [_c_p, _c_f, _c_p, _c_p, _c_sz, _c_p]),
    'ctcasr_conv_s12_bwd_data': (_c_int, [_c_p, _c_p, _c_p] + [_c_int] * 5 + [_c_p, _c_f, _c_p]),
    'ctcasr_conv_s12_wrw_workspace_bytes': (_c_sz, [_c_int] * 4),
    'ctcasr_conv_s12_wrw': (_c_int, [_c_p] * 3 + [_c_int] * 5 + [_c_p, _c_f, _c_p] +
                            [_c_p, _c_sz, _c_p]),
    'ctcasr_conv0_fwd': (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_f, _c_p]),
    'ctcasr_conv0_wrw_workspace_bytes': (_c_sz, [_c_int, _c_int]),
    'ctcasr_conv0_wrw': (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_p, _c_f, _c_p, _c_p, _c_sz,
                                  _c_p]),
    'ctcasr_transpose_batched': (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p]),
    'ctcasr_split_bf16': (_c_int, [_c_p, _c_i64, _c_int, _c_i64, _c_p, _c_int, _c_p, _c_i64, _c_i64,
                                   _c_p]),
    'ctcasr_split_f16': (_c_int, [_c_p, _c_i64, _c_int, _c_i64, _c_f, _c_p, _c_int, _c_p, _c_i64,
                                  _c_i64, _c_p]),
    'ctcasr_colmax_scale': (_c_int, [_c_p, _c_i64, _c_int, _c_i64, _c_p, _c_p, _c_p, _c_p]),
    'ctcasr_colscale_from_max': (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p]),
    'ctcasr_split_f16_cols': (_c_int, [_c_p, _c_i64, _c_int, _c_i64, _c_p, _c_f, _c_p, _c_int, _c_p,
                                       _c_i64, _c_i64, _c_p]),
    'ctcasr_split_f16_rows': (_c_int, [_c_p, _c_i64, _c_int, _c_i64, _c_p, _c_int, _c_p, _c_i64,
                                       _c_i64, _c_p, _c_p]),
    'ctcasr_rescale_rows': (_c_int, [_c_p, _c_i64, _c_p, _c_f, _c_p, _c_i64, _c_i64, _c_int, _c_int,
                                     _c_p]),
    'ctcasr_gemm_split_nt': (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_int, _c_int,
                                      _c_int, _c_p]),
    'ctcasr_gemm_split_tn': (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_int, _c_int,
                                      _c_int, _c_p]),
    'ctcasr_rnn_f16_recurrence': (_c_int, [_c_int] * 7),
    'ctcasr_collective_traffic': (_c_int, [_c_int, _c_int, _c_p, _c_p, _c_i64, _c_i64, _c_p]),
    'ctcasr_wgrad16_packed_bytes': (_c_sz, [_c_int, _c_int]),
    'ctcasr_wgrad16_pack': (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_i64, _c_int, _c_p, _c_f, _c_p,
                                     _c_p]),
    'ctcasr_wgrad16_gemm': (_c_int, [_c_p, _c_int, _c_int, _c_p, _c_p, _c_int, _c_int, _c_f, _c_p,
                                     _c_i64, _c_p, _c_int, _c_int, _c_f, _c_p, _c_i64, _c_int, _c_p,
                                     _c_p]),
    'ctcasr_wgrad16_sync_ints': (_c_sz, [_c_int, _c_int, _c_int]),
    'ctcasr_dgrad16_packed_bytes': (_c_sz, [_c_int]),
    'ctcasr_dgrad16_pack_weights': (_c_int, [_c_p, _c_i64, _c_int, _c_int, _c_f, _c_p, _c_p]),
    'ctcasr_dgrad16_supported': (_c_int, [_c_int] * 4),
    'ctcasr_dgrad16_published_offsets': (_c_int, [_c_int, _c_int, _c_int, _c_p, _c_p]),
    'ctcasr_dgrad16_blockscaled': (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_p, _c_f, _c_int, _c_p,
                                            _c_i64] + [_c_int] * 5 + [_c_p]),
    'ctcasr_features_num_frames': (_c_int, [_c_int]),
    'ctcasr_features_tables_bytes': (_c_sz, []),
    'ctcasr_features_init_tables': (_c_int, [_c_p, _c_int, _c_p]),
    'ctcasr_features_workspace_bytes': (_c_sz, [_c_int, _c_int]),
    'ctcasr_features': (_c_int, [_c_p, _c_p] + [_c_int] * 5 + [_c_p, _c_p, _c_int, _c_p, _c_p,
                                 _c_sz, _c_p]),
    'ctcasr_spec_augment': (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_u64] + [_c_int] * 5 +
                            [_c_p, _c_p]),
    'ctcasr_resample_num_samples': (_c_int, [_c_int, _c_int]),
    'ctcasr_speed_perturb': (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_p, _c_int, _c_p, _c_p]),
    'ctcasr_noise_mix_workspace_bytes': (_c_sz, [_c_int]),
    'ctcasr_noise_mix': (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_p, _c_p, _c_int, _c_u64] +
                         [_c_int] * 3 + [_c_p] * 5 + [_c_sz, _c_p]),
    'ctcasr_reverb': (_c_int, [_c_p, _c_p, _c_int, _c_int] + [_c_p] * 4 + [_c_int, _c_u64, _c_int] +
                      [_c_p] * 3),
    'ctcasr_vad_energy': (_c_int, [_c_p, _c_i64, _c_p, _c_p, _c_p]),
    'ctcasr_gather_segments': (_c_int, [_c_p, _c_i64, _c_p, _c_p, _c_int, _c_int] + [_c_p] * 3),
    'ctcasr_resample_plan': (_c_int, [_c_int, _c_int] + [_c_p] * 4),
    'ctcasr_resample_chunk': (_c_int, [_c_int, _c_int]),
    'ctcasr_resample_out_samples': (_c_i64, [_c_i64, _c_int, _c_int]),
    'ctcasr_resample_table_bytes': (_c_sz, [_c_int, _c_int]),
    'ctcasr_resample_table': (_c_int, [_c_int, _c_int, _c_p, _c_p]),
    'ctcasr_resample': (_c_int, [_c_p, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_p, _c_p, _c_i64,
                                 _c_p, _c_p]),
    'ctcasr_adam_step': (_c_int, [_c_p] * 4 + [_c_i64] + [_c_f] * 4 + [_c_i64, _c_f, _c_p, _c_p]),
    'ctcasr_adam_step_clipped': (_c_int, [_c_p] * 4 + [_c_i64] + [_c_f] * 4 +
                                 [_c_i64, _c_f, _c_p, _c_p, _c_p]),
    'ctcasr_adam_step_ema': (_c_int, [_c_p] * 5 + [_c_i64] + [_c_f] * 4 +
                             [_c_i64, _c_f, _c_p, _c_p, _c_f, _c_p]),
    'ctcasr_grad_norm_workspace_bytes': (_c_sz, [_c_i64, _c_int]),
    'ctcasr_grad_norm': (_c_int, [_c_p, _c_i64, _c_p, _c_int, _c_f, _c_f] + [_c_p] * 4 +
                         [_c_sz, _c_p]),
    'ctcasr_seq_bn_workspace_bytes': (_c_sz, [_c_i64, _c_int]),
    'ctcasr_seq_bn_fwd': (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int] + [_c_p] * 4 +
                          [_c_d, _c_d] + [_c_p] * 4 + [_c_sz, _c_p]),
    'ctcasr_seq_bn_infer': (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int] + [_c_p] * 4 +
                            [_c_d, _c_p, _c_p]),
    'ctcasr_seq_bn_bwd': (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int] + [_c_p] * 7 +
                          [_c_sz, _c_p]),
    'ctcasr_step_guard': (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'ctcasr_rnn_timeout_word_offset': (_c_sz, [_c_int] * 5),
    'ctcasr_absmax': (_c_int, [_c_p, _c_i64, _c_p, _c_p]),
    'ctcasr_occupy_cus': (_c_int, [_c_int, _c_int, _c_p]),
}

_lib = None

# Optional per-entry-point timing: set ``EVENTS = {}`` and every wrapped call listed in
# ``TIMED`` is bracketed by HIP events on the launch stream (``drain_events`` returns ms sums).
EVENTS = None
TIMED = ('rnn_fwd', 'rnn_bwd', 'ctc_loss_fwd_bwd', 'dgrad16')


class _Timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if EVENTS is not None and self.name in TIMED:
            self.start = torch.cuda.Event(enable_timing=True)
            self.stop = torch.cuda.Event(enable_timing=True)
            self.start.record()
        return self

    def __exit__(self, *exc):
        if EVENTS is not None and self.name in TIMED:
            self.stop.record()
            EVENTS.setdefault(self.name, []).append((self.start, self.stop))
        return False


def drain_events():
    """{name: (calls, total_ms)} for the events collected so far; call after a synchronize."""
    global EVENTS
    out = {}
    for name, pairs in (EVENTS or {}).items():
        out[name] = (len(pairs), sum(a.elapsed_time(b) for a, b in pairs))
    if EVENTS is not None:
        EVENTS = {}
    return out


class CtcAsrError(RuntimeError):
    """Non-zero status from the C ABI."""


def load(path=None):
    """Load the library once; raises if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get('CTCASR_LIB') or LIB_PATH      # (A/B builds: tools/build_alt.sh)
    if not os.path.exists(path):
        raise CtcAsrError('{} is missing - build it with `python -m ctc_asr_amd.build`; the '
                          'MI355X path has no CPU fallback.'.format(path))
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the ABI does not export the symbol
        fn.restype, fn.argtypes = restype, argtypes
    if lib.ctcasr_abi_version() != ABI_VERSION:
        raise CtcAsrError('libctcasr ABI version mismatch')
    # probe builds of the kernels (tools/build_alt.sh -DPRNN_PROBE_...) compute wrong results on
    # purpose: never let one stand in for the product library by accident
    if lib.ctcasr_build_flags() & BUILD_PROBE_WRONG_RESULTS and \
            os.environ.get('CTCASR_ALLOW_PROBE_BUILD') != '1':
        raise CtcAsrError('{} is a timing-probe build (ctcasr_build_flags() = {:#x}: results are '
                          'wrong on purpose); set CTCASR_ALLOW_PROBE_BUILD=1 to load it anyway.'
                          .format(path, lib.ctcasr_build_flags()))
    _lib = lib
    return lib


def _check(code, what):
    if code != 0:
        raise CtcAsrError('{} failed: {} ({})'.format(
            what, load().ctcasr_error_string(code).decode(), code))


def _dev(tensor, dtype=torch.float32, name='tensor'):
    if tensor is None:
        return None
    if not tensor.is_cuda:
        raise CtcAsrError('{} must live in HBM (got a CPU tensor); there is no CPU path.'
                          .format(name))
    if tensor.dtype != dtype:
        raise CtcAsrError('{} must be {} (got {}).'.format(name, dtype, tensor.dtype))
    if not tensor.is_contiguous():
        raise CtcAsrError('{} must be contiguous.'.format(name))
    return tensor.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _expect_numel(what, name, tensor, want):
    """The library takes raw pointers and trusts the lengths it is told: refuse an argument
    that does not hold ``want`` elements before its address crosses the ABI."""
    if tensor is not None and tensor.numel() != want:
        raise CtcAsrError('{}: {} holds {} elements, {} expected.'
                          .format(what, name, tensor.numel(), want))


def _last_dim(what, name, tensor):
    if tensor.dim() < 1 or tensor.shape[-1] < 1:
        raise CtcAsrError('{}: {} needs a last dimension of at least one column (got shape {}).'
                          .format(what, name, tuple(tensor.shape)))
    return tensor.shape[-1]


def _on_tensor_device(fn):
    """Run a launching wrapper with the device of its first GPU tensor argument current, so that
    the stream it launches on (`_stream`) and the memory it is given belong to the same GPU even
    when the caller's current device is another one (``CTCModel(cfg, 'cuda:1')`` from a
    process whose current device is 0)."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        for value in list(args) + list(kwargs.values()):
            if torch.is_tensor(value) and value.is_cuda:
                if value.device.index != torch.cuda.current_device():
                    with torch.cuda.device(value.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapper


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------
def set_option(name, value):
    _check(load().ctcasr_set_option(name.encode(), int(value)), 'set_option')


@_on_tensor_device
def log_softmax_fwd(x, out=None):
    rows, classes = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    _check(load().ctcasr_log_softmax_fwd(_dev(x, name='x'), _dev(out, name='out'), rows, classes,
                                         _stream()), 'log_softmax_fwd')
    return out


@_on_tensor_device
def log_softmax_bwd(y, dy, out=None):
    rows, classes = y.numel() // y.shape[-1], y.shape[-1]
    out = torch.empty_like(y) if out is None else out
    _check(load().ctcasr_log_softmax_bwd(_dev(y, name='y'), _dev(dy, name='dy'),
                                         _dev(out, name='out'), rows, classes, _stream()),
           'log_softmax_bwd')
    return out


def ctc_loss_workspace_bytes(num_steps, batch, classes, max_label_len):
    return load().ctcasr_ctc_loss_workspace_bytes(num_steps, batch, classes, max_label_len)


@_on_tensor_device
def ctc_loss_fwd_bwd(logits, labels, label_offsets, seq_len, max_label_len, blank=None,
                     grad_scale=1.0, loss=None, grad=None, status=None, workspace=None):
    """logits f32[T,B,C]; labels/label_offsets/seq_len int32 device tensors.
    Returns (loss f32[B], grad f32[T,B,C], status i32[B])."""
    num_steps, batch, classes = logits.shape
    blank = classes - 1 if blank is None else blank
    dev = logits.device
    loss = torch.empty(batch, dtype=torch.float32, device=dev) if loss is None else loss
    grad = torch.empty_like(logits) if grad is None else grad
    status = torch.empty(batch, dtype=torch.int32, device=dev) if status is None else status
    need = ctc_loss_workspace_bytes(num_steps, batch, classes, max_label_len)
    if workspace is None:
        workspace = _workspace(need, dev)
    with _Timed('ctc_loss_fwd_bwd'):
      _check(load().ctcasr_ctc_loss_fwd_bwd(
        _dev(logits, name='logits'), _dev(labels, torch.int32, 'labels'),
        _dev(label_offsets, torch.int32, 'label_offsets'), _dev(seq_len, torch.int32, 'seq_len'),
        num_steps, batch, classes, blank, int(max_label_len), float(grad_scale),
        _dev(loss, name='loss'), _dev(grad, name='grad'), _dev(status, torch.int32, 'status'),
        _dev(workspace, torch.uint8, 'workspace'), workspace.numel(), _stream()),
        'ctc_loss_fwd_bwd')
    return loss, grad, status


def _decode_shape(what, logits, seq_len):
    """(T, B, C) of a decoder's ``logits``; refuses anything but [T, B, C] with one length per
    utterance - the kernels index ``seq_len`` by the batch of ``logits``."""
    if logits.dim() != 3:
        raise CtcAsrError('{}: logits must be [T, B, C] (got {} dimensions).'
                          .format(what, logits.dim()))
    if seq_len.numel() != logits.shape[1]:
        raise CtcAsrError('{}: seq_len holds {} lengths for a batch of {}.'
                          .format(what, seq_len.numel(), logits.shape[1]))
    return logits.shape


@_on_tensor_device
def ctc_greedy_decode(logits, seq_len, blank=None, out=None, out_len=None):
    num_steps, batch, classes = _decode_shape('ctc_greedy_decode', logits, seq_len)
    blank = classes - 1 if blank is None else blank
    dev = logits.device
    out = torch.empty((batch, num_steps), dtype=torch.int32, device=dev) if out is None else out
    out_len = torch.empty(batch, dtype=torch.int32, device=dev) if out_len is None else out_len
    _check(load().ctcasr_ctc_greedy_decode(
        _dev(logits, name='logits'), _dev(seq_len, torch.int32, 'seq_len'), num_steps, batch,
        classes, blank, _dev(out, torch.int32, 'out'), _dev(out_len, torch.int32, 'out_len'),
        _stream()), 'ctc_greedy_decode')
    return out, out_len


class WordLm(ctypes.Structure):
    """``ctcasr_wordlm_t`` of include/ctcasr.h."""
    _fields_ = [(name, _c_p) for name in ('trie_next', 'trie_word', 'ctx_begin', 'succ_word',
                                          'succ_lp', 'succ_ctx', 'ctx_backoff', 'ctx_parent')] + \
               [('num_succ', _c_i64), ('num_nodes', ctypes.c_int32), ('num_ctx', ctypes.c_int32),
                ('order', ctypes.c_int32), ('space', ctypes.c_int32), ('bonus', _c_d),
                ('oov_score', _c_d), ('stats', _c_p)]


def _wordlm_struct(scorer, device, stats=None):
    """(`WordLm` of a scaled `lm.WordLmScorer` on ``device``, the tensors it points into)."""
    tensors = scorer.to(device)
    names = ('trie_next', 'trie_word', 'ctx_begin', 'succ_word', 'succ_lp', 'succ_ctx',
             'ctx_backoff', 'ctx_parent')
    kinds = (torch.int32, torch.int32, torch.int64, torch.int32, torch.float64, torch.int32,
             torch.float64, torch.int32)
    # an empty table has no address to give: nothing of it is read then
    fields = {name: _dev(t, kind, name) if t.numel() else None
              for name, kind, t in zip(names, kinds, tensors)}
    return WordLm(num_succ=scorer.num_successors, num_nodes=scorer.num_nodes,
                  num_ctx=scorer.num_contexts, order=scorer.order, space=scorer.space,
                  bonus=scorer.bonus, oov_score=scorer.oov_score,
                  stats=None if stats is None else _dev(stats, torch.int64, 'stats'),
                  **fields), tensors


def _is_word(scorer):
    """Whether ``scorer`` is a word model (`lm.WordLmScorer`) and not a dense one
    (`lm.LmScorer`): the scorer classes say what they are, and only this function asks."""
    return scorer is not None and scorer.kind == 'word'


def _beam_workspace_bytes(word, num_steps, batch, classes, beam_width):
    # (a dense model and an n-best list need the plain search's pool: csrc/beam.hip)
    sizer = load().ctcasr_ctc_beam_wordlm_workspace_bytes if word else \
        load().ctcasr_ctc_beam_workspace_bytes
    return sizer(num_steps, batch, classes, int(beam_width))


def ctc_beam_search_workspace_bytes(num_steps, batch, classes, beam_width, scorer=None):
    """The workspace of `ctc_beam_search` with the same ``scorer``, for any ``top_paths``."""
    return _beam_workspace_bytes(_is_word(scorer), num_steps, batch, classes, beam_width)


def _lookahead_on(what, scorer, device):
    """A word scorer's look-ahead table on ``device``, or None if it carries none; a table of
    the wrong length or with a non-finite entry is refused."""
    lookahead = getattr(scorer, 'lookahead', None)
    if lookahead is None:
        return None
    lookahead = np.asarray(lookahead)
    if lookahead.shape != (scorer.num_nodes,):
        raise CtcAsrError('{}: the look-ahead table has shape {}, the trie {} nodes.'
                          .format(what, lookahead.shape, scorer.num_nodes))
    if not np.isfinite(lookahead).all():
        raise CtcAsrError('{}: the look-ahead table holds a non-finite entry.'.format(what))
    return scorer.lookahead_to(device)


@_on_tensor_device
def _beam_search(what, logits, seq_len, beam_width, scorer, top_paths, blank, normalization,
                 stats):
    """`ctc_beam_search` under the name ``what``, which the errors carry."""
    num_steps, batch, classes = _decode_shape(what, logits, seq_len)
    if scorer is not None and scorer.num_classes != classes:
        raise CtcAsrError('{}: the scorer has {} classes, the logits {}.'
                          .format(what, scorer.num_classes, classes))
    blank = classes - 1 if blank is None else blank
    dev = logits.device
    word = _is_word(scorer)
    nbest = word or top_paths is not None       # (the word model has n-best kernels only)
    ranks = 1 if top_paths is None else int(top_paths)
    if stats is not None:
        if not word:
            raise CtcAsrError('{}: stats are counted with a word scorer only.'.format(what))
        _expect_numel(what, 'stats', stats, 2 * batch)
    # `keep`: the tables on the device, referenced until the call has returned
    entry, model, keep = 'ctcasr_ctc_beam_decode', (), None
    if word:
        lookahead = _lookahead_on(what, scorer, dev)
        tables, keep = _wordlm_struct(scorer, dev, stats)
        entry, model = entry + '_wordlm', (ctypes.addressof(tables),)
        if lookahead is not None:
            entry, keep = entry + '_lookahead', (keep, lookahead)
            model += (_dev(lookahead, torch.float64, 'trie_lookahead'),)
    elif scorer is not None or nbest:
        entry += '_nbest' if nbest else '_lm'
        keep = scorer.to(dev) if scorer is not None else (None, None, None)
    shape = (batch, max(ranks, 0)) if nbest else (batch,)
    out = torch.empty(shape + (num_steps,), dtype=torch.int32, device=dev)
    out_len = torch.empty(shape, dtype=torch.int32, device=dev)
    logp = torch.empty(shape, dtype=torch.float32, device=dev)
    n_paths = torch.empty(batch, dtype=torch.int32, device=dev) if nbest else None
    workspace = _workspace(_beam_workspace_bytes(word, num_steps, batch, classes, beam_width), dev)
    args = (_dev(logits, name='logits'), _dev(seq_len, torch.int32, 'seq_len'), num_steps, batch,
            classes, blank, int(beam_width), {'max': 0, 'log_softmax': 1}[normalization])
    if nbest:
        args += (ranks,)
    if not word and keep is not None:
        model = (_dev(keep[0], torch.int32, 'lm_next'), _dev(keep[1], name='lm_score'),
                 _dev(keep[2], name='lm_final'), scorer.num_states if scorer is not None else 0)
    args += model + (_dev(out, torch.int32, 'out'), _dev(out_len, torch.int32, 'out_len'),
                     _dev(logp, name='logp'))
    if nbest:
        args += (_dev(n_paths, torch.int32, 'n_paths'),)
    args += (_dev(workspace, torch.uint8, 'workspace'), workspace.numel(), _stream())
    _check(getattr(load(), entry)(*args),
           what + '_lookahead' if entry.endswith('_lookahead') else what)
    del keep
    if bool(((n_paths if nbest else out_len) < 0).any()):
        raise CtcAsrError('{}: prefix-tree pool exhausted'.format(what))
    if not nbest:
        return out, out_len, logp
    if top_paths is None:                       # the word model's top-1: rank 0 of one
        return out[:, 0], out_len[:, 0], logp[:, 0]
    return out, out_len, logp, n_paths


def ctc_beam_search(logits, seq_len, beam_width, scorer=None, top_paths=None, blank=None,
                    normalization='max', stats=None):
    """The CTC beam search of ``logits`` f32 [T, B, C] at ``beam_width``, in every form.

    ``scorer``: None, or a scaled scorer of `lm` fused into the search - an `lm.LmScorer` (a
    dense automaton) or an `lm.WordLmScorer` (a word n-gram over a lexicon trie, K24; one that
    carries a look-ahead table, from ``scaled(..., lookahead=True)``, is searched with look-ahead
    scores inside a word, K26).  ``logp`` includes the model's scores.

    ``top_paths`` None: the best hypothesis, (out i32[B, T], out_len i32[B], logp f32[B]).  An
    integer: the ``top_paths`` best leaves of the final beam, (out i32[B, N, T], out_len
    i32[B, N], logp f32[B, N], n_paths i32[B]); rank 0 is what the top-1 form returns, ranks >=
    n_paths[b] are empty (out_len 0, logp -inf).

    ``stats`` (word scorer only): None or int64 [B, 2] on the device, which receives the
    branches expanded and the word lookups performed per utterance.

    Wrong shapes, a scorer of another class count, a ``stats`` of the wrong size and a look-ahead
    table of the wrong length or with a non-finite entry are refused before anything is launched;
    a ``top_paths`` outside [1, beam_width] is refused by the library."""
    return _beam_search('ctc_beam_search', logits, seq_len, beam_width, scorer, top_paths, blank,
                        normalization, stats)


# The older names, one per model and output form: shims over `ctc_beam_search` and its sizer.
def ctc_beam_workspace_bytes(num_steps, batch, classes, beam_width):
    return _beam_workspace_bytes(False, num_steps, batch, classes, beam_width)


ctc_beam_lm_workspace_bytes = ctc_beam_nbest_workspace_bytes = ctc_beam_workspace_bytes


def ctc_beam_wordlm_workspace_bytes(num_steps, batch, classes, beam_width):
    return _beam_workspace_bytes(True, num_steps, batch, classes, beam_width)


def ctc_beam_decode(logits, seq_len, beam_width, blank=None, normalization='max'):
    return _beam_search('ctc_beam_decode', logits, seq_len, beam_width, None, None, blank,
                        normalization, None)


def ctc_beam_decode_lm(logits, seq_len, beam_width, scorer, blank=None, normalization='max'):
    return _beam_search('ctc_beam_decode_lm', logits, seq_len, beam_width, scorer, None, blank,
                        normalization, None)


def ctc_beam_decode_nbest(logits, seq_len, beam_width, top_paths, scorer=None, blank=None,
                          normalization='max'):
    return _beam_search('ctc_beam_decode_nbest', logits, seq_len, beam_width, scorer,
                        int(top_paths), blank, normalization, None)


def ctc_beam_decode_wordlm(logits, seq_len, beam_width, scorer, top_paths=1, blank=None,
                           normalization='max', stats=None):
    return _beam_search('ctc_beam_decode_wordlm', logits, seq_len, beam_width, scorer,
                        int(top_paths), blank, normalization, stats)


@_on_tensor_device
def wordlm_lookup(scorer, ctx, word):
    """(score f32[n], next_ctx i32[n]) of the pairs (ctx[i], word[i]), int32 on the device: the
    float32 rounding of the back-off walk Wd, by the device function the search uses."""
    if ctx.numel() != word.numel():
        raise CtcAsrError('wordlm_lookup: {} contexts for {} words.'
                          .format(ctx.numel(), word.numel()))
    ctx_ptr, word_ptr = _dev(ctx, torch.int32, 'ctx'), _dev(word, torch.int32, 'word')
    count = ctx.numel()
    tables, keep = _wordlm_struct(scorer, ctx.device)
    score = torch.empty(count, dtype=torch.float32, device=ctx.device)
    next_ctx = torch.empty(count, dtype=torch.int32, device=ctx.device)
    if count:
        _check(load().ctcasr_wordlm_lookup(
            ctypes.addressof(tables), ctx_ptr, word_ptr, count, _dev(score, name='score'),
            _dev(next_ctx, torch.int32, 'next_ctx'), _stream()), 'wordlm_lookup')
    del keep
    return score, next_ctx


def ctc_score_workspace_bytes(num_steps, batch, classes, hyps, max_label_len):
    return load().ctcasr_ctc_score_workspace_bytes(num_steps, batch, classes, int(hyps),
                                                   int(max_label_len))


@_on_tensor_device
def ctc_score(logits, seq_len, labels, label_offsets, utt, max_label_len=None, blank=None,
              score=None, status=None, workspace=None):
    """Exact CTC log-likelihood of H label sequences.  logits f32[T, B, C]; seq_len i32[B];
    labels / label_offsets (i32[H + 1]) as `ctc_loss_fwd_bwd` takes them; utt i32[H] names the
    utterance of each hypothesis.  Returns (score f32[H], status i32[H]).  ``max_label_len``
    defaults to the longest row.  A non-zero status is data, not an error: the caller reads it."""
    num_steps, batch, classes = _decode_shape('ctc_score', logits, seq_len)
    hyps = utt.numel()
    if label_offsets.numel() != hyps + 1:
        raise CtcAsrError('ctc_score: label_offsets holds {} entries for {} hypotheses.'
                          .format(label_offsets.numel(), hyps))
    _dev(label_offsets, torch.int32, 'label_offsets')
    # the ABI takes bare pointers: keep every row the kernel may read inside `labels`
    off64 = label_offsets.long()
    low, high, longest = torch.stack([off64.min(), off64.max(),
                                      (off64[1:] - off64[:-1]).max() if hyps else
                                      off64.new_zeros(())]).tolist()
    if low < 0 or high > labels.numel():
        raise CtcAsrError('ctc_score: a row lies outside `labels`.')
    max_label_len = max(longest, 0) if max_label_len is None else int(max_label_len)
    blank = classes - 1 if blank is None else blank
    dev = logits.device
    score = torch.empty(hyps, dtype=torch.float32, device=dev) if score is None else score
    status = torch.empty(hyps, dtype=torch.int32, device=dev) if status is None else status
    _expect_numel('ctc_score', 'score', score, hyps)
    _expect_numel('ctc_score', 'status', status, hyps)
    if workspace is None:
        workspace = _workspace(ctc_score_workspace_bytes(num_steps, batch, classes, hyps,
                                                         max_label_len), dev)
    # an empty `labels` has no address to give: the kernel reads none of it then
    labels_ptr = _dev(labels, torch.int32, 'labels') if labels.numel() else \
        _dev(label_offsets, torch.int32, 'label_offsets')
    _check(load().ctcasr_ctc_score(
        _dev(logits, name='logits'), _dev(seq_len, torch.int32, 'seq_len'), num_steps, batch,
        classes, blank, labels_ptr, _dev(label_offsets, torch.int32, 'label_offsets'),
        _dev(utt, torch.int32, 'utt'), hyps, max_label_len, _dev(score, name='score'),
        _dev(status, torch.int32, 'status'), _dev(workspace, torch.uint8, 'workspace'),
        workspace.numel(), _stream()), 'ctc_score')
    return score, status


def ctc_mwer_workspace_bytes(num_steps, batch, classes, nbest, max_label_len):
    return load().ctcasr_ctc_mwer_workspace_bytes(num_steps, batch, classes, int(nbest),
                                                  int(max_label_len))


@_on_tensor_device
def ctc_mwer(logits, seq_len, labels, label_offsets, n_hyps, risk, max_label_len=None, blank=None,
             scale=1.0, accumulate=False, grad=None, workspace=None):
    """Gradient of the expected risk over n-best lists (``ctcasr_ctc_mwer``).  logits f32[T, B, C];
    seq_len i32[B]; labels / label_offsets (i32[B * N + 1]) in `ctc_score`'s packed form, row
    ``b * N + i`` being hypothesis i of utterance b; n_hyps i32[B]; risk f32[B * N] (N is read off
    it).  ``accumulate``: the gradient is added to what ``grad`` holds.  Returns (grad f32[T, B,
    C], expected_risk f32[B], score f32[B * N], posterior f32[B * N], status i32[B * N]).
    ``max_label_len`` defaults to the longest row.  A non-zero status is data, not an error."""
    num_steps, batch, classes = _decode_shape('ctc_mwer', logits, seq_len)
    if n_hyps.numel() != batch:
        raise CtcAsrError('ctc_mwer: n_hyps holds {} entries for a batch of {}.'
                          .format(n_hyps.numel(), batch))
    rows = risk.numel()
    if batch < 1 or rows < batch or rows % batch:
        raise CtcAsrError('ctc_mwer: risk holds {} entries for a batch of {}.'
                          .format(rows, batch))
    nbest = rows // batch
    if label_offsets.numel() != rows + 1:
        raise CtcAsrError('ctc_mwer: label_offsets holds {} entries for {} hypotheses.'
                          .format(label_offsets.numel(), rows))
    _dev(label_offsets, torch.int32, 'label_offsets')
    # the ABI takes bare pointers: keep every row the kernel may read inside `labels`
    off64 = label_offsets.long()
    low, high, longest = torch.stack([off64.min(), off64.max(),
                                      (off64[1:] - off64[:-1]).max()]).tolist()
    if low < 0 or high > labels.numel():
        raise CtcAsrError('ctc_mwer: a row lies outside `labels`.')
    max_label_len = max(longest, 0) if max_label_len is None else int(max_label_len)
    blank = classes - 1 if blank is None else blank
    dev = logits.device
    if accumulate and grad is None:
        raise CtcAsrError('ctc_mwer: accumulate needs the gradient to add to.')
    grad = torch.empty_like(logits) if grad is None else grad
    _expect_numel('ctc_mwer', 'grad', grad, logits.numel())
    need = ctc_mwer_workspace_bytes(num_steps, batch, classes, nbest, max_label_len)
    if workspace is None:
        workspace = _workspace(need, dev)
    elif workspace.numel() < need:
        raise CtcAsrError('ctc_mwer: the workspace holds {} bytes, {} needed.'
                          .format(workspace.numel(), need))
    expected_risk = torch.empty(batch, dtype=torch.float32, device=dev)
    score = torch.empty(rows, dtype=torch.float32, device=dev)
    posterior = torch.empty(rows, dtype=torch.float32, device=dev)
    status = torch.empty(rows, dtype=torch.int32, device=dev)
    # an empty `labels` has no address to give: the kernel reads none of it then
    labels_ptr = _dev(labels, torch.int32, 'labels') if labels.numel() else \
        _dev(label_offsets, torch.int32, 'label_offsets')
    _check(load().ctcasr_ctc_mwer(
        _dev(logits, name='logits'), _dev(seq_len, torch.int32, 'seq_len'), num_steps, batch,
        classes, blank, labels_ptr, _dev(label_offsets, torch.int32, 'label_offsets'),
        _dev(n_hyps, torch.int32, 'n_hyps'), _dev(risk, name='risk'), nbest, max_label_len,
        float(scale), int(bool(accumulate)), _dev(grad, name='grad'),
        _dev(expected_risk, name='expected_risk'), _dev(score, name='score'),
        _dev(posterior, name='posterior'), _dev(status, torch.int32, 'status'),
        _dev(workspace, torch.uint8, 'workspace'), workspace.numel(), _stream()), 'ctc_mwer')
    return grad, expected_risk, score, posterior, status


def ctc_align_workspace_bytes(num_steps, batch, classes, max_label_len):
    return load().ctcasr_ctc_align_workspace_bytes(num_steps, batch, classes, max_label_len)


@_on_tensor_device
def ctc_align(logits, labels, label_offsets, seq_len, max_label_len, blank=None, path=None,
              score=None, frame_logp=None, status=None, workspace=None):
    """CTC forced alignment (Viterbi).  logits f32[T,B,C]; labels/label_offsets/seq_len int32
    device tensors, as `ctc_loss_fwd_bwd` takes them.  Returns (path i32[B,T], score f32[B],
    frame_logp f32[B,T], status i32[B]); ``frame_logp=False`` skips that output (returns None).
    A non-zero status is data, not an error: the caller reads it."""
    num_steps, batch, classes = logits.shape
    blank = classes - 1 if blank is None else blank
    dev = logits.device
    if path is None:
        path = torch.empty((batch, num_steps), dtype=torch.int32, device=dev)
    score = torch.empty(batch, dtype=torch.float32, device=dev) if score is None else score
    if frame_logp is None:
        frame_logp = torch.empty((batch, num_steps), dtype=torch.float32, device=dev)
    elif frame_logp is False:
        frame_logp = None
    status = torch.empty(batch, dtype=torch.int32, device=dev) if status is None else status
    if workspace is None:
        workspace = _workspace(ctc_align_workspace_bytes(num_steps, batch, classes,
                                                         max_label_len), dev)
    _check(load().ctcasr_ctc_align(
        _dev(logits, name='logits'), _dev(labels, torch.int32, 'labels'),
        _dev(label_offsets, torch.int32, 'label_offsets'), _dev(seq_len, torch.int32, 'seq_len'),
        num_steps, batch, classes, blank, int(max_label_len), _dev(path, torch.int32, 'path'),
        _dev(score, name='score'), _dev(frame_logp, name='frame_logp'),
        _dev(status, torch.int32, 'status'), _dev(workspace, torch.uint8, 'workspace'),
        workspace.numel(), _stream()), 'ctc_align')
    return path, score, frame_logp, status


def ctc_align_long_workspace_bytes(num_steps, classes, num_labels, tile_frames=0):
    """Bytes `ctc_align_long` needs; 0 for a shape it does not serve."""
    return load().ctcasr_ctc_align_long_workspace_bytes(int(num_steps), int(classes),
                                                        int(num_labels), int(tile_frames))


def _ctc_align_tiled(name, logits, labels, blank, tile_frames, frame_logp, logp, workspace,
                     max_workspace_bytes):
    """`ctc_align_long` and `ctc_align_partial`: one signature, one workspace, two entry points."""
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits.reshape(logits.shape[0], logits.shape[2])
    if logits.dim() != 2:
        raise CtcAsrError('{}: logits must be [T, C] or [T, 1, C] (got shape {}).'
                          .format(name, tuple(logits.shape)))
    num_steps, classes = logits.shape
    num_labels = int(labels.numel())
    blank = classes - 1 if blank is None else int(blank)
    dev = logits.device
    if num_steps > ALIGN_LONG_MAX[0] or num_labels > ALIGN_LONG_MAX[1] or \
            classes > ALIGN_LONG_MAX[2]:
        raise CtcAsrError('{}: T = {}, L = {}, C = {} is outside what the kernel '
                          'serves (T <= {}, L <= {}, C <= {}).'
                          .format(name, num_steps, num_labels, classes, *ALIGN_LONG_MAX))
    need = ctc_align_long_workspace_bytes(num_steps, classes, num_labels, tile_frames)
    if need > int(max_workspace_bytes):
        raise ValueError('{}: T = {} frames x L = {} labels needs a workspace of {} '
                         'bytes, above max_workspace_bytes = {}.'
                         .format(name, num_steps, num_labels, need, int(max_workspace_bytes)))
    if workspace is None:
        workspace = _workspace(need, dev)
    path = torch.empty(num_steps, dtype=torch.int32, device=dev)
    score = torch.empty(1, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    frame_logp = torch.empty(num_steps, dtype=torch.float32, device=dev) if frame_logp else None
    logp = torch.empty((num_steps, classes), dtype=torch.float32, device=dev) if logp else None
    _check(getattr(load(), 'ctcasr_' + name)(
        _dev(logits, name='logits'), _dev(labels, torch.int32, 'labels'), num_steps, classes,
        blank, num_labels, int(tile_frames), _dev(path, torch.int32, 'path'),
        _dev(score, torch.float64, 'score'), _dev(frame_logp, name='frame_logp'),
        _dev(logp, name='logp'), _dev(status, torch.int32, 'status'),
        _dev(workspace, torch.uint8, 'workspace'), workspace.numel(), _stream()), name)
    return path, score, frame_logp, logp, status


@_on_tensor_device
def ctc_align_long(logits, labels, blank=None, tile_frames=0, frame_logp=True, logp=False,
                   workspace=None, max_workspace_bytes=64 << 30):
    """CTC forced alignment (Viterbi) of ONE sequence of any length: the lattice is tiled in the
    workspace (``ctcasr_ctc_align_long``), K11's arithmetic operation for operation.  logits
    f32[T, C] or time-major f32[T, 1, C]; labels int32[L] on the device.  Returns (path i32[T],
    score f64[1], frame_logp f32[T] or None, logp f32[T, C] or None, status i32[1]): ``logp`` is
    the log-softmax table the lattice ran on.  A non-zero status is data, not an error.  The
    workspace grows with T x L (2 bits per cell): a need above ``max_workspace_bytes`` raises
    ValueError before anything is allocated."""
    return _ctc_align_tiled('ctc_align_long', logits, labels, blank, tile_frames, frame_logp,
                            logp, workspace, max_workspace_bytes)


@_on_tensor_device
def ctc_align_partial(logits, labels, blank=None, tile_frames=0, frame_logp=True, logp=False,
                      workspace=None, max_workspace_bytes=64 << 30):
    """`ctc_align_long` for a text that covers only part of the recording
    (``ctcasr_ctc_align_partial``): a label may be `ALIGN_WILDCARD`, one more class that matches
    whatever is said for one frame or more, at the log-probability of the frame's best class.
    Arguments, workspace (`ctc_align_long_workspace_bytes`), errors and the returned tuple are
    `ctc_align_long`'s; on a wildcard frame ``path`` holds the wildcard's odd state and
    ``frame_logp`` the row maximum of ``logp``.  Status 2 also for two wildcards side by side.
    Without a wildcard every output equals `ctc_align_long`'s, bit for bit."""
    return _ctc_align_tiled('ctc_align_partial', logits, labels, blank, tile_frames, frame_logp,
                            logp, workspace, max_workspace_bytes)


def ctc_search_workspace_bytes(num_steps, batch, classes):
    return load().ctcasr_ctc_search_workspace_bytes(int(num_steps), int(batch), int(classes))


@_on_tensor_device
def ctc_search(logits, seq_len, labels, label_offsets, pair_utt, pair_phrase, min_score,
               max_hits=16, max_label_len=None, blank=None, per_frame=False, workspace=None):
    """CTC phrase spotting (``ctcasr_ctc_search``): pair h scores phrase pair_phrase[h] against
    utterance pair_utt[h] on a Viterbi lattice with a free start and a free end.  logits
    f32[T, B, C]; seq_len i32[B]; labels / label_offsets (i32[P + 1]) hold the P phrases, each
    once; min_score f64[P]; pair_utt / pair_phrase i32[H].  Returns (hits i32[H, max_hits, 2],
    hit_score f64[H, max_hits], n_hits i32[H], best_score f64[H], best_span i32[H, 2], end_score
    f64[H, T] or None, end_start i32[H, T] or None, status i32[H]); the per-frame outputs only
    with ``per_frame``.  ``max_label_len`` defaults to the longest phrase.  A non-zero status is
    data, not an error: the caller reads it."""
    num_steps, batch, classes = _decode_shape('ctc_search', logits, seq_len)
    pairs = pair_utt.numel()
    phrases = label_offsets.numel() - 1
    if phrases < 0:
        raise CtcAsrError('ctc_search: label_offsets holds no entry (P + 1 expected).')
    _expect_numel('ctc_search', 'pair_phrase', pair_phrase, pairs)
    _expect_numel('ctc_search', 'min_score', min_score, phrases)
    _dev(label_offsets, torch.int32, 'label_offsets')
    # the ABI takes bare pointers: keep every row the kernel may read inside `labels`
    off64 = label_offsets.long()
    low, high, longest = torch.stack([off64.min(), off64.max(),
                                      (off64[1:] - off64[:-1]).max() if phrases else
                                      off64.new_zeros(())]).tolist()
    if low < 0 or high > labels.numel():
        raise CtcAsrError('ctc_search: a row lies outside `labels`.')
    max_label_len = max(longest, 0) if max_label_len is None else int(max_label_len)
    max_hits = int(max_hits)
    blank = classes - 1 if blank is None else int(blank)
    dev = logits.device
    hits = torch.empty((pairs, max(max_hits, 0), 2), dtype=torch.int32, device=dev)
    hit_score = torch.empty((pairs, max(max_hits, 0)), dtype=torch.float64, device=dev)
    n_hits = torch.empty(pairs, dtype=torch.int32, device=dev)
    best_score = torch.empty(pairs, dtype=torch.float64, device=dev)
    best_span = torch.empty((pairs, 2), dtype=torch.int32, device=dev)
    status = torch.empty(pairs, dtype=torch.int32, device=dev)
    end_score = end_start = None
    if per_frame:
        end_score = torch.empty((pairs, num_steps), dtype=torch.float64, device=dev)
        end_start = torch.empty((pairs, num_steps), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = _workspace(ctc_search_workspace_bytes(num_steps, batch, classes), dev)

    def ptr(tensor, dtype, name):
        # an empty tensor has no address to give: the kernel reads none of it then
        return _dev(tensor, dtype, name) if tensor.numel() else None

    # (an empty `labels`, and `min_score` without a phrase, still need an address: every phrase
    # is empty or out of range then, and neither is read)
    labels_ptr = _dev(labels, torch.int32, 'labels') if labels.numel() else \
        _dev(label_offsets, torch.int32, 'label_offsets')
    _check(load().ctcasr_ctc_search(
        ptr(logits, torch.float32, 'logits'), _dev(seq_len, torch.int32, 'seq_len'), num_steps,
        batch, classes, blank, labels_ptr, _dev(label_offsets, torch.int32, 'label_offsets'),
        phrases, max_label_len,
        _dev(min_score, torch.float64, 'min_score') if phrases else
        _dev(label_offsets, torch.int32, 'label_offsets'),
        _dev(pair_utt, torch.int32, 'pair_utt'), _dev(pair_phrase, torch.int32, 'pair_phrase'),
        pairs, max_hits, ptr(hits, torch.int32, 'hits'),
        ptr(hit_score, torch.float64, 'hit_score'), _dev(n_hits, torch.int32, 'n_hits'),
        _dev(best_score, torch.float64, 'best_score'), _dev(best_span, torch.int32, 'best_span'),
        None if end_score is None else ptr(end_score, torch.float64, 'end_score'),
        None if end_start is None else ptr(end_start, torch.int32, 'end_start'),
        _dev(status, torch.int32, 'status'), _dev(workspace, torch.uint8, 'workspace'),
        workspace.numel(), _stream()), 'ctc_search')
    return hits, hit_score, n_hits, best_score, best_span, end_score, end_start, status


def edit_distance_workspace_bytes(batch, max_hyp_len, max_ref_len):
    return load().ctcasr_edit_distance_workspace_bytes(int(batch), int(max_hyp_len),
                                                       int(max_ref_len))


@_on_tensor_device
def edit_distance(hyp, hyp_offsets, hyp_len, ref, ref_offsets, ref_len, max_hyp_len=None,
                  max_ref_len=None, out=None):
    """Batched edit distance with error counts.  Pair b compares ``hyp[hyp_offsets[b] .. +
    hyp_len[b])`` with ``ref[ref_offsets[b] .. + ref_len[b])``; all six are int32 device tensors
    (``hyp`` / ``ref`` of any shape, read flat).  Returns (distance, substitutions, deletions,
    insertions, status), int32[B] each - the rows of ``out`` (int32 [5, B]) when that is given.
    ``max_*_len`` default to the largest length of their side.  A non-zero status is data, not
    an error: the caller reads it.  Refuses rows that leave their buffer."""
    batch = hyp_len.numel()
    for name, vector in (('hyp_offsets', hyp_offsets), ('ref_offsets', ref_offsets),
                         ('ref_len', ref_len)):
        if vector.numel() != batch:
            raise CtcAsrError('edit_distance: {} holds {} entries for a batch of {}.'
                              .format(name, vector.numel(), batch))
    if batch < 1:
        raise CtcAsrError('edit_distance: the batch is empty.')
    args = [_dev(hyp, torch.int32, 'hyp'), _dev(hyp_offsets, torch.int32, 'hyp_offsets'),
            _dev(hyp_len, torch.int32, 'hyp_len'), _dev(ref, torch.int32, 'ref'),
            _dev(ref_offsets, torch.int32, 'ref_offsets'), _dev(ref_len, torch.int32, 'ref_len')]
    # the ABI takes bare pointers: keep every row the kernel may read inside its buffer
    hyp_len64, ref_len64 = hyp_len.long().clamp(min=0), ref_len.long().clamp(min=0)
    hyp_off64, ref_off64 = hyp_offsets.long(), ref_offsets.long()
    hyp_low, hyp_high, hyp_max, ref_low, ref_high, ref_max = torch.stack([
        hyp_off64.min(), (hyp_off64 + hyp_len64).max(), hyp_len64.max(),
        ref_off64.min(), (ref_off64 + ref_len64).max(), ref_len64.max()]).tolist()
    if hyp_low < 0 or hyp_high > hyp.numel() or ref_low < 0 or ref_high > ref.numel():
        raise CtcAsrError('edit_distance: a row lies outside its buffer.')
    max_hyp_len = hyp_max if max_hyp_len is None else int(max_hyp_len)
    max_ref_len = ref_max if max_ref_len is None else int(max_ref_len)
    dev = hyp_len.device
    if out is None:
        out = torch.empty((5, batch), dtype=torch.int32, device=dev)
    elif tuple(out.shape) != (5, batch):
        raise CtcAsrError('edit_distance: out must be int32 [5, {}].'.format(batch))
    _dev(out, torch.int32, 'out')
    workspace = _workspace(edit_distance_workspace_bytes(batch, max_hyp_len, max_ref_len), dev)
    _check(load().ctcasr_edit_distance(
        *args, batch, max_hyp_len, max_ref_len, *[out[k].data_ptr() for k in range(5)],
        _dev(workspace, torch.uint8, 'workspace'), workspace.numel(), _stream()),
        'edit_distance')
    return out[0], out[1], out[2], out[3], out[4]


def rnn_reserve_bytes(cell, num_steps, batch, hidden):
    return load().ctcasr_rnn_reserve_bytes(CELL_IDS[cell], num_steps, batch, hidden)


def rnn_workspace_bytes(cell, num_steps, batch, hidden):
    return load().ctcasr_rnn_workspace_bytes(CELL_IDS[cell], num_steps, batch, hidden)


def rnn_kernel_events():
    """{'fwd': (launches, total_ms), 'bwd': ...} of the persistent recurrence kernels recorded
    since the last call (needs ``set_option('rnn_kernel_events', 1)``)."""
    launches = (ctypes.c_int * 2)()
    total_ms = (ctypes.c_double * 2)()
    _check(load().ctcasr_rnn_kernel_events(launches, total_ms), 'rnn_kernel_events')
    return {'fwd': (launches[0], total_ms[0]), 'bwd': (launches[1], total_ms[1])}


def rnn_persistent_supported(cell, num_steps, batch, hidden):
    return bool(load().ctcasr_rnn_persistent_supported(CELL_IDS[cell], num_steps, batch, hidden))


@_on_tensor_device
def rnn_poll_error(cell, workspace, num_steps, batch, hidden):
    """Synchronise and raise if any persistent recurrence launch on ``workspace`` since the last
    poll timed out at a grid barrier (sticky word; cleared by this call)."""
    _check(load().ctcasr_rnn_poll_error(_dev(workspace, torch.uint8, 'workspace'),
                                        workspace.numel(), CELL_IDS[cell], num_steps, batch,
                                        hidden, _stream()), 'rnn persistent kernel')


@_on_tensor_device
def rnn_resident_gate(cell, workspace, num_steps, batch, hidden, ticket, max_wait_us=200):
    """Make the CURRENT stream wait (bounded) until the persistent launch carrying ``ticket``
    (``rnn_fwd`` / ``rnn_bwd(..., ticket=...)``) on ``workspace`` has all its workgroups running:
    work enqueued behind the gate cannot take the CUs that launch needs."""
    _check(load().ctcasr_rnn_resident_gate(_dev(workspace, torch.uint8, 'workspace'),
                                           workspace.numel(), CELL_IDS[cell], num_steps, batch,
                                           hidden, int(ticket), int(max_wait_us), _stream()),
           'rnn_resident_gate')


def rnn_gru_drec(reserve, num_steps, batch, hidden):
    """View of drec f32[T, B, 2, 3H] inside a GRU reserve (valid after `rnn_bwd`)."""
    start = load().ctcasr_rnn_gru_drec_offset(num_steps, batch, hidden)
    count = num_steps * batch * 2 * 3 * hidden
    return reserve[start:start + 4 * count].view(torch.float32).view(num_steps, batch, 2,
                                                                      3 * hidden)


@_on_tensor_device
def rnn_workspace(cell, num_steps, batch, hidden, device):
    """A zero-filled workspace for `rnn_fwd` / `rnn_bwd` (the sticky time-out word of the
    persistent kernels must start at zero; launches never clear it, `rnn_poll_error` does)."""
    return torch.zeros(max(int(rnn_workspace_bytes(cell, num_steps, batch, hidden)), 256),
                       dtype=torch.uint8, device=device)


@_on_tensor_device
def rnn_fwd(cell, xw, w_hh, seq_len=None, b_hh_n=None, y=None, reserve=None, workspace=None,
            steps=None, flags=RNN_DEFAULT, xw_bias=None, ticket=0, y16=None):
    """xw f32[T,B,2,G*H], w_hh f32[2,G*H,H] -> (y f32[T,B,2H], reserve, workspace).

    ``steps=(begin, end)`` runs that range of recurrence steps only (`ctcasr_rnn_fwd_steps`): cut
    a pass into calls covering 0..T in ascending order, passing the same ``y``, ``reserve`` and
    ``workspace`` to each.  ``flags``: RNN_DEFAULT / RNN_HALF_CHIP / RNN_WHOLE_CHIP (which
    variant of the persistent kernel runs - a per-call choice, no process-wide state).
    ``xw_bias`` f32[2*G*H] (optional) is added to xw inside the kernel.  ``ticket`` (1..2^24-1):
    the persistent launch posts it once all its workgroups run (`rnn_resident_gate`)."""
    num_steps, batch = xw.shape[0], xw.shape[1]
    hidden = w_hh.shape[2]
    dev = xw.device
    begin, end = (0, num_steps) if steps is None else steps
    if (begin, end) != (0, num_steps) and (y is None or reserve is None or workspace is None):
        raise ValueError('rnn_fwd: a partial step range needs the caller\'s y, reserve and '
                         'workspace (they carry the pass from one call to the next).')
    y = torch.empty((num_steps, batch, 2 * hidden), dtype=torch.float32, device=dev) \
        if y is None else y
    if reserve is None:
        reserve = _workspace(rnn_reserve_bytes(cell, num_steps, batch, hidden), dev)
    if workspace is None:
        workspace = rnn_workspace(cell, num_steps, batch, hidden, dev)
    with _Timed('rnn_fwd'):
      _check(load().ctcasr_rnn_fwd_steps(
        CELL_IDS[cell], _dev(xw, name='xw'), _dev(xw_bias, name='xw_bias'),
        _dev(w_hh, name='w_hh'), _dev(b_hh_n, name='b_hh_n'),
        _dev(seq_len, torch.int32, 'seq_len'), num_steps, batch, hidden, _dev(y, name='y'),
        _dev(y16, torch.float16, 'y16'),
        _dev(reserve, torch.uint8, 'reserve'), _dev(workspace, torch.uint8, 'workspace'),
        workspace.numel(), int(begin), int(end), int(flags) | (int(ticket) & 0xFFFFFF) << 8,
        _stream()), 'rnn_fwd')
    return y, reserve, workspace


@_on_tensor_device
def rnn_bwd(cell, dy, y, w_hh_t, reserve, seq_len=None, b_hh_n=None, dxw=None, dbias=None,
            workspace=None, steps=None, flags=RNN_DEFAULT, ticket=0, colmax=None):
    """dy,y f32[T,B,2H], w_hh_t f32[2,H,G*H] -> dxw f32[T,B,2,G*H].

    ``colmax`` (optional; only where `rnn_bwd_f16_supported`): int32[2*G*H] zeroed by the caller,
    raised to the bit patterns of the largest |dxw| per column over the steps of the call - a
    NaN is skipped (fmaxf), an inf kept: ``nan_to_num(|dxw|, nan=0).amax`` over rows and steps, what
    `colmax_scale`'s own pass over dxw finds.

    ``steps=(begin, end)`` runs that range of recurrence steps only (`ctcasr_rnn_bwd_steps`): cut
    a pass into calls covering T..0 in descending order, passing the same ``dxw`` and
    ``workspace`` to each.  ``dbias`` (optional, zeroed by the caller before the pass): the bias
    gradients are accumulated into it - f32[2*G*H] column sums of dxw, then for the GRU f32[2*3H]
    column sums of drec - complete after the call that covers step 0."""
    num_steps, batch = dy.shape[0], dy.shape[1]
    hidden = w_hh_t.shape[1]
    gates = CELL_GATES[cell]
    dev = dy.device
    begin, end = (0, num_steps) if steps is None else steps
    if (begin, end) != (0, num_steps) and (dxw is None or workspace is None):
        raise ValueError('rnn_bwd: a partial step range needs the caller\'s dxw and workspace '
                         '(they carry the pass from one call to the next).')
    dxw = torch.empty((num_steps, batch, 2, gates * hidden), dtype=torch.float32, device=dev) \
        if dxw is None else dxw
    if workspace is None:
        workspace = rnn_workspace(cell, num_steps, batch, hidden, dev)
    with _Timed('rnn_bwd'):
      _check(load().ctcasr_rnn_bwd_steps(
        CELL_IDS[cell], _dev(dy, name='dy'), _dev(y, name='y'), _dev(w_hh_t, name='w_hh_t'),
        _dev(b_hh_n, name='b_hh_n'), _dev(seq_len, torch.int32, 'seq_len'), num_steps, batch,
        hidden, _dev(reserve, torch.uint8, 'reserve'), _dev(dxw, name='dxw'),
        _dev(dbias, name='dbias'), _dev(colmax, torch.int32, 'colmax'),
        _dev(workspace, torch.uint8, 'workspace'),
        workspace.numel(), int(begin), int(end), int(flags) | (int(ticket) & 0xFFFFFF) << 8,
        _stream()), 'rnn_bwd')
    return dxw


def rnn_fwd_f16_supported(cell, num_steps, batch, hidden, flags=RNN_F16):
    """Whether `rnn_fwd` with these flags runs the fp16-pipe kernel (and can write ``y16``: fp16
    [T*B, 3, 2H], the pieces of y * 2^15 in the layout of `split_f16(order (0, 0, 1))`)."""
    return bool(load().ctcasr_rnn_fwd_f16_supported(CELL_IDS[cell], int(num_steps), int(batch),
                                                    int(hidden), int(flags)))


def rnn_f16_recurrence(cell, num_steps, batch, hidden, flags=RNN_F16, backward=False,
                       ragged=False):
    """Whether a recurrence call with these flags runs an fp16-pipe kernel (include/ctcasr.h)."""
    return bool(load().ctcasr_rnn_f16_recurrence(CELL_IDS[cell], int(num_steps), int(batch),
                                                 int(hidden), int(flags), int(backward),
                                                 int(ragged)))


def rnn_bwd_f16_supported(cell, num_steps, batch, hidden, flags=RNN_F16):
    """Whether `rnn_bwd` with these flags runs the fp16-pipe kernel (and can fill ``colmax``)."""
    return bool(load().ctcasr_rnn_bwd_f16_supported(CELL_IDS[cell], int(num_steps), int(batch),
                                                    int(hidden), int(flags)))


@_on_tensor_device
def bias_act_fwd(y, bias, cutoff, dropout_rate=0.0, seed=0):
    """In place: y = dropout(min(max(y + bias, 0), cutoff)); cutoff <= 0 -> bias add only."""
    cols = _last_dim('bias_act_fwd', 'y', y)
    _expect_numel('bias_act_fwd', 'bias', bias, cols)
    if y.numel() == 0:          # no rows: nothing to do (and an empty tensor has no address)
        return y
    _check(load().ctcasr_bias_act_fwd(_dev(y, name='y'), _dev(bias, name='bias'),
                                      y.numel() // cols, cols, float(cutoff), float(dropout_rate),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), 'bias_act_fwd')
    return y


@_on_tensor_device
def bias_act_bwd(y, dy, cutoff, dropout_rate=0.0, dbias=None, dz=None):
    cols = _last_dim('bias_act_bwd', 'y', y)
    dz = torch.empty_like(dy) if dz is None else dz
    _expect_numel('bias_act_bwd', 'dy', dy, y.numel())
    _expect_numel('bias_act_bwd', 'dz', dz, y.numel())
    _expect_numel('bias_act_bwd', 'dbias', dbias, cols)
    _check(load().ctcasr_bias_act_bwd(_dev(y, name='y'), _dev(dy, name='dy'), _dev(dz, name='dz'),
                                      _dev(dbias, name='dbias'), y.numel() // cols, cols,
                                      float(cutoff), float(dropout_rate), _stream()),
           'bias_act_bwd')
    return dz


@_on_tensor_device
def dropout(src, rate, seed, out=None):
    """out = src * mask(seed) / (1 - rate); same call (same seed) back-propagates a gradient."""
    out = torch.empty_like(src) if out is None else out
    _expect_numel('dropout', 'out', out, src.numel())
    _check(load().ctcasr_dropout(_dev(src, name='src'), _dev(out, name='out'), src.numel(),
                                 float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()),
           'dropout')
    return out


@_on_tensor_device
def colsum_accumulate(dz, dbias):
    cols = _last_dim('colsum_accumulate', 'dz', dz)
    _expect_numel('colsum_accumulate', 'dbias', dbias, cols)
    _check(load().ctcasr_colsum_accumulate(_dev(dz, name='dz'), _dev(dbias, name='dbias'),
                                           dz.numel() // cols, cols, _stream()),
           'colsum_accumulate')
    return dbias


SPLIT_MAX_BLOCKS = 6


@_on_tensor_device
def split_bf16(x, order, out=None):
    """x f32 [rows, cols] (unit column stride, any row stride) -> bf16 ``out[rows, len(order),
    cols]``: block b holds piece ``order[b]`` of the three-piece bfloat16 split x = x1 + x2 + x3
    (include/ctcasr.h: ctcasr_split_bf16).  ``out`` may be any bf16 view of that shape with unit
    column stride (a row / column range of a bigger buffer, blocks stacked along the rows...)."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise CtcAsrError('split_bf16: x must be an f32 matrix in HBM with unit column stride.')
    rows, cols = x.shape
    order = [int(v) for v in order]
    if out is None:
        out = torch.empty((rows, len(order), cols), dtype=torch.bfloat16, device=x.device)
    elif (out.dtype != torch.bfloat16 or tuple(out.shape) != (rows, len(order), cols) or
          out.stride(2) != 1 or out.device != x.device):
        raise CtcAsrError('split_bf16: out must be a bf16 [rows, blocks, cols] view with unit '
                          'column stride on the device of x.')
    arr = (ctypes.c_int * len(order))(*order)
    _check(load().ctcasr_split_bf16(x.data_ptr(), rows, cols, x.stride(0) if rows > 1 else cols,
                                    arr, len(order), out.data_ptr(),
                                    out.stride(0) if rows > 1 else len(order) * cols,
                                    out.stride(1) if len(order) > 1 else cols, _stream()),
           'split_bf16')
    return out


@_on_tensor_device
def split_f16(x, scale, order, out=None):
    """x f32 [rows, cols] -> fp16 ``out[rows, len(order), cols]``: block b holds piece ``order[b]``
    (0 / 1) of the two-piece fp16 split of x * scale (include/ctcasr.h: ctcasr_split_f16).  The
    caller guarantees |x| * scale < 65504."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise CtcAsrError('split_f16: x must be an f32 matrix in HBM with unit column stride.')
    rows, cols = x.shape
    order = [int(v) for v in order]
    if out is None:
        out = torch.empty((rows, len(order), cols), dtype=torch.float16, device=x.device)
    elif (out.dtype != torch.float16 or tuple(out.shape) != (rows, len(order), cols) or
          out.stride(2) != 1 or out.device != x.device):
        raise CtcAsrError('split_f16: out must be an fp16 [rows, blocks, cols] view with unit '
                          'column stride on the device of x.')
    arr = (ctypes.c_int * len(order))(*order)
    _check(load().ctcasr_split_f16(x.data_ptr(), rows, cols, x.stride(0) if rows > 1 else cols,
                                   float(scale), arr, len(order), out.data_ptr(),
                                   out.stride(0) if rows > 1 else len(order) * cols,
                                   out.stride(1) if len(order) > 1 else cols, _stream()),
           'split_f16')
    return out


def _f32_matrix(t, name):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
        raise CtcAsrError('{} must be an f32 matrix in HBM with unit column stride.'.format(name))


def _f16_out(out, rows, blocks, cols, device):
    if out is None:
        return torch.empty((rows, blocks, cols), dtype=torch.float16, device=device)
    if (out.dtype != torch.float16 or tuple(out.shape) != (rows, blocks, cols) or
            out.stride(2) != 1 or out.device != device):
        raise CtcAsrError('out must be an fp16 [rows, blocks, cols] view with unit column stride.')
    return out


@_on_tensor_device
def colscale_from_max(max_bits):
    """(scale, inv_scale) f32[cols] of `colmax_scale` from column maxima already known: int32[cols]
    bit patterns of max |x[:, c]| (what `rnn_bwd(..., colmax=)` accumulates)."""
    cols = max_bits.numel()
    scale = torch.empty(cols, dtype=torch.float32, device=max_bits.device)
    inv_scale = torch.empty(cols, dtype=torch.float32, device=max_bits.device)
    _check(load().ctcasr_colscale_from_max(_dev(max_bits, torch.int32, 'max_bits'), cols,
                                           scale.data_ptr(), inv_scale.data_ptr(), _stream()),
           'colscale_from_max')
    return scale, inv_scale


@_on_tensor_device
def colmax_scale(x, scale=None, inv_scale=None):
    """Power-of-two scale per column of x f32 [rows, cols] (largest magnitude -> [2^13, 2^14)) and
    its inverse: (scale f32[cols], inv_scale f32[cols]) (ctcasr_colmax_scale)."""
    _f32_matrix(x, 'colmax_scale: x')
    rows, cols = x.shape
    scale = torch.empty(cols, dtype=torch.float32, device=x.device) if scale is None else scale
    inv_scale = torch.empty(cols, dtype=torch.float32, device=x.device) \
        if inv_scale is None else inv_scale
    _expect_numel('colmax_scale', 'scale', scale, cols)
    _expect_numel('colmax_scale', 'inv_scale', inv_scale, cols)
    work = torch.empty(cols, dtype=torch.int32, device=x.device)
    # (no rows: every scale is 1; an empty tensor has no address, the library wants one)
    _check(load().ctcasr_colmax_scale(x.data_ptr() if rows else work.data_ptr(), rows, cols,
                                      x.stride(0) if rows > 1 else cols,
                                      work.data_ptr(), _dev(scale, name='scale'),
                                      _dev(inv_scale, name='inv_scale'), _stream()), 'colmax_scale')
    return scale, inv_scale


@_on_tensor_device
def split_f16_cols(x, col_scale, scale, order, out=None):
    """Two fp16 pieces of x[r][c] * col_scale[c] * scale -> fp16 [rows, len(order), cols]."""
    _f32_matrix(x, 'split_f16_cols: x')
    rows, cols = x.shape
    order = [int(v) for v in order]
    out = _f16_out(out, rows, len(order), cols, x.device)
    if col_scale is None:
        raise CtcAsrError('split_f16_cols: col_scale is required (one f32 scale per column).')
    _expect_numel('split_f16_cols', 'col_scale', col_scale, cols)
    arr = (ctypes.c_int * len(order))(*order)
    _check(load().ctcasr_split_f16_cols(
        x.data_ptr(), rows, cols, x.stride(0) if rows > 1 else cols, _dev(col_scale, name='scale'),
        float(scale), arr, len(order), out.data_ptr(),
        out.stride(0) if rows > 1 else len(order) * cols,
        out.stride(1) if len(order) > 1 else cols, _stream()), 'split_f16_cols')
    return out


@_on_tensor_device
def split_f16_rows(x, order, out=None, inv_scale=None):
    """Two fp16 pieces of every row of x scaled by that row's own power of two -> (fp16 [rows,
    len(order), cols], inv_scale f32[rows])."""
    _f32_matrix(x, 'split_f16_rows: x')
    rows, cols = x.shape
    order = [int(v) for v in order]
    out = _f16_out(out, rows, len(order), cols, x.device)
    inv_scale = torch.empty(rows, dtype=torch.float32, device=x.device) \
        if inv_scale is None else inv_scale
    arr = (ctypes.c_int * len(order))(*order)
    _check(load().ctcasr_split_f16_rows(
        x.data_ptr(), rows, cols, x.stride(0) if rows > 1 else cols, arr, len(order),
        out.data_ptr(), out.stride(0) if rows > 1 else len(order) * cols,
        out.stride(1) if len(order) > 1 else cols, _dev(inv_scale, name='inv_scale'), _stream()),
        'split_f16_rows')
    return out, inv_scale


@_on_tensor_device
def rescale_rows(t, row_factor, alpha, out, accumulate=False):
    """out[r][c] (+)= t[r][c] * row_factor[r] * alpha."""
    _f32_matrix(t, 'rescale_rows: t')
    _f32_matrix(out, 'rescale_rows: out')
    rows, cols = t.shape
    if tuple(out.shape) != (rows, cols) or row_factor.numel() != rows:
        raise CtcAsrError('rescale_rows: shapes disagree.')
    _check(load().ctcasr_rescale_rows(
        t.data_ptr(), t.stride(0) if rows > 1 else cols, _dev(row_factor, name='row_factor'),
        float(alpha), out.data_ptr(), out.stride(0) if rows > 1 else cols, rows, cols,
        int(accumulate), _stream()), 'rescale_rows')
    return out


@_on_tensor_device
def gemm_split_nt(a, b, out=None, accumulate=False):
    """out[M, N] (+)= a[M, K] . b[N, K]^T, fp32 matrices with unit column stride (row strides
    free), computed on the bf16 matrix pipe from in-register three-piece splits
    (include/ctcasr.h: ctcasr_gemm_split_nt)."""
    for name, t in (('a', a), ('b', b)):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
            raise CtcAsrError('gemm_split_nt: {} must be an f32 matrix in HBM with unit column '
                              'stride.'.format(name))
    m, k = a.shape
    n = b.shape[0]
    if b.shape[1] != k:
        raise CtcAsrError('gemm_split_nt: a [M, K] and b [N, K] disagree on K.')
    if out is None:
        if accumulate:
            raise CtcAsrError('gemm_split_nt: accumulate needs out.')
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    elif (out.dtype != torch.float32 or tuple(out.shape) != (m, n) or out.stride(1) != 1 or
          out.device != a.device):
        raise CtcAsrError('gemm_split_nt: out must be an f32 [M, N] view with unit column stride.')
    _check(load().ctcasr_gemm_split_nt(a.data_ptr(), a.stride(0) if m > 1 else k, b.data_ptr(),
                                       b.stride(0) if n > 1 else k, out.data_ptr(),
                                       out.stride(0) if m > 1 else n, m, n, k, int(accumulate),
                                       _stream()), 'gemm_split_nt')
    return out


def dgrad16_supported(cell, num_steps, batch, hidden):
    """Whether the block-scaled data-gradient kernel covers a backward pass of this shape (it reads
    what the fp16-pipe LSTM-1024 backward recurrence published; include/ctcasr.h, ABI v6)."""
    return bool(load().ctcasr_dgrad16_supported(CELL_IDS[cell], int(num_steps), int(batch),
                                                int(hidden)))


@_on_tensor_device
def wgrad16_pack(x, rows_total, row0, stages, scale, col_scale=None, out=None):
    """Rows [row0, row0 + 32 * stages) of ``x`` (an f32 matrix view [>= rows_total, cols] with unit
    column stride; rows outside [0, rows_total) read as zeros), every column times col_scale[c]
    times scale, as fp16 pieces transposed into MFMA fragment order (include/ctcasr.h:
    ctcasr_wgrad16_pack) - an operand of `wgrad16_gemm`.  uint8 buffer."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise CtcAsrError('wgrad16_pack: x must be an f32 matrix in HBM with unit column stride.')
    cols = x.shape[1]
    if not 0 < int(rows_total) <= x.shape[0]:
        raise CtcAsrError('wgrad16_pack: rows_total = {} but x holds {} rows.'
                          .format(rows_total, x.shape[0]))
    if col_scale is not None:
        _expect_numel('wgrad16_pack', 'col_scale', col_scale, cols)
        if col_scale.device != x.device:
            raise CtcAsrError('wgrad16_pack: col_scale lives on {}, x on {}.'
                              .format(col_scale.device, x.device))
    need = load().ctcasr_wgrad16_packed_bytes(int(stages), cols)
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or out.numel() < need or not out.is_contiguous() or \
            out.device != x.device:
        raise CtcAsrError('wgrad16_pack: out must be a contiguous uint8 buffer of {} bytes.'
                          .format(need))
    _check(load().ctcasr_wgrad16_pack(
        x.data_ptr(), x.stride(0), int(rows_total), cols, int(row0), int(stages),
        _dev(col_scale, name='col_scale'), float(scale), out.data_ptr(), _stream()),
        'wgrad16_pack')
    return out


@_on_tensor_device
def wgrad16_gemm(d_packed, m, stages, inv_scale, x_packed, x_stage0, x_scale, dw_x,
                 y_packed=None, y_stage0=0, y_scale=1.0, dw_y=None, parts=1):
    """dw_x [m, nx] += D^T X and (optional) dw_y [m, ny] += D^T Y over `stages` stages of 32 rows,
    from operands packed by `wgrad16_pack` (include/ctcasr.h: ctcasr_wgrad16_gemm).  `parts`
    workgroups per tile add in order through the device's zeroed sync words (one buffer per device:
    launches of different streams / models that meet at a tile's word take turns - part 0 takes
    the word by compare-and-swap from 0 to the launch's ticket, part q > 0 adds when it reads
    ticket | q, the last part hands it back as 0; at most 4095 parts)."""
    parts = max(1, min(int(parts), int(stages), 4095))
    if (y_packed is None) != (dw_y is None):
        raise CtcAsrError('wgrad16_gemm: y_packed and dw_y come together.')
    for name, t in (('dw_x', dw_x), ('dw_y', dw_y)):
        if t is not None and (t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or
                              t.stride(1) != 1 or t.shape[0] != m):
            raise CtcAsrError('wgrad16_gemm: {} must be an f32 [m, n] view in HBM with unit '
                              'column stride.'.format(name))
    # the kernel reads whole stages by DMA: every packed operand has to hold what the launch
    # will read of it, the second operands from stage 0 of their buffer on
    for name, t, first, cols in (('d_packed', d_packed, 0, m),
                                 ('x_packed', x_packed, x_stage0, dw_x.shape[1]),
                                 ('y_packed', y_packed, y_stage0,
                                  0 if dw_y is None else dw_y.shape[1])):
        if t is None:
            continue
        if int(first) < 0:
            raise CtcAsrError('wgrad16_gemm: the first stage of {} is negative.'.format(name))
        need = load().ctcasr_wgrad16_packed_bytes(int(first) + int(stages), cols)
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < need:
            raise CtcAsrError('wgrad16_gemm: {} must be a contiguous uint8 buffer of at least {} '
                              'bytes (got {}).'.format(name, need, t.numel()))
    if inv_scale is None or inv_scale.numel() < m:
        raise CtcAsrError('wgrad16_gemm: inv_scale holds fewer than m = {} scales.'.format(m))
    for name, t in (('d_packed', d_packed), ('x_packed', x_packed), ('inv_scale', inv_scale),
                    ('y_packed', y_packed), ('dw_y', dw_y)):
        if t is not None and t.device != dw_x.device:
            raise CtcAsrError('wgrad16_gemm: {} lives on {}, dw_x on {}.'
                              .format(name, t.device, dw_x.device))
    sync = None
    if parts > 1:
        need = load().ctcasr_wgrad16_sync_ints(int(m), dw_x.shape[1], 0 if dw_y is None else dw_y.shape[1])
        sync = _WGRAD16_SYNC.get(dw_x.device.index)
        if sync is None or sync.numel() < need:
            sync = _WGRAD16_SYNC[dw_x.device.index] = torch.zeros(max(need, 4096), dtype=torch.int32,
                                                            device=dw_x.device)
    _check(load().ctcasr_wgrad16_gemm(
        d_packed.data_ptr(), int(m), int(stages), _dev(inv_scale, name='inv_scale'),
        x_packed.data_ptr(), int(x_stage0), dw_x.shape[1], float(x_scale), dw_x.data_ptr(),
        dw_x.stride(0), None if y_packed is None else y_packed.data_ptr(), int(y_stage0),
        0 if dw_y is None else dw_y.shape[1], float(y_scale),
        None if dw_y is None else dw_y.data_ptr(), 0 if dw_y is None else dw_y.stride(0),
        parts, None if sync is None else sync.data_ptr(), _stream()), 'wgrad16_gemm')


_WGRAD16_SYNC = {}


def _wgrad16_sync_of(device):
    device = torch.device(device)
    return _WGRAD16_SYNC.get(torch.cuda.current_device() if device.index is None else device.index)


def wgrad16_sync_words(device):
    """The int32 sync words `wgrad16_gemm` launches on `device` share (word 0: the sticky
    time-out word, then one turn word per tile; all zero between launches), or None while no
    launch with parts > 1 has made them."""
    return _wgrad16_sync_of(device)


def wgrad16_gave_up_waiting(device):
    """True if a part of a `wgrad16_gemm` launch on `device` ever stopped waiting for its turn
    (the sticky word 0 of the sync words; synchronises)."""
    sync = _wgrad16_sync_of(device)
    return bool(sync is not None and int(sync[0].item()) != 0)


def wgrad16_check(device):
    """Raise `CtcAsrError` if a part of a `wgrad16_gemm` launch on `device` gave up waiting for
    its turn since the last check (it, and every part after it, left without adding: the weight
    gradients of that step are incomplete - `step_guard` has dropped its update), and hand the
    words back zeroed.  Synchronises; `CTCModel.check_rnn_error` calls it with the recurrence
    kernels' time-out poll."""
    sync = _wgrad16_sync_of(device)
    if sync is not None and int(sync[0].item()) != 0:
        sync.zero_()
        torch.cuda.synchronize(sync.device)
        raise CtcAsrError('wgrad16_gemm: a part of a weight-gradient tile timed out waiting for '
                          'its turn to add; the step\'s update was not applied ({}).'.format(
                              load().ctcasr_error_string(-5).decode()))



def dgrad16_packed_bytes(n):
    return int(load().ctcasr_dgrad16_packed_bytes(int(n)))


def dgrad16_published_offsets(num_steps, batch, hidden):
    """(exchange, inverse scales) byte offsets inside a recurrence workspace of what the fp16-pipe
    backward recurrence publishes for a pass over (num_steps, batch)."""
    exchange, scales = ctypes.c_size_t(), ctypes.c_size_t()
    _check(load().ctcasr_dgrad16_published_offsets(int(num_steps), int(batch), int(hidden),
                                                   ctypes.byref(exchange), ctypes.byref(scales)),
           'dgrad16_published_offsets')
    return exchange.value, scales.value


@_on_tensor_device
def dgrad16_pack_weights(w_ih, hidden, scale, out=None):
    """fp16 pieces of ``w_ih`` [2 * 4 * hidden, n] * scale in the K order / fragment order the
    block-scaled data-gradient kernel reads (uint8 buffer of ctcasr_dgrad16_packed_bytes(n))."""
    if (w_ih.dim() != 2 or w_ih.dtype != torch.float32 or not w_ih.is_cuda or
            w_ih.stride(1) != 1 or w_ih.shape[0] != 8 * hidden):
        raise CtcAsrError('dgrad16_pack_weights: w_ih must be an f32 [2 * 4H, n] matrix in HBM '
                          'with unit column stride.')
    n = w_ih.shape[1]
    need = load().ctcasr_dgrad16_packed_bytes(n)
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=w_ih.device)
    elif out.dtype != torch.uint8 or out.numel() < need or not out.is_contiguous() or \
            out.device != w_ih.device:
        raise CtcAsrError('dgrad16_pack_weights: out must be a contiguous uint8 buffer of {} bytes.'
                          .format(need))
    _check(load().ctcasr_dgrad16_pack_weights(w_ih.data_ptr(), w_ih.stride(0), int(hidden), n,
                                              float(scale), out.data_ptr(), _stream()),
           'dgrad16_pack_weights')
    return out


@_on_tensor_device
def dgrad16_blockscaled(workspace, num_steps, batch, hidden, packed, scale, n, out=None,
                        steps=None, dirs=(0, 2), accumulate=False):
    """dx [T * B, n] (+)= dxw . W_ih from the fp16 pieces an fp16-pipe backward recurrence pass
    over (num_steps, batch) left in ``workspace`` and the packed pieces of W_ih
    (`dgrad16_pack_weights`); ``steps`` = (t_lo, t_hi) restricts the rows, ``dirs`` the directions
    whose gate columns are summed (include/ctcasr.h: ctcasr_dgrad16_blockscaled)."""
    if not workspace.is_cuda or not packed.is_cuda:
        raise CtcAsrError('dgrad16_blockscaled: workspace and packed weights must live in HBM.')
    rows = num_steps * batch
    if out is None:
        if accumulate:
            raise CtcAsrError('dgrad16_blockscaled: accumulate needs out.')
        out = torch.empty((rows, n), dtype=torch.float32, device=workspace.device)
    elif (out.dtype != torch.float32 or tuple(out.shape) != (rows, n) or out.stride(1) != 1 or
          out.device != workspace.device):
        raise CtcAsrError('dgrad16_blockscaled: out must be an f32 [T * B, n] view with unit '
                          'column stride.')
    t_lo, t_hi = (0, num_steps) if steps is None else steps
    if not 0 <= int(t_lo) < int(t_hi) <= num_steps:
        raise CtcAsrError('dgrad16_blockscaled: steps = ({}, {}) is no range inside [0, {}].'
                          .format(t_lo, t_hi, num_steps))
    if len(dirs) != 2 or not 0 <= int(dirs[0]) < int(dirs[1]) <= 2:
        raise CtcAsrError('dgrad16_blockscaled: dirs = {} is no range inside [0, 2].'
                          .format(tuple(dirs)))
    if packed.device != workspace.device:
        raise CtcAsrError('dgrad16_blockscaled: packed weights and workspace live on different '
                          'devices.')
    need = dgrad16_packed_bytes(n)
    if packed.numel() * packed.element_size() < need or not packed.is_contiguous():
        raise CtcAsrError('dgrad16_blockscaled: packed holds {} bytes, {} expected for n = {}.'
                          .format(packed.numel() * packed.element_size(), need, n))
    # what the recurrence publishes: the zero block and one block per step, then the inverse scales
    x_off, s_off = dgrad16_published_offsets(num_steps, batch, hidden)
    need = max(x_off + (num_steps + 1) * 2 * batch * 4 * hidden * 4,
               s_off + num_steps * 2 * (hidden // 16) * 32 * 4)
    if workspace.numel() * workspace.element_size() < need or not workspace.is_contiguous():
        raise CtcAsrError('dgrad16_blockscaled: workspace holds {} bytes, the published operand '
                          'of ({}, {}) ends at {}.'.format(
                              workspace.numel() * workspace.element_size(), num_steps, batch, need))
    with _Timed('dgrad16'):
        _check(load().ctcasr_dgrad16_blockscaled(
            workspace.data_ptr(), int(num_steps), int(batch), int(hidden), packed.data_ptr(),
            float(scale), int(n), out.data_ptr(), out.stride(0), int(t_lo), int(t_hi),
            int(dirs[0]), int(dirs[1]), int(accumulate), _stream()), 'dgrad16_blockscaled')
    return out


@_on_tensor_device
def gemm_split_tn(a, b, out, accumulate=True):
    """out[M, N] (+)= a[K, M]^T . b[K, N] - a product over the ROW axis of both fp32 operands
    (weight gradients) - on the bf16 matrix pipe from in-register three-piece splits
    (include/ctcasr.h: ctcasr_gemm_split_tn).  Unit column strides, any row strides, any K."""
    for name, t in (('a', a), ('b', b), ('out', out)):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
            raise CtcAsrError('gemm_split_tn: {} must be an f32 matrix in HBM with unit column '
                              'stride.'.format(name))
    k, m = a.shape
    n = b.shape[1]
    if b.shape[0] != k or tuple(out.shape) != (m, n):
        raise CtcAsrError('gemm_split_tn: a [K, M], b [K, N] and out [M, N] disagree.')
    _check(load().ctcasr_gemm_split_tn(a.data_ptr(), a.stride(0) if k > 1 else m, b.data_ptr(),
                                       b.stride(0) if k > 1 else n, out.data_ptr(),
                                       out.stride(0) if m > 1 else n, m, n, k, int(accumulate),
                                       _stream()), 'gemm_split_tn')
    return out


def conv_s12_supported(freq_in, cout):
    """Whether the own 11x21 / stride (1,2) convolution kernels cover this layer shape."""
    return bool(load().ctcasr_conv_s12_supported(int(freq_in), int(cout)))


def conv_s12_packed_floats(cout):
    return 2 * 11 * 21 * 32 * cout


def _conv_dims(what, name, tensor, ndim):
    """The conv wrappers read B, T, F, C off their arguments' shapes: an argument with another
    number of dimensions is refused, not misread."""
    if tensor.dim() != ndim:
        raise CtcAsrError('{}: {} must have {} dimensions (got shape {}).'
                          .format(what, name, ndim, tuple(tensor.shape)))
    return tuple(int(d) for d in tensor.shape)


def _conv_scale(what, x_scale):
    x_scale = float(x_scale)
    if not (x_scale > 0.0 and x_scale != float('inf')):
        raise CtcAsrError('{}: x_scale must be a positive finite number (got {}).'
                          .format(what, x_scale))
    return x_scale


def _conv_mask(what, dz, act, relu_cutoff, dbias, cout):
    """``act`` is read at dz's own indices and ``dbias`` holds one sum per output channel."""
    if act is not None:
        if tuple(act.shape) != tuple(dz.shape):
            raise CtcAsrError('{}: act must be shaped like dz {} (got {}).'
                              .format(what, tuple(dz.shape), tuple(act.shape)))
        if not float(relu_cutoff) > 0.0:
            raise CtcAsrError('{}: act needs relu_cutoff > 0 (got {}).'.format(what, relu_cutoff))
    _expect_numel(what, 'dbias', dbias, cout)


@_on_tensor_device
def conv_s12_pack_weights(weight, packed=None):
    """Fragment-ordered copies (backward, forward) of w f32[cout,32,11,21] ([Cout,Cin,kt,kf])."""
    cout = weight.shape[0] if weight.dim() == 4 else 0
    if tuple(weight.shape[1:]) != (32, 11, 21) or cout not in (32, 96):
        raise CtcAsrError('the conv_s12 kernels cover w [32|96, 32, 11, 21] only.')
    _expect_numel('conv_s12_pack_weights', 'packed', packed, conv_s12_packed_floats(cout))
    packed = torch.empty(conv_s12_packed_floats(cout), dtype=torch.float32,
                         device=weight.device) if packed is None else packed
    _check(load().ctcasr_conv_s12_pack_weights(_dev(weight, name='weight'),
                                               _dev(packed, name='packed'), cout, _stream()),
           'conv_s12_pack_weights')
    return packed


@_on_tensor_device
def conv_s12_fwd(x, packed, cout, bias=None, out=None, relu_cutoff=0.0, time_major=False):
    """x f32[B,T,F,32] (NHWC) -> conv(x) + bias, f32[B,T,F/2,cout]; 11x21 taps, stride (1,2),
    TensorFlow SAME padding.  ``packed`` from `conv_s12_pack_weights`.  ``relu_cutoff`` > 0 fuses
    min(max(., 0), cutoff) into the epilogue; ``time_major`` writes [T,B,F/2,cout] instead."""
    batch, frames, freq, cin = _conv_dims('conv_s12_fwd', 'x', x, 4)
    if cin != 32 or not conv_s12_supported(freq, cout):
        raise CtcAsrError('conv_s12_fwd: unsupported layer shape {} -> {} channels'.format(
            tuple(x.shape), cout))
    _expect_numel('conv_s12_fwd', 'packed', packed, conv_s12_packed_floats(cout))
    _expect_numel('conv_s12_fwd', 'bias', bias, cout)
    _expect_numel('conv_s12_fwd', 'out', out, batch * frames * (freq // 2) * cout)
    shape = (frames, batch, freq // 2, cout) if time_major else (batch, frames, freq // 2, cout)
    out = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else out
    with _Timed('conv_s12_fwd'):
        _check(load().ctcasr_conv_s12_fwd(_dev(x, name='x'), _dev(packed, name='packed'),
                                          _dev(bias, name='bias'), _dev(out, name='y'), batch,
                                          frames, freq, cout, float(relu_cutoff),
                                          1 if time_major else 0, _stream()), 'conv_s12_fwd')
    return out


@_on_tensor_device
def conv_s12_pack_weights16(weight, packed=None):
    """weight f32[cout, 32, 11, 21] -> uint8 buffer for `conv_s12_fwd16`: the bit pattern of
    max |w| (found on the device) and the two fp16 pieces of w * s_w in fragment order."""
    cout = weight.shape[0] if weight.dim() == 4 else 0
    nbytes = load().ctcasr_conv_s12_pack16_bytes(int(cout))
    if nbytes == 0 or tuple(weight.shape[1:]) != (32, 11, 21):
        raise CtcAsrError('conv_s12_pack_weights16: unsupported kernel shape {}'.format(
            tuple(weight.shape)))
    if packed is None or packed.numel() != nbytes:
        packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _check(load().ctcasr_conv_s12_pack_weights16(_dev(weight, name='weight'),
                                                 _dev(packed, torch.uint8, 'packed'), int(cout),
                                                 _stream()), 'conv_s12_pack_weights16')
    return packed


@_on_tensor_device
def conv_s12_fwd16(x, x_scale, packed16, cout, bias=None, out=None, relu_cutoff=0.0,
                   time_major=False):
    """`conv_s12_fwd` with its products on the fp16 matrix pipe (two fp16 pieces per operand,
    three products, fp32 accumulation): for x with a known bound, bound * x_scale < 65504
    (``x_scale`` a power of two).  ``packed16`` from `conv_s12_pack_weights16`."""
    batch, frames, freq, cin = _conv_dims('conv_s12_fwd16', 'x', x, 4)
    if cin != 32 or not conv_s12_supported(freq, cout):
        raise CtcAsrError('conv_s12_fwd16: unsupported layer shape {} -> {} channels'.format(
            tuple(x.shape), cout))
    x_scale = _conv_scale('conv_s12_fwd16', x_scale)
    _expect_numel('conv_s12_fwd16', 'packed16', packed16,
                  load().ctcasr_conv_s12_pack16_bytes(int(cout)))
    _expect_numel('conv_s12_fwd16', 'bias', bias, cout)
    _expect_numel('conv_s12_fwd16', 'out', out, batch * frames * (freq // 2) * cout)
    shape = (frames, batch, freq // 2, cout) if time_major else (batch, frames, freq // 2, cout)
    out = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else out
    with _Timed('conv_s12_fwd'):
        _check(load().ctcasr_conv_s12_fwd16(_dev(x, name='x'), x_scale,
                                            _dev(packed16, torch.uint8, 'packed16'),
                                            _dev(bias, name='bias'), _dev(out, name='y'), batch,
                                            frames, freq, cout, float(relu_cutoff),
                                            1 if time_major else 0, _stream()), 'conv_s12_fwd16')
    return out


def _conv_s12_dz(what, dz, time_major):
    """(batch, frames, freq_out, cout) of a supported layer's dz, whichever way it is laid out."""
    dims = _conv_dims(what, 'dz', dz, 4)
    frames, batch = (dims[0], dims[1]) if time_major else (dims[1], dims[0])
    if not conv_s12_supported(2 * dims[2], dims[3]):
        raise CtcAsrError('{}: unsupported layer shape {}'.format(what, tuple(dz.shape)))
    return batch, frames, dims[2], dims[3]


@_on_tensor_device
def conv_s12_bwd_data(dz, packed, out=None, time_major=False, act=None, relu_cutoff=0.0):
    """dz f32[B,T,F/2,cout] (NHWC; ``time_major``: [T,B,F/2,cout]) -> dx f32[B,T,F,32].
    ``act`` (the layer's stored output, same layout): dz is the gradient w.r.t. that output and
    the mask of min(max(., 0), relu_cutoff) is applied while dz is staged."""
    batch, frames, freq_out, cout = _conv_s12_dz('conv_s12_bwd_data', dz, time_major)
    _conv_mask('conv_s12_bwd_data', dz, act, relu_cutoff, None, cout)
    _expect_numel('conv_s12_bwd_data', 'packed', packed, conv_s12_packed_floats(cout))
    _expect_numel('conv_s12_bwd_data', 'out', out, batch * frames * 2 * freq_out * 32)
    out = torch.empty((batch, frames, 2 * freq_out, 32), dtype=torch.float32, device=dz.device) \
        if out is None else out
    with _Timed('conv_s12_bwd_data'):
        _check(load().ctcasr_conv_s12_bwd_data(_dev(dz, name='dz'), _dev(packed, name='packed'),
                                               _dev(out, name='dx'), batch, frames,
                                               2 * freq_out, cout, 1 if time_major else 0,
                                               _dev(act, name='act'), float(relu_cutoff),
                                               _stream()), 'conv_s12_bwd_data')
    return out


@_on_tensor_device
def conv_s12_bwd_data16(dz, packed16, out=None, time_major=False, act=None, relu_cutoff=0.0):
    """`conv_s12_bwd_data` with its products on the fp16 matrix pipe: every dz cell (frame,
    position) is scaled by its own power of two while it is staged - no bound on dz is assumed.
    ``packed16`` from `conv_s12_pack_weights16`."""
    batch, frames, freq_out, cout = _conv_s12_dz('conv_s12_bwd_data16', dz, time_major)
    _conv_mask('conv_s12_bwd_data16', dz, act, relu_cutoff, None, cout)
    _expect_numel('conv_s12_bwd_data16', 'packed16', packed16,
                  load().ctcasr_conv_s12_pack16_bytes(int(cout)))
    _expect_numel('conv_s12_bwd_data16', 'out', out, batch * frames * 2 * freq_out * 32)
    out = torch.empty((batch, frames, 2 * freq_out, 32), dtype=torch.float32, device=dz.device) \
        if out is None else out
    with _Timed('conv_s12_bwd_data'):
        _check(load().ctcasr_conv_s12_bwd_data16(_dev(dz, name='dz'),
                                                 _dev(packed16, torch.uint8, 'packed16'),
                                                 _dev(out, name='dx'), batch, frames,
                                                 2 * freq_out, cout, 1 if time_major else 0,
                                                 _dev(act, name='act'), float(relu_cutoff),
                                                 _stream()), 'conv_s12_bwd_data16')
    return out


@_on_tensor_device
def conv_s12_wrw(dz, x, out=None, time_major=False, act=None, relu_cutoff=0.0, dbias=None):
    """Kernel gradient of the same layer: dz f32[B,T,F/2,cout] (``time_major``: [T,B,F/2,cout]),
    x f32[B,T,F,32] (NHWC) -> dw f32[cout,32,11,21].  ``act`` / ``relu_cutoff``: see
    `conv_s12_bwd_data`; ``dbias`` f32[cout] (zeroed by the caller) then receives the bias
    gradient, the column sums of the masked dz."""
    batch, frames, freq_out, cout = _conv_s12_dz('conv_s12_wrw', dz, time_major)
    if tuple(x.shape) != (batch, frames, 2 * freq_out, 32):
        raise CtcAsrError('conv_s12_wrw: unsupported layer shape {} / {}'.format(
            tuple(dz.shape), tuple(x.shape)))
    _conv_mask('conv_s12_wrw', dz, act, relu_cutoff, dbias, cout)
    _expect_numel('conv_s12_wrw', 'out', out, cout * 32 * 11 * 21)
    out = torch.empty((cout, 32, 11, 21), dtype=torch.float32, device=x.device) if out is None \
        else out
    workspace = _workspace(load().ctcasr_conv_s12_wrw_workspace_bytes(batch, frames,
                                                                      2 * freq_out, cout),
                           x.device)
    with _Timed('conv_s12_wrw'):
        _check(load().ctcasr_conv_s12_wrw(_dev(dz, name='dz'), _dev(x, name='x'),
                                          _dev(out, name='dw'), batch, frames, 2 * freq_out, cout,
                                          1 if time_major else 0, _dev(act, name='act'),
                                          float(relu_cutoff), _dev(dbias, name='dbias'),
                                          _dev(workspace, torch.uint8, 'workspace'),
                                          workspace.numel(), _stream()), 'conv_s12_wrw')
    return out


@_on_tensor_device
def conv_s12_wrw16(dz, x, x_scale, out=None, time_major=False, act=None, relu_cutoff=0.0,
                   dbias=None):
    """`conv_s12_wrw` with its products on the fp16 matrix pipe: for x with a known bound,
    bound * x_scale < 65504 (``x_scale`` a power of two); dz is scaled per output channel on the
    device."""
    batch, frames, freq_out, cout = _conv_s12_dz('conv_s12_wrw16', dz, time_major)
    if tuple(x.shape) != (batch, frames, 2 * freq_out, 32):
        raise CtcAsrError('conv_s12_wrw16: unsupported layer shape {} / {}'.format(
            tuple(dz.shape), tuple(x.shape)))
    x_scale = _conv_scale('conv_s12_wrw16', x_scale)
    _conv_mask('conv_s12_wrw16', dz, act, relu_cutoff, dbias, cout)
    _expect_numel('conv_s12_wrw16', 'out', out, cout * 32 * 11 * 21)
    out = torch.empty((cout, 32, 11, 21), dtype=torch.float32, device=x.device) if out is None \
        else out
    workspace = _workspace(load().ctcasr_conv_s12_wrw16_workspace_bytes(batch, frames,
                                                                        2 * freq_out, cout),
                           x.device)
    with _Timed('conv_s12_wrw'):
        _check(load().ctcasr_conv_s12_wrw16(_dev(dz, name='dz'), _dev(x, name='x'),
                                            x_scale, _dev(out, name='dw'), batch, frames,
                                            2 * freq_out, cout, 1 if time_major else 0,
                                            _dev(act, name='act'), float(relu_cutoff),
                                            _dev(dbias, name='dbias'),
                                            _dev(workspace, torch.uint8, 'workspace'),
                                            workspace.numel(), _stream()), 'conv_s12_wrw16')
    return out


def _conv0_x(what, x):
    batch, frames, freq = _conv_dims(what, 'x', x, 3)
    if freq != 80:
        raise CtcAsrError('{} covers x [B,T,80] only (got {}).'.format(what, tuple(x.shape)))
    return batch, frames


@_on_tensor_device
def conv0_fwd(x, weight, bias=None, out=None, relu_cutoff=0.0):
    """First DS2 convolution: x f32[B,T,80] -> f32[B,ceil(T/2),40,32] (NHWC); weight
    f32[32,1,11,41], stride (2,2), TensorFlow SAME padding; ``relu_cutoff`` > 0 fuses
    min(max(., 0), cutoff) into the epilogue."""
    batch, frames = _conv0_x('conv0_fwd', x)
    if tuple(weight.shape) != (32, 1, 11, 41):
        raise CtcAsrError('conv0_fwd covers x [B,T,80] and w [32,1,11,41] only.')
    _expect_numel('conv0_fwd', 'bias', bias, 32)
    _expect_numel('conv0_fwd', 'out', out, batch * ((frames + 1) // 2) * 40 * 32)
    out = torch.empty((batch, (frames + 1) // 2, 40, 32), dtype=torch.float32,
                      device=x.device) if out is None else out
    with _Timed('conv0_fwd'):
        _check(load().ctcasr_conv0_fwd(_dev(x, name='x'), _dev(weight, name='weight'),
                                       _dev(bias, name='bias'), _dev(out, name='y'), batch,
                                       frames, float(relu_cutoff), _stream()), 'conv0_fwd')
    return out


@_on_tensor_device
def conv0_pack_weights16(weight, out=None):
    """weight f32[32, 1, 11, 41] -> uint8 buffer for `conv0_fwd16` (fp16 pieces in fragment order,
    scale found on the device); re-pack whenever the weights change."""
    if tuple(weight.shape) != (32, 1, 11, 41):
        raise CtcAsrError('conv0_pack_weights16 covers w [32,1,11,41] only.')
    nbytes = load().ctcasr_conv0_pack16_bytes()
    _expect_numel('conv0_pack_weights16', 'out', out, nbytes)
    out = torch.empty(nbytes, dtype=torch.uint8, device=weight.device) if out is None else out
    _check(load().ctcasr_conv0_pack_weights16(_dev(weight, name='weight'),
                                              _dev(out, torch.uint8, 'packed16'), _stream()),
           'conv0_pack_weights16')
    return out


@_on_tensor_device
def conv0_fwd16(x, packed16, bias=None, out=None, relu_cutoff=0.0):
    """`conv0_fwd` with its products on the fp16 matrix pipe (no bound on x is assumed)."""
    batch, frames = _conv0_x('conv0_fwd16', x)
    _expect_numel('conv0_fwd16', 'packed16', packed16, load().ctcasr_conv0_pack16_bytes())
    _expect_numel('conv0_fwd16', 'bias', bias, 32)
    _expect_numel('conv0_fwd16', 'out', out, batch * ((frames + 1) // 2) * 40 * 32)
    out = torch.empty((batch, (frames + 1) // 2, 40, 32), dtype=torch.float32,
                      device=x.device) if out is None else out
    with _Timed('conv0_fwd'):
        _check(load().ctcasr_conv0_fwd16(_dev(x, name='x'), _dev(packed16, torch.uint8, 'packed16'),
                                         _dev(bias, name='bias'), _dev(out, name='y'), batch,
                                         frames, float(relu_cutoff), _stream()), 'conv0_fwd16')
    return out


@_on_tensor_device
def conv0_wrw16(dz, x, out=None, act=None, relu_cutoff=0.0, dbias=None):
    """`conv0_wrw` with its products on the fp16 matrix pipe."""
    batch, frames = _conv0_x('conv0_wrw16', x)
    if tuple(dz.shape) != (batch, (frames + 1) // 2, 40, 32):
        raise CtcAsrError('conv0_wrw16 covers x [B,T,80], dz [B,ceil(T/2),40,32] only.')
    _conv_mask('conv0_wrw16', dz, act, relu_cutoff, dbias, 32)
    _expect_numel('conv0_wrw16', 'out', out, 32 * 11 * 41)
    out = torch.empty((32, 1, 11, 41), dtype=torch.float32, device=x.device) if out is None \
        else out
    workspace = _workspace(load().ctcasr_conv0_wrw16_workspace_bytes(batch, frames), x.device)
    with _Timed('conv0_wrw'):
        _check(load().ctcasr_conv0_wrw16(_dev(dz, name='dz'), _dev(x, name='x'),
                                         _dev(out, name='dw'), batch, frames,
                                         _dev(act, name='act'), float(relu_cutoff),
                                         _dev(dbias, name='dbias'),
                                         _dev(workspace, torch.uint8, 'workspace'),
                                         workspace.numel(), _stream()), 'conv0_wrw16')
    return out


@_on_tensor_device
def conv0_wrw(dz, x, out=None, act=None, relu_cutoff=0.0, dbias=None):
    """Kernel gradient of the first DS2 convolution: dz f32[B,ceil(T/2),40,32] (NHWC),
    x f32[B,T,80] -> dw f32[32,1,11,41]; ``act`` / ``relu_cutoff`` / ``dbias`` as in
    `conv_s12_wrw`."""
    batch, frames = _conv0_x('conv0_wrw', x)
    if tuple(dz.shape) != (batch, (frames + 1) // 2, 40, 32):
        raise CtcAsrError('conv0_wrw covers x [B,T,80], dz [B,ceil(T/2),40,32] only.')
    _conv_mask('conv0_wrw', dz, act, relu_cutoff, dbias, 32)
    _expect_numel('conv0_wrw', 'out', out, 32 * 11 * 41)
    out = torch.empty((32, 1, 11, 41), dtype=torch.float32, device=x.device) if out is None \
        else out
    workspace = _workspace(load().ctcasr_conv0_wrw_workspace_bytes(batch, frames), x.device)
    with _Timed('conv0_wrw'):
        _check(load().ctcasr_conv0_wrw(_dev(dz, name='dz'), _dev(x, name='x'),
                                       _dev(out, name='dw'), batch, frames, _dev(act, name='act'),
                                       float(relu_cutoff), _dev(dbias, name='dbias'),
                                       _dev(workspace, torch.uint8, 'workspace'),
                                       workspace.numel(), _stream()), 'conv0_wrw')
    return out


@_on_tensor_device
def transpose_batched(src, out=None):
    """src f32[N, R, C] -> out f32[N, C, R]."""
    if src.dim() != 3:
        raise CtcAsrError('transpose_batched: src must be [N, R, C] (got {} dimensions).'
                          .format(src.dim()))
    batch, rows, cols = src.shape
    out = torch.empty((batch, cols, rows), dtype=torch.float32, device=src.device) \
        if out is None else out
    if tuple(out.shape) != (batch, cols, rows):
        raise CtcAsrError('transpose_batched: out must be [N, C, R] = {} (got {}).'
                          .format((batch, cols, rows), tuple(out.shape)))
    _check(load().ctcasr_transpose_batched(_dev(src, name='src'), _dev(out, name='out'), batch,
                                           rows, cols, _stream()), 'transpose_batched')
    return out


@_on_tensor_device
def adam_step(param, grad, m, v, step, lr=1e-5, beta1=0.9, beta2=0.999, epsilon=1e-8,
              grad_scale=1.0, skip=None, grad_factor=None, ema=None, ema_alpha=None):
    """TensorFlow-form Adam over the flat arenas.  ``skip`` (optional int32 device tensor): the
    update is dropped on the device when skip[0] != 0 (`step_guard`).  ``grad_factor`` (optional
    float32 device tensor of one element, `grad_norm`'s clip factor): the gradients are scaled by
    ``grad_scale * grad_factor[0]``, one float32 product, without the host reading the factor.
    ``ema`` (optional float32 device tensor of ``param.numel()`` elements) with ``ema_alpha``
    (a float in [0, 1]): the same launch also moves the average, ``ema += ema_alpha * (param_new
    - ema)`` (`ctcasr_adam_step_ema`); param, m and v come out the same bits either way."""
    for name, tensor in (('grad', grad), ('m', m), ('v', v)):
        _expect_numel('adam_step', name, tensor, param.numel())
    if skip is not None and skip.numel() < 1:
        raise CtcAsrError('adam_step: skip holds no word.')
    if ema is not None:
        _expect_numel('adam_step', 'ema', ema, param.numel())
        if ema_alpha is None:
            raise CtcAsrError('adam_step: ema needs ema_alpha.')
        if grad_factor is not None:
            _expect_numel('adam_step', 'grad_factor', grad_factor, 1)
        _check(load().ctcasr_adam_step_ema(
            _dev(param, name='param'), _dev(grad, name='grad'), _dev(m, name='m'),
            _dev(v, name='v'), _dev(ema, name='ema'), param.numel(), float(lr), float(beta1),
            float(beta2), float(epsilon), int(step), float(grad_scale),
            _dev(skip, torch.int32, 'skip'), _dev(grad_factor, name='grad_factor'),
            float(ema_alpha), _stream()), 'adam_step')
        return
    if ema_alpha is not None:
        raise CtcAsrError('adam_step: ema_alpha without ema.')
    if grad_factor is not None:
        _expect_numel('adam_step', 'grad_factor', grad_factor, 1)
        _check(load().ctcasr_adam_step_clipped(
            _dev(param, name='param'), _dev(grad, name='grad'), _dev(m, name='m'),
            _dev(v, name='v'), param.numel(), float(lr), float(beta1), float(beta2),
            float(epsilon), int(step), float(grad_scale), _dev(skip, torch.int32, 'skip'),
            _dev(grad_factor, name='grad_factor'), _stream()), 'adam_step')
        return
    _check(load().ctcasr_adam_step(_dev(param, name='param'), _dev(grad, name='grad'),
                                   _dev(m, name='m'), _dev(v, name='v'), param.numel(), float(lr),
                                   float(beta1), float(beta2), float(epsilon), int(step),
                                   float(grad_scale), _dev(skip, torch.int32, 'skip'), _stream()),
           'adam_step')


def grad_norm_workspace_bytes(n, segments):
    return load().ctcasr_grad_norm_workspace_bytes(int(n), int(segments))


@_on_tensor_device
def grad_norm(grad, seg_offsets, grad_scale=1.0, max_norm=0.0, skip=None, out=None,
              workspace=None):
    """Norms of the segments of the flat float32 ``grad`` and what follows from them, all on the
    device: returns ``(norms, clip_factor)`` - ``norms`` float32[segments + 1], one per segment
    and the global norm last, each ``grad_scale * sqrt(sum x^2)`` summed in float64 in a fixed
    order; ``clip_factor`` float32[1] = ``max_norm / global`` where that clips, 0 when the global
    norm is not finite, else exactly 1 (`adam_step(grad_factor=...)`).  ``seg_offsets``: int64
    device tensor [segments + 1], ascending from 0 to ``grad.numel()``, interior entries multiples
    of 4.  ``skip`` (the words of `step_guard`): [0] is raised when the global norm is not
    finite, never cleared.  ``out``: a float32 device tensor of segments + 2 elements to hold the
    norms followed by the factor; ``workspace``: uint8, `grad_norm_workspace_bytes`."""
    segments = seg_offsets.numel() - 1
    if segments < 1:
        raise CtcAsrError('grad_norm: seg_offsets holds {} offsets, at least 2 needed.'
                          .format(seg_offsets.numel()))
    if segments > GRAD_NORM_MAX_SEGMENTS:
        raise CtcAsrError('grad_norm: {} segments, at most {} supported.'
                          .format(segments, GRAD_NORM_MAX_SEGMENTS))
    if skip is not None and skip.numel() < 1:
        raise CtcAsrError('grad_norm: skip holds no word.')
    if out is None:
        out = torch.empty(segments + 2, dtype=torch.float32, device=grad.device)
    _expect_numel('grad_norm', 'out', out, segments + 2)
    need = grad_norm_workspace_bytes(grad.numel(), segments)
    if workspace is None:
        workspace = _workspace(need, grad.device)
    elif workspace.numel() < need:
        raise CtcAsrError('grad_norm: workspace holds {} bytes, {} needed.'
                          .format(workspace.numel(), need))
    out_ptr = _dev(out, name='out')
    _check(load().ctcasr_grad_norm(_dev(grad, name='grad'), grad.numel(),
                                   _dev(seg_offsets, torch.int64, 'seg_offsets'), segments,
                                   float(grad_scale), float(max_norm), out_ptr,
                                   out_ptr + 4 * (segments + 1), _dev(skip, torch.int32, 'skip'),
                                   _dev(workspace, torch.uint8, 'workspace'), workspace.numel(),
                                   _stream()), 'grad_norm')
    return out[:segments + 1], out[segments + 1:]


def seq_bn_workspace_bytes(rows, channels):
    return load().ctcasr_seq_bn_workspace_bytes(int(rows), int(channels))


def _seq_bn_shape(what, x, lengths, per_channel):
    """(T, B, C) of a ``seq_bn_*`` call; refuses what the kernels would index out of bounds."""
    if x.dim() != 3:
        raise CtcAsrError('{}: x must be [T, B, C] (got {} dimensions).'.format(what, x.dim()))
    steps, batch, channels = x.shape
    if channels < 4 or channels % 4 != 0:
        raise CtcAsrError('{}: {} channels; a multiple of 4 is needed.'.format(what, channels))
    if steps < 1 or batch < 1:
        raise CtcAsrError('{}: x is empty (shape {}).'.format(what, tuple(x.shape)))
    if lengths is not None:
        _expect_numel(what, 'lengths', lengths, batch)
    for name, tensor in per_channel:
        _expect_numel(what, name, tensor, channels)
    return steps, batch, channels


def _seq_bn_workspace(what, workspace, rows, channels, device):
    need = seq_bn_workspace_bytes(rows, channels)
    if workspace is None:
        return _workspace(need, device)
    if workspace.numel() < need:
        raise CtcAsrError('{}: workspace holds {} bytes, {} needed.'
                          .format(what, workspace.numel(), need))
    return workspace


@_on_tensor_device
def seq_bn_fwd(x, lengths, gamma, beta, running_mean, running_var, decay, eps, workspace=None):
    """Sequence-wise batch normalisation, training mode: ``x`` float32 [T, B, C] is normalised
    per channel over the counted rows - row (t, b) counts when ``lengths`` (int32 [B]) is None or
    ``t < clamp(lengths[b], 0, T)`` - with statistics summed in float64 in a fixed order.
    Returns ``(y, mean, rstd)``: y = (x - mean) * (gamma * rstd) + beta on counted rows and +0
    elsewhere; ``mean`` / ``rstd`` float32 [C] are what `seq_bn_bwd` takes.  Moves
    ``running_mean`` / ``running_var`` (float32 [C], in place) by
    ``decay * running + (1 - decay) * batch``; a channel with non-finite statistics, and a batch
    without a counted row, leave them alone."""
    steps, batch, channels = _seq_bn_shape(
        'seq_bn_fwd', x, lengths, (('gamma', gamma), ('beta', beta),
                                   ('running_mean', running_mean), ('running_var', running_var)))
    workspace = _seq_bn_workspace('seq_bn_fwd', workspace, steps * batch, channels, x.device)
    y = torch.empty_like(x)
    mean = torch.empty(channels, dtype=torch.float32, device=x.device)
    rstd = torch.empty(channels, dtype=torch.float32, device=x.device)
    _check(load().ctcasr_seq_bn_fwd(
        _dev(x, name='x'), _dev(lengths, torch.int32, 'lengths'), steps, batch, channels,
        _dev(gamma, name='gamma'), _dev(beta, name='beta'),
        _dev(running_mean, name='running_mean'), _dev(running_var, name='running_var'),
        float(decay), float(eps), _dev(y, name='y'), _dev(mean, name='mean'),
        _dev(rstd, name='rstd'), _dev(workspace, torch.uint8, 'workspace'), workspace.numel(),
        _stream()), 'seq_bn_fwd')
    return y, mean, rstd


@_on_tensor_device
def seq_bn_infer(x, lengths, gamma, beta, running_mean, running_var, eps):
    """`seq_bn_fwd`'s ``y`` with the running statistics in place of the batch's: mean =
    ``running_mean``, rstd = 1 / sqrt(``running_var`` + eps).  One launch; writes no statistics."""
    steps, batch, channels = _seq_bn_shape(
        'seq_bn_infer', x, lengths, (('gamma', gamma), ('beta', beta),
                                     ('running_mean', running_mean),
                                     ('running_var', running_var)))
    y = torch.empty_like(x)
    _check(load().ctcasr_seq_bn_infer(
        _dev(x, name='x'), _dev(lengths, torch.int32, 'lengths'), steps, batch, channels,
        _dev(gamma, name='gamma'), _dev(beta, name='beta'),
        _dev(running_mean, name='running_mean'), _dev(running_var, name='running_var'),
        float(eps), _dev(y, name='y'), _stream()), 'seq_bn_infer')
    return y


@_on_tensor_device
def seq_bn_bwd(dy, x, lengths, mean, rstd, gamma, dgamma, dbeta, workspace=None):
    """Backward pass of `seq_bn_fwd`: returns ``dx`` (+0 on uncounted rows) and ADDS the
    gradients of gamma and beta to ``dgamma`` / ``dbeta`` (float32 [C], in place).  ``x``,
    ``lengths``: as given to the forward pass; ``mean``, ``rstd``: what it returned."""
    steps, batch, channels = _seq_bn_shape(
        'seq_bn_bwd', x, lengths, (('mean', mean), ('rstd', rstd), ('gamma', gamma),
                                   ('dgamma', dgamma), ('dbeta', dbeta)))
    if tuple(dy.shape) != tuple(x.shape):
        raise CtcAsrError('seq_bn_bwd: dy has shape {}, x has {}.'
                          .format(tuple(dy.shape), tuple(x.shape)))
    workspace = _seq_bn_workspace('seq_bn_bwd', workspace, steps * batch, channels, x.device)
    dx = torch.empty_like(x)
    _check(load().ctcasr_seq_bn_bwd(
        _dev(dy, name='dy'), _dev(x, name='x'), _dev(lengths, torch.int32, 'lengths'), steps,
        batch, channels, _dev(mean, name='mean'), _dev(rstd, name='rstd'),
        _dev(gamma, name='gamma'), _dev(dgamma, name='dgamma'), _dev(dbeta, name='dbeta'),
        _dev(dx, name='dx'), _dev(workspace, torch.uint8, 'workspace'), workspace.numel(),
        _stream()), 'seq_bn_bwd')
    return dx


def rnn_timeout_words(cell, workspace, num_steps, batch, hidden):
    """Device addresses (ints; 0 = none) of the sticky time-out words of the persistent kernels'
    row blocks inside ``workspace`` - what `step_guard` reads."""
    out = []
    for block in range(2):
        off = load().ctcasr_rnn_timeout_word_offset(CELL_IDS[cell], int(num_steps), int(batch),
                                                    int(hidden), block)
        out.append(0 if off == ctypes.c_size_t(-1).value else workspace.data_ptr() + off)
    return out


@_on_tensor_device
def step_guard(status, per_utterance_loss, timeout_words=(0, 0), out=None, wgrad_word=True):
    """out int32[2]: [0] = 1 when this step's gradients must not be applied (a CTC status word
    != 0, a non-finite per-utterance loss, a persistent recurrence that timed out, a part of a
    `wgrad16_gemm` tile on this device that gave up waiting for its turn), [1] = the time-out words
    or-ed (bit 30: the weight-gradient word).  Everything stays on the device
    (`adam_step(skip=out)`)."""
    _expect_numel('step_guard', 'per_utterance_loss', per_utterance_loss, status.numel())
    if out is None:
        out = torch.empty(2, dtype=torch.int32, device=status.device)
    elif out.numel() < 2:
        raise CtcAsrError('step_guard: out holds {} words, 2 needed.'.format(out.numel()))
    sync = _WGRAD16_SYNC.get(status.device.index) if wgrad_word else None
    _check(load().ctcasr_step_guard(_dev(status, torch.int32, 'status'),
                                    _dev(per_utterance_loss, name='per_utterance_loss'),
                                    status.numel(), timeout_words[0] or None,
                                    timeout_words[1] or None,
                                    None if sync is None else sync.data_ptr(),
                                    _dev(out, torch.int32, 'out'), _stream()), 'step_guard')
    return out


def occupy_cus(workgroups, busy_us):
    """Diagnostic: `workgroups` workgroups hold their CUs for `busy_us` on the current stream (the
    CU footprint of a collective's ring kernels; `engine.GradientReducer(stand_in=...)`)."""
    _check(load().ctcasr_occupy_cus(int(workgroups), int(busy_us), _stream()), 'occupy_cus')


@_on_tensor_device
def collective_traffic(scratch_a, scratch_b, workgroups, busy_us, payload_bytes):
    """Diagnostic: `occupy_cus` with a ring all-reduce's memory traffic - 2 x payload_bytes of
    a[i] += b[i] streamed through the scratch pair, paced over busy_us (include/ctcasr.h)."""
    _check(load().ctcasr_collective_traffic(
        int(workgroups), int(busy_us), _dev(scratch_a, name='scratch_a'),
        _dev(scratch_b, name='scratch_b'), scratch_a.numel(), int(payload_bytes), _stream()),
        'collective_traffic')


@_on_tensor_device
def absmax(x, out):
    """out (one int32 word, zeroed by the caller) = max(out, bit pattern of max |x|)."""
    if out.numel() < 1:
        raise CtcAsrError('absmax: out holds no word.')
    _check(load().ctcasr_absmax(_dev(x.reshape(-1), name='x'), x.numel(),
                                _dev(out, torch.int32, 'out'), _stream()), 'absmax')
    return out


_FEATURE_TABLES = {}


def features_num_frames(num_samples):
    return load().ctcasr_features_num_frames(int(num_samples))


@_on_tensor_device
def features(pcm, num_samples, feature_type='mel', normalization='local',
             drop_every_second_frame=False, sampling_rate=16000, out=None, out_len=None):
    """pcm int16[B, N] (device), num_samples int32[B] (device) -> (f32[B, T, 80], i32[B]).
    Only sampling_rate 16000 is served (CtcAsrError otherwise); a row whose num_samples lies
    outside [1, N] gets length 0 and all-zero frames."""
    if pcm.dtype != torch.int16:
        raise CtcAsrError('pcm must be int16 (raw WAV samples, not rescaled).')
    batch, max_samples = pcm.shape
    dev = pcm.device
    key = (dev.index, int(sampling_rate))
    if key not in _FEATURE_TABLES:
        tables = _workspace(load().ctcasr_features_tables_bytes(), dev)
        _check(load().ctcasr_features_init_tables(_dev(tables, torch.uint8, 'tables'),
                                                  int(sampling_rate), _stream()),
               'features_init_tables')
        _FEATURE_TABLES[key] = tables
    tables = _FEATURE_TABLES[key]
    frames = features_num_frames(max_samples)
    if drop_every_second_frame:
        frames = (frames + 1) // 2
    out = torch.empty((batch, frames, 80), dtype=torch.float32, device=dev) if out is None else out
    out_len = torch.empty(batch, dtype=torch.int32, device=dev) if out_len is None else out_len
    workspace = _workspace(load().ctcasr_features_workspace_bytes(batch, max_samples), dev)
    _check(load().ctcasr_features(
        _dev(pcm, torch.int16, 'pcm'), _dev(num_samples, torch.int32, 'num_samples'), batch,
        max_samples, {'mel': 0, 'mfcc': 1}[feature_type],
        {'none': 0, 'local': 1, 'local_scalar': 2}[normalization],
        1 if drop_every_second_frame else 0, _dev(tables, torch.uint8, 'tables'),
        _dev(out, name='out'), out.shape[1], _dev(out_len, torch.int32, 'out_len'),
        _dev(workspace, torch.uint8, 'workspace'), workspace.numel(), _stream()), 'features')
    return out, out_len


def _batch_of(what, name, tensor, batch):
    """One entry per row of the batch, or a message that names both numbers."""
    if tensor.numel() != batch:
        raise CtcAsrError('{}: {} holds {} entries for a batch of {}.'
                          .format(what, name, tensor.numel(), batch))


@_on_tensor_device
def spec_augment(features, lengths, seed, n_freq, freq_width, n_time, time_width,
                 time_permille=1000, intervals=None):
    """SpecAugment in place on ``features`` float32[B, T, 80] with ``lengths`` int32[B] (device):
    ``n_freq`` bands of up to ``freq_width`` columns over the frames of each row, ``n_time`` spans
    of up to ``min(time_width, length * time_permille / 1000)`` frames over all columns, stored
    as 0.0 - the per-column mean under 'local' normalisation, and zero all the same under the
    others.  The draws are integer functions of (``seed``, row, mask) pinned in
    include/ctcasr.h.  ``intervals``: optional int32[B, n_freq + n_time, 2] device tensor that
    receives (start, width) of every mask.  Returns ``features``."""
    if features.dim() != 3 or features.shape[2] != 80:
        raise CtcAsrError('spec_augment: features must be [B, T, 80] (got shape {}).'
                          .format(tuple(features.shape)))
    batch, frames = features.shape[0], features.shape[1]
    _batch_of('spec_augment', 'lengths', lengths, batch)
    for name, count in (('n_freq', n_freq), ('n_time', n_time)):
        if not 0 <= int(count) <= SPEC_AUGMENT_MAX_MASKS:
            raise CtcAsrError('spec_augment: {} is {}, 0..{} supported.'
                              .format(name, count, SPEC_AUGMENT_MAX_MASKS))
    _expect_numel('spec_augment', 'intervals', intervals,
                  batch * (int(n_freq) + int(n_time)) * 2)
    feat_ptr = _dev(features, name='features')
    len_ptr = _dev(lengths, torch.int32, 'lengths')
    int_ptr = _dev(intervals, torch.int32, 'intervals')
    if batch == 0:
        return features
    _check(load().ctcasr_spec_augment(
        feat_ptr, len_ptr, batch, frames, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_freq),
        int(freq_width), int(n_time), int(time_width), int(time_permille), int_ptr, _stream()),
        'spec_augment')
    return features


def resample_num_samples(n, percent):
    """Samples that ``n`` samples come to at ``percent`` % speed: max(1, n * 100 // percent); 0
    for n < 1 or a percent outside 50..200."""
    return load().ctcasr_resample_num_samples(int(n), int(percent))


@_on_tensor_device
def speed_perturb(pcm, num_samples, percent, max_out=None):
    """Resample every row of ``pcm`` int16[B, N] (``num_samples`` int32[B]) to ``percent`` int32[B]
    per cent of its speed (50..200; 100 is a bit copy), all device tensors -> (int16[B, max_out],
    int32[B]).  ``max_out``: columns of the result; callers that know the lengths on the host pass
    the largest `resample_num_samples`.  Without it the result is sized for the slowest speed the
    kernel serves (2 N), which costs no synchronisation.  A row longer than ``max_out`` is cut
    to it and its count says so."""
    if pcm.dim() != 2:
        raise CtcAsrError('speed_perturb: pcm must be [B, N] (got {} dimensions).'
                          .format(pcm.dim()))
    batch, max_in = pcm.shape
    _batch_of('speed_perturb', 'num_samples', num_samples, batch)
    _batch_of('speed_perturb', 'percent', percent, batch)
    pcm_ptr = _dev(pcm, torch.int16, 'pcm')
    num_ptr = _dev(num_samples, torch.int32, 'num_samples')
    pct_ptr = _dev(percent, torch.int32, 'percent')
    if max_out is None:
        max_out = 2 * max_in
    max_out = max(int(max_out), 1)
    out = torch.empty((batch, max_out), dtype=torch.int16, device=pcm.device)
    out_samples = torch.empty(batch, dtype=torch.int32, device=pcm.device)
    if batch == 0:
        return out, out_samples
    _check(load().ctcasr_speed_perturb(pcm_ptr, num_ptr, pct_ptr, batch, max_in,
                                       _dev(out, torch.int16, 'out'), max_out,
                                       _dev(out_samples, torch.int32, 'out_samples'), _stream()),
           'speed_perturb')
    return out, out_samples


def noise_mix_workspace_bytes(batch):
    return load().ctcasr_noise_mix_workspace_bytes(int(batch))


@_on_tensor_device
def noise_mix(pcm, num_samples, bank, clip_offsets, seed, snr_lo_db, snr_hi_db,
              prob_permille=1000, out=None, draws=None, powers=None, gain=None):
    """Mix noise into the rows of ``pcm`` int16[B, N] (``num_samples`` int32[B]) at a drawn SNR.
    ``bank`` int16[*]: the noise clips back to back; ``clip_offsets`` int64[K + 1] (device): where
    each starts, the last entry the bank's length.  Row b is mixed with probability
    ``prob_permille`` / 1000, with a run of a drawn clip that starts at a drawn offset and wraps
    at the clip's end, scaled to a whole number of dB drawn from ``snr_lo_db``..``snr_hi_db`` -
    integer functions of (``seed``, row) pinned in include/ctcasr.h.  ``out``: int16[B, N],
    ``pcm`` itself for in place; a new tensor when None.  Optional device tensors: ``draws``
    int32[B, 4] (status, clip, offset, snr), ``powers`` int64[B, 2] (speech, noise), ``gain``
    float32[B].  Returns ``out``."""
    if pcm.dim() != 2:
        raise CtcAsrError('noise_mix: pcm must be [B, N] (got {} dimensions).'.format(pcm.dim()))
    batch, max_samples = pcm.shape
    _batch_of('noise_mix', 'num_samples', num_samples, batch)
    if clip_offsets.numel() < 2:
        raise CtcAsrError('noise_mix: clip_offsets holds {} offsets, at least 2 needed.'
                          .format(clip_offsets.numel()))
    if bank.numel() < 1:
        raise CtcAsrError('noise_mix: the noise bank is empty.')
    if out is None:
        out = torch.empty_like(pcm)
    _expect_numel('noise_mix', 'out', out, batch * max_samples)
    _expect_numel('noise_mix', 'draws', draws, batch * 4)
    _expect_numel('noise_mix', 'powers', powers, batch * 2)
    _expect_numel('noise_mix', 'gain', gain, batch)
    pcm_ptr = _dev(pcm, torch.int16, 'pcm')
    num_ptr = _dev(num_samples, torch.int32, 'num_samples')
    bank_ptr = _dev(bank, torch.int16, 'bank')
    off_ptr = _dev(clip_offsets, torch.int64, 'clip_offsets')
    out_ptr = _dev(out, torch.int16, 'out')
    draws_ptr = _dev(draws, torch.int32, 'draws')
    powers_ptr = _dev(powers, torch.int64, 'powers')
    gain_ptr = _dev(gain, torch.float32, 'gain')
    for name, tensor in (('num_samples', num_samples), ('bank', bank),
                         ('clip_offsets', clip_offsets), ('out', out), ('draws', draws),
                         ('powers', powers), ('gain', gain)):
        if tensor is not None and tensor.device != pcm.device:
            raise CtcAsrError('noise_mix: {} lives on {}, pcm on {}.'
                              .format(name, tensor.device, pcm.device))
    workspace = _workspace(noise_mix_workspace_bytes(batch), pcm.device)
    _check(load().ctcasr_noise_mix(
        pcm_ptr, num_ptr, batch, max_samples, bank_ptr, off_ptr, clip_offsets.numel() - 1,
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(snr_lo_db), int(snr_hi_db), int(prob_permille),
        out_ptr, draws_ptr, powers_ptr, gain_ptr, _dev(workspace, torch.uint8, 'workspace'),
        workspace.numel(), _stream()), 'noise_mix')
    return out


@_on_tensor_device
def reverb(pcm, num_samples, taps, rir_offsets, rir_delay, rir_scale, seed, prob_permille=1000,
           out=None, draws=None):
    """Convolve the rows of ``pcm`` int16[B, N] (``num_samples`` int32[B]) with a drawn room
    impulse response.  ``taps`` int16[*]: the responses back to back; ``rir_offsets`` int64[R + 1]:
    where each starts, the last entry the bank's length; ``rir_delay`` int32[R]: the tap of the
    direct path; ``rir_scale`` float32[R] (all device tensors; `reverb.RirBank` holds such a
    bank).  Row b is reverberated with probability ``prob_permille`` / 1000 by a response drawn
    from (``seed``, row) - integer functions and exact integer sums pinned in include/ctcasr.h;
    rows that are not, and the columns behind a row's length, are bit copies.  ``out``:
    int16[B, N], never ``pcm`` itself; a new tensor when None.  ``draws``: optional int32[B, 2]
    (status, response).  Returns ``out``."""
    if pcm.dim() != 2:
        raise CtcAsrError('reverb: pcm must be [B, N] (got {} dimensions).'.format(pcm.dim()))
    batch, max_samples = pcm.shape
    _batch_of('reverb', 'num_samples', num_samples, batch)
    if rir_offsets.numel() < 2:
        raise CtcAsrError('reverb: rir_offsets holds {} offsets, at least 2 needed.'
                          .format(rir_offsets.numel()))
    num_rirs = rir_offsets.numel() - 1
    if taps.numel() < 1:
        raise CtcAsrError('reverb: the bank of impulse responses is empty.')
    if out is None:
        out = torch.empty_like(pcm)
    _expect_numel('reverb', 'rir_delay', rir_delay, num_rirs)
    _expect_numel('reverb', 'rir_scale', rir_scale, num_rirs)
    _expect_numel('reverb', 'out', out, batch * max_samples)
    _expect_numel('reverb', 'draws', draws, batch * 2)
    pcm_ptr = _dev(pcm, torch.int16, 'pcm')
    num_ptr = _dev(num_samples, torch.int32, 'num_samples')
    taps_ptr = _dev(taps, torch.int16, 'taps')
    off_ptr = _dev(rir_offsets, torch.int64, 'rir_offsets')
    delay_ptr = _dev(rir_delay, torch.int32, 'rir_delay')
    scale_ptr = _dev(rir_scale, torch.float32, 'rir_scale')
    out_ptr = _dev(out, torch.int16, 'out')
    draws_ptr = _dev(draws, torch.int32, 'draws')
    for name, tensor in (('num_samples', num_samples), ('taps', taps),
                         ('rir_offsets', rir_offsets), ('rir_delay', rir_delay),
                         ('rir_scale', rir_scale), ('out', out), ('draws', draws)):
        if tensor is not None and tensor.device != pcm.device:
            raise CtcAsrError('reverb: {} lives on {}, pcm on {}.'
                              .format(name, tensor.device, pcm.device))
    if out_ptr == pcm_ptr:
        raise CtcAsrError('reverb: out is pcm; the kernel reads the neighbours of a sample, so '
                          'it cannot work in place.')
    _check(load().ctcasr_reverb(
        pcm_ptr, num_ptr, batch, max_samples, taps_ptr, off_ptr, delay_ptr, scale_ptr, num_rirs,
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(prob_permille), out_ptr, draws_ptr, _stream()),
        'reverb')
    return out


def _recording(what, pcm):
    if pcm.dim() != 1:
        raise CtcAsrError('{}: pcm must be one recording, int16[n] (got {} dimensions).'
                          .format(what, pcm.dim()))
    if pcm.numel() < 1:
        raise CtcAsrError('{}: the recording is empty.'.format(what))
    return _dev(pcm, torch.int16, 'pcm')


@_on_tensor_device
def vad_energy(pcm):
    """One pass over a recording, ``pcm`` int16[n] on the device (a slice of a tensor will do: any
    2-byte aligned start) -> (energy int64[F], hist int32[VAD_LEVELS]), F = ceil(n / VAD_HOP):
    the sum of squares of every hop of VAD_HOP samples as an exact integer, and how many hops have
    each level (`vad.level`).  Both device tensors; integer sums, so every run gives the same bits."""
    ptr = _recording('vad_energy', pcm)
    n = pcm.numel()
    energy = torch.empty((n + VAD_HOP - 1) // VAD_HOP, dtype=torch.int64, device=pcm.device)
    hist = torch.empty(VAD_LEVELS, dtype=torch.int32, device=pcm.device)    # (counts fit: F < 2^31)
    _check(load().ctcasr_vad_energy(ptr, n, _dev(energy, torch.int64, 'energy'),
                                    _dev(hist, torch.int32, 'hist'), _stream()), 'vad_energy')
    return energy, hist


@_on_tensor_device
def gather_segments(pcm, seg_start, seg_len, max_samples=None, out=None, num_samples=None):
    """Pieces of a recording as the rows of a batch: ``pcm`` int16[n], ``seg_start`` int64[B] and
    ``seg_len`` int32[B] in samples (all device tensors) -> (int16[B, max_samples], int32[B]), the
    input of `features`.  Row b holds ``pcm[seg_start[b] : seg_start[b] + len]`` and zeros behind
    it, ``len`` being ``seg_len[b]`` clipped to the recording and to ``max_samples``; a row that
    starts outside the recording or has no length is all zero with count 0.  ``max_samples``:
    columns of the result; None reads the largest ``seg_len`` back (one synchronisation)."""
    batch = seg_start.numel()
    if batch < 1:
        raise CtcAsrError('gather_segments: no segments.')
    _batch_of('gather_segments', 'seg_len', seg_len, batch)
    ptr = _recording('gather_segments', pcm)
    start_ptr = _dev(seg_start, torch.int64, 'seg_start')
    len_ptr = _dev(seg_len, torch.int32, 'seg_len')
    if max_samples is None:
        max_samples = int(seg_len.max())
    max_samples = max(int(max_samples), 1)
    if out is None:
        out = torch.empty((batch, max_samples), dtype=torch.int16, device=pcm.device)
    if num_samples is None:
        num_samples = torch.empty(batch, dtype=torch.int32, device=pcm.device)
    _expect_numel('gather_segments', 'out', out, batch * max_samples)
    _expect_numel('gather_segments', 'num_samples', num_samples, batch)
    for name, tensor in (('seg_start', seg_start), ('seg_len', seg_len), ('out', out),
                         ('num_samples', num_samples)):
        if tensor.device != pcm.device:
            raise CtcAsrError('gather_segments: {} lives on {}, pcm on {}.'
                              .format(name, tensor.device, pcm.device))
    _check(load().ctcasr_gather_segments(
        ptr, pcm.numel(), start_ptr, len_ptr, batch, max_samples, _dev(out, torch.int16, 'out'),
        _dev(num_samples, torch.int32, 'num_samples'), _stream()), 'gather_segments')
    return out, num_samples


# format codes of ctcasr_resample (CTCASR_PCM_*), by the dtype scipy.io.wavfile reads a file as
# (24-bit files come as int32, left-justified)
RESAMPLE_FORMATS = {torch.int16: 0, torch.uint8: 1, torch.int32: 2, torch.float32: 3}
_RESAMPLE_TABLES = {}


def resample_plan(rate_in, rate_out=16000):
    """(M, L, radius, taps) of a pair of rates: ``rate_in / rate_out = M / L`` in lowest terms and
    the filter's ``2 * radius + 2`` taps (include/ctcasr.h, K19).  Raises `CtcAsrError` for a rate
    outside 4000..192000 and for a pair whose table of ``L * taps`` weights is not served."""
    out = [_c_int() for _ in range(4)]
    _check(load().ctcasr_resample_plan(int(rate_in), int(rate_out),
                                       *[ctypes.byref(v) for v in out]),
           'resample_plan({}, {})'.format(rate_in, rate_out))
    return tuple(v.value for v in out)


def resample_chunk(rate_in, rate_out=16000):
    """Consecutive outputs one workgroup of `resample` owns; 0 for a pair that is not served.
    Informative - a tuning detail that may change with the kernel, and that no result depends on;
    the tests use it to put recordings across the seams."""
    return load().ctcasr_resample_chunk(int(rate_in), int(rate_out))


def resample_out_samples(n, rate_in, rate_out=16000):
    """Samples that ``n`` frames at ``rate_in`` come to at ``rate_out``: max(1, n * L // M); 0 for
    n < 1, n > 2^31 - 1 or a pair of rates that is not served."""
    return load().ctcasr_resample_out_samples(int(n), int(rate_in), int(rate_out))


def resample_table(rate_in, rate_out, device):
    """The filter weights of a pair of rates, float32 [L, taps] on ``device`` (flat, padded to 16
    bytes): computed by one launch the first time a pair is asked for on a device - on the current
    stream, which is synchronised once, so that the table may then be read from any stream - and
    kept."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise CtcAsrError('resample_table: {} is no GPU; there is no CPU path.'.format(device))
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (int(rate_in), int(rate_out), device.index)
    if key not in _RESAMPLE_TABLES:
        resample_plan(rate_in, rate_out)          # (raises for a pair that is not served)
        nbytes = load().ctcasr_resample_table_bytes(int(rate_in), int(rate_out))
        with torch.cuda.device(device):
            table = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            _check(load().ctcasr_resample_table(int(rate_in), int(rate_out),
                                                _dev(table, name='table'), _stream()),
                   'resample_table')
            # later calls may read the table from any stream: finish it before it is handed out
            # (one synchronisation per pair of rates and device)
            torch.cuda.current_stream().synchronize()
        _RESAMPLE_TABLES[key] = table
    return _RESAMPLE_TABLES[key]


@_on_tensor_device
def resample_launch(samples, rate_in, rate_out=16000):
    """`resample` without the read-back: (int16 [n_out], status int32 [1]), both on the device.
    Bit 0 of the status: a float32 sample was not finite."""
    if samples.dim() not in (1, 2):
        raise CtcAsrError('resample: samples must be [n] or [n, channels] (got {} dimensions).'
                          .format(samples.dim()))
    if samples.dtype not in RESAMPLE_FORMATS:
        raise CtcAsrError('resample: samples are {}; uint8, int16, int32 and float32 are served.'
                          .format(samples.dtype))
    n = samples.shape[0]
    channels = samples.shape[1] if samples.dim() == 2 else 1
    if n < 1:
        raise CtcAsrError('resample: the recording is empty.')
    if not 1 <= channels <= RESAMPLE_MAX_CHANNELS:
        raise CtcAsrError('resample: {} channels, 1..{} are served.'
                          .format(channels, RESAMPLE_MAX_CHANNELS))
    ptr = _dev(samples, samples.dtype, 'samples')
    table = resample_table(rate_in, rate_out, samples.device)
    n_out = resample_out_samples(n, rate_in, rate_out)
    if n_out < 1:
        raise CtcAsrError('resample: {} frames are more than the 2^31 - 1 served.'.format(n))
    out = torch.empty(n_out, dtype=torch.int16, device=samples.device)
    status = torch.empty(1, dtype=torch.int32, device=samples.device)
    _check(load().ctcasr_resample(
        ptr, RESAMPLE_FORMATS[samples.dtype], channels, n, int(rate_in), int(rate_out),
        _dev(table, name='table'), _dev(out, torch.int16, 'out'), n_out,
        _dev(status, torch.int32, 'status'), _stream()), 'resample')
    return out, status


def resample(samples, rate_in, rate_out=16000):
    """One recording to int16 mono at ``rate_out``.  ``samples``: device tensor [n] or
    [n, channels] (1..8, interleaved as in the file) of uint8, int16, int32 or float32 - the
    layouts `scipy.io.wavfile.read` returns - at ``rate_in``.  Channels are averaged, the rate is
    converted with a Hann-windowed sinc (include/ctcasr.h, K19); equal rates apply no filter, and
    mono int16 then comes back bit for bit.  Returns int16 [max(1, n * L // M)] on the device.
    Reads one status word back (a synchronisation) and raises ``ValueError`` for a float32
    recording that holds a non-finite sample."""
    out, status = resample_launch(samples, rate_in, rate_out)
    if int(status.item()) & 1:
        raise ValueError('resample: the recording holds a non-finite sample (NaN or infinity).')
    return out
