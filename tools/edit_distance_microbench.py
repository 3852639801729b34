#!/usr/bin/env python
"""Times the scoring of decodes: ctcasr_edit_distance alone (HIP events), the whole
`metrics.error_counts` path (packing, upload, launch, download) and the host functions it
replaces, on one evaluation group - 176 utterances of 10 s in 11 batches of 16, label pairs plus
word pairs, decodes with about 10 % label edits - and on a few length mixes.  The width-64 beam
search launch over the same group is timed beside them.  ``--plans`` times one long pair per
LDS layout of the kernel instead.  Prints one JSON line per case; nothing is gated on the
numbers."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip, metrics, synth  # noqa: E402
from ctc_asr_amd.labels import ALPHABET, decode, encode  # noqa: E402
from ctc_asr_amd.model import CTCModel, ModelConfig, init_params  # noqa: E402

GROUP, BATCH, CHARS, FRAMES = 176, 16, 160, 500


def events_ms(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def wall_ms(fn, iters=10, warmup=2):
    """Host clock around work that ends on the host (a download, or no GPU at all)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    begin = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - begin) * 1e3 / iters


def with_edits(rng, label, rate):
    """``label`` with about ``rate`` of its positions substituted, deleted or followed by an
    insertion, in equal parts."""
    out = []
    for symbol in label:
        kind = rng.random()
        if kind < rate / 3:
            continue
        out.append(int(rng.integers(1, 28)) if kind < 2 * rate / 3 else symbol)
        if kind > 1 - rate / 3:
            out.append(int(rng.integers(1, 28)))
    return out


def kernel_only(hyps, refs):
    """A closure that launches the kernel on rows already in HBM, and its output tensor."""
    def dev(values):
        return torch.tensor(np.asarray(values, dtype=np.int32), device='cuda')

    def packed(rows):
        lengths = np.array([len(r) for r in rows])
        flat = [v for r in rows for v in r] or [0]
        return dev(flat), dev(np.cumsum(lengths) - lengths), dev(lengths), int(lengths.max())

    hyp, hyp_off, hyp_len, max_hyp = packed(hyps)
    ref, ref_off, ref_len, max_ref = packed(refs)
    out = torch.empty((5, len(hyps)), dtype=torch.int32, device='cuda')
    workspace = torch.empty(max(256, hip.edit_distance_workspace_bytes(len(hyps), max_hyp,
                                                                       max_ref)),
                            dtype=torch.uint8, device='cuda')
    lib, stream = hip.load(), torch.cuda.current_stream().cuda_stream

    def launch():
        code = lib.ctcasr_edit_distance(
            hyp.data_ptr(), hyp_off.data_ptr(), hyp_len.data_ptr(), ref.data_ptr(),
            ref_off.data_ptr(), ref_len.data_ptr(), len(hyps), max_hyp, max_ref,
            *[out[k].data_ptr() for k in range(5)], workspace.data_ptr(), workspace.numel(),
            stream)
        assert code == 0, code
    return launch, out


def peaked_logits(rng, labels, frames, classes=29):
    """Logits of a trained model's shape: each label on a frame of its own, the blank elsewhere,
    noise over everything."""
    logits = rng.normal(size=(frames, len(labels), classes)).astype(np.float32)
    logits[:, :, classes - 1] += 6.0
    for b, label in enumerate(labels):
        at = np.sort(rng.choice(frames // 2, size=len(label), replace=False)) * 2
        logits[at, b, classes - 1] -= 6.0
        logits[at, b, label] += 6.0
    return logits


def evaluation_group(model):
    rng = np.random.default_rng(0)
    texts = [synth.random_label(rng, CHARS) for _ in range(GROUP)]
    truths = [encode(t) for t in texts]
    decoded = [with_edits(rng, t, 0.10) for t in truths]
    decoded_texts = [decode(d) for d in decoded]
    labels = np.array(truths, dtype=np.int32)
    batches = [(labels[i:i + BATCH], texts[i:i + BATCH], decoded[i:i + BATCH],
                decoded_texts[i:i + BATCH]) for i in range(0, GROUP, BATCH)]

    host = [CTCModel.error_rates_fn(*b) for b in batches]
    gpu = [model.error_counts_fn(*b) for b in batches]
    for want, got in zip(host, gpu):     # the figures below time the same answer
        for a, b in zip(want, got[:4]):
            assert a.tobytes() == b.tobytes()
    host_ms = wall_ms(lambda: [CTCModel.error_rates_fn(*b) for b in batches], iters=2, warmup=0)
    per_batch_ms = wall_ms(lambda: [model.error_counts_fn(*b) for b in batches])

    original_words, decoded_words = metrics.word_ids(texts, decoded_texts)
    hyps, refs = decoded + decoded_words, truths + original_words

    def one_call():
        words = metrics.word_ids(texts, decoded_texts)
        return metrics.error_counts(decoded + words[1], truths + words[0], 'cuda')
    one_call_ms = wall_ms(one_call)
    launch, _ = kernel_only(hyps, refs)
    kernel_ms = events_ms(launch)

    logits = torch.tensor(peaked_logits(rng, truths, FRAMES), device='cuda')
    seq_len = torch.full((GROUP,), FRAMES, dtype=torch.int32, device='cuda')
    beam_ms = events_ms(lambda: hip.ctc_beam_decode(logits, seq_len, 64), iters=5, warmup=1)
    cells = sum(len(h) * len(r) for h, r in zip(hyps, refs))
    edits = sum(int(c[0]) for c in metrics.error_counts(decoded, truths, 'cuda'))
    print(json.dumps({
        'case': 'evaluation group', 'utterances': GROUP, 'pairs': len(hyps), 'cells': cells,
        'label_edit_rate': round(edits / (GROUP * CHARS), 4),
        'host_error_rates_fn_ms': round(host_ms, 2),
        'error_counts_fn_11_batches_ms': round(per_batch_ms, 3),
        'word_ids_error_counts_one_call_ms': round(one_call_ms, 3),
        'kernel_ms': round(kernel_ms, 4), 'beam64_launch_ms': round(beam_ms, 2)}))


def length_mixes():
    rng = np.random.default_rng(1)

    def rows(lengths, alphabet=28):
        return [rng.integers(1, alphabet, size=int(n)).tolist() for n in lengths]

    mixes = (
        ('600 short pairs', rng.integers(0, 40, size=600), rng.integers(0, 40, size=600)),
        ('8 pairs of 1000', [1000] * 8, [1000] * 8),
        ('176 of 160 and one of 3000', [160] * 176 + [3000], [160] * 176 + [3000]),
        ('one of 3000 alone', [3000], [3000]),
        ('64 pairs of 5000 (carry in workspace)', [300] * 64, [5000] * 64),
    )
    for name, hyp_lens, ref_lens in mixes:
        hyps, refs = rows(hyp_lens), rows(ref_lens)
        launch, out = kernel_only(hyps, refs)
        kernel_ms = events_ms(launch, iters=10, warmup=2)
        path_ms = wall_ms(lambda: metrics.error_counts(hyps, refs, 'cuda'), iters=5, warmup=1)
        cells = sum(len(h) * len(r) for h, r in zip(hyps, refs))
        line = {'case': name, 'pairs': len(hyps), 'cells': cells,
                'kernel_ms': round(kernel_ms, 4), 'error_counts_ms': round(path_ms, 3),
                'kernel_gcells_per_s': round(cells / kernel_ms / 1e6, 2)}
        if cells <= 10e6:
            begin = time.perf_counter()
            want = [metrics.levenshtein(h, r) for h, r in zip(hyps, refs)]
            line['host_levenshtein_ms'] = round((time.perf_counter() - begin) * 1e3, 1)
            assert out[0].cpu().tolist() == want
        print(json.dumps(line))


def plans():
    """``--plans``: one long pair per layout of ``ed_plan`` (the pairs of
    tests/test_gpu_edit_distance_plans.py by size), kernel time and the time per step of the
    pair's wave - a pair is one chain of strips x (ref_len + width - 1) dependent steps."""
    rng = np.random.default_rng(2)
    cases = (
        ('4790 x 4800, 4 waves, carry in LDS', [4790], [4800]),
        ('4801 x 4801, 4 waves, carry in the workspace', [4801], [4801]),
        ('9601 x 9601, 2 waves, workspace', [9601], [9601]),
        ('19201 x 19201, 1 wave, workspace', [19201], [19201]),
        ('two rows of 32767 x 32767, 1 wave, workspace', [32767] * 2, [32767] * 2),
        ('32767 x 70, 512 strips, carry in LDS', [32767], [70]),
        ('70 x 32767, 1 wave, workspace', [70], [32767]),
    )
    for name, hyp_lens, ref_lens in cases:
        hyps = [rng.integers(1, 28, size=n).tolist() for n in hyp_lens]
        refs = [rng.integers(1, 28, size=n).tolist() for n in ref_lens]
        launch, _ = kernel_only(hyps, refs)
        kernel_ms = events_ms(launch, iters=3, warmup=1)
        steps = sum(ref_lens[0] + min(64, hyp_lens[0] - base) - 1
                    for base in range(0, hyp_lens[0], 64))
        print(json.dumps({'case': name, 'pairs': len(hyps), 'steps_per_pair': steps,
                          'kernel_ms': round(kernel_ms, 3),
                          'ns_per_step': round(kernel_ms * 1e6 / steps, 1)}), flush=True)


def main():
    if '--plans' in sys.argv[1:]:
        return plans()
    assert len(ALPHABET) == 27
    cfg = ModelConfig(used_model='ds2', conv_filters=(4, 4), rnn_cell='lstm', cudnn=True,
                      num_units_dense=32, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0)
    model = CTCModel(cfg, 'cuda', params=init_params(cfg, 0))     # (scoring needs its device)
    evaluation_group(model)
    length_mixes()


if __name__ == '__main__':
    main()
