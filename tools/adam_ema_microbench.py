"""Times the optimizer launch over the C3 arena (122 M parameters) three ways - Adam alone
(ctcasr_adam_step_clipped), Adam with the parameters' moving average fused in
(ctcasr_adam_step_ema), Adam followed by a separate torch ``lerp_`` - and the C3 training step
with grad_accum_steps 1 and 2 (per micro-step).
    python tools/adam_ema_microbench.py [--no-step]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip  # noqa: E402


def timed(fn, reps=20, warm=3):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(reps):
        fn(warm + i)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def optimizer_launches(n=122_000_000):
    p, g, m, v = (torch.randn(n, device='cuda') * 0.01 for _ in range(4))
    v.abs_()
    ema = p.clone()
    one = torch.ones(1, device='cuda')
    forms = {
        'adam_step_clipped (28 B)': lambda i: hip.adam_step(p, g, m, v, 1 + i, grad_factor=one),
        'adam_step_ema (36 B)': lambda i: hip.adam_step(p, g, m, v, 1 + i, grad_factor=one,
                                                         ema=ema, ema_alpha=1e-3),
        'adam_step_clipped + lerp_ (40 B)': lambda i: (
            hip.adam_step(p, g, m, v, 1 + i, grad_factor=one), ema.lerp_(p, 1e-3)),
    }
    for (name, fn), nbytes in zip(forms.items(), (28, 36, 40)):
        ms = timed(fn)
        print('{:36s} {:.3f} ms  {:.2f} TB/s'.format(name, ms, n * nbytes / ms / 1e9))


def c3_step(steps=6):
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.model import ModelConfig
    # C3 of BASELINE.json: 3 convolutions, 4 x BiLSTM-1024, 16 utterances of 10 s
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32, 96), num_units_dense=2048,
                      num_layers_rnn=4, num_units_rnn=1024, rnn_cell='lstm', cudnn=True)
    rng = np.random.default_rng(0)
    feats = torch.tensor(rng.normal(size=(16, 1000, 80)).astype(np.float32), device='cuda')
    flen = torch.full((16,), 1000, dtype=torch.int32)
    labels = [list(rng.integers(1, 28, size=100)) for _ in range(16)]
    for accum in (1, 2):
        trainer = Trainer(cfg, device='cuda', seed=1, grad_accum_steps=accum)
        for _ in range(2 * accum):
            trainer.train_step(feats, flen, labels, check=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps * accum):
            trainer.train_step(feats, flen, labels, check=False)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / (steps * accum)
        print('C3 step, grad_accum_steps={}: {:.2f} ms per micro-step'.format(accum, ms))
        del trainer
        torch.cuda.empty_cache()


if __name__ == '__main__':
    hip.load()
    optimizer_launches()
    if '--no-step' not in sys.argv:
        c3_step()
