"""Numpy float64 restatement of the sequence-wise batch normalisation (include/ctcasr.h "K20",
`CTCModel` with ``rnn_batch_norm``), and the float64 torch model the assembled network is held to.

The kernel arithmetic is restated operation by operation: the sums are added in the pinned order
(chunks of ``rows_per_chunk`` consecutive rows by row number, ascending rows inside a chunk,
ascending chunks), and where the contract names an fp32 operation (``mean``, ``rstd``, ``a``,
``xhat``, ``m1``, ``m2``) the value is rounded to fp32 exactly there.  ``pinned=False`` drops every
fp32 rounding: plain float64 batch normalisation over the counted rows, which
tests/test_batchnorm_host.py holds to ``torch.nn.functional.batch_norm`` and autograd.

Bounds.  Each ``*_bound`` below is the tolerance of the corresponding kernel output, computed
from the inputs and the restatement's own values, never from a kernel's output:
  y    2^-22 (|a| (|x| + |mean|) + |beta|): four fp32 roundings' worth of the terms y is made of
       (x - mean, the product, the sum, and one ulp of difference in mean or rstd)
  dx   2^-22 (|a| (|dy| + |m1| + |xhat m2|) + |dx|)
  dgamma  2^-22 sum |dy xhat|
mean, rstd, the running values and dbeta are fp64 results rounded once: one fp32 ulp.
"""

import numpy as np
import torch

from oracle import torch_ref

EPS = 1e-5


def f32(v):
    """Round to fp32, keep carrying float64."""
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def counted(steps, batch, lengths):
    """bool [T, B]: row (t, b) is counted when lengths is None or t < clamp(lengths[b], 0, T)."""
    if lengths is None:
        return np.ones((steps, batch), dtype=bool)
    clamped = np.clip(np.asarray(lengths, dtype=np.int64), 0, steps)
    return np.arange(steps)[:, None] < clamped[None, :]


def pinned_sums(a, b, mask, rows_per_chunk):
    """(sum of a, sum of a * b) per channel over the counted rows, float64, in the pinned order.
    ``a``, ``b``: float64 [rows, C] holding fp32 values (their product is then exact)."""
    rows, channels = a.shape
    s1, s2 = np.zeros(channels), np.zeros(channels)
    for lo in range(0, rows, rows_per_chunk):
        c1, c2 = np.zeros(channels), np.zeros(channels)
        for r in range(lo, min(lo + rows_per_chunk, rows)):
            if mask[r]:
                c1 = c1 + a[r]
                c2 = c2 + a[r] * b[r]
        s1, s2 = s1 + c1, s2 + c2
    return s1, s2


def forward(x, lengths, gamma, beta, running_mean, running_var, decay, eps=EPS,
            rows_per_chunk=64, pinned=True):
    """Training-mode forward pass.  Returns a dict: y, y_bound [T, B, C]; mean, rstd (fp32 values
    when ``pinned``), mean64, var64, running_mean, running_var (the moved values), a, n."""
    rnd = f32 if pinned else (lambda v: np.asarray(v, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    steps, batch, channels = x.shape
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mask = counted(steps, batch, lengths)
    n = int(mask.sum())
    flat, flat_mask = x.reshape(steps * batch, channels), mask.reshape(-1)
    run_mean = np.asarray(running_mean, np.float64).copy()
    run_var = np.asarray(running_var, np.float64).copy()
    if n == 0:
        zero = np.zeros(channels)
        return dict(y=np.zeros_like(x), y_bound=np.zeros_like(x), mean=zero, rstd=zero,
                    mean64=zero, var64=zero, running_mean=run_mean, running_var=run_var,
                    a=zero, n=0, mask=mask)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        s1, s2 = pinned_sums(flat, flat, flat_mask, rows_per_chunk)
        mean64 = s1 / n
        var64 = s2 / n - mean64 * mean64
        var64 = np.where(var64 < 0.0, 0.0, var64)          # (a NaN stays)
        rstd64 = 1.0 / np.sqrt(var64 + eps)
        mean, rstd = rnd(mean64), rnd(rstd64)
        a = rnd(gamma * rstd)
        y = np.where(mask[:, :, None], (x - mean) * a + beta, 0.0)
        y_bound = 2.0 ** -22 * (np.abs(a) * (np.abs(x) + np.abs(mean)) + np.abs(beta))
        y_bound = np.where(mask[:, :, None], y_bound, 0.0)
        ok = np.isfinite(mean64) & np.isfinite(var64)
        run_mean = np.where(ok, rnd(decay * run_mean + (1.0 - decay) * mean64), run_mean)
        run_var = np.where(ok, rnd(decay * run_var + (1.0 - decay) * var64), run_var)
    return dict(y=y, y_bound=y_bound, mean=mean, rstd=rstd, mean64=mean64, var64=var64,
                running_mean=run_mean, running_var=run_var, a=a, n=n, mask=mask)


def infer(x, lengths, gamma, beta, running_mean, running_var, eps=EPS, pinned=True):
    """Running-statistics forward pass: (y, y_bound)."""
    rnd = f32 if pinned else (lambda v: np.asarray(v, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    mask = counted(x.shape[0], x.shape[1], lengths)[:, :, None]
    mean = np.asarray(running_mean, np.float64)
    rstd = rnd(1.0 / np.sqrt(np.asarray(running_var, np.float64) + eps))
    a = rnd(np.asarray(gamma, np.float64) * rstd)
    beta = np.asarray(beta, np.float64)
    y = np.where(mask, (x - mean) * a + beta, 0.0)
    bound = 2.0 ** -22 * (np.abs(a) * (np.abs(x) + np.abs(mean)) + np.abs(beta))
    return y, np.where(mask, bound, 0.0)


def backward(dy, x, lengths, mean, rstd, gamma, rows_per_chunk=64, pinned=True):
    """Backward pass from the saved ``mean`` / ``rstd``.  Returns a dict: dx, dx_bound [T, B, C];
    dgamma, dbeta (the sums s2, s1 in float64, NOT yet added to anything), dgamma_bound, m1, m2."""
    rnd = f32 if pinned else (lambda v: np.asarray(v, dtype=np.float64))
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    steps, batch, channels = x.shape
    mean, rstd = np.asarray(mean, np.float64), np.asarray(rstd, np.float64)
    mask = counted(steps, batch, lengths)
    n = int(mask.sum())
    with np.errstate(invalid='ignore', over='ignore'):
        xhat = rnd(rnd(x - mean) * rstd)
        a = rnd(np.asarray(gamma, np.float64) * rstd)
        s1, s2 = pinned_sums(dy.reshape(-1, channels), xhat.reshape(-1, channels),
                             mask.reshape(-1), rows_per_chunk)
        m1 = rnd(s1 / n) if n else np.zeros(channels)
        m2 = rnd(s2 / n) if n else np.zeros(channels)
        keep = mask[:, :, None]
        dx = np.where(keep, a * ((dy - m1) - xhat * m2), 0.0)
        bound = 2.0 ** -22 * (np.abs(a) * (np.abs(dy) + np.abs(m1) + np.abs(xhat * m2)) +
                              np.abs(dx))
        dgamma_bound = 2.0 ** -22 * np.where(keep, np.abs(dy * xhat), 0.0).sum(axis=(0, 1))
    return dict(dx=dx, dx_bound=np.where(keep, bound, 0.0), dgamma=s2, dbeta=s1,
                dgamma_bound=dgamma_bound, m1=m1, m2=m2, n=n)


def ulp32(value):
    """One fp32 unit in the last place at |value| (float64 array), at least the smallest normal's."""
    value = np.abs(np.asarray(value, dtype=np.float64)).astype(np.float32)
    return np.spacing(np.maximum(value, np.float32(2.0 ** -126))).astype(np.float64)


class BatchNormRefModel(torch_ref.TorchRefModel):
    """`oracle.torch_ref.TorchRefModel` with the input of recurrent layers 2..L normalised per
    channel over the counted frames: float64 autograd, gamma / beta as Parameters, a training mode
    (batch statistics; moves the running ones) and a running-statistics mode."""

    def __init__(self, params, bn_params, used_model='ds2', rnn_cell='lstm', cudnn=True,
                 decay=0.99, eps=EPS, dtype=torch.float64):
        """``bn_params``: [(gamma, beta)] for layers 1 .. L-1."""
        super().__init__(params, used_model, rnn_cell, cudnn, dtype=dtype)
        self.bn_gamma = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.as_tensor(np.asarray(g), dtype=dtype).clone())
             for g, _ in bn_params])
        self.bn_beta = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.as_tensor(np.asarray(b), dtype=dtype).clone())
             for _, b in bn_params])
        channels = 2 * self.hidden
        self.running = [[torch.zeros(channels, dtype=dtype), torch.ones(channels, dtype=dtype)]
                        for _ in bn_params]
        self.decay, self.eps = decay, eps
        self.bn_training = True

    def _normalise(self, x, seq_len, index):
        steps = x.shape[0]
        if self.cudnn:
            mask = torch.ones(x.shape[:2] + (1,), dtype=x.dtype)
        else:
            mask = (torch.arange(steps)[:, None] < seq_len.clamp(0, steps)[None, :]) \
                .to(x.dtype)[:, :, None]
        if self.bn_training:
            n = mask.sum()
            mean = (x * mask).sum(dim=(0, 1)) / n
            var = (((x - mean) ** 2) * mask).sum(dim=(0, 1)) / n
            with torch.no_grad():
                run = self.running[index]
                run[0] = self.decay * run[0] + (1.0 - self.decay) * mean.detach()
                run[1] = self.decay * run[1] + (1.0 - self.decay) * var.detach()
        else:
            mean, var = self.running[index]
        y = (x - mean) * torch.rsqrt(var + self.eps) * self.bn_gamma[index] + self.bn_beta[index]
        return y * mask

    def forward(self, features, feature_len):
        batch = features.shape[0]
        if self.used_model == 'ds2':
            out = features.unsqueeze(1)
            for kernel, bias, stride in zip(self.front_kernels, self.front_biases,
                                            torch_ref.DEFAULT_STRIDES):
                k_t, k_f = kernel.shape[0], kernel.shape[1]
                _, pt0, pt1 = torch_ref.same_padding(out.shape[2], k_t, stride[0])
                _, pf0, pf1 = torch_ref.same_padding(out.shape[3], k_f, stride[1])
                out = torch.nn.functional.pad(out, (pf0, pf1, pt0, pt1))
                out = torch.nn.functional.conv2d(out, kernel.permute(3, 2, 0, 1), bias,
                                                 stride=stride)
                out = self._relu_clip(out)
            out = out.permute(0, 2, 3, 1).reshape(batch, out.shape[2], -1)
            seq_len = torch.full((batch,), out.shape[1], dtype=torch.long)
        else:
            out = features
            for kernel, bias in zip(self.front_kernels, self.front_biases):
                out = self._relu_clip(out @ kernel + bias)
            seq_len = torch.as_tensor(feature_len, dtype=torch.long)
        x = out.transpose(0, 1)
        for index, rnn in enumerate(self.rnns):
            if index > 0:
                x = self._normalise(x, seq_len, index - 1)
            if self.cudnn:
                x, _ = rnn(x)
            else:
                packed = torch.nn.utils.rnn.pack_padded_sequence(x, seq_len.cpu(),
                                                                 enforce_sorted=False)
                x, _ = torch.nn.utils.rnn.pad_packed_sequence(rnn(packed)[0],
                                                              total_length=x.shape[0])
        d4 = self._relu_clip(x @ self.dense4_kernel + self.dense4_bias)
        return d4 @ self.logits_kernel + self.logits_bias, seq_len
