"""numpy float64 restatement of one fused Adam + EMA update (`ctcasr_adam_step_ema`,
include/ctcasr.h K12) and of the decay `tf.train.ExponentialMovingAverage(decay, num_updates)`
applies.  Nothing here imports the package: the tests compare the package against it."""

import numpy as np

# one float32 rounding is at most half an ulp: 2^-24 relative to the rounded value
HALF_ULP = 2.0 ** -24


def decay_t(ema_decay, num_updates):
    """min(decay, (1 + k) / (10 + k)), k = the updates counted before this one."""
    k = float(num_updates)
    return min(float(ema_decay), (1.0 + k) / (10.0 + k))


def alpha32(ema_decay, num_updates):
    """What the kernel is handed: 1 - decay_t in float64, rounded to float32 once."""
    return np.float32(1.0 - decay_t(ema_decay, num_updates))


def ema_update(ema_old, param_new, alpha):
    """ema + alpha * (param_new - ema) in float64 from the float32 inputs as they are."""
    ema_old = np.asarray(ema_old, dtype=np.float64)
    param_new = np.asarray(param_new, dtype=np.float64)
    return ema_old + float(alpha) * (param_new - ema_old)


def ema_bound(ema_old, param_new):
    """Elementwise bound on |kernel - ema_update|: three float32 roundings - the difference, the
    product (alpha <= 1) and the sum - each at most half an ulp of a value no larger than
    |param_new| + |ema_old|; a fused multiply-add only drops one of them."""
    return 3.0 * HALF_ULP * (np.abs(np.asarray(param_new, dtype=np.float64)) +
                             np.abs(np.asarray(ema_old, dtype=np.float64)))


def adam_update(param, grad, m, v, step, lr, beta1, beta2, epsilon, grad_scale=1.0):
    """TensorFlow-form Adam in float64: returns (param, m, v)."""
    param, grad, m, v = (np.asarray(x, dtype=np.float64) for x in (param, grad, m, v))
    lr_t = lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    g = grad * grad_scale
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return param - lr_t * m / (np.sqrt(v) + epsilon), m, v
