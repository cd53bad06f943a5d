"""float64 restatement of Caffe's solvers (public BVLC Caffe sgd_solvers/*.cpp and SGDSolver::GetLearningRate / ClipGradients),
written from the formulas, independent of the kernels: the six update rules with L1 / L2 regularisation, the clip factor and
grad_scale, the seven learning-rate policies, and the clip factor itself.

Every update takes and returns float64 arrays; lr_mult / decay_mult are scalars or per-element arrays.  A test rounds the
SCALARS it passes through the C ABI to float32 first (`f32`), so that both sides use the same hyper-parameters."""
import math

import numpy as np

KINDS = {"SGD": 0, "NESTEROV": 1, "ADAGRAD": 2, "RMSPROP": 3, "ADADELTA": 4, "ADAM": 5}


def f64(a):
    return np.asarray(a, np.float64)


def f32(v):
    """The value a float argument of the C ABI carries."""
    return float(np.float32(v))


def clip_factor(sumsq, clip_gradients, norm_scale=1.0):
    """min(1, clip_gradients / l2norm), l2norm = sqrt(sumsq) * norm_scale; 1 when clipping is off (clip_gradients <= 0)."""
    norm = math.sqrt(float(sumsq)) * norm_scale
    if clip_gradients <= 0 or norm <= clip_gradients:
        return 1.0
    return clip_gradients / norm


def effective_gradient(w, g, weight_decay, decay_mult, grad_scale=1.0, clip=1.0, reg="L2"):
    """g' = g * grad_scale * clip + weight_decay * decay_mult * (w | sign(w))"""
    w = f64(w)
    r = w if reg == "L2" else np.sign(w)
    return f64(g) * grad_scale * clip + weight_decay * f64(decay_mult) * r


def update_from_gradient(kind, w, gg, h1, h2, rate, lr_mult=1.0, momentum=0.0, momentum2=0.999, rms_decay=0.99, delta=1e-8, t=1):
    """ComputeUpdateValue + Update on the effective gradient gg.  Returns (w, h1, h2); h2 passes through unchanged for the
    one-history types (it may be None)."""
    kind = kind.upper()
    w, h1, gg = f64(w), f64(h1), f64(gg)
    lr = rate * f64(lr_mult)
    if kind == "SGD":
        h = momentum * h1 + lr * gg
        return w - h, h, h2
    if kind == "NESTEROV":
        h = momentum * h1 + lr * gg
        return w - ((1 + momentum) * h - momentum * h1), h, h2
    if kind == "ADAGRAD":
        h = h1 + gg * gg
        return w - lr * gg / (np.sqrt(h) + delta), h, h2
    if kind == "RMSPROP":
        h = rms_decay * h1 + (1 - rms_decay) * gg * gg
        return w - lr * gg / (np.sqrt(h) + delta), h, h2
    if kind == "ADADELTA":
        h2 = f64(h2)
        hg = momentum * h1 + (1 - momentum) * gg * gg
        u = gg * np.sqrt((h2 + delta) / (hg + delta))
        return w - lr * u, hg, momentum * h2 + (1 - momentum) * u * u
    if kind == "ADAM":
        h2 = f64(h2)
        m = momentum * h1 + (1 - momentum) * gg
        v = momentum2 * h2 + (1 - momentum2) * gg * gg
        corr = math.sqrt(1 - momentum2 ** t) / (1 - momentum ** t)
        return w - lr * corr * m / (np.sqrt(v) + delta), m, v
    raise ValueError(kind)


def update(kind, w, g, h1, h2, rate, lr_mult=1.0, decay_mult=1.0, momentum=0.0, momentum2=0.999, rms_decay=0.99, delta=1e-8,
           weight_decay=0.0, reg="L2", t=1, grad_scale=1.0, clip=1.0):
    """One solver step on the raw gradient g: Normalize, clip and Regularize (effective_gradient), then update_from_gradient."""
    gg = effective_gradient(w, g, weight_decay, decay_mult, grad_scale, clip, reg)
    return update_from_gradient(kind, w, gg, h1, h2, rate, lr_mult, momentum, momentum2, rms_decay, delta, t)


def rate(policy, it, base_lr, gamma=0.1, power=0.0, stepsize=1, stepvalue=(), max_iter=1):
    if policy == "fixed":
        return base_lr
    if policy == "step":
        return base_lr * gamma ** (it // stepsize)
    if policy == "exp":
        return base_lr * gamma ** it
    if policy == "inv":
        return base_lr * (1 + gamma * it) ** -power
    if policy == "multistep":
        return base_lr * gamma ** len([v for v in stepvalue if v <= it])
    if policy == "poly":
        return base_lr * (1 - it / float(max_iter)) ** power
    if policy == "sigmoid":
        return base_lr / (1 + math.exp(-gamma * (it - stepsize)))
    raise ValueError(policy)
