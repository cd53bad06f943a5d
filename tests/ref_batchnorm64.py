"""float64 restatement of Caffe's BatchNormLayer and ScaleLayer over the channel axis (NCHW arrays; an (N, C) blob is (N, C, 1, 1)),
and of the fused chain BatchNorm -> Scale -> ReLU: forward, the moving-average step of the three blobs, backward.  Written from the
published layer definitions; tests/test_batchnorm_ref.py holds it to torch autograd."""
import numpy as np

F64 = np.float64


def _ch(v):
    return np.asarray(v, F64).reshape(1, -1, 1, 1)


def batch_stats(x):
    """(mean, biased variance) per channel of an NCHW array, in float64."""
    x = np.asarray(x, F64)
    mean = x.mean(axis=(0, 2, 3))
    var = ((x - _ch(mean)) ** 2).mean(axis=(0, 2, 3))
    return mean, var


def global_stats(blob_mean, blob_var, factor):
    """use_global_stats: s = 0 if factor == 0 else 1 / factor; mean = s * blob 0, var = s * blob 1."""
    f = float(np.asarray(factor, F64).reshape(-1)[0])
    s = 0.0 if f == 0.0 else 1.0 / f
    return s * np.asarray(blob_mean, F64), s * np.asarray(blob_var, F64)


def moving_average_step(blob_mean, blob_var, factor, mean, var, m, fraction):
    """The update a TRAIN forward with batch statistics makes: factor = factor * f + 1, blob0 = blob0 * f + mean,
    blob1 = blob1 * f + var * (m / (m - 1) if m > 1 else 1)."""
    corr = m / (m - 1.0) if m > 1 else 1.0
    return (np.asarray(blob_mean, F64) * fraction + mean, np.asarray(blob_var, F64) * fraction + np.asarray(var, F64) * corr,
            np.asarray(factor, F64) * fraction + 1.0)


def chain_fwd(x, mean=None, var=None, eps=1e-5, gamma=None, beta=None, relu=False):
    """y = relu?(gamma * xhat + beta), xhat = (x - mean) / sqrt(var + eps); mean / var None: Scale alone (xhat = x).
    Returns (y, xhat, invstd)."""
    x = np.asarray(x, F64)
    c = x.shape[1]
    if mean is None:
        xhat, inv = x, np.ones(c, F64)
    else:
        inv = 1.0 / np.sqrt(np.asarray(var, F64) + eps)
        xhat = (x - _ch(mean)) * _ch(inv)
    y = xhat * _ch(gamma if gamma is not None else np.ones(c)) + _ch(beta if beta is not None else np.zeros(c))
    if relu:
        y = np.maximum(y, 0.0)
    return y, xhat, inv


def masked(dy, y=None):
    """dy' of the chain: dy where the fused ReLU's output is positive, 0 elsewhere (y None: no ReLU)."""
    dy = np.asarray(dy, F64)
    return dy if y is None else np.where(np.asarray(y) > 0, dy, 0.0)


def chain_sums(dy, xhat, y=None):
    """(sum dy', sum dy' * xhat) per channel: d(beta) and d(gamma) when a Scale is in the chain."""
    d = masked(dy, y)
    return d.sum(axis=(0, 2, 3)), (d * np.asarray(xhat, F64)).sum(axis=(0, 2, 3))


def chain_bwd(dy, xhat, inv, gamma=None, y=None, batch=True):
    """dx = gamma * invstd * (dy' - mean(dy') - xhat * mean(dy' xhat)) with batch statistics; with global statistics and for Scale
    alone (inv = 1) dx = gamma * invstd * dy'."""
    d = masked(dy, y)
    c = d.shape[1]
    k = _ch(gamma if gamma is not None else np.ones(c)) * _ch(inv)
    if not batch:
        return k * d
    m = d.shape[0] * d.shape[2] * d.shape[3]
    s1, s2 = chain_sums(dy, xhat, y)
    return k * (d - _ch(s1) / m - np.asarray(xhat, F64) * _ch(s2) / m)
