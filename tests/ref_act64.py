"""float64 reference of the one-bottom activations of csrc/act.hip, from their definitions (Caffe's PReLULayer, TanHLayer and BiasLayer
over the channel axis), on NCHW arrays:

    PReLU  y = x > 0 ? x : a[c] * x      dx (+)= x > 0 ? dy : a[c] * dy      da[c] = sum over n, h, w of dy * x * [x <= 0]
    TanH   y = tanh(x)                   dx (+)= dy * (1 - y * y)
    Bias   y = x + b[c]                  dx (+)= dy                          db[c] = sum over n, h, w of dy

`p` is the parameter: (C,) values, or ONE value (a scalar, () or (1,)) with `shared` - Caffe's channel_shared - whose gradient is the
per-channel sums folded over the channels.  tests/test_act_ref.py holds all of this to torch and to autograd."""
import numpy as np

PRELU, TANH, BIAS = "PReLU", "TanH", "Bias"


def f64(a):
    return np.asarray(a, np.float64)


def _per_channel(p, x, shared):
    p = f64(p)
    if shared:
        return np.full((1, x.shape[1], 1, 1), p.reshape(-1)[0])
    assert p.shape == (x.shape[1],), (p.shape, x.shape)
    return p.reshape(1, -1, 1, 1)


def fwd(mode, x, p=None, shared=False):
    x = f64(x)
    if mode == TANH:
        return np.tanh(x)
    a = _per_channel(p, x, shared)
    return np.where(x > 0.0, x, a * x) if mode == PRELU else x + a


def bwd_data(mode, dy, ref=None, p=None, shared=False, dx_old=None):
    """ref: the layer's INPUT for PReLU, its OUTPUT for TanH, nothing for Bias."""
    dy = f64(dy)
    if mode == PRELU:
        dx = np.where(f64(ref) > 0.0, dy, _per_channel(p, dy, shared) * dy)
    elif mode == TANH:
        dx = dy * (1.0 - f64(ref) ** 2)
    else:
        dx = dy.copy()
    return dx if dx_old is None else dx + f64(dx_old)


def bwd_param(mode, dy, x=None, shared=False):
    """(C,) sums, or with `shared` their fold over the channels as a (1,) array.  TanH has no parameter."""
    assert mode in (PRELU, BIAS)
    dy = f64(dy)
    t = dy * f64(x) * (f64(x) <= 0.0) if mode == PRELU else dy
    s = t.sum(axis=(0, 2, 3))
    return s.sum(keepdims=True) if shared else s


def rel_err(a, b):
    """The project's measure: max |a - b| over max |b|."""
    b = f64(b)
    return float(np.abs(f64(a) - b).max() / max(np.abs(b).max(), 1e-30))
