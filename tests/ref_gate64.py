"""float64 restatement of the four gated-Scale operations, from their definitions alone (NCHW arrays, the gate (N, C)):

    forward     y[n, c, h, w]  = relu?(x[n, c, h, w] * g[n, c] (+ r[n, c, h, w]))
    data grad   dx[n, c, h, w] = dy[n, c, h, w] * g[n, c]                            (+ what dx held, with accumulate)
    gate grad   dg[n, c]       = sum over h, w of dy[n, c, h, w] * x[n, c, h, w]     (+ what dg held, with accumulate)

Nothing here knows how a kernel lays out its work: the tests compare a kernel against this, and tests/test_gate_ref.py compares this
against torch autograd."""
import numpy as np


def gate_fwd(x, g, r=None, relu=False):
    y = np.asarray(x, np.float64) * np.asarray(g, np.float64)[:, :, None, None]
    if r is not None:
        y = y + np.asarray(r, np.float64)
    return np.maximum(y, 0.0) if relu else y


def gate_bwd_data(dy, g, dx_old=None):
    dx = np.asarray(dy, np.float64) * np.asarray(g, np.float64)[:, :, None, None]
    return dx if dx_old is None else dx + np.asarray(dx_old, np.float64)


def gate_bwd_gate(dy, x, dg_old=None):
    dg = (np.asarray(dy, np.float64) * np.asarray(x, np.float64)).sum(axis=(2, 3))
    return dg if dg_old is None else dg + np.asarray(dg_old, np.float64)


def relu_mask(y):
    """d relu(y) / dy as the layers above the gate see it: 1 where the output is positive."""
    return (np.asarray(y, np.float64) > 0.0).astype(np.float64)


def rel_err(a, b):
    """The project's measure: max |a - b| over max |b|."""
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))
