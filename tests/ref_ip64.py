"""Float64 restatement of the InnerProduct layer (Caffe InnerProductLayer, axis 1, no transpose) and of the device layout of its bank.

Plain numpy from the definition: y = x W^T + b over the flattened (c, h, w) axes of the bottom.  `pack_bank` is the permutation
the engine applies once at upload: a row of the NHWC device blob is H*W pixels of cstride channels, the layer's C channels at
coffset, so column (p * cstride + coffset + c) of the packed bank holds column (c * H*W + p) of Caffe's and every other column is
zero (pad channels, or the neighbours of a Concat member, then contribute nothing whatever they hold)."""
import numpy as np


def forward(x, w, b=None, relu=False):
    """x (M, ...), w (N, K) with K = prod(x.shape[1:]) in (c, h, w) order -> (M, N), float64."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    y = x @ np.asarray(w, np.float64).T
    if b is not None:
        y = y + np.asarray(b, np.float64)
    return np.maximum(y, 0.0) if relu else y


def magnitude(x, w, b=None):
    """The same operation on absolute values: the magnitude term of ref64.dot_bound."""
    return forward(np.abs(x), np.abs(w), None if b is None else np.abs(b))


def bwd_data(dy, w, dx=None):
    """dX (M, K) = dY (M, N) W (N, K), added to dx when one is given."""
    g = np.asarray(dy, np.float64) @ np.asarray(w, np.float64)
    return g if dx is None else g + np.asarray(dx, np.float64)


def bwd_weights(x, dy, dw=None, db=None):
    """(dW (N, K), db (N,)) = (dY^T X, column sums of dY), added to dw / db when given."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    dy = np.asarray(dy, np.float64)
    gw, gb = dy.T @ x, dy.sum(axis=0)
    return (gw if dw is None else gw + np.asarray(dw, np.float64)), (gb if db is None else gb + np.asarray(db, np.float64))


def pack_bank(w, C, H, W, cstride=None, coffset=0):
    """Caffe's (N, C*H*W) bank -> (N, H*W*cstride) in the memory order of an NHWC row."""
    w = np.asarray(w)
    n = w.shape[0]
    cs = cstride or C
    assert w.shape == (n, C * H * W) and coffset >= 0 and coffset + C <= cs
    out = np.zeros((n, H * W, cs), w.dtype)
    out[:, :, coffset:coffset + C] = w.reshape(n, C, H * W).transpose(0, 2, 1)
    return out.reshape(n, H * W * cs)


def unpack_bank(p, C, H, W, cstride=None, coffset=0):
    """The inverse of pack_bank (what a snapshot reads back): (N, H*W*cstride) -> (N, C*H*W)."""
    p = np.asarray(p)
    n = p.shape[0]
    cs = cstride or C
    return p.reshape(n, H * W, cs)[:, :, coffset:coffset + C].transpose(0, 2, 1).reshape(n, C * H * W)
