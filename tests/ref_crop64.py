"""Float64 reference of the Crop layer and its adjoint (NCHW, explicit loops over the window: no slicing shortcuts to share a
mistake with the code under test)."""
import numpy as np


def crop(x, offsets, size):
    """y[n, c, i, j] = x[n + o0, c + o1, i + o2, j + o3] over an output of shape `size`; offsets one per axis."""
    x = np.asarray(x, np.float64)
    o = [int(v) for v in offsets]
    for a in range(4):
        if o[a] < 0 or o[a] + size[a] > x.shape[a]:
            raise ValueError("axis %d: offset %d + size %d leaves the extent %d" % (a, o[a], size[a], x.shape[a]))
    y = np.empty(tuple(size), np.float64)
    for n in range(size[0]):
        for c in range(size[1]):
            for i in range(size[2]):
                for j in range(size[3]):
                    y[n, c, i, j] = x[n + o[0], c + o[1], i + o[2], j + o[3]]
    return y


def crop_bwd(dy, offsets, shape, dx=None):
    """The adjoint: dy written into the window of a zero gradient of `shape`, or added into the window of `dx` (which is left
    untouched outside it) when one is given."""
    dy = np.asarray(dy, np.float64)
    o = [int(v) for v in offsets]
    out = np.zeros(tuple(shape), np.float64) if dx is None else np.array(dx, np.float64)
    for n in range(dy.shape[0]):
        for c in range(dy.shape[1]):
            for i in range(dy.shape[2]):
                for j in range(dy.shape[3]):
                    out[n + o[0], c + o[1], i + o[2], j + o[3]] += dy[n, c, i, j]
    return out
