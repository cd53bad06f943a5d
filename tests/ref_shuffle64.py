"""numpy reference of the ShuffleChannel layer (csrc/shuffle.hip), written from the formula; imports nothing of the package.

With n = C / g, for every pixel:  y[j * g + i] = x[i * n + j],  0 <= i < g, 0 <= j < n.  The gradient is the inverse permutation,
dx[i * n + j] (+)= dy[j * g + i].  Arrays are NCHW (or (N, C)); values are moved, never computed, so the element type of the operand is
kept and every comparison against this reference is bit for bit (the accumulate's one add is a float32 add of the same two operands)."""
import numpy as np


def source(c: int, g: int) -> np.ndarray:
    """src[k]: the input channel that output channel k receives."""
    if g < 1 or c % g:
        raise ValueError("group %d does not divide %d channels" % (g, c))
    n = c // g
    src = np.empty(c, np.int64)
    for i in range(g):
        for j in range(n):
            src[j * g + i] = i * n + j
    return src


def fwd(x: np.ndarray, g: int) -> np.ndarray:
    return np.ascontiguousarray(x[:, source(x.shape[1], g)])


def bwd(dy: np.ndarray, g: int, dx0=None) -> np.ndarray:
    """dx of the layer with group g; dx0: the gradient the bottom already holds (accumulate), added in dy's element type."""
    dx = np.empty_like(dy)
    dx[:, source(dy.shape[1], g)] = dy
    return dx if dx0 is None else (dx0 + dx).astype(dy.dtype)
