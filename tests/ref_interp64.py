"""Float64 reference of the Interp layer (bilinear, corners aligned) and its adjoint, NCHW.

Output index o of n2 lies at position o (n1 - 1) / (n2 - 1) of an input of n1 (0 when n1 or n2 is 1); the position is kept in integers:
cell i0 = num // (n2 - 1), neighbour i1 = min(i0 + 1, n1 - 1) with weight lam = (num % (n2 - 1)) / (n2 - 1), num = o (n1 - 1).  Each
axis is a matrix of shape (n2, n1) with at most two entries per row - weights(n1, n2) - and the layer is Wy x Wx^T per plane of the
effective input: the bottom without its -pad_beg leading and -pad_end trailing rows and columns.  The adjoint is the transposed pair;
rows and columns of the bottom that the pads crop, or that no output reads, get zero.  tests/test_interp_ref.py holds both against
torch float64 (align_corners=True) and autograd."""
import numpy as np


def coords(n1, n2):
    """(i0, i1, lam) per output index, integers and float64."""
    if n1 == 1 or n2 == 1:
        z = np.zeros(n2, np.int64)
        return z, z.copy(), np.zeros(n2, np.float64)
    num = np.arange(n2, dtype=np.int64) * (n1 - 1)
    i0 = num // (n2 - 1)
    lam = (num % (n2 - 1)).astype(np.float64) / float(n2 - 1)
    return i0, np.minimum(i0 + 1, n1 - 1), lam


def weights(n1, n2):
    """The (n2, n1) matrix of one axis: row o holds 1 - lam at i0 and lam at i1 (a zero lam leaves no entry at i1)."""
    i0, i1, lam = coords(n1, n2)
    m = np.zeros((n2, n1), np.float64)
    for o in range(n2):
        m[o, i0[o]] += 1.0 - lam[o]
        if lam[o] != 0.0:
            m[o, i1[o]] += lam[o]
    return m


def window(h, w, pad_beg=0, pad_end=0):
    """(first row / column, effective height, effective width) of an h x w bottom under pads <= 0."""
    if pad_beg > 0 or pad_end > 0 or h + pad_beg + pad_end < 1 or w + pad_beg + pad_end < 1:
        raise ValueError("pads %d / %d on %d x %d" % (pad_beg, pad_end, h, w))
    return -pad_beg, h + pad_beg + pad_end, w + pad_beg + pad_end


def interp(x, oh, ow, pad_beg=0, pad_end=0):
    x = np.asarray(x, np.float64)
    off, he, we = window(x.shape[2], x.shape[3], pad_beg, pad_end)
    return np.einsum("oh,nchw,pw->ncop", weights(he, oh), x[:, :, off:off + he, off:off + we], weights(we, ow))


def interp_mag(x, oh, ow, pad_beg=0, pad_end=0):
    """The magnitude term of ref64.dot_bound: the interpolation of |x| (all weights are >= 0)."""
    return interp(np.abs(np.asarray(x, np.float64)), oh, ow, pad_beg, pad_end)


def interp_bwd(dy, h, w, pad_beg=0, pad_end=0, dx=None):
    """dX of an h x w bottom: zero where nothing feeds a pixel, or added into `dx` when one is given."""
    dy = np.asarray(dy, np.float64)
    off, he, we = window(h, w, pad_beg, pad_end)
    out = np.zeros(dy.shape[:2] + (h, w), np.float64) if dx is None else np.array(dx, np.float64)
    out[:, :, off:off + he, off:off + we] += np.einsum("oh,ncop,pw->nchw", weights(he, dy.shape[2]), dy, weights(we, dy.shape[3]))
    return out


def interp_bwd_mag(dy, h, w, pad_beg=0, pad_end=0):
    return interp_bwd(np.abs(np.asarray(dy, np.float64)), h, w, pad_beg, pad_end)


def fed(h, w, oh, ow, pad_beg=0, pad_end=0):
    """Boolean (h, w): the pixels of the bottom that at least one output reads with a weight that is not zero."""
    off, he, we = window(h, w, pad_beg, pad_end)
    m = np.zeros((h, w), bool)
    m[off:off + he, off:off + we] = np.outer((weights(he, oh) != 0).any(0), (weights(we, ow) != 0).any(0))
    return m


def max_feeders(h, w, oh, ow, pad_beg=0, pad_end=0):
    """The largest number of output pixels that feed one input pixel: the length of the adjoint's longest sum."""
    _, he, we = window(h, w, pad_beg, pad_end)
    return int((weights(he, oh) != 0).sum(0).max()) * int((weights(we, ow) != 0).sum(0).max())
