"""float64 reference of the rectangular (and, with equal axes, the square dilated) convolution, its data gradient and its weight
gradient, written from the definition (a loop over the filter taps, einsum over the channels).  It shares no code with
csrc/rconv.hip, which it checks.

    y[n, o, i, j] = b[o] + sum over c, r, q of w[o, c, r, q] * x[n, c, i*sh - ph + r*d, j*sw - pw + q*d],   zeros outside the image
    OH = (H + 2 ph - (d (kh - 1) + 1)) // sh + 1,   OW = (W + 2 pw - (d (kw - 1) + 1)) // sw + 1

Blobs are NCHW, w is the Caffe blob (Cout, Cin, kh, kw); pad and stride are (h, w) pairs, d is one dilation for both axes.  The
`_mag` forms are the same operations on absolute values: the magnitude term of ref64.dot_bound."""
import numpy as np


def out_size(h, k, pad, stride, dil):
    return (h + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def out_hw(h, w, kh, kw, pad, stride, dil):
    return out_size(h, kh, pad[0], stride[0], dil), out_size(w, kw, pad[1], stride[1], dil)


def _padded(x, pad):
    return np.pad(x, ((0, 0), (0, 0), (pad[0], pad[0]), (pad[1], pad[1]))) if pad[0] or pad[1] else x


def _tap(xp, r, q, dil, stride, oh, ow):
    return xp[:, :, r * dil:r * dil + (oh - 1) * stride[0] + 1:stride[0], q * dil:q * dil + (ow - 1) * stride[1] + 1:stride[1]]


def conv2d(x, w, b, pad, stride, dil):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, c, h, wd = x.shape
    co, ci, kh, kw = w.shape
    assert ci == c
    oh, ow = out_hw(h, wd, kh, kw, pad, stride, dil)
    xp = _padded(x, pad)
    y = np.zeros((n, co, oh, ow))
    for r in range(kh):
        for q in range(kw):
            y += np.einsum("nchw,oc->nohw", _tap(xp, r, q, dil, stride, oh, ow), w[:, :, r, q])
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None, None]
    return y


def conv2d_mag(x, w, b, pad, stride, dil):
    return conv2d(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                  None if b is None else np.abs(np.asarray(b, np.float64)), pad, stride, dil)


def dgrad(dy, w, pad, stride, dil, h, wd):
    """dx[n, c, y, x] = sum over (o, r, q, i, j) with i*sh - ph + r*d == y, j*sw - pw + q*d == x of dy[n, o, i, j] w[o, c, r, q]."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    n, co, oh, ow = dy.shape
    _, c, kh, kw = w.shape
    dxp = np.zeros((n, c, h + 2 * pad[0], wd + 2 * pad[1]))
    for r in range(kh):
        for q in range(kw):
            _tap(dxp, r, q, dil, stride, oh, ow)[...] += np.einsum("nohw,oc->nchw", dy, w[:, :, r, q])
    return dxp[:, :, pad[0]:pad[0] + h, pad[1]:pad[1] + wd]


def dgrad_mag(dy, w, pad, stride, dil, h, wd):
    return dgrad(np.abs(np.asarray(dy, np.float64)), np.abs(np.asarray(w, np.float64)), pad, stride, dil, h, wd)


def wgrad(x, dy, kh, kw, pad, stride, dil):
    """(dw, db): dw[o, c, r, q] = sum over n, i, j of dy[n, o, i, j] x[n, c, i*sh - ph + r*d, j*sw - pw + q*d];  db[o] = sum dy[n, o, :, :]."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n, c, h, wd = x.shape
    _, co, oh, ow = dy.shape
    assert (oh, ow) == out_hw(h, wd, kh, kw, pad, stride, dil)
    xp = _padded(x, pad)
    dw = np.zeros((co, c, kh, kw))
    for r in range(kh):
        for q in range(kw):
            dw[:, :, r, q] = np.einsum("nohw,nchw->oc", dy, _tap(xp, r, q, dil, stride, oh, ow))
    return dw, dy.sum(axis=(0, 2, 3))


def wgrad_mag(x, dy, kh, kw, pad, stride, dil):
    return wgrad(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64)), kh, kw, pad, stride, dil)


def flipped_bank(w):
    """(Cout, Cin, kh, kw) -> the blob of the data-gradient pass, wt[c, o, kh-1-r, kw-1-q] = w[o, c, r, q]."""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def flipped_pad(kh, kw, pad, dil):
    """The per-axis pads of the data-gradient pass of a stride-1 layer: ph' = d (kh - 1) - ph, pw' = d (kw - 1) - pw."""
    return dil * (kh - 1) - pad[0], dil * (kw - 1) - pad[1]
