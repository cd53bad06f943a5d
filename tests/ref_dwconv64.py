"""float64 reference of the depthwise convolution, its data gradient and its weight gradient, written from the definition (a loop over
the filter taps, one product per channel).  It shares no code with csrc/dwconv.hip, which it checks.

    y[n, c, i, j] = b[c] + sum over r, q of w[c, 0, r, q] * x[n, c, i*sh - ph + r*d, j*sw - pw + q*d],   zeros outside the image
    OH = (H + 2 ph - (d (kh - 1) + 1)) // sh + 1,   OW = (W + 2 pw - (d (kw - 1) + 1)) // sw + 1

Blobs are NCHW, w is the Caffe blob (C, 1, kh, kw); pad and stride are (h, w) pairs, d is one dilation for both axes.  The `_mag`
forms are the same operations on absolute values: the magnitude term of ref64.dot_bound."""
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
    assert w.shape[:2] == (c, 1)
    kh, kw = w.shape[2:]
    oh, ow = out_hw(h, wd, kh, kw, pad, stride, dil)
    xp = _padded(x, pad)
    y = np.zeros((n, c, oh, ow))
    for r in range(kh):
        for q in range(kw):
            y += _tap(xp, r, q, dil, stride, oh, ow) * w[None, :, 0, r, q, None, None]
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None, None]
    return y


def conv2d_mag(x, w, b, pad, stride, dil):
    return conv2d(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                  None if b is None else np.abs(np.asarray(b, np.float64)), pad, stride, dil)


def dgrad(dy, w, pad, stride, dil, h, wd):
    """dx[n, c, y, x] = sum over (r, q, i, j) with i*sh - ph + r*d == y, j*sw - pw + q*d == x of dy[n, c, i, j] w[c, 0, r, q]."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    n, c, oh, ow = dy.shape
    kh, kw = w.shape[2:]
    # (a stride can leave rows below the last window: the padded image is at least as large as the windows reach)
    hp = max(h + 2 * pad[0], (oh - 1) * stride[0] + dil * (kh - 1) + 1)
    wp = max(wd + 2 * pad[1], (ow - 1) * stride[1] + dil * (kw - 1) + 1)
    dxp = np.zeros((n, c, hp, wp))
    for r in range(kh):
        for q in range(kw):
            _tap(dxp, r, q, dil, stride, oh, ow)[...] += dy * w[None, :, 0, r, q, None, None]
    return dxp[:, :, pad[0]:pad[0] + h, pad[1]:pad[1] + wd]


def dgrad_mag(dy, w, pad, stride, dil, h, wd):
    return dgrad(np.abs(np.asarray(dy, np.float64)), np.abs(np.asarray(w, np.float64)), pad, stride, dil, h, wd)


def wgrad(x, dy, kh, kw, pad, stride, dil):
    """(dw, db): dw[c, 0, r, q] = sum over n, i, j of dy[n, c, i, j] x[n, c, i*sh - ph + r*d, j*sw - pw + q*d];  db[c] = sum dy[n, c, :, :]."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n, c, h, wd = x.shape
    _, _, oh, ow = dy.shape
    assert (oh, ow) == out_hw(h, wd, kh, kw, pad, stride, dil)
    xp = _padded(x, pad)
    dw = np.zeros((c, 1, kh, kw))
    for r in range(kh):
        for q in range(kw):
            dw[:, 0, r, q] = (dy * _tap(xp, r, q, dil, stride, oh, ow)).sum(axis=(0, 2, 3))
    return dw, dy.sum(axis=(0, 2, 3))


def wgrad_mag(x, dy, kh, kw, pad, stride, dil):
    return wgrad(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64)), kh, kw, pad, stride, dil)


def pack_bank(w, seg=4):
    """Caffe's (C, 1, kh, kw) -> the device bank [kh][kw][C rounded up to `seg`] float32, pad channels zero."""
    c, _, kh, kw = w.shape
    out = np.zeros((kh, kw, (c + seg - 1) // seg * seg), np.float32)
    out[..., :c] = np.asarray(w, np.float32)[:, 0].transpose(1, 2, 0)
    return out
