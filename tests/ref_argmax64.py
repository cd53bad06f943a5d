"""Float64 reference of the ArgMax layer over the channel axis, NCHW, and of the passes the engine fuses in front of it.

Caffe's ArgMaxLayer runs std::partial_sort over (value, index) pairs with std::greater: rank 0 is the largest value and of equal
values the LARGER index comes first.  ranks() restates that with one lexicographic sort per pixel; `tie="smaller"` is the other rule,
kept only so that tests/test_argmax_ref.py can show that a tie case tells the two apart.

Forms of the top: "index" (the k indices), "values" (the k values: Caffe's axis + out_max_val) and "pairs" (Caffe's legacy form with
out_max_val over a bottom with H * W == 1: (N, 2, k), the indices, then the values; without out_max_val "legacy" gives (N, 1, k)).
The fused forms run tests/ref_interp64.py first and take the softmax in float64; ranks are decided on the scores, the reported
values are the probabilities.  Half-float cases hand in the half-rounded input."""
import numpy as np

import ref_interp64 as RI


def as4(x):
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape + (1, 1)) if x.ndim == 2 else x


def ranks(x, top_k=1, tie="larger"):
    """(indices, values) of the top_k ranks over axis 1 of an NCHW (or (N, C)) array: two float64 arrays (N, k, H, W)."""
    x = as4(x)
    c = x.shape[1]
    idx = np.broadcast_to(np.arange(c).reshape(1, c, 1, 1), x.shape)
    # lexsort: the last key is the primary one; ascending (value, +-index), read from the back
    order = np.lexsort((idx if tie == "larger" else -idx, x), axis=1)[:, ::-1][:, :top_k]
    return order.astype(np.float64), np.take_along_axis(x, order, axis=1)


def softmax(x):
    x = as4(x)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def argmax(x, top_k=1, form="index", tie="larger", probs=False):
    """The layer's top in Caffe's shape.  probs: x holds the scores in front of a Softmax - ranks by score, values are probabilities."""
    x = as4(x)
    i, v = ranks(x, top_k, tie)
    if probs:
        v = np.take_along_axis(softmax(x), i.astype(np.int64), axis=1)
    if form == "index":
        return i
    if form == "values":
        return v
    assert x.shape[2] * x.shape[3] == 1, "Caffe's legacy form is taken only where H * W == 1"
    i, v = i[:, :, 0, 0], v[:, :, 0, 0]
    return np.stack([i, v], axis=1) if form == "pairs" else i[:, None, :]


def interp_argmax(x, oh, ow, pad_beg=0, pad_end=0, form="index", tie="larger", probs=False):
    """Interp -> [Softmax ->] ArgMax with top_k 1: (N, 1, oh, ow) indices or values, or (indices, values) for form "pairs"."""
    y = RI.interp(x, oh, ow, pad_beg, pad_end)
    if form == "pairs":
        return argmax(y, 1, "index", tie, probs), argmax(y, 1, "values", tie, probs)
    return argmax(y, 1, form, tie, probs)


def margin(x, top_k=1):
    """The smallest gap between consecutive ranks 0 .. top_k of any pixel (rank k - 1 against rank k decides who is in the top, the
    gaps above it decide their order), relative to the pixel's largest magnitude.  inf for a single channel."""
    x = as4(x)
    k = min(top_k + 1, x.shape[1])
    if k < 2:
        return np.inf
    _, v = ranks(x, k)
    gap = (v[:, :-1] - v[:, 1:]).min(axis=1)
    return float((gap / np.maximum(np.abs(x).max(axis=1), 1e-300)).min())
