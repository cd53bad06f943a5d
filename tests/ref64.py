"""Float64 definitions of the operations the HIP kernels implement, and a derived element-wise error bound.

Plain numpy, written from the textbook definition of each operation (explicit loops over filter taps / window positions and
einsum over channels): independent of oracle/ (no shared im2col, no C library), so the float32 oracle can be held to the
same bound as the kernels (tests/test_guard_harness.py does that first).  Blobs are NCHW; everything is computed in float64
from the inputs as given (for half-float kernels: from the values after they were rounded to half).

The bound.  A kernel that accumulates a dot product of length K in float32 - in any order, by any tree - returns y with
    |y - y64| <= gamma_K * sum_i |x_i| |w_i|,    gamma_K = K u / (1 - K u),  u = 2^-24          (Higham, ASNA 2nd ed., 3.1)
and the rounding of the K products and of the bias addition raises K by two.  `dot_bound` states it as
    C_DOT * (K + 2) * 2^-24 * (sum_i |x_i| |w_i| + |b|)
per ELEMENT, with C_DOT = 2: gamma_K <= 1.01 K u for every K used here, and the factor of two leaves room for a result that
passes through a second float32 rounding (accumulate-into epilogues, a split-K reduction).  The magnitude term is the same
operation applied to |x|, |w|, |b|.  Border pixels see fewer taps, have a smaller magnitude term and so get a TIGHTER
allowance - the opposite of a criterion normalised by the blob's largest value.  Half-float storage adds 2^-11 |y64| for the
one final rounding (products of two halves are exact in float32) plus the smallest half subnormal.

That worst case assumes K rounding errors of the same sign; it is rigorous and, for K in the hundreds, as loose as the old
blob-wide 1e-4.  Rounding errors of a sum behave as independent zero-mean variables, and then the error grows with sqrt(K),
not K (Higham & Mary, "A new approach to probabilistic rounding error analysis", SISC 2019: |y - y64| <= lambda sqrt(K) u
sum |x_i||w_i| with probability 1 - 2 exp(-lambda^2 (1 - u)^2 / 2) per element).  `dot_bound_rms` is that with lambda =
C_RMS = 4 (3e-4 per element before any slack; the float32 oracle and the kernels measure 10 to 25 times below it).  The guarded
cases assert the sharp one; a failure between the two bounds is a summation-order question, beyond the worst case a bug.
"""
import numpy as np

U32 = 2.0 ** -24       # unit roundoff of float32
U16 = 2.0 ** -11       # ... of float16
C_DOT = 2.0
C_RMS = 4.0


def dot_bound(K, mag, c=C_DOT):
    """Allowed |y - y64| per element for a float32-accumulated dot product of length K whose magnitude term is `mag`."""
    return c * (K + 2) * U32 * np.asarray(mag, np.float64) + 1e-37


def dot_bound_rms(K, mag, c=C_RMS):
    """The sqrt(K) allowance (see the module text): what a correct float32 kernel meets with a wide margin."""
    return c * np.sqrt(K + 2.0) * U32 * np.asarray(mag, np.float64) + 1e-37


def dot_bound_f16(K, mag, y64, c=C_RMS):
    return dot_bound_rms(K, mag, c) + U16 * np.abs(y64) + 2.0 ** -24


def worst(y, y64, allow):
    """(largest |y - y64| / allow, flat index of that element); <= 1 passes.  A NaN in y is reported as inf."""
    y = np.asarray(y, np.float64)
    r = np.abs(y - y64) / allow
    r = np.where(np.isfinite(y), r, np.inf)
    i = int(np.argmax(r))
    return float(r.ravel()[i]), i


def f64(a):
    return np.asarray(a, np.float64)


def conv_out(h, k, pad, stride):
    return (h + 2 * pad - k) // stride + 1


def pool_out(h, k, pad, stride):
    """Caffe's ceil-mode pooled size; the last window must start inside the image or its left padding."""
    o = -(-(h + 2 * pad - k) // stride) + 1
    if pad and (o - 1) * stride >= h + pad:
        o -= 1
    return o


def _padded(x, pad, value=0.0):
    if pad == 0:
        return x
    return np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)), constant_values=value)


def conv2d(x, w, b, pad, stride):
    """y[n,o,i,j] = b[o] + sum_{c,r,q} x[n,c,i*s-p+r,j*s-p+q] w[o,c,r,q], zeros outside the image."""
    x, w = f64(x), f64(w)
    n, c, h, wd = x.shape
    co, ci, kh, kw = w.shape
    assert ci == c
    oh, ow = conv_out(h, kh, pad, stride), conv_out(wd, kw, pad, stride)
    xp = _padded(x, pad)
    y = np.zeros((n, co, oh, ow))
    for r in range(kh):
        for q in range(kw):
            tap = xp[:, :, r:r + (oh - 1) * stride + 1:stride, q:q + (ow - 1) * stride + 1:stride]
            y += np.einsum("nchw,oc->nohw", tap, w[:, :, r, q])
    if b is not None:
        y += f64(b)[None, :, None, None]
    return y


def conv2d_mag(x, w, b, pad, stride):
    """The magnitude term of dot_bound for conv2d: the same convolution of |x|, |w|, |b|."""
    return conv2d(np.abs(f64(x)), np.abs(f64(w)), None if b is None else np.abs(f64(b)), pad, stride)


def conv2d_wgrad(x, dy, k, pad, stride):
    """dw[o,c,r,q] = sum_{n,i,j} dy[n,o,i,j] x[n,c,i*s-p+r,j*s-p+q];  db[o] = sum dy[n,o,:,:]."""
    x, dy = f64(x), f64(dy)
    n, c, h, wd = x.shape
    _, co, oh, ow = dy.shape
    xp = _padded(x, pad)
    dw = np.zeros((co, c, k, k))
    for r in range(k):
        for q in range(k):
            tap = xp[:, :, r:r + (oh - 1) * stride + 1:stride, q:q + (ow - 1) * stride + 1:stride]
            dw[:, :, r, q] = np.einsum("nohw,nchw->oc", dy, tap)
    return dw, dy.sum(axis=(0, 2, 3))


def conv2d_dgrad(dy, w, pad, stride, h, wd):
    """dx[n,c,y,x] = sum over (o,r,q,i,j) with i*s-p+r == y, j*s-p+q == x of dy[n,o,i,j] w[o,c,r,q]."""
    dy, w = f64(dy), f64(w)
    n, co, oh, ow = dy.shape
    _, c, kh, kw = w.shape
    dxp = np.zeros((n, c, h + 2 * pad, wd + 2 * pad))
    for r in range(kh):
        for q in range(kw):
            dxp[:, :, r:r + (oh - 1) * stride + 1:stride, q:q + (ow - 1) * stride + 1:stride] += np.einsum("nohw,oc->nchw", dy, w[:, :, r, q])
    return dxp[:, :, pad:pad + h, pad:pad + wd]


def max_pool(x, k, stride, pad):
    """(y, idx): maximum of the window clipped to the image; idx = iy*W+ix of the FIRST maximum in raster order."""
    x = f64(x)
    n, c, h, w = x.shape
    oh, ow = pool_out(h, k, pad, stride), pool_out(w, k, pad, stride)
    y = np.full((n, c, oh, ow), -np.inf)
    idx = np.full((n, c, oh, ow), -1, np.int64)
    for oy in range(oh):
        for ox in range(ow):
            for iy in range(max(oy * stride - pad, 0), min(oy * stride - pad + k, h)):
                for ix in range(max(ox * stride - pad, 0), min(ox * stride - pad + k, w)):
                    v = x[:, :, iy, ix]
                    better = v > y[:, :, oy, ox]
                    y[:, :, oy, ox] = np.where(better, v, y[:, :, oy, ox])
                    idx[:, :, oy, ox] = np.where(better, iy * w + ix, idx[:, :, oy, ox])
    return y, idx


def ave_pool(x, k, stride, pad):
    """Caffe AVE pooling: the sum over the part of the window inside the image, divided by the window's area clipped to the
    image PLUS its padding (the padding counts in the divisor)."""
    x = f64(x)
    n, c, h, w = x.shape
    oh, ow = pool_out(h, k, pad, stride), pool_out(w, k, pad, stride)
    y = np.zeros((n, c, oh, ow))
    for oy in range(oh):
        for ox in range(ow):
            hs, ws = oy * stride - pad, ox * stride - pad
            he, we = min(hs + k, h + pad), min(ws + k, w + pad)
            area = (he - hs) * (we - ws)
            y[:, :, oy, ox] = x[:, :, max(hs, 0):min(he, h), max(ws, 0):min(we, w)].sum(axis=(2, 3)) / area
    return y


def lrn(x, local_size, alpha, beta, k=1.0):
    """(y, scale): scale[c] = k + alpha/n * sum_{c' in window of n centred on c} x[c']^2;  y = x * scale^-beta."""
    x = f64(x)
    c = x.shape[1]
    half = (local_size - 1) // 2
    sq = x * x
    scale = np.full(x.shape, float(k))
    for d in range(-half, half + 1):
        lo, hi = max(0, -d), min(c, c - d)
        scale[:, lo:hi] += alpha / local_size * sq[:, lo + d:hi + d]
    return x * scale ** -beta, scale


def softmax(x):
    x = f64(x)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def sigmoid(x):
    x = f64(x)
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def deconv_depthwise(x, w, b, k, stride, pad):
    """Transposed convolution with one k x k filter per channel (w: [C, k, k]): every input pixel adds x * w at (iy*s-p+r, ix*s-p+q)."""
    x, w = f64(x), f64(w)
    n, c, h, wd = x.shape
    oh, ow = stride * (h - 1) + k - 2 * pad, stride * (wd - 1) + k - 2 * pad
    full = np.zeros((n, c, stride * (h - 1) + k, stride * (wd - 1) + k))
    for r in range(k):
        for q in range(k):
            full[:, :, r:r + (h - 1) * stride + 1:stride, q:q + (wd - 1) * stride + 1:stride] += x * w[None, :, r, q, None, None]
    y = full[:, :, pad:pad + oh, pad:pad + ow].copy()
    if b is not None:
        y += f64(b)[None, :, None, None]
    return y


def deconv_depthwise_bwd(dy, w, k, stride, pad, h, wd):
    """dx[iy,ix] = sum_{r,q} dy[iy*s-p+r, ix*s-p+q] w[r,q] over the positions inside dy."""
    dy, w = f64(dy), f64(w)
    n, c, oh, ow = dy.shape
    full = np.zeros((n, c, stride * (h - 1) + k, stride * (wd - 1) + k))
    full[:, :, pad:pad + oh, pad:pad + ow] = dy
    dx = np.zeros((n, c, h, wd))
    for r in range(k):
        for q in range(k):
            dx += full[:, :, r:r + (h - 1) * stride + 1:stride, q:q + (wd - 1) * stride + 1:stride] * w[None, :, r, q, None, None]
    return dx


def l1_loss(a, b, num, weight=1.0):
    """(loss, da): sum|a-b| / num;  sign(a-b) * weight / num."""
    d = f64(a) - f64(b)
    return float(np.abs(d).sum() / num), np.sign(d) * weight / num


def euclidean_loss(a, b, num, weight=1.0):
    """(loss, da): sum (a-b)^2 / (2 num);  (a-b) * weight / num."""
    d = f64(a) - f64(b)
    return float((d * d).sum() / (2 * num)), d * weight / num


def softmax_loss(x, label, normalize=True, ignore_label=None, weight=1.0):
    """(loss, dx) of SoftmaxWithLoss: x [N,C,H,W] scores, label [N,H,W] class ids; ignored pixels add nothing."""
    p = softmax(x)
    n, c, h, w = p.shape
    lab = np.asarray(label).astype(np.int64)
    valid = np.ones(lab.shape, bool) if ignore_label is None else lab != ignore_label
    safe = np.where(valid, lab, 0)
    picked = np.take_along_axis(p, safe[:, None], axis=1)[:, 0]
    denom = max(int(valid.sum()), 1) if normalize else n
    loss = float(-(np.log(np.maximum(picked, np.finfo(np.float32).tiny)) * valid).sum() / denom)
    dx = p.copy()
    np.put_along_axis(dx, safe[:, None], picked[:, None] - 1.0, axis=1)
    return loss, dx * valid[:, None] * weight / denom


def sgd_update(w, g, hist, rate, momentum, weight_decay, lr_mult, decay_mult, grad_scale=1.0):
    gg = f64(g) * grad_scale + weight_decay * decay_mult * f64(w)
    h = momentum * f64(hist) + rate * lr_mult * gg
    return f64(w) - h, h


def adam_update(w, g, m, v, rate, beta1, beta2, delta, weight_decay, lr_mult, decay_mult, t, grad_scale=1.0):
    gg = f64(g) * grad_scale + weight_decay * decay_mult * f64(w)
    m2 = beta1 * f64(m) + (1 - beta1) * gg
    v2 = beta2 * f64(v) + (1 - beta2) * gg * gg
    corr = np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    return f64(w) - rate * lr_mult * corr * m2 / (np.sqrt(v2) + delta), m2, v2
