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


# ---- half-float kernels: the same definitions with the roundings a kernel makes where it STORES halves ---------------------------
def to_f16_then_f64(a):
    """Round to the nearest half (ties to even, as the hardware conversion does) and return the rounded values as float64."""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def f16_ulp(a):
    """Spacing of the halves at |a| (the subnormal spacing 2^-24 below 2^-14): ONE f16 ulp of every element."""
    a = np.abs(np.asarray(a, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def max_pool_values(x, k, stride, pad):
    """The values of max_pool by a second route: the image padded with -inf (the largest NEGATIVE value stands for 'outside', so an
    all-negative image keeps its own maxima), then the maximum over the k x k shifted, strided views.  Caffe's ceil-mode output size;
    a window that hangs over the bottom / right edge is clipped the same way (the padding there is -inf too)."""
    x = f64(x)
    n, c, h, w = x.shape
    oh, ow = pool_out(h, k, pad, stride), pool_out(w, k, pad, stride)
    hp, wp = (oh - 1) * stride + k, (ow - 1) * stride + k
    xp = np.full((n, c, max(hp, h + pad), max(wp, w + pad)), -np.inf)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    y = np.full((n, c, oh, ow), -np.inf)
    for r in range(k):
        for q in range(k):
            y = np.maximum(y, xp[:, :, r:r + (oh - 1) * stride + 1:stride, q:q + (ow - 1) * stride + 1:stride])
    return y


def lrn_f16(x, local_size, alpha, beta, k=1.0, round_out=True):
    """LRN of a half blob as the half kernels define it: the operands are the halves as given, the arithmetic is exact here (float32 in
    the kernel), and the ONE rounding is the store of y as a half (round_out=False leaves it out: the value the kernel rounds)."""
    y, _ = lrn(x, local_size, alpha, beta, k)
    return to_f16_then_f64(y) if round_out else y


def lrn_f16_allow(y64, local_size, beta):
    """Allowed |y - y64| of a half LRN output against the UNROUNDED float64 value: half an f16 ulp for the store (U16 |y|, or half the
    subnormal spacing) plus the float32 arithmetic in front of it, as lrn_allow of the float32 kernels derives it - (local_size + 2) u on
    the sum of squares -> beta (local_size + 2) u on the factor, 6 u for the power, the product and the conversion."""
    return U16 * np.abs(y64) + 2.0 ** -25 + (beta * (local_size + 2) + 6) * U32 * np.abs(y64)


def pool_lrn_f16(x, k, stride, pad, lrn_first, alpha, beta, lrn_k=1.0, round_out=True):
    """fcn_maxpool_lrn5_fwd_f16 from the definitions: LRN(maxpool(x)) or maxpool(LRN(x)) with local_size 5.  The maximum of halves is
    a half (exact); rounding is monotonic, so the maximum of rounded values is the rounded maximum: one rounding, at the end, either way."""
    if lrn_first:
        y = max_pool_values(lrn(x, 5, alpha, beta, lrn_k)[0], k, stride, pad)
    else:
        y = lrn(max_pool_values(x, k, stride, pad), 5, alpha, beta, lrn_k)[0]
    return to_f16_then_f64(y) if round_out else y


def pool_lrn_conv1x1_f16(x, w, b, k, stride, pad, alpha, beta, lrn_k=1.0, relu=False):
    """(y64, allowance) of fcn_maxpool_lrn5_conv1x1_fwd_f16: pool (exact) -> LRN -> 1x1 convolution + bias (+ ReLU).  The kernel
    STORES the normalised tile as halves (the matrix cores multiply halves), so the reference rounds there too, multiplies in float64 and
    leaves the final rounding to the allowance:
        dot_bound_f16(C, mag, y64)                           float32 accumulation of C products + the one rounding of y
      + 2 * (one f16 ulp of the largest |w_c mid_c|)          the kernel's float32 LRN lands on the other side of a rounding tie on about one
                                                              normalised value in 700 (12 u32 / u16); such a value differs by ONE f16 ulp, and
                                                              an output may see a flipped value in its largest products twice.
    w: [Cout, C] or [Cout, C, 1, 1]."""
    w = f64(w).reshape(w.shape[0], -1)
    mid = to_f16_then_f64(lrn(max_pool_values(x, k, stride, pad), 5, alpha, beta, lrn_k)[0])
    y64 = np.einsum("nchw,oc->nohw", mid, w)
    mag = np.einsum("nchw,oc->nohw", np.abs(mid), np.abs(w))
    if b is not None:
        y64 = y64 + f64(b)[None, :, None, None]
        mag = mag + np.abs(f64(b))[None, :, None, None]
    top = np.zeros_like(y64)
    for c in range(mid.shape[1]):      # largest single product of every output, one input channel at a time
        top = np.maximum(top, np.abs(w[:, c])[None, :, None, None] * np.abs(mid[:, c])[:, None])
    allow = dot_bound_f16(mid.shape[1], mag, y64) + 2 * 2.0 * U16 * top
    return (np.maximum(y64, 0) if relu else y64), allow


def conv2d_image_ones(x3, w, b, pad, stride):
    """(y64, mag, border) of the first layer on an image whose channels 3 and 4 are the constant 1 (FCN_CONV_IMAGE_ONES).  x3: the
    three real channels [N, 3, H, W]; w: [Cout, >= 5, k, k] whose channels 3 and 4 are the filters of the two constant channels.
    The constant channels count ONLY over the taps that lie inside the image (outside it the padded image is 0, not 1):
        y[n,o,i,j] = b[o] + sum_{c<3,r,q} x3[...] w[o,c,r,q] + sum_{(r,q) inside} (w[o,3,r,q] + w[o,4,r,q]).
    border: boolean [OH, OW], True where some tap of the window falls outside the image."""
    x3, w = f64(x3), f64(w)
    n, _, h, wd = x3.shape
    co, _, kh, kw = w.shape
    oh, ow = conv_out(h, kh, pad, stride), conv_out(wd, kw, pad, stride)
    y = conv2d(x3, w[:, :3], b, pad, stride)
    mag = conv2d_mag(x3, w[:, :3], b, pad, stride)
    shift = w[:, 3] + w[:, 4]
    ashift = np.abs(w[:, 3]) + np.abs(w[:, 4])
    border = np.zeros((oh, ow), bool)
    for i in range(oh):
        for j in range(ow):
            r0, q0 = i * stride - pad, j * stride - pad
            rs = [r for r in range(kh) if 0 <= r0 + r < h]
            qs = [q for q in range(kw) if 0 <= q0 + q < wd]
            border[i, j] = len(rs) < kh or len(qs) < kw
            y[:, :, i, j] += shift[:, rs][:, :, qs].sum(axis=(1, 2))[None]
            mag[:, :, i, j] += ashift[:, rs][:, :, qs].sum(axis=(1, 2))[None]
    return y, mag, border
