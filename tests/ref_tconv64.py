"""float64 reference of the transposed (fractionally-strided) convolution, in the SCATTER form: every tap adds a * w into the
strided lattice of a padded canvas, the canvas is cropped by `pad` at the top / left and cut or extended by zeros to the explicit
output size.  It shares no
code with the phase decomposition of csrc/tconv.hip that it checks.

    b[n, cb, oy, ox] = bias[cb] + sum over ca, r, q, iy, ix with oy + pad - r == stride*iy, ox + pad - q == stride*ix
                                   of w[ca, cb, r, q] * a[n, ca, iy, ix]

a: (N, Ca, H, W); w: (Ca, Cb, kh, kw) - the Caffe blob of a group-1 Deconvolution; out_hw: (OH, OW) or None for Caffe's
s(H-1) + k - 2p."""
import numpy as np


def out_size(h, k, stride, pad):
    return stride * (h - 1) + k - 2 * pad


def tconv2d(a, w, bias, pad, stride, out_hw=None):
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    n, ca, h, wd = a.shape
    ca_w, cb, kh, kw = w.shape
    assert ca_w == ca
    oh0, ow0 = out_size(h, kh, stride, pad), out_size(wd, kw, stride, pad)
    oh, ow = (oh0, ow0) if out_hw is None else out_hw
    assert oh0 <= oh < oh0 + stride and ow0 <= ow < ow0 + stride, "explicit output size outside [s(H-1)+k-2p, +s-1]"
    canvas = np.zeros((n, cb, stride * (h - 1) + kh, stride * (wd - 1) + kw))
    for r in range(kh):
        for q in range(kw):
            canvas[:, :, r:r + stride * (h - 1) + 1:stride, q:q + stride * (wd - 1) + 1:stride] += np.einsum("nahw,ab->nbhw", a, w[:, :, r, q])
    # crop by pad; rows / columns past the canvas (under no window of the convolution this is the adjoint of) are zeros.  With
    # pad > 0 an output size above Caffe's reaches into the canvas' trailing pad rows, which do hold contributions.
    out = np.zeros((n, cb, oh, ow))
    ch, cw = min(oh, canvas.shape[2] - pad), min(ow, canvas.shape[3] - pad)
    out[:, :, :ch, :cw] = canvas[:, :, pad:pad + ch, pad:pad + cw]
    if bias is not None:
        out += np.asarray(bias, np.float64)[None, :, None, None]
    return out


def tconv2d_mag(a, w, bias, pad, stride, out_hw=None):
    """The magnitude term of the error bound: the same operation on |a|, |w|, |bias|."""
    return tconv2d(np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(w, np.float64)),
                   None if bias is None else np.abs(np.asarray(bias, np.float64)), pad, stride, out_hw)


def pack_bank(w):
    """The kernel's bank layout [kh][kw][Cb][round4(Ca)] of a (Ca, Cb, kh, kw) blob (what fcn_tconv_bank_pack_f32 writes)."""
    w = np.asarray(w)
    ca, cb, kh, kw = w.shape
    out = np.zeros((kh, kw, cb, (ca + 3) // 4 * 4), w.dtype)
    out[..., :ca] = w.transpose(2, 3, 1, 0)
    return out


def device_blob(w):
    """(Ca, Cb, kh, kw) -> [Ca][kh][kw][round4(Cb)]: how the engine keeps a group-1 Deconvolution blob on the device (and, with
    Ca = Cout, Cb = Cin, exactly the OHWI bank of a Convolution)."""
    w = np.asarray(w)
    ca, cb, kh, kw = w.shape
    out = np.zeros((ca, kh, kw, (cb + 3) // 4 * 4), w.dtype)
    out[..., :cb] = w.transpose(0, 2, 3, 1)
    return out
