"""Reference for MAX pooling with its mask and for the SegNet fork's Upsample layer, in numpy, from Caffe's definitions (it shares no
code with the kernels).

  max_pool_argmax   PoolingLayer, pool: MAX with two tops: ceil-mode extents (the last window must start inside the image or the left
                    padding), the window clipped to the image, the FIRST maximum in raster order (strict '>' from -FLT_MAX); the mask
                    holds iy * W + ix in the plane of the bottom, -1 where no element exceeded the start value.
  unpool            UpsampleLayer forward: the top starts as zeros and the pooled pixels are scattered SERIALLY in ascending (py, px)
                    order, top[mask] = bottom - so where several windows name one pixel the last writer wins.
  unpool_bwd        UpsampleLayer backward: bottom_diff = top_diff[mask], a gather; with `dx` the one float32 add of an accumulating
                    launch, performed in float32.
Nothing here rounds: the values move as they are, in the element type they come in."""
import numpy as np


def pool_out(h, k, s, p):
    o = -(-(h + 2 * p - k) // s) + 1
    if p > 0 and (o - 1) * s >= h + p:
        o -= 1
    return o


def max_pool_argmax(x, k, s, p):
    """(y, idx): x is (N, C, H, W); y has x's element type, idx is int32."""
    n, c, h, w = x.shape
    ph, pw = pool_out(h, k, s, p), pool_out(w, k, s, p)
    lowest = np.finfo(x.dtype).min
    y = np.full((n, c, ph, pw), lowest, x.dtype)
    idx = np.full((n, c, ph, pw), -1, np.int32)
    for py in range(ph):
        for px in range(pw):
            y0, x0 = max(py * s - p, 0), max(px * s - p, 0)
            y1, x1 = min(py * s - p + k, h), min(px * s - p + k, w)
            for iy in range(y0, y1):              # raster order; a strict '>' keeps the first maximum
                for ix in range(x0, x1):
                    v = x[:, :, iy, ix]
                    better = v > y[:, :, py, px]
                    y[:, :, py, px] = np.where(better, v, y[:, :, py, px])
                    idx[:, :, py, px] = np.where(better, iy * w + ix, idx[:, :, py, px])
    return y, idx


def unpool(x, idx, h, w):
    """x, idx: (N, C, PH, PW) -> (N, C, h, w) of x's element type: zeros, then the serial scatter."""
    n, c, ph, pw = x.shape
    y = np.zeros((n, c, h * w), x.dtype)
    nn, cc = np.meshgrid(np.arange(n), np.arange(c), indexing="ij")
    for py in range(ph):
        for px in range(pw):
            at = idx[:, :, py, px]
            ok = at >= 0
            y[nn[ok], cc[ok], at[ok]] = x[:, :, py, px][ok]
    return y.reshape(n, c, h, w)


def unpool_bwd(dy, idx, dx=None):
    """dy: (N, C, H, W), idx: (N, C, PH, PW) -> dx (N, C, PH, PW) float32; `dx` given: dx + the gathered values, one float32 add."""
    n, c, h, w = dy.shape
    flat = dy.reshape(n, c, h * w)
    ok = idx >= 0
    got = np.take_along_axis(flat, np.where(ok, idx, 0).reshape(n, c, -1).astype(np.int64), axis=2).reshape(idx.shape)
    got = np.where(ok, got, np.float32(0)).astype(np.float32)
    return got if dx is None else (dx.astype(np.float32) + got).astype(np.float32)


def mask_nchw(idx):
    """Caffe's mask blob: the indices as float32."""
    return idx.astype(np.float32)
