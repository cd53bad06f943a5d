"""float64 backward of Caffe's AVE pooling, written from PoolingLayer::Backward_cpu: every window (oy, ox) hands
dY[oy][ox] / pool_size(oy, ox) to each input pixel it contains, where pool_size is the window clipped to the image PLUS its
padding (the divisor of the forward pass, ref64.ave_pool).  tests/test_avepool_bwd_abi.py holds it to torch autograd."""
import numpy as np

import ref64


def ave_pool_bwd(dy, k, stride, pad, h, w):
    """dX (n, c, h, w) of dY (n, c, oh, ow); pixels under no window (stride > k) come out zero."""
    dy = ref64.f64(dy)
    n, c, oh, ow = dy.shape
    assert (oh, ow) == (ref64.pool_out(h, k, pad, stride), ref64.pool_out(w, k, pad, stride))
    dx = np.zeros((n, c, h, w))
    for oy in range(oh):
        for ox in range(ow):
            hs, ws = oy * stride - pad, ox * stride - pad
            he, we = min(hs + k, h + pad), min(ws + k, w + pad)
            area = (he - hs) * (we - ws)
            dx[:, :, max(hs, 0):min(he, h), max(ws, 0):min(we, w)] += (dy[:, :, oy, ox] / area)[:, :, None, None]
    return dx


def cover_count(k, stride, pad, h, w):
    """(h, w) array: how many windows contain each input pixel - the length of the sum the kernel forms there."""
    oh, ow = ref64.pool_out(h, k, pad, stride), ref64.pool_out(w, k, pad, stride)
    cnt = np.zeros((h, w))
    for oy in range(oh):
        for ox in range(ow):
            hs, ws = oy * stride - pad, ox * stride - pad
            cnt[max(hs, 0):min(hs + k, h), max(ws, 0):min(ws + k, w)] += 1
    return cnt


# (k, stride, pad, h, w) of the guarded cases: pad > 0, a ceil-mode last window that the image clips, the auxiliary heads' 5x5 / s3 on
# 14x14, stride > k (pixels under no window), global pooling (7x7 on 7x7, 56x56 on 56x56) and a stride == kernel pyramid level
CASES = [(3, 2, 1, 7, 6), (3, 1, 1, 4, 5), (3, 2, 0, 7, 6), (5, 3, 0, 14, 14), (2, 3, 0, 5, 4), (7, 7, 0, 7, 7), (7, 1, 0, 7, 7),
         (56, 56, 0, 56, 56), (8, 8, 0, 16, 24)]
