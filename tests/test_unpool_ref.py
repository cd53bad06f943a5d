"""tests/ref_unpool64.py against torch on the CPU, where the two agree by definition, and against cases worked by hand (no GPU).

torch.nn.functional.max_pool2d(ceil_mode=True, return_indices=True) / max_unpool2d and Caffe share the window rule for 2 x 2 / stride 2
on even extents (no clipped window, no window that starts outside); odd extents differ and are the reference's alone - worked by
hand below, as is the duplicate-index rule of overlapping windows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_unpool64 as R


@pytest.mark.parametrize("shape", [(1, 3, 4, 6), (2, 5, 6, 8), (2, 8, 32, 48)], ids=str)
def test_k2_s2_on_even_extents_is_torch(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    n, c, h, w = shape
    assert R.pool_out(h, 2, 2, 0) == h // 2 and R.pool_out(w, 2, 2, 0) == w // 2      # the chosen shapes: whole windows only
    y, idx = R.max_pool_argmax(x, 2, 2, 0)
    ty, tidx = F.max_pool2d(torch.from_numpy(x), 2, 2, 0, ceil_mode=True, return_indices=True)
    assert np.array_equal(y, ty.numpy()) and np.array_equal(idx, tidx.numpy())
    v = rng.standard_normal(y.shape).astype(np.float32)
    up = R.unpool(v, idx, h, w)
    tup = F.max_unpool2d(torch.from_numpy(v), tidx, 2, 2, 0, output_size=(h, w))
    assert up.dtype == np.float32 and np.array_equal(up, tup.numpy())
    assert np.count_nonzero(up) == v.size                                              # no duplicates: every pooled value lands
    # the adjoint of the scatter is the gather
    dy = rng.standard_normal(shape).astype(np.float32)
    vt = torch.from_numpy(v).requires_grad_(True)
    (F.max_unpool2d(vt, tidx, 2, 2, 0, output_size=(h, w)) * torch.from_numpy(dy)).sum().backward()
    assert np.array_equal(R.unpool_bwd(dy, idx), vt.grad.numpy())
    base = rng.standard_normal(y.shape).astype(np.float32)
    assert np.array_equal(R.unpool_bwd(dy, idx, dx=base), base + vt.grad.numpy())


def test_ties_take_the_first_maximum_in_raster_order_and_windows_are_clipped():
    x = np.ones((1, 1, 5, 5), np.float32)
    y, idx = R.max_pool_argmax(x, 3, 2, 0)                      # windows start at rows / columns 0 and 2
    assert y.shape == (1, 1, 2, 2) and np.array_equal(idx[0, 0], [[0, 2], [10, 12]])
    y, idx = R.max_pool_argmax(x, 2, 2, 0)                      # ceil mode: 3 x 3, the last window is one row / column wide
    assert np.array_equal(idx[0, 0], [[0, 2, 4], [10, 12, 14], [20, 22, 24]])
    y, idx = R.max_pool_argmax(x, 3, 2, 1)                      # padded: the first window starts at -1 and is clipped to 0
    assert R.pool_out(5, 3, 2, 1) == 3 and np.array_equal(idx[0, 0], [[0, 1, 3], [5, 6, 8], [15, 16, 18]])
    assert R.pool_out(7, 3, 2, 1) == 4 and R.pool_out(9, 3, 2, 1) == 5 and R.pool_out(7, 2, 2, 0) == 4 and R.pool_out(6, 3, 2, 1) == 4
    assert R.pool_out(4, 2, 2, 1) == 3                          # the third window starts at 3, inside the image
    assert R.pool_out(3, 2, 2, 1) == 2                          # a third window would start at 3 = h, in the right padding: dropped


def test_overlapping_windows_that_share_an_argmax_the_last_writer_wins():
    """3 x 3 / stride 2 on 5 x 5 with a single peak in the middle: all four windows hold pixel (2, 2), so all four masks say 12.  The
    serial scatter writes the four pooled values to that one pixel in the order (0,0), (0,1), (1,0), (1,1): the last one stays, and
    everything else is zero.  Backward hands every window the gradient of the pixel it names."""
    x = np.zeros((1, 1, 5, 5), np.float32)
    x[0, 0, 2, 2] = 5.0
    y, idx = R.max_pool_argmax(x, 3, 2, 0)
    assert np.array_equal(y[0, 0], [[5, 5], [5, 5]]) and np.array_equal(idx[0, 0], [[12, 12], [12, 12]])
    v = np.array([[1, 2], [3, 4]], np.float32).reshape(1, 1, 2, 2)
    up = R.unpool(v, idx, 5, 5)
    want = np.zeros((5, 5), np.float32)
    want[2, 2] = 4.0
    assert np.array_equal(up[0, 0], want)
    dy = np.arange(25, dtype=np.float32).reshape(1, 1, 5, 5)
    assert np.array_equal(R.unpool_bwd(dy, idx)[0, 0], [[12, 12], [12, 12]])
    # two channels with different masks move independently
    x2 = np.concatenate([x, np.ones_like(x)], axis=1)
    _, idx2 = R.max_pool_argmax(x2, 3, 2, 0)
    up2 = R.unpool(np.concatenate([v, v], axis=1), idx2, 5, 5)
    assert np.array_equal(up2[0, 0], want) and up2[0, 1, 0, 0] == 1 and up2[0, 1, 0, 2] == 2 and up2[0, 1, 2, 0] == 3 and up2[0, 1, 2, 2] == 4
    assert np.count_nonzero(up2[0, 1]) == 4


def test_a_window_without_a_maximum_names_no_pixel():
    x = np.full((1, 1, 2, 2), np.finfo(np.float32).min, np.float32)
    y, idx = R.max_pool_argmax(x, 2, 2, 0)
    assert idx[0, 0, 0, 0] == -1
    assert not R.unpool(np.ones((1, 1, 1, 1), np.float32), idx, 2, 2).any()
    assert R.unpool_bwd(np.ones((1, 1, 2, 2), np.float32), idx)[0, 0, 0, 0] == 0
    assert R.mask_nchw(idx).dtype == np.float32 and R.mask_nchw(idx)[0, 0, 0, 0] == -1.0


def test_halves_keep_their_element_type():
    x = np.random.default_rng(3).standard_normal((1, 2, 7, 9)).astype(np.float16)
    y, idx = R.max_pool_argmax(x, 2, 2, 0)
    assert y.dtype == np.float16 and y.shape == (1, 2, 4, 5)
    up = R.unpool(y, idx, 7, 9)
    assert up.dtype == np.float16 and up.max() == y.max() and np.count_nonzero(up) <= y.size
