"""tests/ref_interp64.py, the integer statement of Interp's positions, against torch float64 (F.interpolate, bilinear,
align_corners=True) and its autograd - no GPU.  The two differ only in how the position is rounded: 1e-13 covers it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_interp64 as R

SHAPES = [(5, 7, 33, 49), (1, 1, 6, 6), (2, 3, 6, 6), (6, 6, 6, 6), (9, 11, 3, 4), (17, 17, 3, 3), (3, 1, 7, 5), (7, 9, 1, 1), (4, 5, 1, 6)]
CROPPED = [(9, 9, 5, 5, -1, -2), (9, 9, 9, 9, -1, -2), (8, 6, 11, 3, 0, -3), (8, 6, 4, 9, -2, 0)]


def torch_pair(x, dy, oh, ow, pad_beg=0, pad_end=0):
    t = torch.tensor(x, requires_grad=True)
    h, w = x.shape[2:]
    y = F.interpolate(t[:, :, -pad_beg:h + pad_end, -pad_beg:w + pad_end], size=(oh, ow), mode="bilinear", align_corners=True)
    y.backward(torch.tensor(dy))
    return y.detach().numpy(), t.grad.numpy()


@pytest.mark.parametrize("case", [s + (0, 0) for s in SHAPES] + CROPPED)
def test_forward_and_adjoint_against_torch(case):
    h, w, oh, ow, pb, pe = case
    rng = np.random.default_rng(h * 100 + ow)
    x, dy = rng.standard_normal((2, 3, h, w)), rng.standard_normal((2, 3, oh, ow))
    y, dx = torch_pair(x, dy, oh, ow, pb, pe)
    assert np.abs(R.interp(x, oh, ow, pb, pe) - y).max() < 1e-13
    got = R.interp_bwd(dy, h, w, pb, pe)
    assert np.abs(got - dx).max() < 1e-13
    base = rng.standard_normal(x.shape)
    assert np.abs(R.interp_bwd(dy, h, w, pb, pe, dx=base) - (base + dx)).max() < 1e-13
    # <x-bar, A x> == <A^T y-bar, x>: the adjoint is the forward's own
    assert abs((R.interp(x, oh, ow, pb, pe) * dy).sum() - (got * x).sum()) < 1e-11
    assert np.array_equal(got != 0, np.broadcast_to(R.fed(h, w, oh, ow, pb, pe), got.shape)), "fed() is where the adjoint is not zero"


def test_exact_cases():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 2, 6, 6))
    assert np.array_equal(R.interp(x, 6, 6), x)                                   # equal extents: a copy
    x = rng.standard_normal((1, 2, 17, 17))
    assert np.array_equal(R.interp(x, 3, 3), x[:, :, ::8, ::8])                   # shrink_factor 8: every 8th pixel as it is
    lab = rng.integers(0, 21, (2, 1, 321, 321)).astype(np.float64)
    lab[rng.random(lab.shape) < 0.1] = 255
    assert np.array_equal(R.interp(lab, 41, 41), lab[:, :, ::8, ::8])             # the published label_shrink
    assert R.fed(17, 17, 3, 3).sum() == 9 and R.fed(9, 9, 9, 9, -1, -2).sum() == 36


def test_feeders():
    assert R.max_feeders(5, 7, 33, 49) == 15 * 15      # both axes zoom by 8: seven outputs on either side of a pixel, and its own
    assert R.max_feeders(6, 6, 6, 6) == 1 and R.max_feeders(17, 17, 3, 3) == 1 and R.max_feeders(1, 1, 6, 6) == 36
    i0, i1, lam = R.coords(41, 321)
    assert list(i0[:9]) == [0] * 8 + [1] and lam[4] == 0.5 and i1[-1] == 40 and lam[-1] == 0.0
