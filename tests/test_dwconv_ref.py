"""The float64 reference of the depthwise convolution (tests/ref_dwconv64.py) against torch: forward against
torch.nn.functional.conv2d(groups=C) in float64, both gradients against autograd.  Non-square images, strides 1 and 2, dilation 2,
unequal pads, per-axis kernels.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_dwconv64 as R

# (kh, kw), (ph, pw), (sh, sw), dilation, (H, W)
CASES = [((3, 3), (1, 1), (1, 1), 1, (7, 9)), ((3, 3), (1, 1), (2, 2), 1, (7, 9)), ((3, 3), (1, 1), (2, 2), 1, (8, 10)),
         ((3, 3), (2, 2), (1, 1), 2, (9, 10)), ((3, 3), (2, 2), (2, 2), 2, (9, 10)), ((5, 5), (2, 2), (2, 2), 1, (9, 8)),
         ((3, 5), (0, 2), (2, 1), 1, (11, 9)), ((3, 1), (1, 0), (1, 1), 1, (5, 6)), ((3, 3), (1, 2), (1, 2), 1, (7, 9)),
         ((7, 7), (3, 3), (1, 1), 1, (6, 5)), ((1, 1), (0, 0), (2, 2), 1, (7, 9))]


@pytest.mark.parametrize("k,pad,s,dil,hw", CASES)
def test_reference_matches_torch(k, pad, s, dil, hw):
    rng = np.random.default_rng(k[0] * 10 + k[1] + dil)
    n, c = 2, 5
    x = rng.standard_normal((n, c) + hw)
    w = rng.standard_normal((c, 1) + k)
    b = rng.standard_normal(c)
    tx, tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b))
    ty = F.conv2d(tx, tw, tb, stride=s, padding=pad, dilation=dil, groups=c)
    y = R.conv2d(x, w, b, pad, s, dil)
    assert y.shape == tuple(ty.shape) == (n, c) + R.out_hw(hw[0], hw[1], k[0], k[1], pad, s, dil)
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-12, atol=1e-12)
    dy = rng.standard_normal(y.shape)
    ty.backward(torch.tensor(dy))
    np.testing.assert_allclose(R.dgrad(dy, w, pad, s, dil, hw[0], hw[1]), tx.grad.numpy(), rtol=1e-12, atol=1e-12)
    dw, db = R.wgrad(x, dy, k[0], k[1], pad, s, dil)
    np.testing.assert_allclose(dw, tw.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(db, tb.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_magnitudes_dominate_and_the_bank_is_tap_major():
    rng = np.random.default_rng(3)
    x, w = rng.standard_normal((1, 6, 5, 7)), rng.standard_normal((6, 1, 3, 3))
    assert np.all(R.conv2d_mag(x, w, None, (1, 1), (1, 1), 1) >= np.abs(R.conv2d(x, w, None, (1, 1), (1, 1), 1)))
    bank = R.pack_bank(w)
    assert bank.shape == (3, 3, 8) and bank.dtype == np.float32
    assert np.array_equal(bank[1, 2, :6], w[:, 0, 1, 2].astype(np.float32)) and not bank[..., 6:].any()
    assert R.pack_bank(w, 8).shape == (3, 3, 8) and R.pack_bank(w[:5], 8).shape == (3, 3, 8) and R.pack_bank(w[:4]).shape == (3, 3, 4)
