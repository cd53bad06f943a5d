"""tests/ref_dconv64.py against torch.nn.functional.conv2d(..., dilation=d) and its autograd, both in float64 (no GPU): the
reference the guarded dilated-convolution tests trust is held to a second, independent statement of the operation first."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64
import ref_dconv64 as D

CASES = [  # n, cin, cout, h, w, k, pad, stride, dil
    (2, 5, 7, 7, 9, 3, 2, 1, 2), (1, 3, 4, 5, 6, 3, 12, 1, 12), (1, 4, 6, 11, 13, 3, 0, 1, 4), (1, 3, 5, 9, 10, 5, 4, 1, 2),
    (2, 2, 3, 8, 7, 2, 0, 1, 3), (1, 4, 4, 6, 5, 1, 0, 1, 3), (1, 5, 6, 7, 9, 3, 1, 1, 1), (2, 3, 4, 11, 9, 3, 2, 2, 2),
    (1, 4, 5, 13, 11, 3, 1, 2, 3), (1, 3, 3, 9, 9, 3, 1, 1, 4),
]


@pytest.mark.parametrize("n,ci,co,h,w,k,pad,s,d", CASES)
def test_forward_and_gradients_match_torch_float64(n, ci, co, h, w, k, pad, s, d):
    rng = np.random.default_rng(h * 100 + w + k + d)
    x = rng.standard_normal((n, ci, h, w))
    wt = rng.standard_normal((co, ci, k, k))
    b = rng.standard_normal(co)
    tx, tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, wt, b))
    ty = F.conv2d(tx, tw, tb, stride=s, padding=pad, dilation=d)
    y = D.conv2d(x, wt, b, pad, s, d)
    assert y.shape == tuple(ty.shape) == (n, co, D.out_size(h, k, pad, s, d), D.out_size(w, k, pad, s, d))
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-12, atol=1e-12)
    dy = rng.standard_normal(y.shape)
    ty.backward(torch.tensor(dy))
    np.testing.assert_allclose(D.dgrad(dy, wt, pad, s, d, h, w), tx.grad.numpy(), rtol=1e-12, atol=1e-12)
    dw, db = D.wgrad(x, dy, k, k, pad, s, d)
    np.testing.assert_allclose(dw, tw.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(db, tb.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_dilation_one_is_the_dense_reference():
    rng = np.random.default_rng(3)
    x, wt, b = rng.standard_normal((2, 4, 8, 9)), rng.standard_normal((5, 4, 3, 3)), rng.standard_normal(5)
    assert np.array_equal(D.conv2d(x, wt, b, 1, 2, 1), ref64.conv2d(x, wt, b, 1, 2))
    dy = rng.standard_normal((2, 5, 4, 5))
    assert np.array_equal(D.dgrad(dy, wt, 1, 2, 1, 8, 9), ref64.conv2d_dgrad(dy, wt, 1, 2, 8, 9))
    assert np.array_equal(D.wgrad(x, dy, 3, 3, 1, 2, 1)[0], ref64.conv2d_wgrad(x, dy, 3, 1, 2)[0])


@pytest.mark.parametrize("k,pad,d", [(3, 2, 2), (3, 1, 4), (5, 4, 2)])
def test_the_data_gradient_is_the_convolution_with_the_flipped_bank(k, pad, d):
    """What the engine does for a stride-1 layer: dX = dconv(dY, flipped bank, pad' = d (k-1) - pad, the same dilation)."""
    rng = np.random.default_rng(k + d)
    h, w = 9, 11
    wt = rng.standard_normal((6, 4, k, k))
    dy = rng.standard_normal((2, 6, D.out_size(h, k, pad, 1, d), D.out_size(w, k, pad, 1, d)))
    via = D.conv2d(dy, D.flipped_bank(wt), None, d * (k - 1) - pad, 1, d)
    np.testing.assert_allclose(via, D.dgrad(dy, wt, pad, 1, d, h, w), rtol=1e-12, atol=1e-12)


def test_magnitude_forms_bound_the_values():
    rng = np.random.default_rng(5)
    x, wt, b = rng.standard_normal((1, 3, 7, 7)), rng.standard_normal((4, 3, 3, 3)), rng.standard_normal(4)
    assert np.all(D.conv2d_mag(x, wt, b, 2, 1, 2) >= np.abs(D.conv2d(x, wt, b, 2, 1, 2)))
    dy = rng.standard_normal((1, 4, 7, 7))
    assert np.all(D.dgrad_mag(dy, wt, 2, 1, 2, 7, 7) >= np.abs(D.dgrad(dy, wt, 2, 1, 2, 7, 7)))
    assert np.all(D.wgrad_mag(x, dy, 3, 3, 2, 1, 2)[0] >= np.abs(D.wgrad(x, dy, 3, 3, 2, 1, 2)[0]))
