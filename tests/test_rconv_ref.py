"""tests/ref_rconv64.py against torch.nn.functional.conv2d with per-axis stride / padding, a dilation and its autograd, both in float64
(no GPU): the reference the guarded rectangular- and dilated-convolution tests trust is held to a second, independent statement of the operation first."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64
import ref_rconv64 as R

CASES = [  # n, cin, cout, (h, w), (kh, kw), (ph, pw), (sh, sw), dil
    (2, 5, 7, (7, 9), (1, 7), (0, 3), (1, 1), 1), (2, 5, 7, (7, 9), (7, 1), (3, 0), (1, 1), 1), (1, 3, 4, (6, 5), (1, 7), (0, 3), (1, 1), 1),
    (1, 4, 6, (5, 6), (1, 3), (0, 1), (1, 1), 1), (1, 4, 6, (5, 6), (3, 1), (1, 0), (1, 1), 1), (2, 3, 5, (11, 9), (3, 5), (0, 2), (2, 1), 1),
    (1, 2, 3, (8, 13), (1, 5), (0, 0), (1, 2), 1), (1, 4, 4, (9, 10), (3, 1), (2, 0), (1, 1), 2), (2, 3, 4, (8, 7), (2, 3), (0, 2), (1, 1), 2),
    (1, 5, 6, (7, 9), (3, 3), (1, 2), (1, 1), 1), (1, 3, 3, (12, 11), (3, 2), (1, 1), (2, 3), 2),
    # square dilated layers: equal axes, written (k, k), (p, p), (s, s), d
    (2, 5, 7, (7, 9), (3, 3), (2, 2), (1, 1), 2), (1, 3, 4, (5, 6), (3, 3), (12, 12), (1, 1), 12), (1, 4, 6, (11, 13), (3, 3), (0, 0), (1, 1), 4),
    (1, 3, 5, (9, 10), (5, 5), (4, 4), (1, 1), 2), (2, 2, 3, (8, 7), (2, 2), (0, 0), (1, 1), 3), (1, 4, 4, (6, 5), (1, 1), (0, 0), (1, 1), 3),
    (1, 5, 6, (7, 9), (3, 3), (1, 1), (1, 1), 1), (2, 3, 4, (11, 9), (3, 3), (2, 2), (2, 2), 2), (1, 4, 5, (13, 11), (3, 3), (1, 1), (2, 2), 3),
    (1, 3, 3, (9, 9), (3, 3), (1, 1), (1, 1), 4),
]


@pytest.mark.parametrize("n,ci,co,hw,k,pad,s,d", CASES)
def test_forward_and_gradients_match_torch_float64(n, ci, co, hw, k, pad, s, d):
    rng = np.random.default_rng(hw[0] * 100 + hw[1] + 7 * k[0] + k[1] + d)
    h, w = hw
    x = rng.standard_normal((n, ci, h, w))
    wt = rng.standard_normal((co, ci) + k)
    b = rng.standard_normal(co)
    tx, tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, wt, b))
    ty = F.conv2d(tx, tw, tb, stride=s, padding=pad, dilation=d)
    y = R.conv2d(x, wt, b, pad, s, d)
    assert y.shape == tuple(ty.shape) == (n, co) + R.out_hw(h, w, k[0], k[1], pad, s, d)
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-12, atol=1e-12)
    dy = rng.standard_normal(y.shape)
    ty.backward(torch.tensor(dy))
    np.testing.assert_allclose(R.dgrad(dy, wt, pad, s, d, h, w), tx.grad.numpy(), rtol=1e-12, atol=1e-12)
    dw, db = R.wgrad(x, dy, k[0], k[1], pad, s, d)
    np.testing.assert_allclose(dw, tw.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(db, tb.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_a_square_problem_is_the_dense_reference():
    rng = np.random.default_rng(3)
    x, wt, b = rng.standard_normal((2, 4, 8, 9)), rng.standard_normal((5, 4, 3, 3)), rng.standard_normal(5)
    assert np.array_equal(R.conv2d(x, wt, b, (1, 1), (2, 2), 1), ref64.conv2d(x, wt, b, 1, 2))
    dy = rng.standard_normal((2, 5, 4, 5))
    assert np.array_equal(R.dgrad(dy, wt, (1, 1), (2, 2), 1, 8, 9), ref64.conv2d_dgrad(dy, wt, 1, 2, 8, 9))
    assert np.array_equal(R.wgrad(x, dy, 3, 3, (1, 1), (2, 2), 1)[0], ref64.conv2d_wgrad(x, dy, 3, 1, 2)[0])


@pytest.mark.parametrize("k,pad,d", [((1, 7), (0, 3), 1), ((7, 1), (3, 0), 1), ((3, 1), (2, 0), 2), ((2, 3), (0, 2), 2), ((3, 5), (2, 1), 1),
                                     ((1, 3), (0, 0), 2), ((3, 3), (1, 2), 1),
                                     ((3, 3), (2, 2), 2), ((3, 3), (1, 1), 4), ((5, 5), (4, 4), 2)])      # square dilated layers
def test_the_data_gradient_is_the_convolution_with_the_flipped_bank(k, pad, d):
    """What the engine does for a stride-1 layer: dX = rconv(dY, flipped bank, ph' = d (kh-1) - ph, pw' = d (kw-1) - pw, the same d),
    on a non-square image, with kh != kw or ph != pw - and with equal axes, the square dilated layer."""
    rng = np.random.default_rng(k[0] * 10 + k[1] + d)
    h, w = 9, 11
    wt = rng.standard_normal((6, 4) + k)
    dy = rng.standard_normal((2, 6) + R.out_hw(h, w, k[0], k[1], pad, (1, 1), d))
    via = R.conv2d(dy, R.flipped_bank(wt), None, R.flipped_pad(k[0], k[1], pad, d), (1, 1), d)
    assert via.shape == (2, 4, h, w)
    np.testing.assert_allclose(via, R.dgrad(dy, wt, pad, (1, 1), d, h, w), rtol=1e-12, atol=1e-12)


def test_magnitude_forms_bound_the_values():
    rng = np.random.default_rng(5)
    x, wt, b = rng.standard_normal((1, 3, 7, 8)), rng.standard_normal((4, 3, 1, 5)), rng.standard_normal(4)
    assert np.all(R.conv2d_mag(x, wt, b, (0, 2), (1, 1), 1) >= np.abs(R.conv2d(x, wt, b, (0, 2), (1, 1), 1)))
    dy = rng.standard_normal((1, 4, 7, 8))
    assert np.all(R.dgrad_mag(dy, wt, (0, 2), (1, 1), 1, 7, 8) >= np.abs(R.dgrad(dy, wt, (0, 2), (1, 1), 1, 7, 8)))
    assert np.all(R.wgrad_mag(x, dy, 1, 5, (0, 2), (1, 1), 1)[0] >= np.abs(R.wgrad(x, dy, 1, 5, (0, 2), (1, 1), 1)[0]))


def test_magnitude_forms_bound_the_values_of_a_square_dilated_layer():
    """k3 d2 p2 on 7 x 7, equal axes."""
    rng = np.random.default_rng(5)
    x, wt, b = rng.standard_normal((1, 3, 7, 7)), rng.standard_normal((4, 3, 3, 3)), rng.standard_normal(4)
    assert np.all(R.conv2d_mag(x, wt, b, (2, 2), (1, 1), 2) >= np.abs(R.conv2d(x, wt, b, (2, 2), (1, 1), 2)))
    dy = rng.standard_normal((1, 4, 7, 7))
    assert np.all(R.dgrad_mag(dy, wt, (2, 2), (1, 1), 2, 7, 7) >= np.abs(R.dgrad(dy, wt, (2, 2), (1, 1), 2, 7, 7)))
    assert np.all(R.wgrad_mag(x, dy, 3, 3, (2, 2), (1, 1), 2)[0] >= np.abs(R.wgrad(x, dy, 3, 3, (2, 2), (1, 1), 2)[0]))
