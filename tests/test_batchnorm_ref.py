"""tests/ref_batchnorm64.py against torch in float64: F.batch_norm in training and eval mode gives the normalisation and - through autograd -
the backward of the fused chain; the Caffe-style sum / factor update is held to a hand-written recurrence over three steps."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_batchnorm64 as R


def _case(seed, shape=(3, 5, 4, 6)):
    rng = np.random.default_rng(seed)
    n, c, h, w = shape
    x = rng.standard_normal(shape) * 2.0 + rng.standard_normal((1, c, 1, 1)) * 3.0
    return x, rng.standard_normal(c) + 1.5, rng.standard_normal(c), rng.standard_normal(shape), rng


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("scale", [False, True])
def test_batch_statistics_forward_and_backward(scale, relu):
    x, gamma, beta, dy, _ = _case(1)
    eps = 1e-5
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True) if scale else None
    bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True) if scale else None
    yt = F.batch_norm(xt, None, None, gt, bt, True, 0.1, eps)
    if relu:
        yt = torch.relu(yt)
    yt.backward(torch.tensor(dy))
    mean, var = R.batch_stats(x)
    y, xhat, inv = R.chain_fwd(x, mean, var, eps, gamma if scale else None, beta if scale else None, relu)
    assert np.allclose(y, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
    dx = R.chain_bwd(dy, xhat, inv, gamma if scale else None, y if relu else None, batch=True)
    assert np.allclose(dx, xt.grad.numpy(), rtol=1e-10, atol=1e-12)
    if scale:
        dbeta, dgamma = R.chain_sums(dy, xhat, y if relu else None)
        assert np.allclose(dbeta, bt.grad.numpy(), rtol=1e-11, atol=1e-12) and np.allclose(dgamma, gt.grad.numpy(), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("factor", [0.0, 2.5])
def test_global_statistics_forward_and_backward(factor):
    x, gamma, beta, dy, rng = _case(2)
    c = x.shape[1]
    b0, b1 = rng.standard_normal(c), rng.random(c) + 0.5
    mean, var = R.global_stats(b0, b1, [factor])
    if factor == 0.0:
        assert np.all(mean == 0) and np.all(var == 0)
    else:
        assert np.allclose(mean, b0 / factor) and np.allclose(var, b1 / factor)
    eps = 1e-3
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = torch.relu(F.batch_norm(xt, torch.tensor(mean), torch.tensor(var), torch.tensor(gamma), torch.tensor(beta), False, 0.1, eps))
    yt.backward(torch.tensor(dy))
    y, xhat, inv = R.chain_fwd(x, mean, var, eps, gamma, beta, True)
    assert np.allclose(y, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.chain_bwd(dy, xhat, inv, gamma, y, batch=False), xt.grad.numpy(), rtol=1e-11, atol=1e-12)


def test_scale_alone():
    x, gamma, beta, dy, _ = _case(3, (2, 3, 1, 1))
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    gt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (gamma, beta))
    (xt * gt.view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)).backward(torch.tensor(dy))
    y, xhat, inv = R.chain_fwd(x, gamma=gamma, beta=beta)
    assert np.array_equal(xhat, x) and np.allclose(y, x * gamma.reshape(1, -1, 1, 1) + beta.reshape(1, -1, 1, 1))
    dbeta, dgamma = R.chain_sums(dy, xhat)
    assert np.allclose(R.chain_bwd(dy, xhat, inv, gamma, batch=False), xt.grad.numpy())
    assert np.allclose(dbeta, bt.grad.numpy()) and np.allclose(dgamma, gt.grad.numpy())


@pytest.mark.parametrize("shape", [(2, 3, 4, 4), (1, 3, 1, 1)])
def test_moving_average_recurrence_over_three_steps(shape):
    """blob2 = blob2 f + 1, blob0 = blob0 f + mean, blob1 = blob1 f + var * (m / (m - 1) if m > 1 else 1); with m = 1 the variance enters
    as it is (zero).  After three steps the global statistics are the geometric-weight averages of the batches' statistics."""
    rng = np.random.default_rng(4)
    f = 0.9
    c = shape[1]
    m = shape[0] * shape[2] * shape[3]
    b0, b1, b2 = np.zeros(c), np.zeros(c), np.zeros(1)
    assert R.global_stats(b0, b1, b2)[0].tolist() == [0.0] * c      # factor == 0: the scale is 0, not 1 / 0
    means, uvars = [], []
    for _ in range(3):
        x = rng.standard_normal(shape) + 2.0
        mean, var = R.batch_stats(x)
        assert np.allclose(mean, x.mean(axis=(0, 2, 3))) and np.allclose(var, x.var(axis=(0, 2, 3)))
        b0, b1, b2 = R.moving_average_step(b0, b1, b2, mean, var, m, f)
        means.append(mean)
        uvars.append(x.var(axis=(0, 2, 3), ddof=1) if m > 1 else var)
    wts = np.array([f * f, f, 1.0])
    assert np.allclose(b2, wts.sum())
    assert np.allclose(b0, sum(w * v for w, v in zip(wts, means))) and np.allclose(b1, sum(w * v for w, v in zip(wts, uvars)))
    gm, gv = R.global_stats(b0, b1, b2)
    assert np.allclose(gm, sum(w * v for w, v in zip(wts, means)) / wts.sum())
    if m == 1:
        assert np.all(gv == 0)
