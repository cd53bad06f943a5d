"""The float64 InnerProduct reference (tests/ref_ip64.py) against torch.nn.functional.linear / autograd in float64 (no GPU)."""
import numpy as np
import pytest
import torch

import ref_ip64 as R
from fcn_object_detector_amd.storage import ip_pack_bank, ip_unpack_bank


@pytest.mark.parametrize("shape,n", [((3, 20), 7), ((2, 5, 3, 4), 6), ((1, 16, 1, 1), 4)])
def test_forward_and_gradients(shape, n):
    rng = np.random.default_rng(len(shape) + n)
    x, w, b = rng.standard_normal(shape), rng.standard_normal((n, int(np.prod(shape[1:])))), rng.standard_normal(n)
    dy = rng.standard_normal((shape[0], n))
    tx, tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b))
    ty = torch.nn.functional.linear(tx.reshape(shape[0], -1), tw, tb)
    ty.backward(torch.tensor(dy))
    assert np.allclose(R.forward(x, w, b), ty.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(R.forward(x, w, b, relu=True), np.maximum(R.forward(x, w, b), 0))
    assert np.allclose(R.bwd_data(dy, w), tx.grad.numpy().reshape(shape[0], -1), rtol=1e-12, atol=1e-12)
    gw, gb = R.bwd_weights(x, dy)
    assert np.allclose(gw, tw.grad.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(gb, tb.grad.numpy(), rtol=1e-12, atol=1e-12)
    gw2, gb2 = R.bwd_weights(x, dy, dw=gw, db=gb)
    assert np.allclose(gw2, 2 * gw) and np.allclose(gb2, 2 * gb) and np.allclose(R.bwd_data(dy, w, dx=R.bwd_data(dy, w)), 2 * R.bwd_data(dy, w))


@pytest.mark.parametrize("c,h,w,cs,co", [(5, 3, 4, 8, 0), (6, 2, 2, 6, 0), (4, 3, 3, 16, 8), (3, 1, 1, 4, 0)])
def test_bank_permutation(c, h, w, cs, co):
    """A row of the NHWC device blob times the packed bank equals the (c, h, w) product, whatever the pad channels and the
    neighbours of a Concat member hold."""
    rng = np.random.default_rng(c * h + cs)
    x, bank = rng.standard_normal((2, c, h, w)), rng.standard_normal((5, c * h * w))
    rows = rng.standard_normal((2, h, w, cs)) * 1e3          # garbage outside the slice
    rows[..., co:co + c] = x.transpose(0, 2, 3, 1)
    p = R.pack_bank(bank, c, h, w, cs, co)
    assert p.shape == (5, h * w * cs) and np.count_nonzero(p) == bank.size
    assert np.allclose(rows.reshape(2, -1) @ p.T, R.forward(x, bank), rtol=1e-12, atol=1e-12)
    assert np.array_equal(R.unpack_bank(p, c, h, w, cs, co), bank)
    if co == 0:      # the engine's own packing (whole buffers only) is this permutation, in both element types, and inverts exactly
        b32 = bank.astype(np.float32)
        assert np.array_equal(ip_pack_bank(b32, c, h, w, cs), R.pack_bank(b32, c, h, w, cs))
        assert np.array_equal(ip_pack_bank(b32, c, h, w, cs, np.float16), R.pack_bank(b32, c, h, w, cs).astype(np.float16))
        assert np.array_equal(ip_unpack_bank(ip_pack_bank(b32, c, h, w, cs), c, h, w, cs), b32)
