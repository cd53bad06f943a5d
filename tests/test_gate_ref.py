"""tests/ref_gate64.py against torch autograd in float64, and proof that the guarded cases can fail - without a GPU.

The reference of tests/test_gpu_guarded_gate.py is held to (x * g[:, :, None, None] + r).relu() and its gradients to x and g as autograd
computes them.  Then, for every case of tests/gate_cases.py, the two mistakes a kernel of this kind can make are made on purpose in
numpy - the gate of image 0 used for every image, and the pixel sum of the gate gradient cut at the first slab - and the wrong result
must miss the true one by far more than the tolerance of the GPU test (rel_err < 1e-4): a case that such a kernel would pass checks
nothing."""
import numpy as np
import pytest
import torch

import gate_cases as GC
import ref_gate64 as R

TOL = 1e-4      # the project's rel_err bound for float32 results (tests/test_gpu_guarded_gate.py)


@pytest.mark.parametrize("shape", GC.SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_the_reference_is_what_autograd_computes(shape, relu):
    x, g, r, dy, dx0, dg0 = GC.operands(shape)
    tx, tg, tr = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, g, r))
    y = tx * tg[:, :, None, None] + tr
    y = y.relu() if relu else y
    y.backward(torch.tensor(dy, dtype=torch.float64))
    y64 = R.gate_fwd(x, g, r, relu)
    assert R.rel_err(y64, y.detach().numpy()) < 1e-14
    # the layers above hand the gate dy under the ReLU's mask; the residual's gradient is that masked dy itself
    dym = dy * R.relu_mask(y64) if relu else dy.astype(np.float64)
    assert R.rel_err(R.gate_bwd_data(dym, g), tx.grad.numpy()) < 1e-14
    assert R.rel_err(R.gate_bwd_gate(dym, x), tg.grad.numpy()) < 1e-13
    assert R.rel_err(dym, tr.grad.numpy()) < 1e-14
    # without the residual, and accumulating into gradients that already hold something
    assert np.array_equal(R.gate_fwd(x, g), x.astype(np.float64) * g.astype(np.float64)[:, :, None, None])
    assert R.rel_err(R.gate_bwd_data(dym, g, dx0), tx.grad.numpy() + dx0) < 1e-14
    assert R.rel_err(R.gate_bwd_gate(dym, x, dg0), tg.grad.numpy() + dg0) < 1e-13


@pytest.mark.parametrize("shape", GC.SHAPES + GC.ODD_SHAPES)
def test_the_gate_of_image_0_for_every_image_is_caught(shape):
    x, g, r, dy, _dx0, _dg0 = GC.operands(shape)
    wrong = np.broadcast_to(g[:1], g.shape)
    assert R.rel_err(R.gate_fwd(x, wrong, r, True), R.gate_fwd(x, g, r, True)) > 100 * TOL
    assert R.rel_err(R.gate_fwd(x, wrong), R.gate_fwd(x, g)) > 100 * TOL
    assert R.rel_err(R.gate_bwd_data(dy, wrong), R.gate_bwd_data(dy, g)) > 100 * TOL
    # the gate gradient of image n from the pixels of image 0
    assert R.rel_err(np.broadcast_to(R.gate_bwd_gate(dy[:1], x[:1]), g.shape), R.gate_bwd_gate(dy, x)) > 100 * TOL


@pytest.mark.parametrize("shape", [s for s in GC.SHAPES if GC.crosses_a_slab(s)])
def test_a_pixel_sum_cut_at_the_first_slab_is_caught(shape):
    n, h, w, c = shape
    x, _g, _r, dy, _dx0, _dg0 = GC.operands(shape)
    keep = (np.arange(h * w) < GC.first_slab(c)).reshape(1, 1, h, w)
    assert R.rel_err(R.gate_bwd_gate(dy * keep, x), R.gate_bwd_gate(dy, x)) > 100 * TOL


def test_the_cases_cover_what_they_claim():
    assert {s[0] for s in GC.SHAPES} == {2, 3} and {s[1] * s[2] for s in GC.SHAPES} == {1, 5, 49, 300} and {s[3] for s in GC.SHAPES} == {6, 8, 20, 68}
    assert [GC.first_slab(c) for c in (6, 8, 20, 68)] == [128, 128, 32, 16]
    crossing = [s for s in GC.SHAPES if GC.crosses_a_slab(s)]
    assert {s[3] for s in crossing} == {6, 8, 20, 68} and {s[1] * s[2] for s in crossing} == {49, 300}
    assert [(s[0], s[1] * s[2], s[3]) for s in GC.ODD_SHAPES] == [(2, 5, 5), (2, 49, 13), (2, 5, 7), (2, 49, 3)]
