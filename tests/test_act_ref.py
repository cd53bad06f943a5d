"""tests/ref_act64.py against torch and autograd in float64, and proof that the guarded cases can fail - without a GPU.

The reference of tests/test_gpu_guarded_act.py is held to torch.nn.functional.prelu, torch.tanh and a broadcast add, and every gradient
(data, slopes, bias, the shared slope) to autograd.  Then, for every case of tests/act_cases.py, the mistakes a kernel of this kind can
make are made on purpose in numpy, and the wrong result must miss the true one by more than 100 x the tolerance of the GPU test
(rel_err < 1e-4): a case that such a kernel would pass checks nothing.
  - the slope (bias) of channel c applied to channel c + 1;
  - the shared slope taken per channel: a vector read where one value stands, and the per-channel sums left unfolded;
  - the boundary at zero.  In the SLOPE gradient `x <= 0` and `x < 0` give the same sum, bit for bit: an exact zero contributes
    dy * 0 either way (shown below), so no test could tell them apart there and none pretends to.  Where the boundary does count is
    the data gradient, `x > 0` taken as `x >= 0` (dy instead of a * dy at a zero): that one is caught, on inputs a quarter of which are
    exact zeros;
  - the pixel sum cut at the first slab;
  - the data gradient read from y instead of the kept x, with negative slopes so that the signs differ.
Last, every forward is evaluated independently in numpy float32 on operands rounded to half and rounded to half once: that result
lies inside the half-float allowances of the GPU test, so those allowances admit a correct implementation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import act_cases as AC
import ref64
import ref_act64 as R

TOL = 1e-4      # the project's rel_err bound for float32 results (tests/test_gpu_guarded_act.py)
FAR = 100 * TOL
CASES = pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


@CASES
@pytest.mark.parametrize("shared", [False, True])
def test_prelu_is_what_torch_and_autograd_compute(case, shared):
    x, a, _b, dy, dx0 = AC.operands(case)
    p = np.array([AC.SHARED_SLOPE], np.float32) if shared else a
    tx, tp = t64(x, True), t64(p, True)
    y = F.prelu(tx, tp)
    y.backward(t64(dy))
    assert R.rel_err(R.fwd(R.PRELU, x, p, shared), y.detach().numpy()) < 1e-14
    # torch takes the subgradient 0-side at x == 0 as the definitions above do: a * dy, and dy * 0 for the slope
    assert R.rel_err(R.bwd_data(R.PRELU, dy, x, p, shared), tx.grad.numpy()) < 1e-14
    assert R.rel_err(R.bwd_data(R.PRELU, dy, x, p, shared, dx0), tx.grad.numpy() + dx0) < 1e-14
    assert R.rel_err(R.bwd_param(R.PRELU, dy, x, shared), tp.grad.numpy()) < 1e-12
    assert R.bwd_param(R.PRELU, dy, x, shared).shape == ((1,) if shared else (case[1],))


@CASES
def test_tanh_and_bias_are_what_torch_and_autograd_compute(case):
    x, _a, b, dy, dx0 = AC.operands(case)
    tx = t64(x, True)
    y = torch.tanh(tx)
    y.backward(t64(dy))
    y64 = R.fwd(R.TANH, x)
    assert R.rel_err(y64, y.detach().numpy()) < 1e-14
    assert R.rel_err(R.bwd_data(R.TANH, dy, y64), tx.grad.numpy()) < 1e-13
    assert R.rel_err(R.bwd_data(R.TANH, dy, y64, dx_old=dx0), tx.grad.numpy() + dx0) < 1e-13
    tx, tb = t64(x, True), t64(b, True)
    y = tx + tb.reshape(1, -1, 1, 1)
    y.backward(t64(dy))
    assert R.rel_err(R.fwd(R.BIAS, x, b), y.detach().numpy()) < 1e-14
    assert np.array_equal(R.bwd_data(R.BIAS, dy), tx.grad.numpy()) and R.rel_err(R.bwd_data(R.BIAS, dy, dx_old=dx0), tx.grad.numpy() + dx0) < 1e-14
    assert R.rel_err(R.bwd_param(R.BIAS, dy), tb.grad.numpy()) < 1e-12


@pytest.mark.parametrize("case", AC.CASES + AC.ODD_C, ids=AC.case_id)
def test_the_parameter_of_the_neighbouring_channel_is_caught(case):
    x, a, b, dy, _dx0 = AC.operands(case)
    assert R.rel_err(R.fwd(R.PRELU, x, np.roll(a, 1)), R.fwd(R.PRELU, x, a)) > FAR
    assert R.rel_err(R.bwd_data(R.PRELU, dy, x, np.roll(a, 1)), R.bwd_data(R.PRELU, dy, x, a)) > FAR
    assert R.rel_err(np.roll(R.bwd_param(R.PRELU, dy, x), 1), R.bwd_param(R.PRELU, dy, x)) > FAR
    assert R.rel_err(R.fwd(R.BIAS, x, np.roll(b, 1)), R.fwd(R.BIAS, x, b)) > FAR
    assert R.rel_err(np.roll(R.bwd_param(R.BIAS, dy), 1), R.bwd_param(R.BIAS, dy)) > FAR


@pytest.mark.parametrize("case", AC.CASES + AC.ODD_C, ids=AC.case_id)
def test_the_shared_slope_taken_per_channel_is_caught(case):
    x, a, _b, dy, _dx0 = AC.operands(case)
    one = np.array([AC.SHARED_SLOPE], np.float32)
    vec = a.copy()
    vec[0] = AC.SHARED_SLOPE                    # what a lane finds at param[c] when it should read param[0]: anything but the slope
    assert R.rel_err(R.fwd(R.PRELU, x, vec), R.fwd(R.PRELU, x, one, True)) > FAR
    assert R.rel_err(R.bwd_data(R.PRELU, dy, x, vec), R.bwd_data(R.PRELU, dy, x, one, True)) > FAR
    # the per-channel sums left unfolded: channel 0's sum where the sum over all channels belongs
    assert R.rel_err(R.bwd_param(R.PRELU, dy, x)[:1], R.bwd_param(R.PRELU, dy, x, True)) > FAR
    assert R.rel_err(R.bwd_param(R.BIAS, dy)[:1], R.bwd_param(R.BIAS, dy, shared=True)) > FAR


@CASES
def test_the_boundary_at_zero(case):
    x, a, _b, dy, _dx0 = AC.operands(case)
    assert (x == 0.0).any() and (x < 0.0).any()
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    # the slope gradient cannot tell `x <= 0` from `x < 0`: the terms at the zeros are dy * 0
    assert np.array_equal((dy64 * x64 * (x64 < 0.0)).sum(axis=(0, 2, 3)), R.bwd_param(R.PRELU, dy, x))
    # the data gradient can: dy where a * dy belongs
    wrong = np.where(x64 >= 0.0, dy64, a.astype(np.float64).reshape(1, -1, 1, 1) * dy64)
    assert R.rel_err(wrong, R.bwd_data(R.PRELU, dy, x, a)) > FAR
    wrong = np.where(x64 >= 0.0, dy64, AC.SHARED_SLOPE * dy64)
    assert R.rel_err(wrong, R.bwd_data(R.PRELU, dy, x, [AC.SHARED_SLOPE], True)) > FAR


@pytest.mark.parametrize("case", [c for c in AC.CASES if AC.crosses_a_slab(c)], ids=AC.case_id)
def test_a_pixel_sum_cut_at_the_first_slab_is_caught(case):
    p, c = case
    x, _a, _b, dy, _dx0 = AC.operands(case)
    keep = (np.arange(p) < AC.first_slab(c)).reshape(1, 1, 1, p)
    for shared in (False, True):
        assert R.rel_err(R.bwd_param(R.PRELU, dy * keep, x, shared), R.bwd_param(R.PRELU, dy, x, shared)) > FAR
        assert R.rel_err(R.bwd_param(R.BIAS, dy * keep, shared=shared), R.bwd_param(R.BIAS, dy, shared=shared)) > FAR


@CASES
def test_a_data_gradient_read_from_y_is_caught(case):
    x, a, _b, dy, _dx0 = AC.operands(case)
    for p, shared in ((a, False), (np.array([AC.SHARED_SLOPE], np.float32), True)):
        y = R.fwd(R.PRELU, x, p, shared)
        assert ((y > 0) != (x > 0)).any()       # a negative slope turns a negative input into a positive output
        assert R.rel_err(R.bwd_data(R.PRELU, dy, y, p, shared), R.bwd_data(R.PRELU, dy, x, p, shared)) > FAR


def half_allowance(mode, y64, mag):
    """The allowances of tests/test_gpu_guarded_act.py.  PReLU and Bias: one float32 rounding on the magnitude, half an ulp of the half
    for the store, half the subnormal spacing.  TanH: faithful rounding - within one ulp of the half - of the float64 value, which any
    float32 tanh accurate to 2^-12 meets: half an ulp for the store plus the function's own error, which then is below another half."""
    if mode == R.TANH:
        return 2 * ref64.U16 * np.abs(y64) + 2.0 ** -24
    return ref64.U32 * mag + ref64.U16 * np.abs(y64) + 2.0 ** -24


def half_magnitude(mode, x64, p64, shared):
    """|y| for PReLU (one product), |x| + |b| for Bias (one sum)."""
    if mode == R.BIAS:
        return np.abs(x64) + np.abs(p64).reshape(1, -1, 1, 1)
    return np.abs(R.fwd(mode, x64, p64, shared)) if mode == R.PRELU else None


@pytest.mark.parametrize("case", AC.CASES + AC.ODD_C, ids=AC.case_id)
def test_the_half_float_allowances_admit_a_float32_evaluation(case):
    x, a, b, _dy, _dx0 = AC.operands(case)
    xh = x.astype(np.float16)
    x32, x64 = xh.astype(np.float32), xh.astype(np.float64)
    for mode, p, shared in ((R.PRELU, a, False), (R.PRELU, np.array([AC.SHARED_SLOPE], np.float32), True), (R.TANH, None, False), (R.BIAS, b, False)):
        if mode == R.TANH:
            y32 = np.tanh(x32)
        else:
            p32 = np.full(case[1], p[0], np.float32).reshape(1, -1, 1, 1) if shared else p.reshape(1, -1, 1, 1)
            y32 = np.where(x32 > 0, x32, p32 * x32) if mode == R.PRELU else x32 + p32
        assert y32.dtype == np.float32
        y16 = y32.astype(np.float16)
        y64 = R.fwd(mode, x64, p, shared)
        ratio, at = ref64.worst(y16, y64, half_allowance(mode, y64, half_magnitude(mode, x64, None if p is None else p.astype(np.float64), shared)))
        assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (mode, at, ratio)


def test_the_cases_cover_what_they_claim():
    assert {c for _p, c in AC.CASES} == {6, 8, 10, 20, 68} and {1, 5, 49, 300} <= {p for p, _c in AC.CASES}
    assert [AC.first_slab(c) for c in (6, 8, 10, 20, 68)] == [128, 128, 64, 32, 16]
    for c in (6, 10, 20, 68):                   # one count on each side of the slab boundary
        assert (AC.first_slab(c), c) in AC.CASES and (AC.first_slab(c) + 1, c) in AC.CASES
        assert AC.slabs((AC.first_slab(c), c)) == 1 and AC.slabs((AC.first_slab(c) + 1, c)) == 2
    assert sorted(AC.slabs(c) for c in AC.CASES if AC.slabs(c) > 64) == [66, 66]
    assert sorted(c for _p, c in AC.ODD_C) == [3, 5, 7, 13] and not set(AC.ODD_C) & set(AC.CASES)
    x, a, _b, _dy, _dx0 = AC.operands(AC.CASES[3])
    assert (a < 0).any() and (a > 0).any() and (a == 0).any() and AC.SHARED_SLOPE < 0 and 0.15 < (x == 0).mean() < 0.35
