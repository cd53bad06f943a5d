"""tests/ref_neuron64.py against torch and autograd in float64, and proof that the guarded cases can fail - without a GPU.

The reference of tests/test_gpu_guarded_neuron.py is held to F.elu, clamp, abs, F.softplus and x * sigmoid(beta x), and every data
gradient to autograd - away from the kinks, where autograd picks a subgradient of its own: at the bounds of a Clip the layer's rule is
the strict one (zero), at x = 0 AbsVal gives zero; both are asserted here as the rule, element by element.
Then, for every case of tests/neuron_cases.py, the mistakes this code invites are made on purpose in numpy, and the wrong result must
miss the true one by more than 100 x the bound of the GPU test (rel_err < 1e-4): a case that such a kernel would pass checks nothing.
  - a gradient read from x where the layer reads y (ELU, BNLL), and from y where it reads x (AbsVal, Swish).  For a Clip the two are the
    same thing - lo < y < hi exactly when lo < x < hi - which is shown, not hidden;
  - non-strict Clip bounds: the gradient passed where y equals a bound;
  - sign(0) = 1;
  - beta left out of the Swish derivative (the configurations with beta != 1);
  - alpha taken as 1 (the ELU configurations with another alpha), forward and gradient.
Last, the half-float allowance of the GPU test.  Per element it is
    4 * EVAL32[mode] * 2^-24 * |y| + 2^-11 * |y| + 2^-24:
the float32 evaluation, half an ulp of the half for the store, half the subnormal spacing.  EVAL32 is not reasoned out but measured
here: the worst relative error, in units of 2^-24, of a numpy float32 evaluation of the layer's formula against the float64 reference
over all cases and configurations, on float32 operands and on operands rounded to half.  The factor 4 is there because the device's
expf / expm1f / log1pf are not numpy's.  The constants below are those measurements rounded up; the test asserts that a fresh
measurement stays under them, and that the allowance admits that float32 evaluation rounded to half."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import neuron_cases as NC
import ref64
import ref_neuron64 as R

TOL = 1e-4      # the project's rel_err bound for float32 results (tests/test_gpu_guarded_neuron.py)
FAR = 100 * TOL
CASES = pytest.mark.parametrize("case", NC.CASES, ids=NC.case_id)
# measured by test_eval32_is_what_a_float32_evaluation_measures (printed there), rounded up to the next half unit; Clip and AbsVal are exact
# (measured: ELU 3.029, BNLL 3.702, Swish 15.41 - the float32 rounding of beta = -1.3 times |beta x| up to 32.5 is most of the last one)
EVAL32 = {R.ELU: 3.5, R.CLIP: 0.0, R.ABSVAL: 0.0, R.BNLL: 4.0, R.SWISH: 15.5}


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def torch_fwd(mode, tx, a, b):
    if mode == R.ELU:
        return F.elu(tx, alpha=a)
    if mode == R.CLIP:
        return torch.clamp(tx, a, b)
    if mode == R.ABSVAL:
        return torch.abs(tx)
    if mode == R.BNLL:
        return F.softplus(tx, threshold=1e9)
    return tx * torch.sigmoid(a * tx)


@CASES
def test_the_reference_is_what_torch_and_autograd_compute(case):
    x, dy, dx0 = NC.operands(case)
    for name, mode, a, b in NC.CONFIGS:
        tx = t64(x, True)
        y = torch_fwd(mode, tx, a, b)
        y.backward(t64(dy))
        y64 = R.fwd(mode, x, a, b)
        assert R.rel_err(y64, y.detach().numpy()) < 1e-14, name
        x64 = x.astype(np.float64)
        kink = (x64 == a) | (x64 == b) if mode == R.CLIP else (x64 == 0.0) if mode in (R.ABSVAL, R.ELU) else np.zeros(x.shape, bool)
        dx = R.bwd(mode, dy, R.ref_of(mode, x, a, b), a, b)
        assert np.abs(dx - tx.grad.numpy())[~kink].max(initial=0.0) < 1e-13 * max(np.abs(dx).max(), 1.0), name
        if mode in (R.CLIP, R.ABSVAL):
            assert kink.any() and np.all(dx[kink] == 0.0), name      # the strict bounds; sign(0) = 0
        if mode == R.ELU:
            assert np.allclose(dx[kink], a * dy.astype(np.float64)[kink], rtol=1e-15, atol=0), name      # y = 0 is the alpha side
        assert R.rel_err(R.bwd(mode, dy, R.ref_of(mode, x, a, b), a, b, dx0), dx + dx0) < 1e-15, name


def test_bnll_far_from_zero_and_the_form_that_reads_y():
    """-expm1(-y) is Caffe's e / (e + 1) with e = exp(min(x, 50)); at very negative x it keeps every bit, and y itself is x to the last
    bit beyond +-40."""
    x = np.array([-700.0, -80.0, -30.0, -1.0, 0.0, 1.0, 30.0, 50.0, 80.0, 700.0])
    y = R.fwd(R.BNLL, x)
    e = np.exp(np.minimum(x, 50.0))
    assert np.allclose(R.bwd(R.BNLL, np.ones_like(x), y), e / (e + 1.0), rtol=1e-13, atol=0.0)
    assert y[0] == np.exp(-700.0) and y[-1] == 700.0 and y[4] == np.log(2.0)


@CASES
def test_a_gradient_read_from_the_wrong_blob_is_caught(case):
    x, dy, _dx0 = NC.operands(case)
    for name, mode, a, b in NC.CONFIGS:
        y = R.fwd(mode, x, a, b)
        right, wrong = (y, x) if R.READS[mode] == "y" else (x, y)
        err = R.rel_err(R.bwd(mode, dy, wrong, a, b), R.bwd(mode, dy, right, a, b))
        if mode == R.CLIP:
            assert err == 0.0, name      # (lo < y < hi exactly when lo < x < hi: nothing to tell apart)
        elif mode == R.SWISH and a == 0.0:
            assert err == 0.0, name      # (beta 0: the derivative is the constant 1 / 2)
        else:
            assert err > FAR, "%s: %.3g" % (name, err)


@CASES
def test_non_strict_clip_bounds_are_caught(case):
    x, dy, _dx0 = NC.operands(case)
    for name, mode, a, b in NC.CONFIGS:
        if mode != R.CLIP:
            continue
        y = R.fwd(mode, x, a, b)
        assert (x == a).any() and (x == b).any(), name
        wrong = dy.astype(np.float64) * ((y >= a) & (y <= b))
        assert R.rel_err(wrong, R.bwd(mode, dy, y, a, b)) > FAR, name
        one_side = dy.astype(np.float64) * ((y > a) & (y <= b))
        assert R.rel_err(one_side, R.bwd(mode, dy, y, a, b)) > FAR, name


@CASES
def test_sign_of_zero_taken_as_one_is_caught(case):
    x, dy, _dx0 = NC.operands(case)
    assert (x == 0.0).any()
    for s0 in (1.0, -1.0):
        wrong = dy.astype(np.float64) * np.where(x == 0.0, s0, np.sign(x.astype(np.float64)))
        assert R.rel_err(wrong, R.bwd(R.ABSVAL, dy, x)) > FAR


@CASES
def test_beta_left_out_of_the_swish_derivative_is_caught(case):
    x, dy, _dx0 = NC.operands(case)
    n = 0
    for name, mode, a, _b in NC.CONFIGS:
        if mode != R.SWISH or a == 1.0:
            continue
        x64 = x.astype(np.float64)
        s = 1.0 / (1.0 + np.exp(-a * x64))
        y = x64 * s
        wrong = dy * (y + s * (1.0 - y))
        assert R.rel_err(wrong, R.bwd(mode, dy, x, a)) > FAR, name
        n += 1
    assert n == 2


@CASES
def test_alpha_taken_as_one_is_caught(case):
    x, dy, _dx0 = NC.operands(case)
    n = 0
    for name, mode, a, _b in NC.CONFIGS:
        if mode != R.ELU or a == 1.0:
            continue
        y = R.fwd(mode, x, a)
        assert R.rel_err(R.fwd(mode, x, 1.0), y) > FAR, name
        assert R.rel_err(R.bwd(mode, dy, y, 1.0), R.bwd(mode, dy, y, a)) > FAR, name
        n += 1
    assert n == 2


def eval32(mode, x32, a, b):
    """The layer's formula in numpy float32, as the kernel writes it."""
    assert x32.dtype == np.float32
    a, b, one = np.float32(a), np.float32(b), np.float32(1.0)
    with np.errstate(over="ignore"):
        if mode == R.ELU:
            y = np.where(x32 > 0, x32, a * np.expm1(x32))
        elif mode == R.CLIP:
            y = np.minimum(np.maximum(x32, a), b)
        elif mode == R.ABSVAL:
            y = np.abs(x32)
        elif mode == R.BNLL:
            y = np.where(x32 > 0, x32 + np.log1p(np.exp(-x32)), np.log1p(np.exp(x32)))
        else:
            y = x32 / (one + np.exp(-a * x32))
    assert y.dtype == np.float32
    return y


def half_allowance(mode, y64):
    """The per-element allowance of a half result (see the module text)."""
    return (4.0 * EVAL32[mode] * ref64.U32 + ref64.U16) * np.abs(y64) + 2.0 ** -24


def test_eval32_is_what_a_float32_evaluation_measures():
    worst = {m: 0.0 for m in R.MODES}
    for case in NC.CASES + NC.ODD_C:
        x, _dy, _dx0 = NC.operands(case)
        for x32 in (x, x.astype(np.float16).astype(np.float32)):
            for _name, mode, a, b in NC.CONFIGS:
                y64 = R.fwd(mode, x32, a, b)
                err = np.abs(eval32(mode, x32, a, b).astype(np.float64) - y64)
                live = y64 != 0.0
                assert np.all(err[~live] == 0.0)
                worst[mode] = max(worst[mode], float((err[live] / np.abs(y64[live])).max(initial=0.0) / ref64.U32))
    print("EVAL32 measured (units of 2^-24): %s" % {m: round(v, 3) for m, v in worst.items()})
    for m in R.MODES:
        assert worst[m] <= EVAL32[m], (m, worst[m])
        assert EVAL32[m] <= worst[m] + 0.5, "%s: the constant %.1f is not the measurement %.3f rounded up" % (m, EVAL32[m], worst[m])


@pytest.mark.parametrize("case", NC.CASES + NC.ODD_C, ids=NC.case_id)
def test_the_half_float_allowance_admits_a_float32_evaluation(case):
    x, _dy, _dx0 = NC.operands(case)
    x32 = x.astype(np.float16).astype(np.float32)
    for name, mode, a, b in NC.CONFIGS:
        y16 = eval32(mode, x32, a, b).astype(np.float16)
        y64 = R.fwd(mode, x32, a, b)
        ratio, at = ref64.worst(y16, y64, half_allowance(mode, y64))
        assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (name, at, ratio)


def test_the_cases_cover_what_they_claim():
    assert {c for _p, c in NC.CASES} == {6, 8, 10, 20, 68} and {p for p, _c in NC.CASES} == {1, 5, 49, 300} and len(NC.CASES) == 20
    assert all(c % 2 == 1 for _p, c in NC.ODD_C)
    for case in NC.CASES + NC.ODD_C:
        x, dy, _dx0 = NC.operands(case)
        if case[0] * case[1] >= 6:
            assert all((x == v).any() for v in NC.SPECIAL), case
        assert np.all(x.astype(np.float16).astype(np.float32)[np.isin(x, NC.SPECIAL)] == x[np.isin(x, NC.SPECIAL)])
        assert not (dy == 0.0).any()
    x, _dy, _dx0 = NC.operands((300, 20))
    assert (np.abs(x) > 20).any() and ((x > 0) & (x < 6)).any() and ((x > -3.5) & (x < -0.5)).any() and 0.4 < np.isin(x, NC.SPECIAL).mean() < 0.6
    modes = {m for _n, m, _a, _b in NC.CONFIGS}
    assert modes == set(R.MODES)
    assert any(m == R.SWISH and a < 0 for _n, m, a, _b in NC.CONFIGS) and any(m == R.SWISH and a == 0 for _n, m, a, _b in NC.CONFIGS)
    assert any(m == R.ELU and a == 0 for _n, m, a, _b in NC.CONFIGS) and any(m == R.CLIP and b < 0 for _n, m, _a, b in NC.CONFIGS)
    # the grid-stride loop: one trip in every small case, two in the two large ones
    assert all(NC.trips(p, c, 4) == 1 and NC.trips(p, c, 8) == 1 for p, c in NC.CASES + NC.ODD_C)
    assert NC.trips(*NC.TRIP_F32, 4) == 2 and NC.trips(NC.TRIP_F32[0] - 21, 68, 4) == 1 and NC.tile(*NC.TRIP_F32, 4)[:3] == (16, 16, 2)
    assert NC.trips(*NC.TRIP_F16, 8) == 2 and NC.trips(NC.TRIP_F16[0] - 21, 68, 8) == 1 and NC.tile(*NC.TRIP_F16, 8)[:3] == (16, 16, 1)
    assert NC.TRIP_F32[0] * 76 * 4 < 6 << 20 and NC.TRIP_F16[0] * 88 * 2 < 6 << 20
