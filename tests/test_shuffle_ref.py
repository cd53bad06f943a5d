"""tests/ref_shuffle64.py - the numpy reference of the ShuffleChannel layer - against torch, and the cases of tests/shuffle_cases.py on the
reference alone (no GPU): each of them can fail.

The reference against `reshape -> transpose -> reshape` in torch float64 and its gradient against autograd.  Then, for every guarded case
and every pixel count it runs at: the operands have no two equal channels in a pixel; the result differs from the one with g and C / g
swapped (the inverse permutation) - in every case but the two self-inverse ones, (9, 3) and (16, 4), and the two identity cases - and from the input (the identity)
- in every case but the two identity cases; a gradient computed with the accumulate flag ignored differs from the right one."""
import numpy as np
import pytest
import torch

import ref_shuffle64 as R
import shuffle_cases as SC

CASES = pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)


def torch_shuffle(x: torch.Tensor, g: int) -> torch.Tensor:
    n, c = x.shape[:2]
    rest = tuple(x.shape[2:])
    return x.reshape((n, g, c // g) + rest).transpose(1, 2).reshape((n, c) + rest)


@CASES
@pytest.mark.parametrize("shape", [(2, 3, 5), (3,)], ids=["4-d", "2-d"])
def test_the_reference_is_torchs_reshape_transpose_reshape_and_its_gradient_autograds(case, shape):
    c, g = case
    rng = np.random.default_rng(c * 31 + g)
    full = (shape[0], c) + tuple(shape[1:])
    x, dy, dx0 = (rng.standard_normal(full) for _ in range(3))
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = torch_shuffle(xt, g)
    assert np.array_equal(R.fwd(x, g), yt.detach().numpy())
    yt.backward(torch.tensor(dy))
    assert np.array_equal(R.bwd(dy, g), xt.grad.numpy())
    assert np.array_equal(R.bwd(dy, g, dx0), dx0 + xt.grad.numpy())
    assert np.array_equal(R.bwd(dy, g), R.fwd(dy, c // g))      # the gradient is the forward launch with group C / g
    assert np.array_equal(R.bwd(R.fwd(x, g), g), x)


def test_the_formula_on_a_case_written_out():
    x = np.arange(6, dtype=np.float32).reshape(1, 6, 1, 1)
    assert R.fwd(x, 3).reshape(-1).tolist() == [0, 2, 4, 1, 3, 5]      # y[j * 3 + i] = x[i * 2 + j]
    assert R.fwd(x, 2).reshape(-1).tolist() == [0, 3, 1, 4, 2, 5]
    assert R.source(6, 3).tolist() == [0, 2, 4, 1, 3, 5]
    with pytest.raises(ValueError):
        R.source(6, 4)
    with pytest.raises(ValueError):
        R.source(6, 0)


@CASES
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_every_guarded_case_can_fail(case, half):
    c, g = case
    dt = np.float16 if half else np.float32
    for p in SC.pixel_counts(c, 8 if half else 4):
        x, y0 = SC.operands(p, c, dt)
        assert x.dtype == dt and np.array_equal(x.astype(np.float64), SC.operands(p, c, np.float64)[0])      # exact in the element type
        flat = x.reshape(c, p)
        assert all(len(set(flat[:, q].tolist())) == c for q in range(p)), "two channels of a pixel are equal"
        y = R.fwd(x, g)
        assert y.dtype == dt
        if case in SC.IDENTITY:
            assert np.array_equal(y, x)
            continue
        assert not np.array_equal(y, x), "the case cannot tell the shuffle from the identity"
        # ... in every pixel, not only somewhere
        assert all(not np.array_equal(y.reshape(c, p)[:, q], flat[:, q]) for q in range(p))
        if case in SC.SELF_INVERSE:
            assert g * g == c and np.array_equal(y, R.fwd(x, c // g))
        else:
            assert g != c // g and not np.array_equal(y, R.fwd(x, c // g)), "the case cannot tell the permutation from its inverse"
            assert all(not np.array_equal(y.reshape(c, p)[:, q], R.fwd(x, c // g).reshape(c, p)[:, q]) for q in range(p))
        if not half:
            dx, plain = R.bwd(x, g, y0), R.bwd(x, g)
            assert not np.array_equal(dx, plain) and not np.array_equal(dx, y0), "the case cannot tell an ignored accumulate flag"
            assert np.array_equal(dx.astype(np.float64), y0.astype(np.float64) + plain.astype(np.float64))      # the sum is exact in float32


def test_the_case_list_is_the_issues():
    assert set(SC.CASES) >= {(6, 3), (10, 5), (12, 3), (24, 2), (72, 3), (136, 2), (9, 3), (15, 5), (12, 2), (20, 5), (16, 4)}
    assert all(g in (1, c) for c, g in SC.IDENTITY) and all(c % g == 0 for c, g in SC.CASES)
    assert [cs for cs in SC.CASES if cs[1] * cs[1] == cs[0]] == SC.SELF_INVERSE


def test_the_tile_and_the_second_trip():
    assert SC.tile(1, 6, 4)[:3] == (2, 128, 1) and SC.tile(1, 72, 4)[:3] == (16, 16, 2) and SC.tile(1, 136, 8)[:3] == (16, 16, 2)
    assert SC.tile(1, 72, 8)[:3] == (16, 16, 1) and SC.tile(1, 9, 8)[:3] == (2, 128, 1)
    assert SC.pixel_counts(6, 4) == (1, 127, 129) and SC.pixel_counts(136, 4) == (1, 15, 17)
    for (p, c, g), epg in ((SC.TRIP_F32, 4), (SC.TRIP_F16, 8)):
        assert SC.trips(p, c, epg) == 2 and SC.trips(p - 22, c, epg) == 1 and c % g == 0 and g != c // g
    for c, _g in SC.CASES:      # the small counts stay in one trip
        for epg in (4, 8):
            assert all(SC.trips(p, c, epg) == 1 for p in SC.pixel_counts(c, epg))
