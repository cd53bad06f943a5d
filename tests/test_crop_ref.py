"""The float64 Crop reference against plain numpy slicing / np.pad, and the adjoint identity (no GPU)."""
import numpy as np
import pytest

import ref_crop64 as R

CASES = [((2, 5, 7, 9), (0, 0, 0, 0), (2, 5, 7, 9)), ((2, 5, 7, 9), (0, 0, 2, 3), (2, 5, 4, 6)), ((1, 6, 8, 8), (0, 2, 1, 0), (1, 3, 7, 5)),
         ((3, 1, 4, 10), (0, 0, 3, 9), (3, 1, 1, 1))]


@pytest.mark.parametrize("shape,off,size", CASES)
def test_forward_is_a_slice(shape, off, size):
    x = np.random.default_rng(0).standard_normal(shape)
    want = x[tuple(slice(o, o + s) for o, s in zip(off, size))]
    assert np.array_equal(R.crop(x, off, size), want)


@pytest.mark.parametrize("shape,off,size", CASES)
def test_backward_is_a_zero_pad_and_accumulates_inside_only(shape, off, size):
    rng = np.random.default_rng(1)
    dy = rng.standard_normal(size)
    pad = [(o, e - o - s) for o, e, s in zip(off, shape, size)]
    assert np.array_equal(R.crop_bwd(dy, off, shape), np.pad(dy, pad))
    base = rng.standard_normal(shape)
    got = R.crop_bwd(dy, off, shape, dx=base)
    assert np.array_equal(got, base + np.pad(dy, pad))
    outside = np.pad(np.zeros(size), pad, constant_values=1).astype(bool)
    assert np.array_equal(got[outside], base[outside])


@pytest.mark.parametrize("shape,off,size", CASES)
def test_adjointness(shape, off, size):
    rng = np.random.default_rng(2)
    x, g = rng.standard_normal(shape), rng.standard_normal(size)
    lhs, rhs = float((R.crop(x, off, size) * g).sum()), float((x * R.crop_bwd(g, off, shape)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_a_window_that_leaves_the_blob_is_refused():
    with pytest.raises(ValueError):
        R.crop(np.zeros((1, 1, 4, 4)), (0, 0, 2, 0), (1, 1, 3, 4))
