"""The float64 ArgMax reference (tests/ref_argmax64.py) and the cases of tests/argmax_cases.py, on the CPU.

The reference is held against a literal restatement of Caffe's loop (a sort of (value, index) pairs, descending); every margin case
keeps its margin at EVERY pixel - none is excluded, for float32 and for half-rounded inputs - and every tie case gives another answer
under the other tie rule, so a kernel with that rule cannot pass it."""
import numpy as np
import pytest

import argmax_cases as A
import ref_argmax64 as R
import ref_interp64 as RI


def caffe_loop(x, top_k):
    """ArgMaxLayer::Forward_cpu over axis 1: partial_sort of pairs with std::greater."""
    n, c, h, w = x.shape
    idx, val = np.zeros((n, top_k, h, w)), np.zeros((n, top_k, h, w))
    for i in range(n):
        for y in range(h):
            for z in range(w):
                pairs = sorted(((float(x[i, ch, y, z]), ch) for ch in range(c)), reverse=True)[:top_k]
                idx[i, :, y, z] = [p[1] for p in pairs]
                val[i, :, y, z] = [p[0] for p in pairs]
    return idx, val


@pytest.mark.parametrize("c,top_k", [(1, 1), (5, 2), (5, 5), (21, 5)])
def test_reference_is_caffes_loop(c, top_k):
    for x in (A.plain_ties(c, 9, False).astype(np.float64), np.random.default_rng(c).standard_normal((2, c, 3, 4))):
        i, v = caffe_loop(x, top_k)
        assert np.array_equal(R.argmax(x, top_k), i) and np.array_equal(R.argmax(x, top_k, "values"), v)


def test_forms_and_shapes():
    x = np.random.default_rng(0).standard_normal((3, 7))
    i, v = R.ranks(x, 4)
    assert R.argmax(x, 4, "legacy").shape == (3, 1, 4) and R.argmax(x, 4, "pairs").shape == (3, 2, 4)
    assert np.array_equal(R.argmax(x, 4, "pairs")[:, 0], i[:, :, 0, 0]) and np.array_equal(R.argmax(x, 4, "pairs")[:, 1], v[:, :, 0, 0])
    p = R.softmax(x)
    assert np.allclose(p.sum(1), 1.0) and np.array_equal(R.argmax(x, 4, probs=True), R.argmax(p, 4))
    assert np.allclose(R.argmax(x, 4, "values", probs=True), R.argmax(p, 4, "values"), rtol=1e-15, atol=0)
    assert np.array_equal(R.argmax(np.full((1, 6), 2.0), 6)[0, :, 0, 0], [5, 4, 3, 2, 1, 0])
    assert np.array_equal(R.argmax(np.full((1, 6), 2.0), 6, tie="smaller")[0, :, 0, 0], [0, 1, 2, 3, 4, 5])


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", A.PLAIN_SHAPES + A.SWITCH_SHAPES, ids=lambda s: "c%d-p%d" % (s[0], s[4]))
def test_plain_margin_cases_keep_their_margin_at_every_pixel(shape, half):
    c, _, _, _, pixels = shape
    for k in (A.top_ks(c) if shape in A.PLAIN_SHAPES else (1, 5)):
        for negative in (False, True):
            x = A.plain_margin(c, pixels, k, half, negative).astype(np.float64)
            assert R.margin(x, k) >= A.MARGIN, (c, k, negative, R.margin(x, k))
            assert not negative or x.max() < 0
            # the probabilities of the fused Softmax keep their order and a margin too (what an unfused half engine would compare)
            if k <= 5 and not negative:
                assert R.margin(R.softmax(x), k) >= A.MARGIN, (c, k)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("softmax", [False, True], ids=["scores", "softmax"])
@pytest.mark.parametrize("geom", A.FUSED_GEOMS, ids=lambda g: "-".join(str(v) for v in g))
def test_fused_margin_cases_keep_their_margin_at_every_pixel(geom, softmax, half):
    n, c, h, w, oh, ow, pb, pe = geom
    x, seed = A.fused_margin(*geom, half, softmax)
    y = RI.interp(x.astype(np.float64), oh, ow, pb, pe)
    assert y.shape == (n, c, oh, ow) and R.margin(y, 1) >= A.MARGIN
    if softmax:
        assert R.margin(R.softmax(y), 1) >= A.MARGIN
    # and the once-more rounded blend of the unfused half path keeps the order
    if half:
        assert np.array_equal(R.argmax(y.astype(np.float16).astype(np.float64)), R.argmax(y))


def differs(a, b):
    return not np.array_equal(a, b)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_tie_cases_tell_the_rules_apart(half):
    for c, _, _, _, pixels in A.PLAIN_SHAPES:
        if c < 2:
            continue
        for k in A.top_ks(c):
            x = A.plain_equal(c, pixels, half).astype(np.float64)
            assert np.array_equal(R.argmax(x, k)[0, :, 0, 0], np.arange(c - 1, c - 1 - k, -1))
            assert differs(R.argmax(x, k), R.argmax(x, k, tie="smaller"))
        if c >= 4:
            x = A.plain_ties(c, pixels, half).astype(np.float64)
            assert differs(R.argmax(x, 1), R.argmax(x, 1, tie="smaller"))
    for n, c, h, w, oh, ow, pb, pe in A.FUSED_GEOMS:
        if c < 3:
            continue
        x = A.fused_constant_planes(n, c, h, w, half).astype(np.float64)
        got = R.interp_argmax(x, oh, ow, pb, pe)
        assert (got == c - 1).all() and (R.interp_argmax(x, oh, ow, pb, pe, tie="smaller") == 1).all()
    n, c, h, w, oh, ow, pb, pe = A.FUSED_GEOMS[0]
    x = A.fused_integers(n, c, h, w, half).astype(np.float64)
    y = RI.interp(x, oh, ow, pb, pe)
    assert np.array_equal(y * 16, np.round(y * 16)), "weights in quarters: the blends of small integers are exact"
    assert differs(R.interp_argmax(x, oh, ow, pb, pe), R.interp_argmax(x, oh, ow, pb, pe, tie="smaller"))
