"""Guard-banded, poisoned-buffer tests of the validation-pass kernels (csrc/eval.hip) against tests/ref_eval64.py, -m gpu.

fcn_accuracy_f32 works on integer counts, so its two tops must equal the reference's float32 quotients EXACTLY; fcn_score_accumulate_f32
adds once per element per call in float32, so after k calls the accumulator must hold the bits of a host float32 running sum.  Every
buffer is a guarded allocation; padding channels and the bytes between the views hold NaN poison, which must neither reach a result
nor change."""
import numpy as np
import pytest

import ref_eval64 as E
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def workspace(g):
    n = int(L.load().fcn_accuracy_workspace_bytes())
    assert n > 0 and n % 4 == 0
    return g.put(n, name="workspace")


def run_accuracy(g, x, lab, cstride, top_k, ignore, per_class, label_cstride=1, at_end=False):
    n, c, h, w = x.shape
    xd = g.put(poisoned_nhwc(x, cstride), at_end=at_end, name="scores")
    ld = g.put(poisoned_nhwc(lab.astype(np.float32), label_cstride), at_end=at_end, name="labels")
    acc = g.put(4, name="accuracy")
    per = g.put(4 * c, at_end=True, name="per class") if per_class else None
    ws = workspace(g)
    L.call("fcn_accuracy_f32", xd.ptr, ld.ptr, acc.ptr, per.ptr if per else None, n, n * h * w, c, cstride, label_cstride, top_k,
           0 if ignore is None else 1, 0 if ignore is None else ignore, ws.ptr, None)
    L.call("fcn_device_sync")
    assert np.array_equal(bits(xd.read((n, h, w, cstride))), bits(poisoned_nhwc(x, cstride))), "the scores were modified"
    return acc.read((1,))[0], (per.read((c,)) if per else None)


def make_case(seed, n, c, h, w, ignore, ties=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    if ties:      # a few levels only: most pixels have several channels tied with the label's score
        x = rng.integers(0, 3, (n, c, h, w)).astype(np.float32)
    lab = rng.integers(0, c, (n, 1, h, w))
    if ignore is not None:
        lab[rng.random(lab.shape) < 0.2] = ignore
    lab.reshape(-1)[::37] = c + 3      # out of range: valid and wrong, never an index
    lab.reshape(-1)[5::41] = -2
    return x, lab


GEOMETRY = [(2, 2), (2, 4), (3, 4), (3, 7), (12, 12), (12, 16), (21, 21), (21, 24)]


@pytest.mark.parametrize("c,cstride,top_k", [(c, cs, k) for c, cs in GEOMETRY for k in (1, 3) if k <= c])
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("per_class", [False, True])
def test_accuracy_matches_reference_exactly(g, c, cstride, top_k, ignore, per_class):
    n, h, w = 2, 19, 23      # 874 pixels: three whole workgroup tiles and a partial one
    x, lab = make_case(c * 100 + cstride, n, c, h, w, ignore)
    acc, per = run_accuracy(g, x, lab, cstride, top_k, ignore, per_class, at_end=(cstride % 2 == 1))
    want, want_per = E.accuracy(x, lab, top_k, ignore)
    assert bits(acc) == bits(want), (acc, want)
    if per_class:
        assert np.array_equal(bits(per), bits(want_per))


@pytest.mark.parametrize("pixels_hw", [(1, 1), (1, 255), (16, 16), (1, 257), (300, 301)])
def test_accuracy_pixel_counts_and_label_stride(g, pixels_hw):
    h, w = pixels_hw
    x, lab = make_case(h * 1000 + w, 1, 5, h, w, 9)
    acc, per = run_accuracy(g, x, lab, 8, 1, 9, True, label_cstride=3)
    want, want_per = E.accuracy(x, lab, 1, 9)
    assert bits(acc) == bits(want) and np.array_equal(bits(per), bits(want_per))


def test_accuracy_engineered_ties_and_repeatable(g):
    x, lab = make_case(7, 2, 12, 40, 33, 255, ties=True)
    for top_k in (1, 3):
        a1, p1 = run_accuracy(g, x, lab, 12, top_k, 255, True)
        a2, p2 = run_accuracy(g, x, lab, 12, top_k, 255, True)
        want, want_per = E.accuracy(x, lab, top_k, 255)
        assert bits(a1) == bits(want) == bits(a2)
        assert np.array_equal(bits(p1), bits(want_per)) and np.array_equal(bits(p1), bits(p2))
    # the ties matter: with ">" instead of ">=" the label would win them
    strict = sum(1 for v, l in zip(x.transpose(0, 2, 3, 1).reshape(-1, 12), lab.reshape(-1)) if 0 <= l < 12 and np.sum(v > v[l]) < 1)
    assert strict > E.accuracy_counts(x, lab, 1, 255)[0]


def test_accuracy_all_pixels_ignored_is_zero(g):
    x = np.random.default_rng(1).standard_normal((1, 4, 9, 9)).astype(np.float32)
    acc, per = run_accuracy(g, x, np.full((1, 1, 9, 9), 255), 4, 1, 255, True)
    assert bits(acc) == bits(np.float32(0)) and np.array_equal(bits(per), bits(np.zeros(4, np.float32)))


def test_accuracy_refuses_bad_arguments(g):
    x = g.put(poisoned((4, 4)), name="x")
    lab = g.put(np.zeros(4, np.float32), name="label")
    acc, ws = g.put(4, name="acc"), workspace(g)
    lib = L.load()
    assert lib.fcn_accuracy_f32(x.ptr, lab.ptr, acc.ptr, None, 1, 4, 4, 3, 1, 1, 0, 0, ws.ptr, None) != 0      # stride < C
    assert lib.fcn_accuracy_f32(x.ptr, lab.ptr, acc.ptr, None, 1, 4, 4, 4, 1, 0, 0, 0, ws.ptr, None) != 0      # top_k < 1
    assert lib.fcn_accuracy_f32(x.ptr, lab.ptr, acc.ptr, None, 1, 4, 4, 4, 1, 1, 0, 0, None, None) != 0        # no workspace
    assert acc.unchanged() and x.unchanged()


def accumulate(g, blobs, cstride, coffset, at_end=False):
    """k calls over k different inputs into one accumulator that starts at zero -> (accumulator NCHW, the last input read back)."""
    n, c, h, w = blobs[0].shape
    acc = g.put(np.zeros((n, c, h, w), np.float32), at_end=at_end, name="accumulator")
    for i, b in enumerate(blobs):
        full = poisoned_nhwc(b, cstride, coffset)
        xd = g.put(full, at_end=at_end, name="x%d" % i)
        L.call("fcn_score_accumulate_f32", acc.ptr, xd.ptr, n, h * w, c, cstride, coffset, None)
        L.call("fcn_device_sync")
        back = xd.read((n, h, w, cstride))
        assert np.array_equal(bits(back), bits(full)) and slice_untouched(back, coffset, c)
    return acc.read((n, c, h, w))


def spread(seed, shape, k=5):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(k)]


def test_score_accumulate_scalar(g):
    xs = spread(0, (1, 1, 1, 1))
    got = accumulate(g, xs, 1, 0)
    assert np.array_equal(bits(got), bits(E.running_sum(xs)))


@pytest.mark.parametrize("n,c", [(1, 21), (3, 5)])
def test_score_accumulate_vectors(g, n, c):
    """pixels == 1: loss vectors and the Accuracy per-class top."""
    xs = spread(c, (n, c, 1, 1))
    assert np.array_equal(bits(accumulate(g, xs, c + 3, 2)), bits(E.running_sum(xs)))


@pytest.mark.parametrize("n,c,h,w,cstride,coffset,at_end", [
    (2, 4, 7, 9, 12, 4, False),        # a sliced view at an aligned offset: 16-byte loads
    (1, 3, 5, 13, 8, 5, False),        # ... at an unaligned one: scalar loads
    (2, 21, 17, 19, 24, 0, False),     # a score map, channel tiles 16 + 5, pixel tiles 5 x 64 + 3
    (1, 2, 64, 64, 4, 0, False),       # coverage-like: whole pixel tiles
    (1, 5, 9, 11, 5, 0, True),         # odd stride, payload flush against the back red zone
])
def test_score_accumulate_maps(g, n, c, h, w, cstride, coffset, at_end):
    xs = spread(n * c * h + w, (n, c, h, w))
    got = accumulate(g, xs, cstride, coffset, at_end)
    assert np.array_equal(bits(got), bits(E.running_sum(xs)))


def test_score_accumulate_refuses_bad_arguments(g):
    acc = g.put(np.zeros(16, np.float32), name="acc")
    x = g.put(poisoned((16,)), name="x")
    lib = L.load()
    assert lib.fcn_score_accumulate_f32(acc.ptr, x.ptr, 1, 4, 4, 3, 0, None) != 0      # stride < C
    assert lib.fcn_score_accumulate_f32(acc.ptr, x.ptr, 1, 2, 4, 6, 3, None) != 0      # view runs past the stride
    assert lib.fcn_score_accumulate_f32(acc.ptr, None, 1, 4, 4, 4, 0, None) != 0
    assert acc.unchanged() and x.unchanged()
