"""The half-float side of the guard-band harness (tests/gpu_util.py) and of the float64 reference (tests/ref64.py), without a GPU.

numpy functions stand in for the half kernels on HostMemory allocations.  Each KIND of defect the cases of
tests/test_gpu_guarded_f16.py look for must be reported, and a clean run must pass: a consumed read one slab row in front of the
image, a consumed weight row past Cout, a half written into the pad lane of an 8-half group, a 16-byte store that spills into the next
slice, dst_f16 = 1 writing channel 3, and a border-pixel error of two f16 ulps in a small-magnitude channel that the blob-wide criterion
lets through.  Then every new ref64 function is compared with a second, independent formulation."""
import numpy as np
import pytest
from scipy.signal import correlate

import ref64
from gpu_util import (GUARD_BYTES, GuardedBuffer, GuardError, Guards, HostMemory, channels_untouched, nchw, poison_free, poisoned, poisoned_nhwc,
                      slice_untouched)

HOST = HostMemory()
F16 = np.float16


def h16view(buf: GuardedBuffer, count: int, first: int = 0) -> np.ndarray:
    """`count` halves of the ALLOCATION starting `first` halves from the payload's first one (negative / beyond: the red zones)."""
    start = buf.offset + 2 * first
    return buf.handle[start:start + 2 * count].view(F16)


def halves(a):
    return np.asarray(a).astype(F16).astype(np.float32)


# ---- a streaming-convolution stand-in: 3x3 / pad 1 on halves, slab rows fetched from the allocation itself ---------------------------
def conv3_standin(xb, wb, yb, n, h, w, cin, xcs, xo, cout, ycs, yo, slab_rows_in_front=0, weight_rows=None, spill=0, pad_lane=False):
    """y = conv3x3(x, w) with float32 accumulation and one rounding.  Defects on request: `slab_rows_in_front` takes the row above image 0
    from the bytes in FRONT of the blob instead of the zero padding; `weight_rows` multiplies that many bank rows (> cout: rows past the
    bank); `spill` stores that many extra halves behind the slice; `pad_lane` writes the half behind the slice's last channel."""
    rows = n * h
    x = h16view(xb, (rows + slab_rows_in_front) * w * xcs, -slab_rows_in_front * w * xcs).reshape(rows + slab_rows_in_front, w, xcs)
    x = x[..., xo:xo + cin].astype(np.float32)
    nw = weight_rows or cout
    wt = h16view(wb, nw * 9 * cin).reshape(nw, 3, 3, cin).astype(np.float32)
    y = h16view(yb, n * h * w * ycs).reshape(n, h, w, ycs)
    for img in range(n):
        for i in range(h):
            for j in range(w):
                acc = np.zeros(nw, np.float32)
                for r in range(3):
                    for q in range(3):
                        ii, jj = i + r - 1, j + q - 1
                        if not 0 <= jj < w:
                            continue
                        if 0 <= ii < h:
                            row = slab_rows_in_front + img * h + ii
                        elif ii < 0 and img == 0 and slab_rows_in_front:
                            row = 0                                  # the defect: the slab row above image 0 is fetched, not zeroed
                        else:
                            continue
                        acc += wt[:, r, q] @ x[row, jj]
                out = acc[:cout] if weight_rows is None else acc[:cout] + (acc[cout:].sum() if nw > cout else 0)
                y[img, i, j, yo:yo + cout + spill] = np.concatenate([out, np.full(spill, 1.0, np.float32)]).astype(F16)
                if pad_lane:
                    y[img, i, j, yo + cout] = 0
    return y


def conv3_case(**defect):
    rng = np.random.default_rng(5)
    n, h, w, cin, xcs, xo, cout, ycs, yo = 2, 4, 5, 16, 32, 8, 24, 40, 8
    x = halves(rng.standard_normal((n, cin, h, w)))
    wt = halves(rng.standard_normal((cout, cin, 3, 3)) / 12)
    with Guards(mem=HOST) as g:
        xb = g.put(poisoned_nhwc(x, xcs, xo, dtype=F16), name="x")
        wb = g.put(np.ascontiguousarray(wt.transpose(0, 2, 3, 1)).astype(F16), at_end=True, name="w")
        yb = g.put(poisoned((n, h, w, ycs), dtype=F16), name="y")
        conv3_standin(xb, wb, yb, n, h, w, cin, xcs, xo, cout, ycs, yo, **defect)
        full = yb.read((n, h, w, ycs), F16)
        y = nchw(full.astype(np.float32), cout, yo)
        y64, mag = ref64.conv2d(x, wt, None, 1, 1), ref64.conv2d_mag(x, wt, None, 1, 1)
        return poison_free(y), ref64.worst(y, y64, ref64.dot_bound_f16(cin * 9, mag, y64))[0], slice_untouched(full, yo, cout)


def test_a_clean_half_convolution_passes():
    free, ratio, untouched = conv3_case()
    assert free and ratio <= 1.0 and untouched


def test_a_slab_row_in_front_of_the_image_reaches_y_as_nan():
    free, ratio, _ = conv3_case(slab_rows_in_front=1)
    assert not free and ratio == np.inf


def test_a_weight_row_past_cout_reaches_y_as_nan():
    free, ratio, _ = conv3_case(weight_rows=25)
    assert not free and ratio == np.inf


def test_a_half_in_the_pad_lane_of_an_eight_half_group_is_seen():
    _, _, untouched = conv3_case(pad_lane=True)
    assert not untouched


def test_a_sixteen_byte_store_that_spills_into_the_next_slice_is_seen():
    _, _, untouched = conv3_case(spill=8)
    assert not untouched


def test_channels_untouched_takes_the_union_of_several_slices():
    full = poisoned((3, 24), dtype=F16)
    full[:, 0:8] = 1
    full[:, 16:20] = 2
    written = np.zeros(24, bool)
    written[0:8] = written[16:20] = True
    assert channels_untouched(full, written)
    full[1, 20] = 0
    assert not channels_untouched(full, written)
    huge = poisoned((2, 16), "huge", F16)
    assert channels_untouched(huge, np.zeros(16, bool), "huge") and not channels_untouched(huge, np.zeros(16, bool))


def test_a_refused_call_must_leave_the_whole_allocation_alone():
    b = GuardedBuffer(poisoned(24, dtype=F16), mem=HOST)
    assert b.unchanged()
    h16view(b, 1, 3)[0] = 1                                       # inside the payload: check() does not look there, unchanged() does
    b.check()
    assert not b.unchanged()
    c = GuardedBuffer(64, mem=HOST)
    h16view(c, 1, -1)[0] = 0
    assert not c.unchanged()
    with pytest.raises(GuardError):
        c.check()


def test_the_last_tiles_slab_behind_an_image_at_the_end_reads_poison():
    """at_end=True puts the image's last byte in front of the back red zone: the first half behind it is a NaN (a slab that runs on)."""
    x = poisoned_nhwc(np.ones((1, 8, 2, 3), np.float32), 8, dtype=F16)
    b = GuardedBuffer(x, at_end=True, mem=HOST)
    assert b.offset + b.nbytes == b.total - GUARD_BYTES
    assert np.all(np.isnan(h16view(b, 64, x.size))) and not np.isnan(h16view(b, 1, x.size - 1)[0])


# ---- the image kernels' three output modes -------------------------------------------------------------------------------------------
def preprocess_standin(dst, vals, mode, writes_channel_3=False):
    px = h16view(dst, vals.shape[0] * 8).reshape(-1, 8)
    if mode == 3:
        px[:, :3], px[:, 3:5], px[:, 5:] = vals, 1, 0
    else:
        px[:, :3] = vals
        if writes_channel_3:
            px[:, 3] = 0


def pixels_ok(out, want, mode):
    ok = np.array_equal(out[..., :3], want.astype(F16))
    if mode == 1:
        return ok and slice_untouched(out, 0, 3)
    return ok and bool(np.all(out[..., 3:5] == F16(1)) and np.all(out[..., 5:].view(np.uint16) == 0))


@pytest.mark.parametrize("mode,bad,passes", [(1, False, True), (1, True, False), (3, False, True)])
def test_half_image_modes_are_pinned_per_half(mode, bad, passes):
    vals = np.random.default_rng(1).random((30, 3)).astype(np.float32)
    with Guards(mem=HOST) as g:
        dst = g.put(poisoned((30, 8), dtype=F16), at_end=True)
        preprocess_standin(dst, vals, mode, writes_channel_3=bad)
        assert pixels_ok(dst.read((30, 8), F16), vals, mode) == passes
    with Guards(mem=HOST) as g:                                   # the whole-pixel form where only three halves were asked for
        dst = g.put(poisoned((30, 8), dtype=F16), at_end=True)
        preprocess_standin(dst, vals, 3)
        assert not pixels_ok(dst.read((30, 8), F16), vals, 1)


# ---- the per-element bound against the blob-wide one ---------------------------------------------------------------------------------
def test_two_ulps_on_a_small_border_element_pass_blob_wide_and_fail_per_element():
    rng = np.random.default_rng(2)
    n, cin, h, w, cout = 1, 16, 6, 6, 8
    x = halves(rng.standard_normal((n, cin, h, w)))
    wt = halves(rng.standard_normal((cout, cin, 3, 3)) / 12)
    wt[3] = halves(wt[3] / 64)                                    # a small-magnitude channel
    y64, mag = ref64.conv2d(x, wt, None, 1, 1), ref64.conv2d_mag(x, wt, None, 1, 1)
    y = y64.astype(F16)
    allow = ref64.dot_bound_f16(cin * 9, mag, y64)
    assert ref64.worst(y.astype(np.float64), y64, allow)[0] <= 1.0
    bad = y.copy()
    bad[0, 3, 0, 0] = np.nextafter(np.nextafter(bad[0, 3, 0, 0], F16(np.inf)), F16(np.inf))      # two f16 ulps, corner pixel
    err = np.abs(bad.astype(np.float64) - y64)
    assert err.max() <= np.abs(y64).max() * 2.0 ** -10          # the criterion of tests/test_gpu_f16.py lets it through
    ratio, at = ref64.worst(bad.astype(np.float64), y64, allow)
    assert ratio > 1.0 and np.unravel_index(at, y64.shape) == (0, 3, 0, 0)


# ---- the new ref64 functions against independent formulations ------------------------------------------------------------------------
def test_rounding_helpers():
    a = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 1e-8, -0.1, 2049.0])
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 0.0, float(F16(-0.1)), 2048.0])      # ties to even
    assert np.array_equal(ref64.to_f16_then_f64(a), want)
    v = np.array([0.0, 1e-7, 6.1e-5, 1.0, 1.999, 2.0, 1000.0, 32768.0])
    assert np.array_equal(ref64.f16_ulp(v), np.spacing(v.astype(F16)).astype(np.float64))
    assert np.array_equal(ref64.f16_ulp(-v), ref64.f16_ulp(v))


@pytest.mark.parametrize("k,s,p,h,w", [(3, 2, 0, 6, 7), (3, 1, 1, 5, 4), (3, 2, 1, 7, 6), (2, 2, 0, 5, 8), (3, 1, 1, 1, 9), (5, 3, 2, 9, 1), (3, 2, 0, 57, 61)])
def test_max_pool_values_equals_the_window_loop(k, s, p, h, w):
    x = -np.abs(np.random.default_rng(h).standard_normal((2, 3, h, w))) - 0.25      # all negative: a zero pad would win
    assert np.array_equal(ref64.max_pool_values(x, k, s, p), ref64.max_pool(x, k, s, p)[0])


def lrn_loops(x, ls, alpha, beta, k):
    n, c, h, w = x.shape
    y = np.zeros_like(x)
    for ch in range(c):
        lo, hi = max(0, ch - (ls - 1) // 2), min(c, ch + (ls - 1) // 2 + 1)
        y[:, ch] = x[:, ch] * (k + alpha / ls * (x[:, lo:hi] ** 2).sum(axis=1)) ** -beta
    return y


@pytest.mark.parametrize("lrn_first", [0, 1])
def test_half_lrn_and_pool_lrn_against_loops(lrn_first):
    x = halves(np.random.default_rng(3).standard_normal((2, 16, 7, 6)) * 100).astype(np.float64)
    y = ref64.lrn_f16(x, 5, 1e-4, 0.75, round_out=False)
    assert np.allclose(y, lrn_loops(x, 5, 1e-4, 0.75, 1.0), rtol=1e-14, atol=0)
    assert np.array_equal(ref64.lrn_f16(x, 5, 1e-4, 0.75), y.astype(F16).astype(np.float64))
    got = ref64.pool_lrn_f16(x, 3, 2, 0, lrn_first, 1e-4, 0.75, round_out=False)
    pool = lambda a: ref64.max_pool(a, 3, 2, 0)[0]
    want = pool(lrn_loops(x, 5, 1e-4, 0.75, 1.0)) if lrn_first else lrn_loops(pool(x), 5, 1e-4, 0.75, 1.0)
    assert np.allclose(got, want, rtol=1e-14, atol=0)
    # rounding is monotonic: rounding before the maximum (what a kernel that stores the normalised blob does) changes nothing
    if lrn_first:
        assert np.array_equal(ref64.pool_lrn_f16(x, 3, 2, 0, 1, 1e-4, 0.75), pool(ref64.to_f16_then_f64(lrn_loops(x, 5, 1e-4, 0.75, 1.0))))
    # the allowance: the correctly rounded value passes, a value one f16 ulp off does not
    allow = ref64.lrn_f16_allow(got, 5, 0.75)
    good = ref64.to_f16_then_f64(got)
    assert ref64.worst(good, got, allow)[0] <= 1.0
    assert ref64.worst(good + ref64.f16_ulp(good), got, allow)[0] > 1.0


@pytest.mark.parametrize("relu", [False, True])
def test_pool_lrn_conv1x1_reference_and_its_allowance(relu):
    rng = np.random.default_rng(4)
    x = halves(-np.abs(rng.standard_normal((2, 64, 9, 7))) * 40 - 1)
    w = halves(rng.standard_normal((64, 64)) * 0.1)
    b = rng.standard_normal(64).astype(np.float32)
    y64, allow = ref64.pool_lrn_conv1x1_f16(x, w, b, 3, 2, 0, 1e-4, 0.75, 1.0, relu=relu)
    mid = lrn_loops(ref64.max_pool(x, 3, 2, 0)[0], 5, 1e-4, 0.75, 1.0).astype(F16).astype(np.float64)
    want = np.tensordot(mid, w.astype(np.float64), axes=([1], [1])).transpose(0, 3, 1, 2) + b[None, :, None, None]
    want = np.maximum(want, 0) if relu else want
    assert np.allclose(y64, want, rtol=1e-13, atol=1e-13)
    # a float32 evaluation of the same three layers (rounded where the kernel rounds) lies inside the allowance; an unrounded-LRN one
    # that is then off by one output ulp does not
    mid32 = mid.astype(np.float32)
    y32 = np.einsum("nchw,oc->nohw", mid32, w) + b[None, :, None, None]
    y16 = (np.maximum(y32, 0) if relu else y32).astype(F16)
    assert ref64.worst(y16.astype(np.float64), y64, allow)[0] <= 1.0
    off = y16.astype(np.float64) + 4 * ref64.f16_ulp(y16)
    assert ref64.worst(off, y64, allow)[0] > 1.0
    mag = np.einsum("nchw,oc->nohw", np.abs(mid), np.abs(w.astype(np.float64))) + np.abs(b)[None, :, None, None]
    assert np.all(allow > 0) and np.all(allow < 2.0 ** -9 * mag)      # (below one f16 ulp of the magnitude term: not a loose bound)


def test_image_ones_reference_against_scipy_correlation_and_loops():
    rng = np.random.default_rng(6)
    n, h, w, cout = 2, 9, 11, 4
    x3 = halves(rng.random((n, 3, h, w)))
    wt = rng.standard_normal((cout, 5, 7, 7))
    b = rng.standard_normal(cout)
    y, mag, border = ref64.conv2d_image_ones(x3, wt, b, 3, 2)
    x5 = np.concatenate([x3.astype(np.float64), np.ones((n, 2, h, w))], axis=1)
    xp = np.pad(x5, ((0, 0), (0, 0), (3, 3), (3, 3)))      # zeros outside the image: the constant channels are 0 there, not 1
    for img in range(n):
        for o in range(cout):
            full = sum(correlate(xp[img, c], wt[o, c], mode="valid") for c in range(5))[::2, ::2] + b[o]
            assert np.allclose(y[img, o], full, rtol=1e-12, atol=1e-12)
    assert np.allclose(y, ref64.conv2d(x5, wt, b, 3, 2), rtol=1e-12, atol=1e-12)
    assert np.allclose(mag, ref64.conv2d_mag(x5, wt, b, 3, 2), rtol=1e-12, atol=1e-12)
    oh, ow = y.shape[2:]
    want_border = np.array([[not (3 <= 2 * i and 2 * i + 3 < h and 3 <= 2 * j and 2 * j + 3 < w) for j in range(ow)] for i in range(oh)])
    assert np.array_equal(border, want_border) and border.any() and not border.all()
    # counting the constant channels over ALL 49 taps (a kernel without the border table) is wrong exactly at the border
    naive = ref64.conv2d(x3, wt[:, :3], b, 3, 2) + (wt[:, 3] + wt[:, 4]).sum(axis=(1, 2))[None, :, None, None]
    diff = np.abs(naive - y).max(axis=(0, 1)) > 1e-9
    assert np.array_equal(diff, border)
