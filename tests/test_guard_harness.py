"""The guard-band harness of tests/gpu_util.py and the float64 reference of tests/ref64.py, checked without a GPU.

numpy functions stand in for kernels (a HostMemory allocation is a byte array, so a stand-in can do to it exactly what a
stray kernel would do to device memory): every failure class the guarded GPU cases rely on must be REPORTED - a write in
front of the payload, behind it, into a slack channel, a pad read that reaches the result as NaN, a pad read that wins a
MAX - and a clean run must pass.  Then the float32 oracle is held to ref64's element-wise bound on convolution cases, and
ref64's other operations are compared with the oracle's independent implementations."""
import numpy as np
import pytest

import ref64
from gpu_util import (GUARD_BYTES, POISON_WORD, GuardedBuffer, GuardError, Guards, HostMemory, nchw, poison_free, poison_value, poisoned,
                      poisoned_nhwc, slice_untouched)
from oracle import caffe_ref as R

HOST = HostMemory()


def f32view(buf: GuardedBuffer, count: int, first: int = 0) -> np.ndarray:
    """`count` floats of the ALLOCATION starting `first` floats from the payload's first one (negative / beyond: the red zones)."""
    start = buf.offset + 4 * first
    return buf.handle[start:start + 4 * count].view(np.float32)


def relu_standin(xb, yb, count, first=0, extra=0):
    """y[first .. count + extra) = x > 0 ? x : 0 (the kernels' ReLU: a NaN becomes 0): first < 0 starts in front of the buffers,
    extra > 0 runs past their end."""
    x, y = f32view(xb, count + extra - first, first), f32view(yb, count + extra - first, first)
    y[...] = np.where(x > 0, x, 0)


def test_the_poison_word_reads_as_nan_nan_nan_and_no_pixel_index():
    assert POISON_WORD == 0x7FC07FC0
    word = np.uint32(POISON_WORD)
    assert np.isnan(word.view(np.float32))
    halves = np.frombuffer(word.tobytes(), np.float16)
    assert halves.size == 2 and np.all(np.isnan(halves))
    assert int(word.view(np.int32)) == 2143322048          # as an argmax: beyond iy*W+ix of any image that fits in memory
    assert list(word.tobytes()) == [0xC0, 0x7F, 0xC0, 0x7F]
    assert np.isnan(poison_value("nan", np.float32)) and np.isnan(poison_value("nan", np.float16))
    assert poison_value("nan", np.int32) == 2143322048 and poison_value("nan", np.uint8) == 0xC0
    assert poison_value("huge", np.float32) == np.float32(3e38) and poison_value("huge", np.float16) == np.float16(65504)


@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1003])
def test_layout_of_a_guarded_allocation(count, at_end):
    a = np.arange(count, dtype=np.float32)
    b = GuardedBuffer(a, at_end=at_end, mem=HOST)
    base = b.handle.ctypes.data
    assert b.total == 2 * GUARD_BYTES + (4 * count + 15) // 16 * 16 and b.ptr == base + b.offset
    if at_end:
        assert b.offset + b.nbytes == b.total - GUARD_BYTES      # the payload's last byte is the last one before the back red zone
    else:
        assert b.offset == GUARD_BYTES and b.ptr % 16 == base % 16
    assert np.array_equal(b.read((count,)), a)
    # everything that is not payload reads as NaN to a float kernel, including the bytes that round the payload to 16
    around = np.concatenate([f32view(b, 8, -8), f32view(b, 8, count)])
    assert np.all(np.isnan(around))
    b.check()


def test_a_clean_run_passes():
    x = np.linspace(-2, 2, 1003, dtype=np.float32)
    with Guards(mem=HOST) as g:
        xd, yd = g.put(x), g.put(x.nbytes)
        relu_standin(xd, yd, x.size)
        y = yd.read(x.shape)
        assert np.array_equal(y, np.maximum(x, 0)) and poison_free(y)


def test_a_write_in_front_of_the_payload_is_reported():
    x = np.ones(64, np.float32)
    with pytest.raises(GuardError, match=r"in front of the payload.*first modified byte at -8, last at -1"):
        with Guards(mem=HOST) as g:
            xd, yd = g.put(x), g.put(x.nbytes, name="y")
            relu_standin(xd, yd, x.size, first=-2)            # (x's red zone reads as NaN, the ReLU stores 0 for it)
    # the input's red zones were only read: they are intact
    xd = GuardedBuffer(x, mem=HOST)
    assert xd.modified() is None


def test_a_write_behind_the_payload_is_reported_with_its_extent():
    x = np.ones(1003, np.float32)
    with pytest.raises(GuardError, match=r"red zone of y written behind the payload \(4012 bytes\): first modified byte at \+4012, last at \+4023"):
        with Guards(mem=HOST) as g:
            xd, yd = g.put(x), g.put(x.nbytes, name="y")
            relu_standin(xd, yd, x.size, extra=3)             # a vector tail that rounds 1003 up to 1006
    # a single byte at the far end of the back zone is seen too, and an at_end payload reports offsets from ITS first byte
    b = GuardedBuffer(np.zeros(5, np.uint8), at_end=True, mem=HOST)
    b.handle[b.total - 1] ^= 1
    assert b.modified() == (5 + GUARD_BYTES - 1,) * 2
    with pytest.raises(GuardError):
        b.check()


def test_a_failing_assertion_in_the_body_is_not_masked_by_the_guard_check():
    with pytest.raises(ZeroDivisionError):
        with Guards(mem=HOST) as g:
            yd = g.put(16)
            f32view(yd, 1, -1)[0] = 0.0
            1 / 0


def test_a_write_into_a_slack_channel_is_reported():
    n, c, h, w, cs, co = 1, 4, 3, 5, 12, 4
    full = poisoned((n, h, w, cs))
    assert slice_untouched(full, co, c)
    good = full.copy()
    good[..., co:co + c] = 1.0                                 # the kernel's own slice
    assert slice_untouched(good, co, c)
    for stray in (co - 1, co + c, 0, cs - 1):                  # a neighbour channel either side, the pixel's first and last channel
        bad = good.copy()
        bad[0, 1, 2, stray] = 1.0
        assert not slice_untouched(bad, co, c)
    bad = good.copy()
    bad[0, 2, 4, cs - 1] = np.float32(np.nan)                  # another NaN than the poison's: equal under isnan, not bit for bit
    assert np.isnan(bad[0, 2, 4, cs - 1]) and not slice_untouched(bad, co, c)
    halves = poisoned((1, 2, 2, 16), dtype=np.float16)
    halves[..., 8:16] = np.float16(2)
    assert slice_untouched(halves, 8, 8) and not slice_untouched(halves, 0, 8)
    idx = poisoned((1, 2, 2, 8), dtype=np.int32)
    assert np.all(idx == 2143322048) and not poison_free(idx)


def lrn_standin(xfull, coffset, c, reads_neighbours):
    """A 5-wide LRN of channels coffset .. coffset + c - 1 of an NHWC buffer; the wrong one takes its window from the BUFFER's
    channels (what a kernel does that forgets the slice ends where another branch's activations begin)."""
    src = xfull if reads_neighbours else xfull[..., coffset:coffset + c]
    lo = coffset if reads_neighbours else 0
    sq = np.pad(src.astype(np.float64) ** 2, ((0, 0),) * 3 + ((2, 2),))
    s = sum(sq[..., lo + d:lo + d + c] for d in range(5))
    return xfull[..., coffset:coffset + c] * (1 + 1e-4 / 5 * s) ** -0.75


def test_a_consumed_pad_read_reaches_the_result_as_nan():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 8, 3, 4)).astype(np.float32)
    xfull = poisoned_nhwc(x, 16, 4)
    want = ref64.lrn(x, 5, 1e-4, 0.75)[0].transpose(0, 2, 3, 1)
    good = lrn_standin(xfull, 4, 8, reads_neighbours=False)
    assert poison_free(good) and np.allclose(good, want, rtol=1e-12)
    bad = lrn_standin(xfull, 4, 8, reads_neighbours=True)
    assert not poison_free(bad)
    assert np.all(np.isnan(bad[..., [0, 1, 6, 7]])) and poison_free(bad[..., 2:6])      # exactly the channels whose window crosses the slice
    assert ref64.worst(nchw(bad, 8), ref64.lrn(x, 5, 1e-4, 0.75)[0], 1e-6)[0] == np.inf      # and the bound check reports a NaN as a failure
    # with a ZERO pad - what the suite used before - the same wrong kernel is silent
    silent = lrn_standin(np.nan_to_num(xfull, nan=0.0), 4, 8, reads_neighbours=True)
    assert np.array_equal(silent, good)


def maxpool_standin(xfull, coffset, c, k, clips):
    """k x k / stride 1 / pad k//2 MAX pooling of a channel slice of ONE image; the wrong one does not clip its windows to the image
    and reads what lies around it in memory instead: the previous / next row's pixels and, at the corners, the red zones."""
    _, h, w, cs = xfull.shape
    red = np.full((w + 1, cs), xfull[0, 0, 0, 0], xfull.dtype)      # (the buffer's first channel is slack: the red zones hold the same poison)
    flat = np.concatenate([red, xfull.reshape(-1, cs), red])
    out = np.full((h, w, c), -np.inf, np.float32)
    for oy in range(h):
        for ox in range(w):
            for iy in range(oy - k // 2, oy + k // 2 + 1):
                for ix in range(ox - k // 2, ox + k // 2 + 1):
                    if clips and not (0 <= iy < h and 0 <= ix < w):
                        continue
                    v = flat[w + 1 + iy * w + ix, coffset:coffset + c]
                    out[oy, ox] = np.where(v > out[oy, ox], v, out[oy, ox])
    return out


def test_a_consumed_pad_read_under_max_needs_the_huge_poison():
    rng = np.random.default_rng(2)
    x = -np.abs(rng.standard_normal((1, 4, 4, 5))).astype(np.float32) - 1      # all negative: a zero pad would win, too
    want = ref64.max_pool(x, 3, 1, 1)[0].transpose(0, 2, 3, 1)[0]
    for kind in ("nan", "huge"):
        xfull = poisoned_nhwc(x, 8, 4, poison=kind)
        assert np.array_equal(maxpool_standin(xfull, 4, 4, 3, clips=True), want)
        wrong = maxpool_standin(xfull, 4, 4, 3, clips=False)
        if kind == "nan":
            # `v > m` is false for a NaN: the over-read of the red zone in front of row 0 leaves no trace in the result ...
            assert poison_free(wrong, "nan") and np.array_equal(wrong[0, 0], want[0, 0])
        else:
            # ... and it does with the huge poison (the corner windows reach in front of / behind the image)
            assert not poison_free(wrong, "huge") and np.all(wrong[0, 0] == np.float32(3e38)) and np.all(wrong[-1, -1] == np.float32(3e38))
            assert np.array_equal(wrong[1:-1, 1:-1], want[1:-1, 1:-1])
    # a wrong channel offset reads the neighbour branch
    assert not poison_free(maxpool_standin(poisoned_nhwc(x, 8, 4, poison="huge"), 2, 4, 3, clips=True), "huge")


# ---- ref64 against the float32 oracle -------------------------------------------------------------------------------
CONV_CASES = [
    # cin, cout, k, stride, pad, h, w, n
    (4, 64, 7, 2, 3, 61, 45, 1), (16, 33, 5, 1, 2, 17, 28, 1), (24, 36, 5, 1, 2, 14, 14, 2), (40, 4, 3, 1, 1, 12, 7, 1),
    (96, 36, 3, 1, 1, 9, 11, 1), (16, 8, 7, 1, 3, 5, 4, 1), (1024, 4, 1, 1, 0, 9, 5, 1), (8, 8, 3, 2, 0, 15, 15, 3),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_the_float32_oracle_meets_the_derived_bound(case):
    """oracle/caffe_ref.py::conv2d (an OpenBLAS float32 GEMM over im2col) against the tap-by-tap float64 sum: every ELEMENT
    within dot_bound - border and corner pixels, whose magnitude term is small, included."""
    cin, cout, k, s, p, h, w, n = case
    rng = np.random.default_rng(hash(case) % 2**32)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    y64 = ref64.conv2d(x, wt, b, p, s)
    y32 = R.conv2d(x, wt, b, p, s)
    assert y32.shape == y64.shape == (n, cout, ref64.conv_out(h, k, p, s), ref64.conv_out(w, k, p, s))
    mag = ref64.conv2d_mag(x, wt, b, p, s)
    K = cin * k * k
    for allow in (ref64.dot_bound(K, mag), ref64.dot_bound_rms(K, mag)):
        ratio, at = ref64.worst(y32, y64, allow)
        assert ratio <= 1.0, "element %d: %.3g of its allowance" % (at, ratio)
    assert ref64.worst(y32, y64, ref64.dot_bound_rms(K, mag))[0] < 0.25      # (the margin the module text speaks of)
    # the sharp bound is not vacuous: an error in ONE corner pixel that the blob-wide criterion rel_err < 1e-4 lets through fails it
    wrong = y32.astype(np.float64)
    wrong[0, 0, 0, 0] += 0.9e-4 * np.abs(y64).max()
    assert np.abs(wrong - y64).max() / np.abs(y64).max() < 1e-4
    assert ref64.worst(wrong, y64, ref64.dot_bound_rms(K, mag))[0] > 1.0


def test_the_bound_tightens_where_windows_are_clipped():
    x = np.ones((1, 4, 6, 6), np.float32)
    w = np.ones((1, 4, 3, 3), np.float32)
    mag = ref64.conv2d_mag(x, w, None, 1, 1)[0, 0]
    assert mag[0, 0] == 16 and mag[0, 3] == 24 and mag[3, 3] == 36      # 4/9, 6/9, 9/9 of the window
    allow = ref64.dot_bound(36, mag)
    assert allow[0, 0] < allow[0, 3] < allow[3, 3]


def test_ref64_gradients_match_the_oracles_backward():
    rng = np.random.default_rng(3)
    for cin, cout, k, s, p, h, w in [(8, 12, 3, 1, 1, 7, 9), (4, 8, 5, 2, 2, 11, 10), (16, 4, 1, 1, 0, 5, 5)]:
        x = rng.standard_normal((2, cin, h, w)).astype(np.float32)
        wt = rng.standard_normal((cout, cin, k, k)).astype(np.float32)
        dy = rng.standard_normal((2, cout, ref64.conv_out(h, k, p, s), ref64.conv_out(w, k, p, s))).astype(np.float32)
        dw, db, dx = R.conv2d_backward(x, wt, dy, p, s)
        dw64, db64 = ref64.conv2d_wgrad(x, dy, k, p, s)
        assert np.allclose(dw, dw64, rtol=1e-4, atol=1e-4) and np.allclose(db, db64, rtol=1e-4, atol=1e-4)
        assert np.allclose(dx, ref64.conv2d_dgrad(dy, wt, p, s, h, w), rtol=1e-4, atol=1e-4)
        # <dy, conv(x)> == <dw, w> == <dx, x>: the three definitions agree with each other, not only with the oracle
        lhs = float((ref64.conv2d(x, wt, None, p, s) * dy).sum())
        assert np.isclose(lhs, float((dw64 * wt).sum()), rtol=1e-10) and np.isclose(lhs, float((ref64.conv2d_dgrad(dy, wt, p, s, h, w) * x).sum()), rtol=1e-10)


@pytest.mark.parametrize("k,s,p,h,w", [(3, 2, 0, 15, 21), (3, 1, 1, 9, 7), (2, 2, 0, 8, 6), (3, 2, 1, 10, 11), (3, 1, 1, 1, 6), (5, 3, 2, 7, 1)])
def test_ref64_pooling_matches_the_oracle(k, s, p, h, w):
    rng = np.random.default_rng(4)
    x = -np.abs(rng.standard_normal((2, 5, h, w))).astype(np.float32)
    x[0, :, 0, 0] = x[0, :, 0, min(1, w - 1)]
    y, idx = ref64.max_pool(x, k, s, p)
    ry, ridx = R.max_pool(x, k, s, p, return_index=True)
    assert np.array_equal(y, ry) and np.array_equal(idx, ridx) and y.max() < 0      # the padding never wins
    assert np.allclose(ref64.ave_pool(x, k, s, p), R.ave_pool(x, k, s, p), rtol=1e-6, atol=1e-7)


def test_ref64_pointwise_and_losses_match_the_oracle():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 10, 3, 4)) * 30).astype(np.float32)
    for ls in (5, 3):
        y, sc = ref64.lrn(x, ls, 1e-4, 0.75, 1.0)
        ry, rsc = R.lrn_across(x, ls, 1e-4, 0.75, 1.0, return_scale=True)
        assert np.allclose(y, ry, rtol=1e-5) and np.allclose(sc, rsc, rtol=1e-6)
    big = (rng.random((2, 5, 3, 3)) * 180 - 90).astype(np.float32)
    big[0, :, 1, 1] = 37.5                                     # a pixel of equal logits
    p = ref64.softmax(big)
    assert np.all(np.isfinite(p)) and np.allclose(p.sum(axis=1), 1, rtol=1e-12) and np.allclose(p[0, :, 1, 1], 0.2, rtol=1e-12)
    assert np.allclose(p, R.softmax(big), rtol=1e-4, atol=1e-30)
    s = ref64.sigmoid(np.array([-100.0, -1.0, 0.0, 1.0, 100.0]))
    assert s[0] == np.exp(-100.0) / (1 + np.exp(-100.0)) and s[2] == 0.5 and s[4] == 1.0 and np.allclose(s[1] + s[3], 1)
    a, b = rng.standard_normal((2, 2, 4, 3, 3)).astype(np.float32)
    assert np.isclose(ref64.l1_loss(a, b, 2)[0], R.l1_loss(a, b), rtol=1e-5) and np.allclose(ref64.l1_loss(a, b, 2, 0.5)[1], R.l1_loss_grad(a, b, 0.5))
    assert np.isclose(ref64.euclidean_loss(a, b, 2)[0], R.euclidean_loss(a, b), rtol=1e-5)
    assert np.allclose(ref64.euclidean_loss(a, b, 2, 2.0)[1], R.euclidean_loss_grad(a, b, 2.0), rtol=1e-5, atol=1e-7)
    sc = rng.standard_normal((2, 5, 3, 3)).astype(np.float32) * 4
    lab = rng.integers(0, 5, (2, 3, 3)).astype(np.float32)
    lab[0, 0, 0] = 255
    loss, dx = ref64.softmax_loss(sc, lab, True, 255, 1.0)
    assert np.isclose(loss, R.softmax_loss(sc, lab, True, 255), rtol=1e-5)
    assert np.allclose(dx, R.softmax_loss_grad(sc, lab, True, 255, 1.0), rtol=1e-4, atol=1e-7) and not dx[0, :, 0, 0].any()
    c, k, st, pd, h = 6, 4, 2, 1, 5
    xd = rng.standard_normal((2, c, h, h)).astype(np.float32)
    wd = rng.standard_normal((c, 1, k, k)).astype(np.float32)
    yd = ref64.deconv_depthwise(xd, wd[:, 0], None, k, st, pd)
    assert np.allclose(yd, R.deconv2d(xd, wd, None, pd, st, group=c), rtol=1e-5, atol=1e-5)
    dy = rng.standard_normal(yd.shape).astype(np.float32)
    dxd = ref64.deconv_depthwise_bwd(dy, wd[:, 0], k, st, pd, h, h)
    assert np.allclose(dxd, R.deconv2d_backward_data(dy, wd, pd, st, group=c), rtol=1e-5, atol=1e-5)
    assert np.isclose(float((yd * dy).sum()), float((dxd * xd).sum()), rtol=1e-10)


# ---- byte kernels: what the guarded byte / integer tests (tests/test_gpu_guarded_{augment,scene,masks,detect}.py) rely on ----
def invert_standin(src: GuardedBuffer, dst: GuardedBuffer, count: int, skip=(), extra=0):
    """dst[i] = 255 - src[i] for i < count + extra, except the indices in `skip`: a byte kernel that forgets elements / runs past the end."""
    s = src.handle[src.offset:src.offset + count + extra]
    d = dst.handle[dst.offset:dst.offset + count + extra]
    keep = np.ones(count + extra, bool)
    keep[list(skip)] = False
    d[keep] = 255 - s[keep]


def test_a_byte_written_just_behind_a_byte_payload_is_reported():
    from gpu_util import complement
    img = np.arange(35, dtype=np.uint8)                       # 35 bytes at the end of their allocation: an odd start address
    want = 255 - img
    with Guards(mem=HOST) as g:
        src, dst = g.put(img, at_end=True), g.put(complement(want), at_end=True)
        assert src.ptr % 2 == 1
        invert_standin(src, dst, img.size)
        assert np.array_equal(dst.read(img.shape, np.uint8), want) and src.unchanged()
    with pytest.raises(GuardError, match=r"behind the payload \(35 bytes\): first modified byte at \+35, last at \+35"):
        with Guards(mem=HOST) as g:
            src, dst = g.put(img, at_end=True), g.put(complement(want), at_end=True, name="dst")
            invert_standin(src, dst, img.size, extra=1)       # (the source's red zone holds 0xC0 there: 255 - 0xC0 is stored)


def test_an_unwritten_byte_fails_the_equality_because_of_the_complement_prefill():
    """0xC0, the poison byte, is a legitimate pixel: an output prefilled with poison would PASS where the expected byte is 0xC0 and was never
    written.  Prefilled with ~want, no unwritten byte can equal its expected value."""
    from gpu_util import complement
    img = np.full(64, 255 - 0xC0, np.uint8)                   # every expected byte is the poison byte
    want = 255 - img
    assert np.all(want == poison_value("nan", np.uint8))
    with Guards(mem=HOST) as g:
        src, dst = g.put(img, at_end=True), g.put(want.nbytes)                    # poison prefill (C0 7F C0 7F ..): the forgotten byte 16 goes unnoticed
        invert_standin(src, dst, img.size, skip=(16,))
        assert np.array_equal(dst.read(img.shape, np.uint8), want)
    with Guards(mem=HOST) as g:
        src, dst = g.put(img, at_end=True), g.put(complement(want))
        invert_standin(src, dst, img.size, skip=(16,))
        got = dst.read(img.shape, np.uint8)
        assert np.nonzero(got != want)[0].tolist() == [16]
    assert np.all(complement(np.arange(256, dtype=np.uint8)) != np.arange(256, dtype=np.uint8))


def test_a_nan_score_reads_as_background_and_3e38_as_foreground():
    """fcn_score_masks' chain - threshold, x 255, clamp, truncating cast through int32, low byte - on numpy stand-ins: a consumed NaN
    gives byte 0 (background: nothing to see), 3e38 gives 128.  Hence poison='huge' for score maps; `NaN >= thresh` is false as well, so
    the same holds for the coverage maps of fcn_detect_decode_group."""
    def fmaxf(a, b):                                                               # C semantics: a NaN operand yields the other one
        return b if np.isnan(a) else a if np.isnan(b) else max(a, b)

    def fminf(a, b):
        return b if np.isnan(a) else a if np.isnan(b) else min(a, b)

    def chain(v, thresh=np.float32(0.5)):
        v = np.float32(v)
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.float32(0) if v < thresh else v                                 # (NaN < thresh is false: the NaN is kept)
            v = np.float32(v * np.float32(255))
        v = fminf(fmaxf(v, np.float32(-2147483648.0)), np.float32(2147483520.0))
        return int(np.trunc(np.float64(v))) & 0xFF

    assert chain(poison_value("nan", np.float32)) == 0                             # -2147483648 & 0xFF
    assert chain(poison_value("huge", np.float32)) == 128 and chain(1.0) == 255 and chain(1.5) == 126 and chain(0.49) == 0
    assert not (poison_value("nan", np.float32) >= np.float32(0.5)) and poison_value("huge", np.float32) >= np.float32(0.5)
