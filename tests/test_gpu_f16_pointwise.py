"""Guard-banded, poisoned-buffer parity of the half-float pointwise kernels of the VGG16 nets (AVE pooling, depthwise deconvolution,
Eltwise, Softmax, channel copy) against the float64 reference on the SAME f16-rounded inputs, -m gpu.

As tests/test_gpu_guarded.py: every tensor lives in a guarded allocation, pad channels of x and every channel of y outside
[y_coffset, y_coffset + C) hold poison, the result must carry no trace of it and the slack must be bit-identical afterwards.  Bounds:
float32 outputs within ref64's element-wise allowance (a few 1e-6 of the element's own magnitude sum); half outputs equal the float64
result rounded to half, or differ from it by one f16 ulp on at most 1e-3 of the elements (a float32 sum that lands next to a half-way
point rounds the other way; the fraction observed is printed as `ULP <what> <fraction>`).  Every kernel runs twice: identical bits."""
import numpy as np
import pytest

import ref64
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu
H16 = np.float16


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def r16(a):
    return np.asarray(a).astype(H16).astype(np.float32)


def within(y, y64, allow, what):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def half_order(a):
    """Halves as integers in value order (consecutive halves are consecutive integers, -0 and +0 are both 0)."""
    bits = np.ascontiguousarray(a).view(np.uint16).astype(np.int32)
    return np.where(bits & 0x8000, -(bits & 0x7FFF), bits)


def half_exact(y, y64, what, frac=1e-3, allow=None):
    """y (float16) against the float64 result: the correctly rounded half, or its neighbour on at most `frac` of the elements.
    `allow`: the element-wise float32 allowance of a sum that cancels (a result of 1e-4 from terms of size 1 carries the terms'
    float32 rounding, several ulps of so small a half) - such an element may be further than the neighbour but not than `allow`."""
    want = np.asarray(y64).astype(H16)
    assert y.dtype == H16 and y.shape == want.shape
    bad = y != want
    near = np.abs(half_order(y) - half_order(want)) <= 1
    if allow is not None:
        near |= np.abs(y.astype(np.float64) - y64) <= allow
    print("ULP %s %.3g" % (what, bad.mean()))
    assert np.all(near[bad]), "%s: an element is more than one f16 ulp from the rounded float64 result" % what
    # (a tensor of a few hundred elements may hold three such elements)
    assert bad.sum() <= max(3, frac * bad.size), "%s: %.3g of the elements are not the correctly rounded half" % (what, bad.mean())


def twice(run, read):
    run()
    first = read().copy()
    run()
    again = read()
    assert np.array_equal(first.view(np.uint8), again.view(np.uint8)), "two runs differ"
    return first


# ---- AVE pooling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,h,w,k,s,p,xcs,ycs,yo", [
    (1, 512, 56, 56, 56, 56, 0, 512, 512, 0),        # the pyramid levels of train/bounding_box/deploy.prototxt
    (2, 512, 56, 56, 28, 28, 0, 512, 512, 0),
    (1, 512, 56, 56, 14, 14, 0, 512, 512, 0),
    (1, 512, 56, 56, 8, 8, 0, 512, 512, 0),
    (2, 24, 56, 56, 28, 28, 0, 32, 40, 8),           # three groups in a wider pixel, into a slice of a wider buffer
    (2, 11, 9, 7, 3, 2, 1, 16, 24, 8),               # padded windows (the divisor counts the padding), a partial group
    (2, 20, 13, 13, 9, 4, 2, 24, 24, 0),             # cooperative path with clipped windows and a partial last group
])
def test_avepool(g, n, c, h, w, k, s, p, xcs, ycs, yo):
    rng = np.random.default_rng(100 + k + c)
    x = r16(rng.standard_normal((n, c, h, w)) + 1.5)      # a mean far from zero: a wrong divisor shows
    want = ref64.ave_pool(x, k, s, p)
    oh, ow = want.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, 0, dtype=H16), at_end=True, name="x")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=H16), name="y")
    full = twice(lambda: L.call("fcn_avepool_fwd_f16", xd.ptr, yd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, None),
                 lambda: yd.read((n, oh, ow, ycs), H16))
    y = np.ascontiguousarray(full[..., yo:yo + c].transpose(0, 3, 1, 2))
    assert poison_free(y) and slice_untouched(full, yo, c)
    within(y.astype(np.float32), want, ref64.dot_bound_f16(k * k, ref64.ave_pool(np.abs(x), k, s, p), want), "avepool f16 k%d" % k)
    # the float32 sum of k * k terms is sqrt(k * k) u off the float64 sum (3e-7 of the value at 196 terms, 1e-6 at 3136) while a half
    # is 5e-4 .. 1e-3 wide: the share of sums that land on the other side of a half-way point grows with the window
    half_exact(y, want, "avepool k%d" % k, 1e-3 if k * k <= 16 else 1e-2 if k * k <= 1024 else 2e-2)


# ---- depthwise deconvolution ---------------------------------------------------------------------------------------------------------
DECONV = [
    # c, k, s, p, h, w, x_cstride, y_cstride (channels), y_coffset
    (44, 8, 4, 2, 3, 2, 48, 48, 0),          # upscore_pool5_bbox
    (11, 4, 2, 1, 6, 4, 16, 16, 0),          # upscore_pool5 / upscore_pool4
    (512, 4, 2, 1, 5, 3, 512, 512, 0),       # conv5_3/upsample
    (11, 16, 8, 4, 7, 5, 16, 32, 8),         # upscore_pool3, into a slice of a wider buffer
    (128, 56, 28, 14, 1, 1, 128, 128, 0),    # the pyramid's way back to 28 x 28
    (128, 28, 14, 7, 2, 2, 128, 128, 0),
    (128, 13, 7, 3, 4, 4, 128, 128, 0),
    (128, 8, 4, 2, 7, 7, 128, 256, 64),
    (5, 3, 1, 1, 4, 3, 8, 16, 8),            # three taps per axis: the form without tap registers
    (11, 16, 8, 4, 56, 56, 16, 16, 0),       # 448 x 448 outputs: several rows per lane
]


@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("c,k,s,p,h,w,xcs,ycs,yo", DECONV)
def test_depthwise_deconv(g, c, k, s, p, h, w, xcs, ycs, yo, out_f32):
    rng = np.random.default_rng(200 + k + c)
    n = 2
    x = r16(rng.standard_normal((n, c, h, w)))
    wt = rng.standard_normal((c, k, k)).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    want = ref64.deconv_depthwise(x, wt, b, k, s, p)
    mag = ref64.deconv_depthwise(np.abs(x), np.abs(wt), np.abs(b), k, s, p)
    oh, ow = want.shape[2:]
    dt = np.float32 if out_f32 else H16
    xd = g.put(poisoned_nhwc(x, xcs, 0, dtype=H16), at_end=True, name="x")
    wd, bd = g.put(wt, at_end=True, name="w"), g.put(b, at_end=True, name="bias")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=dt), name="y")
    full = twice(lambda: L.call("fcn_deconv_depthwise_fwd_f16", xd.ptr, wd.ptr, bd.ptr, yd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, out_f32, None),
                 lambda: yd.read((n, oh, ow, ycs), dt))
    y = np.ascontiguousarray(full[..., yo:yo + c].transpose(0, 3, 1, 2))
    assert poison_free(y) and slice_untouched(full, yo, c)
    taps = (k + s - 1) // s
    if out_f32:
        within(y, want, ref64.dot_bound_rms(taps * taps, mag), "deconv f32 out k%d s%d" % (k, s))
        assert np.abs(y - want).max() <= 1e-5 * mag.max()
    else:
        allow = ref64.dot_bound_f16(taps * taps, mag, want)
        within(y.astype(np.float32), want, allow, "deconv k%d s%d" % (k, s))
        half_exact(y, want, "deconv k%d s%d" % (k, s), allow=allow)


def test_depthwise_deconv_without_bias(g):
    c, k, s, p, h, w = 11, 4, 2, 1, 3, 5
    rng = np.random.default_rng(7)
    x = r16(rng.standard_normal((1, c, h, w)))
    wt = rng.standard_normal((c, k, k)).astype(np.float32)
    want = ref64.deconv_depthwise(x, wt, None, k, s, p)
    oh, ow = want.shape[2:]
    xd, wd = g.put(poisoned_nhwc(x, 16, 0, dtype=H16), at_end=True), g.put(wt, at_end=True)
    yd = g.put(poisoned((1, oh, ow, 12)), name="y")
    L.call("fcn_deconv_depthwise_fwd_f16", xd.ptr, wd.ptr, None, yd.ptr, 1, h, w, c, 16, k, s, p, oh, ow, 12, 0, 1, None)
    full = yd.read((1, oh, ow, 12))
    assert slice_untouched(full, 0, c)
    within(nchw(full, c), want, ref64.dot_bound_rms(4, ref64.deconv_depthwise(np.abs(x), np.abs(wt), None, k, s, p)), "deconv no bias")


# ---- Eltwise -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [8, 1000, 56 * 56 * 16])
def test_eltwise(g, count):
    rng = np.random.default_rng(count)
    a, b = r16(rng.standard_normal((2, count)) * 4)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for op, want, ca, cb in [(L.ELT_SUM, a64 - 0.5 * b64, 1.0, -0.5), (L.ELT_PROD, a64 * b64, 0.0, 0.0), (L.ELT_MAX, np.maximum(a64, b64), 0.0, 0.0)]:
        ad, bd = g.put(a.astype(H16), at_end=True, name="a"), g.put(b.astype(H16), at_end=True, name="b")
        yd = g.put(poisoned(count, dtype=H16), at_end=True, name="y")
        y = twice(lambda: L.call("fcn_eltwise_fwd_f16", ad.ptr, bd.ptr, yd.ptr, count, op, ca, cb, None), lambda: yd.read((count,), H16))
        assert poison_free(y)
        half_exact(y, want, "eltwise %d" % op)
        # in place: y is a (the engine chains a three-input Eltwise through its top)
        L.call("fcn_eltwise_fwd_f16", ad.ptr, bd.ptr, ad.ptr, count, op, ca, cb, None)
        assert np.array_equal(ad.read((count,), H16).view(np.uint16), y.view(np.uint16))


def test_eltwise_max_ignores_nothing_but_takes_the_larger(g):
    """MAX with the huge poison behind the range: the kernel reads `count` halves and not one more."""
    count = 24
    a = np.linspace(-3, 3, count).astype(H16)
    b = a[::-1].copy()
    ad, bd = g.put(a, at_end=True, poison="huge"), g.put(b, at_end=True, poison="huge")
    yd = g.put(poisoned(count, poison="huge", dtype=H16), at_end=True, poison="huge", name="y")
    L.call("fcn_eltwise_fwd_f16", ad.ptr, bd.ptr, yd.ptr, count, L.ELT_MAX, 0.0, 0.0, None)
    y = yd.read((count,), H16)
    assert np.array_equal(y, np.maximum(a, b)) and poison_free(y, "huge")


# ---- Softmax -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("pixels,c,xcs,ycs", [(3, 4, 8, 8), (1003, 11, 16, 16), (56 * 56, 21, 24, 32), (77, 40, 40, 48)])
def test_softmax(g, pixels, c, xcs, ycs, out_f32):
    rng = np.random.default_rng(300 + c)
    x = r16(rng.random((pixels, c)) * 60 - 30)
    x[0] = 7.5                                      # equal logits
    x[-1] = r16(np.linspace(-30, 30, c))
    dt = np.float32 if out_f32 else H16
    wide = poisoned((pixels, xcs), dtype=H16)
    wide[:, :c] = x
    xd, yd = g.put(wide, at_end=True, name="x"), g.put(poisoned((pixels, ycs), dtype=dt), at_end=True, name="y")
    out = twice(lambda: L.call("fcn_softmax_fwd_f16", xd.ptr, yd.ptr, pixels, c, xcs, ycs, out_f32, None), lambda: yd.read((pixels, ycs), dt))
    y = out[:, :c]
    want = ref64.softmax(x)
    assert poison_free(y) and slice_untouched(out, 0, c)
    if out_f32:
        assert np.all(y[0] == y[0, 0]) and abs(float(y[0, 0]) * c - 1) < 1e-6
        assert np.abs(y.astype(np.float64).sum(axis=1) - 1).max() < 1e-5
        # halves subtract exactly; exp and the sum of C terms carry a few float32 roundings each
        within(y, want, (8 + c) * ref64.U32 * want + 1e-44, "softmax f32 out C%d" % c)
    else:
        half_exact(y, want, "softmax C%d" % c)


# ---- channel copy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels,c,scs,sco,dcs,dco", [
    (784, 128, 128, 0, 1536, 1152),      # a branch of the 1536-channel concat
    (33, 24, 40, 8, 48, 16),             # aligned offsets on both sides
    (10, 11, 16, 0, 32, 8),              # partial last group
    (10, 5, 16, 3, 24, 9),               # unaligned offsets: one half per lane
    (7, 13, 24, 8, 16, 3),
    (1, 1, 8, 7, 8, 0),
])
def test_copy_channels(g, pixels, c, scs, sco, dcs, dco):
    rng = np.random.default_rng(400 + c)
    src = rng.standard_normal((pixels, c)).astype(H16)
    wide = poisoned((pixels, scs), dtype=H16)
    wide[:, sco:sco + c] = src
    sd, dd = g.put(wide, at_end=True, name="src"), g.put(poisoned((pixels, dcs), dtype=H16), at_end=True, name="dst")
    out = twice(lambda: L.call("fcn_copy_channels_f16", sd.ptr, dd.ptr, pixels, c, scs, sco, dcs, dco, None), lambda: dd.read((pixels, dcs), H16))
    assert np.array_equal(out[:, dco:dco + c].view(np.uint16), src.view(np.uint16)) and slice_untouched(out, dco, c)
