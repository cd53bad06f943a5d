"""Guard-banded, poisoned-buffer parity of the transposed convolution (csrc/tconv.hip) against the float64 scatter reference
(tests/ref_tconv64.py), -m gpu.  As in tests/test_gpu_guarded.py: every tensor lives in a guarded allocation, inputs are slices of
wider pixels whose other channels (the pad channels Ca .. round4(Ca)-1 included) hold NaN, outputs are slices of poison-filled
buffers; a case passes when the result meets the element-wise bound c * eps * K * magnitude, carries no poison, the neighbouring
channels and the red zones are bit-identical afterwards, and a second launch gives the same bits."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_tconv64 as T
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def within(y, y64, allow, what=""):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def r4(c):
    return (c + 3) // 4 * 4


def packed_bank(g, w):
    """(Ca, Cb, kh, kw) blob -> the kernel's bank, packed ON THE DEVICE from the engine's blob layout; checked against the host packing."""
    ca, cb, kh, kw = w.shape
    src = g.put(T.device_blob(w), at_end=True, name="blob")
    floats = int(L.load().fcn_tconv_bank_floats(ca, cb, kh, kw))
    assert floats == kh * kw * cb * r4(ca)
    dst = g.put(floats * 4, name="bank")
    L.call("fcn_tconv_bank_pack_f32", src.ptr, dst.ptr, ca, cb, r4(cb), kh, kw, None)
    L.call("fcn_device_sync")
    assert np.array_equal(dst.read((kh, kw, cb, r4(ca))), T.pack_bank(w)), "bank packing differs from the host statement"
    return dst


def tconv_desc(ad, wd, bd, yd, n, h, w, ca, acs, cb, kh, kw, pad, s, oh, ow, bcs, bco, flags=0, y2d=None, y2cs=0, y2co=0):
    d = L.TConvDesc()
    d.a, d.w, d.bias, d.b = ad.ptr, wd.ptr, (bd.ptr if bd is not None else None), yd.ptr
    d.y2 = y2d.ptr if y2d is not None else None
    d.N, d.H, d.W, d.Ca, d.a_cstride = n, h, w, ca, acs
    d.Cb, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = cb, kh, kw, pad, s, oh, ow
    d.b_cstride, d.b_coffset, d.y2_cstride, d.y2_coffset, d.flags = bcs, bco, y2cs, y2co, flags
    return d


def launch(g, descs, twice=None):
    """prepare + launch; with twice = (buffer, shape): a second launch of the same plan must give the same bits."""
    lib = L.load()
    n = len(descs)
    arr = (L.TConvDesc * n)(*descs)
    wsb = int(lib.fcn_tconv2d_workspace_bytes(arr, n))
    assert wsb > 0
    ws = g.put(wsb, name="workspace")
    plan = L.TConvPlan()
    assert int(lib.fcn_tconv2d_num_configs()) >= 1
    L.call("fcn_tconv2d_prepare", arr, n, ws.ptr, -1, C.byref(plan))
    assert plan.n == n and plan.total_tiles > 0
    L.call("fcn_tconv2d_f32", C.byref(plan), None)
    L.call("fcn_device_sync")
    if twice is not None and not (descs[0].flags & L.CONV_ACCUM):
        buf, shape = twice
        first = buf.read(shape).view(np.uint32).copy()
        L.call("fcn_tconv2d_f32", C.byref(plan), None)
        L.call("fcn_device_sync")
        assert np.array_equal(first, buf.read(shape).view(np.uint32)), "two launches on the same inputs differ"
    return plan


def run_case(g, seed, n, ca, cb, h, w, kh, kw, s, pad, extra=(0, 0), flags="", acs=None, bcs=None, bco=0, bias=True):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, ca, h, w)).astype(np.float32)
    wt = (rng.standard_normal((ca, cb, kh, kw)) / np.sqrt(ca)).astype(np.float32)
    b = rng.standard_normal(cb).astype(np.float32) if bias else None
    oh, ow = T.out_size(h, kh, s, pad) + extra[0], T.out_size(w, kw, s, pad) + extra[1]
    acs, bcs = acs or r4(ca), bcs or r4(cb) + bco
    base = rng.standard_normal((n, cb, oh, ow)).astype(np.float32)
    act = np.maximum(rng.standard_normal((n, cb, oh, ow)), 0).astype(np.float32)
    ad = g.put(poisoned_nhwc(a, acs, 0), at_end=True, name="a")
    wd = packed_bank(g, wt)
    bd = g.put(b, at_end=True, name="bias") if bias else None
    yd = g.put(poisoned_nhwc(base, bcs, bco) if "ACCUM" in flags else poisoned((n, oh, ow, bcs)), at_end=True, name="b")
    y2cs, y2co = bcs + 4, 4
    y2d = g.put(poisoned_nhwc(act, y2cs, y2co), at_end=True, name="y2") if "MASK" in flags else None
    fl = sum({"RELU": L.CONV_RELU, "ACCUM": L.CONV_ACCUM, "MASK": L.CONV_MASK}[f] for f in flags.split("+") if f)
    d = tconv_desc(ad, wd, bd, yd, n, h, w, ca, acs, cb, kh, kw, pad, s, oh, ow, bcs, bco, fl, y2d, y2cs, y2co)
    launch(g, [d], twice=(yd, (n, oh, ow, bcs)))
    full = yd.read((n, oh, ow, bcs))
    y = nchw(full, cb, bco)
    y64, mag = T.tconv2d(a, wt, b, pad, s, (oh, ow)), T.tconv2d_mag(a, wt, b, pad, s, (oh, ow))
    if "ACCUM" in flags:
        y64, mag = y64 + base, mag + np.abs(base)
    if "RELU" in flags:
        y64 = np.maximum(y64, 0)
    if "MASK" in flags:
        y64 = y64 * (act > 0)
    what = "tconv k%dx%d s%d p%d %s" % (kh, kw, s, pad, flags)
    assert poison_free(y), "%s: poison (a pad channel, a neighbouring channel or a red zone) reached the result" % what
    taps = -(-kh // s) * -(-kw // s)
    within(y, y64, ref64.dot_bound(taps * ca, mag), what)
    assert slice_untouched(full, bco, cb), "%s: channels of b outside the slice were written" % what
    if "MASK" in flags:
        assert np.all(y[act <= 0] == 0)
        assert np.array_equal(y2d.read((n, oh, ow, y2cs)).view(np.uint32), poisoned_nhwc(act, y2cs, y2co).view(np.uint32)), "y2 was written"
    return y, y64


# k, stride: the shape list of include/fcnhip.h's contract
KS = [(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (7, 2), (3, 3), (16, 8), (32, 16), (2, 4)]


@pytest.mark.parametrize("k,s", KS)
def test_shape_list_every_pad_class(g, k, s):
    """Odd H / W, channel counts off the tile and off 4, N = 2; pads 0, k // 2, k - 1; the largest legal output size too."""
    for i, pad in enumerate(sorted({0, k // 2, k - 1})):
        h, w = (3, 5) if k >= 16 else (7, 9)
        if T.out_size(h, k, s, pad) <= 0:
            continue
        run_case(g, 10 * k + s + i, 2, 5, 7, h, w, k, k, s, pad)
        run_case(g, 11 * k + s + i, 1, 3, 6, h, w, k, k, s, pad, extra=(s - 1, s - 1 if s > 1 else 0), bcs=16, bco=4)


@pytest.mark.parametrize("flags", ["", "RELU", "ACCUM", "MASK", "ACCUM+MASK", "ACCUM+RELU"])
@pytest.mark.parametrize("k,s,pad", [(3, 2, 1), (4, 2, 1), (16, 8, 4), (2, 4, 0)])
def test_epilogues_in_a_channel_slice(g, flags, k, s, pad):
    """bias / ReLU / accumulate / mask, the output a slice of a wider pixel whose neighbours must stay poisoned."""
    run_case(g, 5 + k, 2, 6, 10, 5, 7, k, k, s, pad, extra=(1, 0), flags=flags, acs=12, bcs=24, bco=8)
    run_case(g, 6 + k, 1, 4, 3, 5, 4, k, k, s, pad, flags=flags, bcs=8, bco=4, bias=False)


@pytest.mark.parametrize("ca,cb", [(1, 1), (2, 3), (17, 65), (72, 40), (130, 70)])
def test_channel_counts_across_tiles_and_chunks(g, ca, cb):
    """1 channel; Ca past one 16-channel chunk and off 4; Cb past one 64-channel block; more than 64 lattice pixels per phase."""
    run_case(g, ca + cb, 2, ca, cb, 9, 11, 3, 3, 2, 1, extra=(1, 1))
    run_case(g, ca * cb, 1, ca, cb, 5, 6, 4, 4, 2, 1, flags="ACCUM")


def test_rectangular_kernels(g):
    run_case(g, 1, 2, 5, 6, 5, 7, 3, 5, 2, 1)
    run_case(g, 2, 1, 4, 4, 6, 5, 4, 2, 2, 0, extra=(1, 1), flags="RELU")
    run_case(g, 3, 1, 4, 8, 4, 5, 1, 3, 3, 0)


def test_stride_one_equals_the_flipped_correlation(g):
    y, _ = run_case(g, 4, 1, 8, 8, 6, 7, 3, 3, 1, 1)
    assert y.shape == (1, 8, 6, 7)


def test_several_problems_in_one_launch(g):
    """Problems of different stride and size in one plan: grid rows / columns past a smaller problem's phases and tiles return."""
    rng = np.random.default_rng(9)
    specs = [(2, 5, 7, 7, 9, 3, 2, 1), (1, 8, 4, 3, 4, 16, 8, 4), (1, 3, 70, 5, 5, 2, 4, 0)]
    descs, outs = [], []
    for n, ca, cb, h, w, k, s, pad in specs:
        a = rng.standard_normal((n, ca, h, w)).astype(np.float32)
        wt = rng.standard_normal((ca, cb, k, k)).astype(np.float32)
        b = rng.standard_normal(cb).astype(np.float32)
        oh, ow = T.out_size(h, k, s, pad), T.out_size(w, k, s, pad)
        ad, wd, bd = g.put(poisoned_nhwc(a, r4(ca), 0), at_end=True), packed_bank(g, wt), g.put(b, at_end=True)
        yd = g.put(poisoned((n, oh, ow, r4(cb) + 4)), at_end=True)
        descs.append(tconv_desc(ad, wd, bd, yd, n, h, w, ca, r4(ca), cb, k, k, pad, s, oh, ow, r4(cb) + 4, 4))
        outs.append((yd, (n, oh, ow, r4(cb) + 4), a, wt, b, pad, s, cb, k, ca))
    plan = launch(g, descs)
    assert plan.grid_y == 64
    for yd, shape, a, wt, b, pad, s, cb, k, ca in outs:
        full = yd.read(shape)
        y = nchw(full, cb, 4)
        assert poison_free(y) and slice_untouched(full, 4, cb)
        within(y, T.tconv2d(a, wt, b, pad, s), ref64.dot_bound(-(-k // s) ** 2 * ca, T.tconv2d_mag(a, wt, b, pad, s)), "grouped tconv")


def test_data_gradient_of_a_strided_convolution(g):
    """The use the training engine makes of it: a = dY, the Convolution's own OHWI bank packed on the device, dX of the input's size
    with rows / columns under no window written as zeros."""
    rng = np.random.default_rng(11)
    n, cin, cout, h0, w0, k, s, pad = 2, 6, 9, 12, 10, 3, 2, 0       # (12 - 3) % 2 = 1: the last row of X is under no window
    w = rng.standard_normal((cout, cin, k, k)).astype(np.float32)
    oh, ow = ref64.conv_out(h0, k, pad, s), ref64.conv_out(w0, k, pad, s)
    dy = rng.standard_normal((n, cout, oh, ow)).astype(np.float32)
    ad = g.put(poisoned_nhwc(dy, r4(cout), 0), at_end=True)
    wd = packed_bank(g, w)                                           # (Ca = Cout, Cb = Cin): the blob is the bank as it stands
    xd = g.put(poisoned((n, h0, w0, r4(cin))), at_end=True)
    launch(g, [tconv_desc(ad, wd, None, xd, n, oh, ow, cout, r4(cout), cin, k, k, pad, s, h0, w0, r4(cin), 0)], twice=(xd, (n, h0, w0, r4(cin))))
    full = xd.read((n, h0, w0, r4(cin)))
    dx = nchw(full, cin, 0)
    want = ref64.conv2d_dgrad(dy, w, pad, s, h0, w0)
    mag = ref64.conv2d_dgrad(np.abs(dy), np.abs(w), pad, s, h0, w0)
    assert poison_free(dx) and slice_untouched(full, 0, cin)
    within(dx, want, ref64.dot_bound(4 * cout, mag), "strided dgrad")
    assert np.all(dx[:, :, -1, :] == 0.0)


@pytest.mark.parametrize("pixels,c,cs,co", [(1, 1, 4, 0), (37, 5, 8, 2), (300, 21, 24, 0), (1025, 3, 4, 1)])
def test_channel_sum(g, pixels, c, cs, co):
    rng = np.random.default_rng(pixels)
    dy = rng.standard_normal((1, c, pixels, 1)).astype(np.float32)
    dd = g.put(poisoned_nhwc(dy, cs, co), at_end=True, name="dy")
    db = g.put(poisoned((c + 3,)), at_end=True, name="db")
    for _ in range(2):
        L.call("fcn_channel_sum_f32", dd.ptr, db.ptr, pixels, c, cs, co, None)
        L.call("fcn_device_sync")
        out = db.read((c + 3,))
        if _ == 0:
            first = out.view(np.uint32).copy()
    assert np.array_equal(first, out.view(np.uint32))
    want, mag = dy.astype(np.float64).sum(axis=(0, 2, 3)), np.abs(dy.astype(np.float64)).sum(axis=(0, 2, 3))
    assert poison_free(out[:c]) and np.all(np.isnan(out[c:]))
    within(out[:c], want, ref64.dot_bound(pixels, mag), "channel sum")
