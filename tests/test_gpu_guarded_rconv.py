"""Guard-banded, poisoned-buffer parity of the rectangular and dilated convolution (csrc/rconv.hip) against the float64 reference
(tests/ref_rconv64.py), -m gpu.  As in tests/test_gpu_guarded_tconv.py: every tensor lives in a guarded allocation, inputs are
channel windows of wider pixels whose other channels (the pad channels Cin .. round4(Cin)-1 included) hold NaN, outputs are slices of
poison-filled buffers; a case passes when the result meets the element-wise bound c * eps * K * magnitude, carries no poison, the
neighbouring channels and the red zones are bit-identical afterwards, and a second launch gives the same bits.  Every case runs under
every configuration 0 .. fcn_rconv2d_num_configs() - 1 as well as the built-in choice.  The rectangular cases come first; the square
dilated ones (equal axes: the conv5 / fc6 layers of DeepLab-LargeFOV, the ASPP branches) follow."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_rconv64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, pack_ohwi, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu

FLAGS = {"RELU": L.CONV_RELU, "ACCUM": L.CONV_ACCUM, "MASK": L.CONV_MASK}


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


def configs():
    return [-1] + list(range(int(L.load().fcn_rconv2d_num_configs())))


def rconv_desc(x_ptr, w_ptr, b_ptr, y_ptr, n, h, w, ci, xcs, co, k, pad, s, dil, oh, ow, ycs, yco, flags=0, y2_ptr=None, y2cs=0, y2co=0):
    d = L.RConvDesc()
    d.x, d.w, d.bias, d.y, d.y2 = x_ptr, w_ptr, b_ptr, y_ptr, y2_ptr
    d.N, d.H, d.W, d.Cin, d.x_cstride = n, h, w, ci, xcs
    d.Cout, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = co, k[0], k[1], pad[0], pad[1], s[0], s[1], oh, ow
    d.y_cstride, d.y_coffset, d.y2_cstride, d.y2_coffset, d.flags, d.dilation = ycs, yco, y2cs, y2co, flags, dil
    return d


def launch(g, descs, cfg=-1, twice=None):
    """prepare + launch; with twice = (buffer, shape): a second launch of the same plan must give the same bits."""
    lib = L.load()
    n = len(descs)
    arr = (L.RConvDesc * n)(*descs)
    wsb = int(lib.fcn_rconv2d_workspace_bytes(arr, n))
    assert wsb > 0
    ws = g.put(wsb, name="workspace")
    plan = L.RConvPlan()
    L.call("fcn_rconv2d_prepare", arr, n, ws.ptr, cfg, C.byref(plan))
    assert plan.n == n and plan.total_tiles > 0 and (cfg < 0 or plan.cfg == cfg)
    L.call("fcn_rconv2d_f32", C.byref(plan), None)
    L.call("fcn_device_sync")
    if twice is not None and not (descs[0].flags & L.CONV_ACCUM):
        buf, shape = twice
        first = buf.read(shape).view(np.uint32).copy()
        L.call("fcn_rconv2d_f32", C.byref(plan), None)
        L.call("fcn_device_sync")
        assert np.array_equal(first, buf.read(shape).view(np.uint32)), "two launches on the same inputs differ"
    return plan


def run_fwd(g, seed, n, ci, co, h, w, k, s, pad, dil, flags="", xcs=None, xco=0, ycs=None, yco=0, bias=True, ref=None):
    """x: channels xco .. xco + ci - 1 of pixels of xcs channels (everything else NaN); y: channels yco .. of pixels of ycs channels.
    The reference is computed once and every configuration is held to it on fresh poisoned outputs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ci, h, w)).astype(np.float32)
    wt = (rng.standard_normal((co, ci) + tuple(k)) / np.sqrt(ci)).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32) if bias else None
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
    xcs, ycs = xcs or r4(ci) + xco, ycs or r4(co) + yco
    assert xco % 4 == 0 and xco + r4(ci) <= xcs
    base = rng.standard_normal((n, co, oh, ow)).astype(np.float32)
    act = np.maximum(rng.standard_normal((n, co, oh, ow)), 0).astype(np.float32)
    y64 = R.conv2d(x, wt, b, pad, s, dil) if ref is None else ref(x, wt, b)
    mag = R.conv2d_mag(x, wt, b, pad, s, dil)
    if "ACCUM" in flags:
        y64, mag = y64 + base, mag + np.abs(base)
    if "RELU" in flags:
        y64 = np.maximum(y64, 0)
    if "MASK" in flags:
        y64 = y64 * (act > 0)
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")
    wd = g.put(pack_ohwi(wt), at_end=True, name="bank")
    bd = g.put(b, at_end=True, name="bias") if bias else None
    y2cs, y2co = ycs + 4, 4
    y2_img = poisoned_nhwc(act, y2cs, y2co)
    y2d = g.put(y2_img, at_end=True, name="y2") if "MASK" in flags else None
    fl = sum(FLAGS[f] for f in flags.split("+") if f)
    for cfg in configs():
        yd = g.put(poisoned_nhwc(base, ycs, yco) if "ACCUM" in flags else poisoned((n, oh, ow, ycs)), at_end=True, name="y")
        d = rconv_desc(xd.ptr + 4 * xco, wd.ptr, bd.ptr if bias else None, yd.ptr, n, h, w, ci, xcs, co, k, pad, s, dil, oh, ow, ycs, yco, fl,
                       y2d.ptr if y2d is not None else None, y2cs, y2co)
        launch(g, [d], cfg, twice=(yd, (n, oh, ow, ycs)))
        full = yd.read((n, oh, ow, ycs))
        y = nchw(full, co, yco)
        what = "rconv cfg%d k%dx%d d%d s%dx%d p%dx%d %dx%d %d->%d %s" % (cfg, k[0], k[1], dil, s[0], s[1], pad[0], pad[1], h, w, ci, co, flags)
        assert poison_free(y), "%s: poison (a pad channel, a neighbouring channel or a red zone) reached the result" % what
        within(y, y64, ref64.dot_bound(k[0] * k[1] * ci, mag), what)
        assert slice_untouched(full, yco, co), "%s: channels of y outside the slice were written" % what
        assert xd.unchanged() and wd.unchanged(), "%s: an input was written" % what
        if "MASK" in flags:
            assert np.all(y[act <= 0] == 0)
            assert np.array_equal(y2d.read((n, oh, ow, y2cs)).view(np.uint32), y2_img.view(np.uint32)), "y2 was written"


# (kh, kw), (ph, pw), (sh, sw), dilation, (H, W)
GEOMETRIES = [((1, 7), (0, 3), (1, 1), 1, (7, 9)), ((7, 1), (3, 0), (1, 1), 1, (7, 9)),
              ((1, 7), (0, 3), (1, 1), 1, (6, 5)),      # the image is narrower than the filter
              ((1, 3), (0, 1), (1, 1), 1, (5, 6)), ((3, 1), (1, 0), (1, 1), 1, (5, 6)), ((3, 5), (0, 2), (2, 1), 1, (11, 9)),
              ((1, 5), (0, 0), (1, 2), 1, (8, 13)), ((3, 1), (2, 0), (1, 1), 2, (9, 10)), ((2, 3), (0, 2), (1, 1), 2, (8, 7)),
              ((3, 3), (1, 2), (1, 1), 1, (7, 9))]      # square kernel, unequal pads
IDS = ["k%dx%d-p%dx%d-s%dx%d-d%d-%dx%d" % (k + p + s + (d,) + hw) for k, p, s, d, hw in GEOMETRIES]


@pytest.mark.parametrize("k,pad,s,dil,hw", GEOMETRIES, ids=IDS)
def test_forward_geometries(g, k, pad, s, dil, hw):
    """Cin 5 (a pad channel of NaN), Cout 7 (a scalar tail); then both as channel windows of wider pixels."""
    run_fwd(g, 7 * k[0] + k[1] + dil, 1, 5, 7, hw[0], hw[1], k, s, pad, dil)
    run_fwd(g, 9 * k[0] + k[1] + dil, 1, 5, 7, hw[0], hw[1], k, s, pad, dil, xcs=12, xco=4, ycs=16, yco=4)


def test_a_square_problem_equals_the_dense_convolution(g):
    run_fwd(g, 1, 2, 5, 7, 7, 9, (3, 3), (1, 1), (1, 1), 1, ref=lambda x, w, b: ref64.conv2d(x, w, b, 1, 1))
    run_fwd(g, 2, 1, 4, 8, 9, 8, (3, 3), (2, 2), (0, 0), 1, ref=lambda x, w, b: ref64.conv2d(x, w, b, 0, 2))


def test_tile_crosses_a_row_end_and_the_image_boundary(g):
    """N = 2 on 9 x 11: 99 pixels per image, so the second 64-pixel tile holds the end of image 0 and the start of image 1."""
    run_fwd(g, 3, 2, 5, 7, 9, 11, (1, 7), (1, 1), (0, 3), 1)
    run_fwd(g, 4, 2, 8, 4, 9, 11, (7, 1), (1, 1), (3, 0), 1, flags="RELU")


@pytest.mark.parametrize("ci,co", [(1, 1), (17, 65), (72, 40), (130, 70)])
def test_channel_counts_across_tiles_and_chunks(g, ci, co):
    """1 channel; Cin past one 16-channel chunk and off 4; Cout past one 64-channel block."""
    run_fwd(g, ci + co, 2, ci, co, 9, 11, (1, 7), (1, 1), (0, 3), 1)
    run_fwd(g, ci * co, 1, ci, co, 5, 6, (3, 1), (1, 1), (2, 0), 2, flags="ACCUM")


@pytest.mark.parametrize("flags", ["", "RELU", "ACCUM", "MASK", "ACCUM+MASK"])
def test_epilogues_in_a_channel_slice(g, flags):
    """bias / ReLU / accumulate / mask; x a channel window of a wider pixel, y at coffset 8 and 4 of wider pixels, with and without bias."""
    run_fwd(g, 5, 2, 6, 10, 7, 9, (1, 7), (1, 1), (0, 3), 1, flags=flags, xcs=16, xco=4, ycs=24, yco=8)
    run_fwd(g, 6, 1, 4, 3, 5, 4, (3, 1), (1, 1), (1, 0), 1, flags=flags, ycs=8, yco=4, bias=False)


def test_two_geometries_of_one_input_in_one_launch(g):
    """The 8-grid module of Inception-v3: a 1x3 and a 3x1 problem read one blob in one launch - and a strided 3x5 one with them, so that
    the problems of the plan differ in their pixel counts too."""
    rng = np.random.default_rng(9)
    n, ci, h, w = 2, 6, 8, 7
    x = rng.standard_normal((n, ci, h, w)).astype(np.float32)
    xd = g.put(poisoned_nhwc(x, r4(ci), 0), at_end=True, name="x")
    for cfg in configs():
        descs, outs = [], []
        for (k, pad, s), co in zip((((1, 3), (0, 1), (1, 1)), ((3, 1), (1, 0), (1, 1)), ((3, 5), (0, 2), (2, 1))), (7, 70, 9)):
            wt = rng.standard_normal((co, ci) + k).astype(np.float32)
            b = rng.standard_normal(co).astype(np.float32)
            wd, bd = g.put(pack_ohwi(wt), at_end=True), g.put(b, at_end=True)
            ycs = r4(co) + 4
            oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, 1)
            yd = g.put(poisoned((n, oh, ow, ycs)), at_end=True)
            descs.append(rconv_desc(xd.ptr, wd.ptr, bd.ptr, yd.ptr, n, h, w, ci, r4(ci), co, k, pad, s, 1, oh, ow, ycs, 4))
            outs.append((yd, ycs, wt, b, k, pad, s, co, oh, ow))
        plan = launch(g, descs, cfg)
        assert plan.n == 3 and plan.grid_y == 1
        for yd, ycs, wt, b, k, pad, s, co, oh, ow in outs:
            full = yd.read((n, oh, ow, ycs))
            y = nchw(full, co, 4)
            assert poison_free(y) and slice_untouched(full, 4, co)
            within(y, R.conv2d(x, wt, b, pad, s, 1), ref64.dot_bound(k[0] * k[1] * ci, R.conv2d_mag(x, wt, b, pad, s, 1)), "shared k%dx%d" % k)
    assert xd.unchanged()


def flipped_on_device(g, wt):
    """(Cout, Cin, kh, kw) blob -> its OHWI bank, flipped ON THE DEVICE by fcn_conv_weights_flip_batch_f32 into [Cin][kh][kw][round4(Cout)]."""
    co, ci, kh, kw = wt.shape
    seg = (L.FlipSeg * 1)()
    seg[0].w_offset, seg[0].wt_offset, seg[0].Cout, seg[0].kh, seg[0].kw, seg[0].Cin, seg[0].Cin4, seg[0].Cout4 = 0, 0, co, kh, kw, ci, r4(ci), r4(co)
    wd = g.put(pack_ohwi(wt), at_end=True, name="bank")
    td = g.put(ci * kh * kw * r4(co) * 4, name="flipped bank")
    sd = g.put(np.frombuffer(bytes(seg), np.uint8), name="segments")
    L.call("fcn_conv_weights_flip_batch_f32", wd.ptr, td.ptr, sd.ptr, 1, None)
    L.call("fcn_device_sync")
    assert np.array_equal(td.read((ci, kh, kw, r4(co))), pack_ohwi(R.flipped_bank(wt)))
    return td


def run_dgrad(g, seed, k, pad, dil, flags):
    """dX of a stride-1 layer: the same kernel on dY with the flipped bank, ph' = d (kh-1) - ph, pw' = d (kw-1) - pw, the same dilation;
    MASK reads the activation of the blob below from a slice with poisoned neighbours and leaves it bit-identical."""
    rng = np.random.default_rng(seed)
    n, ci, co, h, w = 2, 6, 9, 12, 10
    wt = rng.standard_normal((co, ci) + k).astype(np.float32)
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, (1, 1), dil)
    dy = rng.standard_normal((n, co, oh, ow)).astype(np.float32)
    base = rng.standard_normal((n, ci, h, w)).astype(np.float32)
    act = np.maximum(rng.standard_normal((n, ci, h, w)), 0).astype(np.float32)
    want, mag = R.dgrad(dy, wt, pad, (1, 1), dil, h, w), R.dgrad_mag(dy, wt, pad, (1, 1), dil, h, w)
    if "ACCUM" in flags:
        want, mag = want + base, mag + np.abs(base)
    if "MASK" in flags:
        want = want * (act > 0)
    dyd = g.put(poisoned_nhwc(dy, r4(co), 0), at_end=True, name="dy")
    td = flipped_on_device(g, wt)
    xcs = r4(ci) + 4
    y2_img = poisoned_nhwc(act, xcs + 4, 8)
    y2d = g.put(y2_img, at_end=True, name="y2") if "MASK" in flags else None
    fl = sum(FLAGS[f] for f in flags.split("+") if f)
    for cfg in configs():
        dxd = g.put(poisoned_nhwc(base, xcs, 4) if "ACCUM" in flags else poisoned((n, h, w, xcs)), at_end=True, name="dx")
        d = rconv_desc(dyd.ptr, td.ptr, None, dxd.ptr, n, oh, ow, co, r4(co), ci, k, R.flipped_pad(k[0], k[1], pad, dil), (1, 1), dil, h, w, xcs, 4, fl,
                       y2d.ptr if y2d is not None else None, xcs + 4, 8)
        launch(g, [d], cfg, twice=(dxd, (n, h, w, xcs)))
        full = dxd.read((n, h, w, xcs))
        dx = nchw(full, ci, 4)
        assert poison_free(dx) and slice_untouched(full, 4, ci)
        within(dx, want, ref64.dot_bound(k[0] * k[1] * co, mag), "rconv dgrad cfg%d k%dx%d d%d p%dx%d %s" % ((cfg,) + k + (dil,) + pad + (flags,)))
        if "MASK" in flags:
            assert np.array_equal(y2d.read(y2_img.shape).view(np.uint32), y2_img.view(np.uint32)), "y2 was written"
    assert dyd.unchanged(), "dY was written"


@pytest.mark.parametrize("k,pad,dil,flags", [((1, 7), (0, 3), 1, ""), ((7, 1), (3, 0), 1, "MASK"), ((1, 7), (0, 2), 1, "ACCUM"),
                                             ((3, 1), (2, 0), 2, "ACCUM+MASK"), ((2, 3), (0, 2), 2, "")])
def test_data_gradient_through_the_flipped_bank(g, k, pad, dil, flags):
    run_dgrad(g, 11 + dil + k[0], k, pad, dil, flags)


def run_wgrad(g, seed, n, ci, co, h, w, k, s, pad, dil, dycs=None, dyco=0, xcs=None, xco=0, with_db=True, min_splits=1, max_splits=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ci, h, w)).astype(np.float32)
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
    dy = rng.standard_normal((n, co, oh, ow)).astype(np.float32)
    dycs, xcs = dycs or r4(co) + dyco, xcs or r4(ci) + xco
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")
    dyd = g.put(poisoned_nhwc(dy, dycs, dyco), at_end=True, name="dy")
    dwd = g.put(co * k[0] * k[1] * r4(ci) * 4, name="dw")
    dbd = g.put(co * 4, at_end=True, name="db") if with_db else None
    d = rconv_desc(xd.ptr + 4 * xco, None, None, dyd.ptr, n, h, w, ci, xcs, co, k, pad, s, dil, oh, ow, dycs, dyco)
    floats = int(L.load().fcn_rconv2d_wgrad_workspace_floats(C.byref(d)))
    slab = co * k[0] * k[1] * r4(ci)
    splits = floats // slab or 1
    assert floats % slab == 0 and splits >= min_splits, "expected at least %d pixel splits, got %d" % (min_splits, splits)
    assert max_splits is None or splits <= max_splits, "expected at most %d pixel splits, got %d" % (max_splits, splits)
    wsd = g.put(floats * 4, name="wgrad workspace") if floats else None
    bits = []
    for _ in range(2):
        L.call("fcn_rconv2d_wgrad_f32", C.byref(d), dwd.ptr, dbd.ptr if with_db else None, wsd.ptr if wsd is not None else None, None)
        L.call("fcn_device_sync")
        bits.append((dwd.read((co, k[0], k[1], r4(ci))).view(np.uint32).copy(), dbd.read((co,)).view(np.uint32).copy() if with_db else None))
    assert np.array_equal(bits[0][0], bits[1][0]), "two weight-gradient launches differ"
    full = dwd.read((co, k[0], k[1], r4(ci)))
    dw = np.ascontiguousarray(full[..., :ci].transpose(0, 3, 1, 2))
    dw64, db64 = R.wgrad(x, dy, k[0], k[1], pad, s, dil)
    mw, mb = R.wgrad_mag(x, dy, k[0], k[1], pad, s, dil)
    what = "rconv wgrad k%dx%d d%d s%dx%d p%dx%d %dx%dx%d %d->%d" % (k + (dil,) + s + pad + (n, h, w, ci, co))
    assert poison_free(full), "%s: dw was not overwritten, or poison reached it" % what
    assert np.array_equal(full[..., ci:].view(np.uint32), np.zeros_like(full[..., ci:], np.uint32)), "%s: pad columns of dw are not exact zeros" % what
    within(dw, dw64, ref64.dot_bound(n * oh * ow, mw), what + " dw")
    if with_db:
        assert np.array_equal(bits[0][1], bits[1][1])
        db = dbd.read((co,))
        assert poison_free(db)
        within(db, db64, ref64.dot_bound(n * oh * ow, mb), what + " db")
    assert xd.unchanged() and dyd.unchanged(), "%s: an input was written" % what


@pytest.mark.parametrize("k,pad,s,dil,hw", [GEOMETRIES[i] for i in (0, 1, 2, 5, 6, 7, 9)], ids=[IDS[i] for i in (0, 1, 2, 5, 6, 7, 9)])
def test_weight_gradient_unsplit(g, k, pad, s, dil, hw):
    """At most 2 x 11 x 9 pixels: one split, the result goes straight to dw and needs no workspace."""
    run_wgrad(g, 20 + dil + k[0], 1, 5, 7, hw[0], hw[1], k, s, pad, dil, max_splits=1)
    run_wgrad(g, 30 + dil + k[1], 2, 3, 6, hw[0], hw[1], k, s, pad, dil, dycs=16, dyco=4, xcs=12, xco=4, with_db=False, max_splits=1)


@pytest.mark.parametrize("ci,co", [(17, 65), (130, 70)])
def test_weight_gradient_channel_counts(g, ci, co):
    run_wgrad(g, ci + co, 2, ci, co, 9, 11, (1, 7), (1, 1), (0, 3), 1)
    run_wgrad(g, ci * co, 2, ci, co, 9, 11, (3, 1), (1, 1), (2, 0), 2)


def test_weight_gradient_over_several_pixel_splits(g):
    """N = 2 on 23 x 25: 1150 pixels at small channel counts, more than one pixel split (slabs summed in ascending order by the
    finishing launch); dY a channel slice at an offset that keeps it off 16 bytes too."""
    run_wgrad(g, 40, 2, 5, 7, 23, 25, (1, 7), (1, 1), (0, 3), 1, min_splits=2)
    run_wgrad(g, 41, 2, 6, 5, 23, 25, (7, 1), (1, 1), (3, 0), 1, dycs=12, dyco=3, min_splits=2, with_db=False)
    run_wgrad(g, 42, 2, 6, 5, 23, 25, (3, 1), (1, 1), (2, 0), 2, dycs=12, dyco=4, min_splits=2)


# ---- square dilated layers: the problem with equal axes.  sq_fwd / sq_wgrad take one kernel extent, pad and stride for both.
def sq_fwd(g, seed, n, ci, co, h, w, k, s, pad, dil, **kw):
    run_fwd(g, seed, n, ci, co, h, w, (k, k), (s, s), (pad, pad), dil, **kw)


def sq_wgrad(g, seed, n, ci, co, h, w, k, s, pad, dil, **kw):
    run_wgrad(g, seed, n, ci, co, h, w, (k, k), (s, s), (pad, pad), dil, **kw)


# k, dilation, pad, stride, (H, W)
SQUARE_GEOMETRIES = [(3, 2, 2, 1, (7, 9)), (3, 12, 12, 1, (5, 6)), (3, 4, 0, 1, (11, 13)), (5, 2, 4, 1, (9, 10)), (2, 3, 0, 1, (8, 7)),
                     (1, 3, 0, 1, (6, 5)), (3, 2, 1, 2, (11, 9)), (3, 3, 2, 2, (13, 11))]


@pytest.mark.parametrize("k,dil,pad,s,hw", SQUARE_GEOMETRIES)
def test_square_dilated_forward_geometries(g, k, dil, pad, s, hw):
    """Cin 5 (a pad channel of NaN), Cout 7 (a scalar tail); the far taps of d12 lie in the padding for most pixels."""
    sq_fwd(g, 7 * k + dil, 1, 5, 7, hw[0], hw[1], k, s, pad, dil)
    sq_fwd(g, 9 * k + dil, 2, 3, 6, hw[0], hw[1], k, s, pad, dil, xcs=12, xco=4, ycs=16, yco=4)


def test_dilation_one_equals_the_dense_convolution(g):
    """(equal axes and dilation 1: the launches of test_a_square_problem_equals_the_dense_convolution, kept as the dilated cases' own)"""
    sq_fwd(g, 1, 2, 5, 7, 7, 9, 3, 1, 1, 1, ref=lambda x, w, b: ref64.conv2d(x, w, b, 1, 1))
    sq_fwd(g, 2, 1, 4, 8, 9, 8, 3, 2, 0, 1, ref=lambda x, w, b: ref64.conv2d(x, w, b, 0, 2))


def test_square_dilated_tile_crosses_a_row_end_and_the_image_boundary(g):
    """N = 2 on 9 x 11: 99 pixels per image, so the second 64-pixel tile holds the end of image 0 and the start of image 1."""
    sq_fwd(g, 3, 2, 5, 7, 9, 11, 3, 1, 2, 2)
    sq_fwd(g, 4, 2, 8, 4, 9, 11, 3, 1, 3, 3, flags="RELU")


@pytest.mark.parametrize("ci,co", [(1, 1), (17, 65), (72, 40), (130, 70)])
def test_square_dilated_channel_counts_across_tiles_and_chunks(g, ci, co):
    """1 channel; Cin past one 16-channel chunk and off 4; Cout past one 64-channel block."""
    sq_fwd(g, ci + co, 2, ci, co, 9, 11, 3, 1, 2, 2)
    sq_fwd(g, ci * co, 1, ci, co, 5, 6, 3, 1, 4, 4, flags="ACCUM")


@pytest.mark.parametrize("flags", ["", "RELU", "ACCUM", "MASK", "ACCUM+MASK"])
def test_square_dilated_epilogues_in_a_channel_slice(g, flags):
    """bias / ReLU / accumulate / mask; x a channel window of a wider pixel, y at coffset 8 and 4 of wider pixels, with and without bias."""
    sq_fwd(g, 5, 2, 6, 10, 7, 9, 3, 1, 2, 2, flags=flags, xcs=16, xco=4, ycs=24, yco=8)
    sq_fwd(g, 6, 1, 4, 3, 5, 4, 3, 1, 2, 2, flags=flags, ycs=8, yco=4, bias=False)


def test_four_dilations_of_one_input_in_one_launch(g):
    """The ASPP head: four problems read the same 17 x 19 blob with dilations 2, 4, 6, 8 (pad == dilation) in one launch."""
    rng = np.random.default_rng(9)
    n, ci, h, w, k = 1, 6, 17, 19, 3
    x = rng.standard_normal((n, ci, h, w)).astype(np.float32)
    xd = g.put(poisoned_nhwc(x, r4(ci), 0), at_end=True, name="x")
    banks = []
    for dil, co in zip((2, 4, 6, 8), (7, 70, 4, 9)):
        wt = rng.standard_normal((co, ci, k, k)).astype(np.float32)
        b = rng.standard_normal(co).astype(np.float32)
        banks.append((dil, co, wt, b, g.put(pack_ohwi(wt), at_end=True), g.put(b, at_end=True)))
    for cfg in configs():
        descs, outs = [], []
        for dil, co, wt, b, wd, bd in banks:
            ycs = r4(co) + 4
            yd = g.put(poisoned((n, h, w, ycs)), at_end=True)
            descs.append(rconv_desc(xd.ptr, wd.ptr, bd.ptr, yd.ptr, n, h, w, ci, r4(ci), co, (k, k), (dil, dil), (1, 1), dil, h, w, ycs, 4))
            outs.append((yd, ycs, wt, b, dil, co))
        plan = launch(g, descs, cfg)
        assert plan.n == 4 and plan.grid_y == 1
        for yd, ycs, wt, b, dil, co in outs:
            full = yd.read((n, h, w, ycs))
            y = nchw(full, co, 4)
            assert poison_free(y) and slice_untouched(full, 4, co)
            pad = (dil, dil)
            within(y, R.conv2d(x, wt, b, pad, (1, 1), dil), ref64.dot_bound(k * k * ci, R.conv2d_mag(x, wt, b, pad, (1, 1), dil)), "aspp d%d" % dil)
    assert xd.unchanged()


@pytest.mark.parametrize("k,dil,pad,flags", [(3, 2, 2, ""), (3, 4, 1, ""), (3, 2, 2, "MASK"), (3, 4, 1, "ACCUM+MASK")])
def test_square_dilated_data_gradient_through_the_flipped_bank(g, k, dil, pad, flags):
    run_dgrad(g, 11 + dil, (k, k), (pad, pad), dil, flags)


@pytest.mark.parametrize("k,dil,pad,s,hw", [SQUARE_GEOMETRIES[i] for i in (0, 1, 2, 7)])
def test_square_dilated_weight_gradient_geometries(g, k, dil, pad, s, hw):
    sq_wgrad(g, 20 + dil, 1, 5, 7, hw[0], hw[1], k, s, pad, dil)
    sq_wgrad(g, 30 + dil, 2, 3, 6, hw[0], hw[1], k, s, pad, dil, dycs=16, dyco=4, xcs=12, xco=4, with_db=False)


@pytest.mark.parametrize("ci,co", [(17, 65), (130, 70)])
def test_square_dilated_weight_gradient_channel_counts(g, ci, co):
    sq_wgrad(g, ci + co, 2, ci, co, 9, 11, 3, 1, 2, 2)


def test_square_dilated_weight_gradient_over_several_pixel_splits(g):
    """N = 2 on 23 x 25: 1150 pixels, more than one pixel split; dY a channel slice at an offset that keeps it off 16 bytes too."""
    sq_wgrad(g, 40, 2, 5, 7, 23, 25, 3, 1, 2, 2, min_splits=2)
    sq_wgrad(g, 41, 2, 6, 5, 23, 25, 3, 1, 4, 4, dycs=12, dyco=3, min_splits=2, with_db=False)
    sq_wgrad(g, 42, 2, 6, 5, 23, 25, 3, 1, 4, 4, dycs=12, dyco=4, min_splits=2)


