"""Guard-banded, poisoned-buffer parity of the depthwise convolution (csrc/dwconv.hip) against the float64 reference
(tests/ref_dwconv64.py), -m gpu.  As in tests/test_gpu_guarded_rconv.py: every tensor lives in a guarded allocation, inputs are channel
windows of wider pixels whose other channels (the pad channels C .. round4(C)-1 included) hold NaN, outputs are slices of poison-filled
buffers; a case passes when the result meets the element-wise bound c * eps * K * magnitude (K = kh*kw for the forward and the data
gradient, N*OH*OW for the weight gradient), carries no poison, the neighbouring channels and the red zones are bit-identical
afterwards, and a second launch gives the same bits.  Every forward case runs under every configuration 0 ..
fcn_dwconv2d_num_configs() - 1 as well as the built-in choice; a configuration that does not take a geometry must say so with
FCN_E_UNSUPPORTED and leave the output untouched."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_dwconv64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu

FLAGS = {"RELU": L.CONV_RELU, "ACCUM": L.CONV_ACCUM, "MASK": L.CONV_MASK}
E_UNSUPPORTED = 3


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
    return [-1] + list(range(int(L.load().fcn_dwconv2d_num_configs())))


def strip_takes(k, s, dil):
    """What include/fcnhip.h says configuration 1 takes."""
    return dil == 1 and s[1] in (1, 2) and k[1] in (1, 3, 5, 7)


def dw_desc(x_ptr, w_ptr, b_ptr, y_ptr, n, h, w, c, xcs, k, pad, s, dil, ycs, yco, flags=0, y2_ptr=None, y2cs=0, y2co=0):
    d = L.dwconv_desc(x_ptr, w_ptr, b_ptr, y_ptr, n, h, w, c, xcs, k[0], k[1], pad[0], pad[1], s[0], s[1], dil, ycs, yco, flags)
    d.y2, d.y2_cstride, d.y2_coffset = y2_ptr, y2cs, y2co
    assert (d.OH, d.OW) == R.out_hw(h, w, k[0], k[1], pad, s, dil)
    return d


def launch(fn, d, cfg, buf, shape, dtype=np.float32):
    """One launch; without FCN_CONV_ACCUM a second launch on the same inputs must give the same bits."""
    lib = L.load()
    L.check(getattr(lib, fn)(C.byref(d), cfg, None))
    L.call("fcn_device_sync")
    if not (d.flags & L.CONV_ACCUM):
        first = buf.read(shape, dtype).view(np.uint16 if np.dtype(dtype).itemsize == 2 else np.uint32).copy()
        L.check(getattr(lib, fn)(C.byref(d), cfg, None))
        L.call("fcn_device_sync")
        assert np.array_equal(first, buf.read(shape, dtype).view(first.dtype)), "two launches on the same inputs differ"


def run_fwd(g, seed, n, c, h, w, k, s, pad, dil, flags="", xcs=None, xco=0, ycs=None, yco=0, bias=True):
    """x: channels xco .. xco + c - 1 of pixels of xcs channels (everything else NaN); y: channels yco .. of pixels of ycs channels.
    The reference is computed once and every configuration is held to it on fresh poisoned outputs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    wt = (rng.standard_normal((c, 1) + tuple(k)) / np.sqrt(k[0] * k[1])).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32) if bias else None
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
    xcs, ycs = xcs or r4(c) + xco, ycs or r4(c) + yco
    assert xco % 4 == 0 and xco + r4(c) <= xcs and yco + c <= ycs
    base = rng.standard_normal((n, c, oh, ow)).astype(np.float32)
    act = np.maximum(rng.standard_normal((n, c, oh, ow)), 0).astype(np.float32)
    y64, mag = R.conv2d(x, wt, b, pad, s, dil), R.conv2d_mag(x, wt, b, pad, s, dil)
    if "ACCUM" in flags:
        y64, mag = y64 + base, mag + np.abs(base)
    if "RELU" in flags:
        y64 = np.maximum(y64, 0)
    if "MASK" in flags:
        y64 = y64 * (act > 0)
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")
    wd = g.put(R.pack_bank(wt), at_end=True, name="bank")
    bd = g.put(b, at_end=True, name="bias") if bias else None
    y2cs, y2co = ycs + 4, 4
    y2_img = poisoned_nhwc(act, y2cs, y2co)
    y2d = g.put(y2_img, at_end=True, name="y2") if "MASK" in flags else None
    fl = sum(FLAGS[f] for f in flags.split("+") if f)
    for cfg in configs():
        y0 = poisoned_nhwc(base, ycs, yco) if "ACCUM" in flags else poisoned((n, oh, ow, ycs))
        yd = g.put(y0, at_end=True, name="y")
        d = dw_desc(xd.ptr + 4 * xco, wd.ptr, bd.ptr if bias else None, yd.ptr, n, h, w, c, xcs, k, pad, s, dil, ycs, yco, fl,
                    y2d.ptr if y2d is not None else None, y2cs, y2co)
        what = "dwconv cfg%d k%dx%d d%d s%dx%d p%dx%d %dx%dx%d c%d %s" % (cfg, k[0], k[1], dil, s[0], s[1], pad[0], pad[1], n, h, w, c, flags)
        if cfg == 1 and not strip_takes(k, s, dil):
            assert L.load().fcn_dwconv2d_fwd_f32(C.byref(d), cfg, None) == E_UNSUPPORTED, what
            assert np.array_equal(yd.read((n, oh, ow, ycs)).view(np.uint32), y0.view(np.uint32)), "%s: a refused call wrote y" % what
            continue
        launch("fcn_dwconv2d_fwd_f32", d, cfg, yd, (n, oh, ow, ycs))
        full = yd.read((n, oh, ow, ycs))
        y = nchw(full, c, yco)
        assert poison_free(y), "%s: poison (a pad channel, a neighbouring channel or a red zone) reached the result" % what
        within(y, y64, ref64.dot_bound(k[0] * k[1], mag), what)
        assert slice_untouched(full, yco, c), "%s: channels of y outside the slice were written" % what
        assert xd.unchanged() and wd.unchanged(), "%s: an input was written" % what
        if "MASK" in flags:
            assert np.all(y[act <= 0] == 0)
            assert np.array_equal(y2d.read((n, oh, ow, y2cs)).view(np.uint32), y2_img.view(np.uint32)), "y2 was written"


# (kh, kw), (ph, pw), (sh, sw), dilation, (H, W): the smallest at which the kernels can go wrong
GEOMETRIES = [((3, 3), (1, 1), (1, 1), 1, (7, 9)), ((3, 3), (1, 1), (2, 2), 1, (7, 9)), ((3, 3), (1, 1), (2, 2), 1, (8, 10)),      # both parities
              ((3, 3), (0, 0), (1, 1), 1, (5, 6)), ((5, 5), (2, 2), (1, 1), 1, (7, 9)), ((5, 5), (2, 2), (2, 2), 1, (9, 8)),
              ((7, 7), (3, 3), (1, 1), 1, (6, 5)),      # the image is narrower than the filter
              ((3, 3), (2, 2), (1, 1), 2, (9, 10)), ((3, 3), (2, 2), (2, 2), 2, (9, 10)),
              ((3, 1), (1, 0), (1, 1), 1, (5, 6)), ((3, 5), (0, 2), (2, 1), 1, (11, 9)), ((1, 1), (0, 0), (2, 2), 1, (7, 9))]
IDS = ["k%dx%d-p%dx%d-s%dx%d-d%d-%dx%d" % (k + p + s + (d,) + hw) for k, p, s, d, hw in GEOMETRIES]


@pytest.mark.parametrize("k,pad,s,dil,hw", GEOMETRIES, ids=IDS)
def test_forward_geometries(g, k, pad, s, dil, hw):
    """C 6 (a partial segment: a pad channel pair of NaN, a scalar tail); then C 20 as a channel window of wider pixels."""
    run_fwd(g, 7 * k[0] + k[1] + dil, 1, 6, hw[0], hw[1], k, s, pad, dil)
    run_fwd(g, 9 * k[0] + k[1] + dil, 1, 20, hw[0], hw[1], k, s, pad, dil, xcs=28, xco=4, ycs=32, yco=4)


def test_channel_counts_and_an_unaligned_slice(g):
    """C 4: one whole segment; C 70: more than one lane row of segments; y at channel offset 2: no 16-byte store anywhere."""
    run_fwd(g, 1, 1, 4, 7, 9, (3, 3), (1, 1), (1, 1), 1)
    run_fwd(g, 2, 1, 70, 7, 9, (3, 3), (2, 2), (1, 1), 1)
    run_fwd(g, 3, 1, 8, 7, 9, (3, 3), (1, 1), (1, 1), 1, ycs=12, yco=2)
    run_fwd(g, 4, 1, 6, 7, 9, (3, 3), (2, 2), (1, 1), 1, ycs=11, yco=2, flags="RELU")      # (a pixel stride off 16 bytes as well)


def test_blocks_cross_image_boundaries_and_a_strip_has_a_tail(g):
    """N = 2 on 9 x 11 with C 20: 990 work items, so a block of 256 lanes holds the end of one image and the start of the next;
    W = 13: 13 output columns are three strips of four and a tail of one (stride 1), 7 columns a strip and a tail of three (stride 2)."""
    run_fwd(g, 5, 2, 20, 9, 11, (3, 3), (1, 1), (1, 1), 1)
    run_fwd(g, 6, 2, 20, 9, 11, (3, 3), (2, 2), (1, 1), 1, flags="RELU")
    run_fwd(g, 7, 1, 6, 5, 13, (3, 3), (1, 1), (1, 1), 1)
    run_fwd(g, 8, 2, 6, 5, 13, (5, 5), (2, 2), (2, 2), 1)


@pytest.mark.parametrize("flags", ["", "RELU", "ACCUM", "MASK", "ACCUM+MASK"])
def test_epilogues_in_a_channel_slice(g, flags):
    """bias / ReLU / accumulate / mask; x a channel window of a wider pixel, y at coffset 8 and 4 of wider pixels, with and without bias."""
    run_fwd(g, 9, 2, 10, 7, 9, (3, 3), (1, 1), (1, 1), 1, flags=flags, xcs=20, xco=4, ycs=24, yco=8)
    run_fwd(g, 10, 1, 3, 5, 4, (3, 3), (2, 2), (1, 1), 1, flags=flags, ycs=8, yco=4, bias=False)
    run_fwd(g, 11, 1, 5, 5, 6, (3, 1), (1, 1), (1, 0), 2, flags=flags, ycs=9, yco=3)      # the scalar path of every epilogue


def run_dgrad(g, seed, n, c, h, w, k, s, pad, dil, flags="", xcs=None, xco=0, dycs=None, dyco=0):
    """dX: channels xco .. xco + c - 1 of pixels of xcs channels in a poisoned buffer; dY a slice of poisoned pixels.  The descriptor is
    the forward problem: x names dX, y names dY; y2 (MASK) is the activation of the blob below, read at dX's pixels."""
    rng = np.random.default_rng(seed)
    wt = rng.standard_normal((c, 1) + tuple(k)).astype(np.float32)
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
    dy = rng.standard_normal((n, c, oh, ow)).astype(np.float32)
    base = rng.standard_normal((n, c, h, w)).astype(np.float32)
    act = np.maximum(rng.standard_normal((n, c, h, w)), 0).astype(np.float32)
    want, mag = R.dgrad(dy, wt, pad, s, dil, h, w), R.dgrad_mag(dy, wt, pad, s, dil, h, w)
    if "ACCUM" in flags:
        want, mag = want + base, mag + np.abs(base)
    if "MASK" in flags:
        want = want * (act > 0)
    xcs, dycs = xcs or r4(c) + xco, dycs or r4(c) + dyco
    dyd = g.put(poisoned_nhwc(dy, dycs, dyco), at_end=True, name="dy")
    wd = g.put(R.pack_bank(wt), at_end=True, name="bank")
    y2cs, y2co = xcs + 4, 4
    y2_img = poisoned_nhwc(act, y2cs, y2co)
    y2d = g.put(y2_img, at_end=True, name="y2") if "MASK" in flags else None
    fl = sum(FLAGS[f] for f in flags.split("+") if f)
    dxd = g.put(poisoned_nhwc(base, xcs, xco) if "ACCUM" in flags else poisoned((n, h, w, xcs)), at_end=True, name="dx")
    d = dw_desc(dxd.ptr + 4 * xco, wd.ptr, None, dyd.ptr, n, h, w, c, xcs, k, pad, s, dil, dycs, dyco, fl, y2d.ptr if y2d is not None else None, y2cs, y2co)
    for cfg in (-1, 0):
        if cfg == 0 and "ACCUM" in flags:
            continue      # (a second pass would accumulate twice: the built-in choice is configuration 0)
        launch("fcn_dwconv2d_dgrad_f32", d, cfg, dxd, (n, h, w, xcs))
    assert L.load().fcn_dwconv2d_dgrad_f32(C.byref(d), 1, None) == E_UNSUPPORTED      # the strip form is forward only
    full = dxd.read((n, h, w, xcs))
    dx = nchw(full, c, xco)
    what = "dwconv dgrad k%dx%d d%d s%dx%d p%dx%d %dx%dx%d c%d %s" % (k + (dil,) + s + pad + (n, h, w, c, flags))
    assert poison_free(dx) and slice_untouched(full, xco, c), "%s: poison in dX, or channels outside the slice were written" % what
    within(dx, want, ref64.dot_bound(k[0] * k[1], mag), what)
    if "MASK" in flags:
        assert np.all(dx[act <= 0] == 0)
        assert np.array_equal(y2d.read(y2_img.shape).view(np.uint32), y2_img.view(np.uint32)), "y2 was written"
    assert dyd.unchanged() and wd.unchanged(), "%s: an input was written" % what


@pytest.mark.parametrize("k,pad,s,dil,hw", GEOMETRIES, ids=IDS)
def test_data_gradient_geometries(g, k, pad, s, dil, hw):
    """Any stride, any pad >= 0: rows and columns under no window come out zero.  C 6, then C 20 in a window with dY off 16 bytes."""
    run_dgrad(g, 11 * k[0] + k[1] + dil, 1, 6, hw[0], hw[1], k, s, pad, dil)
    run_dgrad(g, 13 * k[0] + k[1] + dil, 2, 20, hw[0], hw[1], k, s, pad, dil, xcs=28, xco=4, dycs=27, dyco=3)


@pytest.mark.parametrize("flags", ["ACCUM", "MASK", "ACCUM+MASK"])
def test_data_gradient_epilogues(g, flags):
    run_dgrad(g, 21, 2, 10, 9, 11, (3, 3), (2, 2), (1, 1), 1, flags=flags, xcs=16, xco=4)
    run_dgrad(g, 22, 1, 5, 7, 9, (3, 3), (1, 1), (1, 1), 1, flags=flags)
    run_dgrad(g, 23, 1, 8, 9, 10, (3, 3), (2, 2), (2, 2), 2, flags=flags, dycs=12, dyco=4)


def run_wgrad(g, seed, n, c, h, w, k, s, pad, dil, splits, want_splits, dycs=None, dyco=0, xcs=None, xco=0, with_db=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
    dy = rng.standard_normal((n, c, oh, ow)).astype(np.float32)
    dycs, xcs = dycs or r4(c) + dyco, xcs or r4(c) + xco
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")          # (the pad channels of x and dY hold NaN)
    dyd = g.put(poisoned_nhwc(dy, dycs, dyco), at_end=True, name="dy")
    dwd = g.put(k[0] * k[1] * r4(c) * 4, name="dw")
    dbd = g.put(c * 4, at_end=True, name="db") if with_db else None
    d = dw_desc(xd.ptr + 4 * xco, None, None, dyd.ptr, n, h, w, c, xcs, k, pad, s, dil, dycs, dyco)
    floats = int(L.load().fcn_dwconv2d_wgrad_workspace_floats(C.byref(d), splits))
    slab = (k[0] * k[1] + 1) * r4(c)      # a split's slab: the taps' rows, then db's
    got_splits = floats // slab or 1
    assert floats % slab == 0 and (want_splits is None or got_splits == want_splits), "expected %s pixel splits, got %d" % (want_splits, got_splits)
    wsd = g.put(floats * 4, name="wgrad workspace") if floats else None
    bits = []
    for _ in range(2):
        L.call("fcn_dwconv2d_wgrad_f32", C.byref(d), dwd.ptr, dbd.ptr if with_db else None, wsd.ptr if wsd is not None else None, splits, None)
        L.call("fcn_device_sync")
        bits.append((dwd.read((k[0], k[1], r4(c))).view(np.uint32).copy(), dbd.read((c,)).view(np.uint32).copy() if with_db else None))
    assert np.array_equal(bits[0][0], bits[1][0]), "two weight-gradient launches differ"
    full = dwd.read((k[0], k[1], r4(c)))
    dw = np.ascontiguousarray(full[..., :c].transpose(2, 0, 1))[:, None]
    dw64, db64 = R.wgrad(x, dy, k[0], k[1], pad, s, dil)
    mw, mb = R.wgrad_mag(x, dy, k[0], k[1], pad, s, dil)
    what = "dwconv wgrad k%dx%d d%d s%dx%d p%dx%d %dx%dx%d c%d splits %d" % (k + (dil,) + s + pad + (n, h, w, c, got_splits))
    assert poison_free(full), "%s: dw was not overwritten, or poison reached it" % what
    assert np.array_equal(full[..., c:].view(np.uint32), np.zeros_like(full[..., c:], np.uint32)), "%s: pad channels of dw are not exact zeros" % what
    within(dw, dw64, ref64.dot_bound(n * oh * ow, mw), what + " dw")
    if with_db:
        assert np.array_equal(bits[0][1], bits[1][1])
        db = dbd.read((c,))
        assert poison_free(db)
        within(db, db64, ref64.dot_bound(n * oh * ow, mb), what + " db")
    assert xd.unchanged() and dyd.unchanged(), "%s: an input was written" % what
    return full


def test_weight_gradient_unsplit(g):
    """63 and 50 pixels: the built-in choice is one split, the result goes straight to dw and needs no workspace; db present and NULL."""
    run_wgrad(g, 30, 1, 6, 7, 9, (3, 3), (1, 1), (1, 1), 1, 0, 1)
    run_wgrad(g, 31, 1, 6, 7, 9, (3, 3), (1, 1), (1, 1), 1, 0, 1, with_db=False)
    run_wgrad(g, 32, 2, 5, 9, 10, (3, 3), (2, 2), (2, 2), 2, 0, 1, dycs=11, dyco=3, xcs=12, xco=4)
    run_wgrad(g, 33, 2, 6, 11, 9, (3, 5), (2, 1), (0, 2), 1, 1, 1, with_db=False)      # 15 taps: two tap groups; 90 pixels held to one split


@pytest.mark.parametrize("splits,want", [(0, None), (1, 1), (2, 2), (3, 3), (4, 4)])
def test_weight_gradient_over_pixel_splits(g, splits, want):
    """N = 2 on 33 x 35 with C 36 (nine whole segments: no channel block is full): 2310 pixels under forced splits of 1, 2, 3 and 4 -
    4 does not divide 2310 (splits of 578, 578, 578 and 576 pixels) - and under the built-in choice, which must split too.  The
    splits only change the order of the sum: every count meets the same bound."""
    full = run_wgrad(g, 40, 2, 36, 33, 35, (3, 3), (1, 1), (1, 1), 1, splits, want, with_db=splits != 2)
    if splits == 0:
        d = dw_desc(16, None, None, 16, 2, 33, 35, 36, 36, (3, 3), (1, 1), (1, 1), 1, 36, 0)
        assert int(L.load().fcn_dwconv2d_wgrad_workspace_floats(C.byref(d), 0)) // (10 * 36) > 1
    assert full.shape == (3, 3, 36)


def test_weight_gradient_of_seven_by_seven_taps(g):
    """49 taps: six tap groups, the last one partial; C 70: two channel blocks, the second partial; dY a slice off 16 bytes."""
    run_wgrad(g, 50, 2, 70, 9, 8, (7, 7), (1, 1), (3, 3), 1, 0, None, dycs=75, dyco=3)
    run_wgrad(g, 51, 1, 6, 6, 5, (7, 7), (1, 1), (3, 3), 1, 3, 3, with_db=False)      # the image is narrower than the filter
