"""Guard-banded, poisoned-buffer parity of the HIP kernels against the float64 reference (tests/ref64.py), -m gpu.

Every tensor of every case lives in a guarded allocation (tests/gpu_util.py): inputs are channel slices of wider pixels whose
other channels hold poison, outputs are slices of poison-filled buffers, and around each payload lie 256 KiB red zones of
the same poison.  A case passes when the result meets ref64's element-wise bound, carries no trace of the poison (a consumed
stray READ), the slack channels are bit-identical afterwards (a stray WRITE inside the buffer) and so are the red zones (a
stray write outside it - checked by `Guards` when the block ends).  NaN is the poison wherever it survives the kernel; MAX
poolings (whose `v > m` ignores a NaN) get the huge poison, and the read-poison convolutions run without ReLU."""
import ctypes as C

import numpy as np
import pytest

import ref64
from conftest import CFG_DOT1X1, CFG_FIRST7, N_TILE_CFGS
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, conv_desc, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def within(y, y64, allow, what=""):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def ohwi(w, dtype=np.float32):
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1)).astype(dtype)


def set_cfg(monkeypatch, name, cfg):
    if cfg is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(cfg))


# ---- tiled convolution ----------------------------------------------------------------------------------------------
def guarded_conv(g, case, seed, f16=False, flags=0, at_end=True):
    """One convolution whose x is channels xo .. xo + cin - 1 of a pixel of xcs channels and whose y is channels yo .. of ycs; returns
    what the checks need.  x ends on the last byte in front of its back red zone when at_end."""
    cin, cout, k, s, p, h, w, n, xcs, xo, ycs, yo = case
    dt = np.float16 if f16 else np.float32
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, cin, h, w)).astype(dt).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(dt).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    oh, ow = ref64.conv_out(h, k, p, s), ref64.conv_out(w, k, p, s)
    esz = np.dtype(dt).itemsize
    xd = g.put(poisoned_nhwc(x, xcs, xo, dtype=dt), at_end=at_end, name="x")
    wd, bd = g.put(ohwi(wt, dt), name="w"), g.put(b, name="bias")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=dt), name="y")
    d = conv_desc(xd, wd, bd, yd, n, h, w, cin, xcs, cout, k, p, s, oh, ow, ycs, yo, flags | (L.CONV_F16 if f16 else 0))
    d.x = xd.ptr + esz * xo                                  # a blob inside a concat buffer: the pointer is moved, the stride stays
    L.call("fcn_conv2d_fwd_f32", C.byref(d), None)
    full = yd.read((n, oh, ow, ycs), dt)
    return x, wt, b, full, nchw(full.astype(np.float32), cout, yo)


def check_conv(x, wt, b, p, s, full, y, cout, yo, f16, what):
    y64, mag = ref64.conv2d(x, wt, b, p, s), ref64.conv2d_mag(x, wt, b, p, s)
    K = x.shape[1] * wt.shape[2] * wt.shape[3]
    assert poison_free(y), "%s: the poison around x reached the result" % what
    within(y, y64, ref64.dot_bound_f16(K, mag, y64) if f16 else ref64.dot_bound_rms(K, mag), what)
    assert slice_untouched(full, yo, cout), "%s: channels of y outside the slice were written" % what


# cin, cout, k, stride, pad, h, w, n, x_cstride, x channel offset, y_cstride, y channel offset
SWEEP_CASES = [
    (24, 36, 5, 1, 2, 3, 11, 2, 40, 8, 48, 4),        # taps straddle chunks; H smaller than the filter reach; Cout 36
    (40, 33, 3, 1, 1, 13, 5, 1, 64, 16, 40, 4),       # partial last chunk; Cout 33; 65 output pixels = one more than a 64 multiple
    (16, 4, 7, 1, 3, 9, 7, 1, 32, 8, 8, 4),           # pad 3 with W = 7 = filter width; 63 pixels; Cout 4
    (96, 36, 3, 2, 1, 12, 21, 1, 128, 32, 36, 0),     # stride 2, three whole chunks per tap
]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("cfg", list(range(N_TILE_CFGS)) + [None])
@pytest.mark.parametrize("case", SWEEP_CASES)
def test_tiled_conv_every_configuration(g, monkeypatch, case, cfg, f16):
    set_cfg(monkeypatch, "FCN_CONV_CFG", cfg)
    x, wt, b, full, y = guarded_conv(g, case, SWEEP_CASES.index(case), f16=f16)
    check_conv(x, wt, b, case[4], case[3], full, y, case[1], case[11], f16, "conv cfg %s" % cfg)


EDGE_CASES = [
    (4, 4, 3, 1, 1, 1, 1, 1, 8, 4, 4, 0),             # one pixel: every tap but the centre is padding
    (4, 33, 3, 1, 2, 2, 2, 3, 12, 4, 36, 3),          # pad 2 on a 2 x 2 image, batch 3, y at a channel offset that is not a multiple of 4
    (16, 36, 5, 1, 2, 1, 9, 1, 16, 0, 40, 4),         # one row
    (16, 36, 5, 1, 2, 9, 1, 1, 24, 8, 40, 0),         # one column
    (24, 4, 3, 1, 1, 8, 8, 1, 32, 4, 4, 0),           # 64 pixels exactly
    (24, 4, 3, 1, 1, 8, 16, 1, 32, 4, 8, 4),          # 128
    (24, 4, 3, 1, 1, 43, 3, 1, 32, 4, 4, 0),          # 129
    (24, 4, 3, 1, 1, 127, 1, 1, 32, 4, 4, 0),         # 127
    (40, 36, 1, 1, 0, 5, 51, 1, 48, 8, 36, 0),        # 1x1, 255 pixels
    (96, 33, 1, 1, 0, 257, 1, 1, 96, 0, 33, 0),       # 257 pixels, dense x ending on the last byte
    (4, 68, 7, 2, 3, 9, 9, 2, 4, 0, 68, 0),           # 7x7 stride 2 on four REAL channels, 68 outputs (beyond the first-layer kernel's 64)
    (8, 8, 3, 2, 0, 15, 15, 3, 16, 8, 8, 0),          # stride 2 without padding
]


@pytest.mark.parametrize("case", EDGE_CASES)
def test_tiled_conv_edges(g, monkeypatch, case):
    monkeypatch.delenv("FCN_CONV_CFG", raising=False)
    x, wt, b, full, y = guarded_conv(g, case, 100 + EDGE_CASES.index(case))
    check_conv(x, wt, b, case[4], case[3], full, y, case[1], case[11], False, "conv edge")


@pytest.mark.parametrize("flags", ["RELU", "SIGMOID2", "ACCUM", "MASK"])
@pytest.mark.parametrize("cfg", [None, 5, 23])
def test_conv_epilogues_write_only_their_slices(g, monkeypatch, flags, cfg):
    """The write canary of the epilogues that do not let a NaN through (x is clean here): y, y2 and everything around them."""
    set_cfg(monkeypatch, "FCN_CONV_CFG", cfg)
    rng = np.random.default_rng(7)
    n, cin, cout, h, w, ycs, yo, y2cs, y2o = 2, 24, 36, 7, 5, 48, 8, 40, 4
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * 0.1).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    base = rng.standard_normal((n, cout, h, w)).astype(np.float32)
    act = np.maximum(rng.standard_normal((n, cout, h, w)), 0).astype(np.float32)
    xd, wd, bd = g.put(poisoned_nhwc(x, 32, 4), at_end=True), g.put(ohwi(wt)), g.put(b)
    yd = g.put(poisoned_nhwc(base, ycs, yo) if flags == "ACCUM" else poisoned((n, h, w, ycs)), name="y")
    y2d = g.put(poisoned_nhwc(act, y2cs, y2o) if flags == "MASK" else poisoned((n, h, w, y2cs)), name="y2")
    fl = {"RELU": L.CONV_RELU, "SIGMOID2": L.CONV_SIGMOID2, "ACCUM": L.CONV_ACCUM, "MASK": L.CONV_MASK}[flags]
    d = conv_desc(xd, wd, bd, yd, n, h, w, cin, 32, cout, 3, 1, 1, h, w, ycs, yo, fl, 0.0, y2d, y2cs, y2o)
    d.x = xd.ptr + 16
    L.call("fcn_conv2d_fwd_f32", C.byref(d), None)
    full, full2 = yd.read((n, h, w, ycs)), y2d.read((n, h, w, y2cs))
    y64, mag = ref64.conv2d(x, wt, b, 1, 1), ref64.conv2d_mag(x, wt, b, 1, 1)
    want = {"RELU": np.maximum(y64, 0), "SIGMOID2": y64, "ACCUM": y64 + base, "MASK": y64 * (act > 0)}[flags]
    y = nchw(full, cout, yo)
    assert poison_free(y)
    within(y, want, ref64.dot_bound_rms(cin * 9, mag + np.abs(base) if flags == "ACCUM" else mag), "conv " + flags)
    assert slice_untouched(full, yo, cout)
    if flags == "SIGMOID2":
        assert np.abs(nchw(full2, cout, y2o) - ref64.sigmoid(y64)).max() < 1e-6 and slice_untouched(full2, y2o, cout)
    elif flags == "MASK":
        assert np.all(y[act <= 0] == 0) and np.array_equal(full2.view(np.uint32), poisoned_nhwc(act, y2cs, y2o).view(np.uint32))
    else:
        assert slice_untouched(full2, 0, 0)                 # y2 is not part of the problem: not one byte of it


# ---- first-layer kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,cout", [(1, 9, 9, 64), (2, 7, 45, 40), (1, 5, 201, 64), (3, 17, 33, 36)])
def test_first_layer_kernel(g, n, h, w, cout):
    """conv_first7_kernel: odd sizes, W in {9, 45, 201}, the image ending on the last byte in front of the red zone, a batch whose
    last 8 x 32 tile is partial.  include/fcnhip.h: the kernel multiplies channels 0..2 only - channel 3 of every pixel and of every
    filter tap is the pad channel and is NOT read.  So both hold poison here, and the reference is the three-channel convolution."""
    lib = L.load()
    rng = np.random.default_rng(n * 1000 + w)
    x = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, 3, 7, 7)) * 0.1).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    oh, ow = ref64.conv_out(h, 7, 3, 2), ref64.conv_out(w, 7, 3, 2)
    ycs, yo = cout + 8, 4
    wp = poisoned((cout, 7, 7, 4))
    wp[..., :3] = wt.transpose(0, 2, 3, 1)
    xd, wd, bd = g.put(poisoned_nhwc(x, 4), at_end=True, name="image"), g.put(wp, at_end=True, name="w"), g.put(b)
    yd = g.put(poisoned((n, oh, ow, ycs)), name="y")
    ws = g.put(int(lib.fcn_conv2d_group_workspace_bytes(1)), name="group workspace")
    d = conv_desc(xd, wd, bd, yd, n, h, w, 4, 4, cout, 7, 3, 2, oh, ow, ycs, yo, 0)
    grp = L.ConvGroup()
    L.call("fcn_conv2d_group_prepare", (L.ConvDesc * 1)(d), 1, ws.ptr, CFG_FIRST7, C.byref(grp))
    assert grp.cfg == CFG_FIRST7
    L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), None)
    L.call("fcn_conv2d_group_release", ws.ptr)
    full = yd.read((n, oh, ow, ycs))
    check_conv(x, wt, b, 3, 2, full, nchw(full, cout, yo), cout, yo, False, "first layer")


# ---- lane-split 1x1 kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,cin,xcs,xo,couts", [(1, 3, 3, 36, 48, 8, (8, 8, 8, 3)), (2, 5, 7, 480, 512, 16, (1, 4)), (1, 9, 5, 1024, 1024, 0, (4, 16))])
def test_lane_split_1x1_group(g, n, h, w, cin, xcs, xo, couts):
    """conv_dot1x1_kernel: several problems share ONE poisoned input (a slice of wider pixels) and write different slices of ONE output
    buffer; the pixel count is not a multiple of its four-pixel tile."""
    lib = L.load()
    rng = np.random.default_rng(31)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    xd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x")
    ycs = sum((c + 3) // 4 * 4 + 4 for c in couts) + 4
    yd = g.put(poisoned((n, h, w, ycs)), name="y")
    descs, refs, off = [], [], 4
    for cout in couts:
        wt = (rng.standard_normal((cout, cin, 1, 1)) * 0.05).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        d = conv_desc(xd, g.put(ohwi(wt)), g.put(b), yd, n, h, w, cin, xcs, cout, 1, 0, 1, h, w, ycs, off, 0)
        d.x = xd.ptr + 4 * xo
        descs.append(d)
        refs.append((off, cout, wt, b))
        off += (cout + 3) // 4 * 4 + 4
    ws = g.put(int(lib.fcn_conv2d_group_workspace_bytes(len(descs))), name="group workspace")
    grp = L.ConvGroup()
    L.call("fcn_conv2d_group_prepare", (L.ConvDesc * len(descs))(*descs), len(descs), ws.ptr, CFG_DOT1X1, C.byref(grp))
    assert grp.cfg == CFG_DOT1X1
    L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), None)
    L.call("fcn_conv2d_group_release", ws.ptr)
    full = yd.read((n, h, w, ycs))
    written = np.zeros(ycs, bool)
    for off, cout, wt, b in refs:
        y = nchw(full, cout, off)
        assert poison_free(y)
        within(y, ref64.conv2d(x, wt, b, 0, 1), ref64.dot_bound_rms(cin, ref64.conv2d_mag(x, wt, b, 0, 1)), "dot1x1 cout %d" % cout)
        written[off:off + cout] = True
    assert np.all(full.view(np.uint32)[..., ~written] == poisoned((1,)).view(np.uint32)[0])


# ---- max pooling riding in a convolution group ----------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [5, 23])
def test_pool_fused_into_conv_group(g, cfg):
    rng = np.random.default_rng(32)
    n, h, w, c, xcs, xo = 2, 7, 6, 24, 40, 8
    x = -np.abs(rng.standard_normal((n, c, h, w))).astype(np.float32) - 0.5      # all negative: a zero pad would win the 3x3 / pad 1 windows
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison="huge"), at_end=True, poison="huge", name="x")
    wt = (rng.standard_normal((36, c, 1, 1)) * 0.2).astype(np.float32)
    b = rng.standard_normal(36).astype(np.float32)
    yd = g.put(poisoned((n, h, w, 40)), name="conv y")
    d = conv_desc(xd, g.put(ohwi(wt)), g.put(b), yd, n, h, w, c, xcs, 36, 1, 0, 1, h, w, 40, 4, L.CONV_RELU)
    d.x = xd.ptr + 4 * xo
    ry, ridx = ref64.max_pool(x, 3, 1, 1)
    pd, idd = g.put(poisoned((n, h, w, 32)), name="pooled"), g.put(poisoned((n, h, w, c), dtype=np.int32), name="argmax")
    pl = L.PoolDesc()
    pl.x, pl.y, pl.idx = d.x, pd.ptr, idd.ptr
    pl.N, pl.H, pl.W, pl.C, pl.x_cstride, pl.k, pl.stride, pl.pad, pl.OH, pl.OW, pl.y_cstride, pl.y_coffset = n, h, w, c, xcs, 3, 1, 1, h, w, 32, 4
    ws = g.put(int(L.load().fcn_conv2d_group_workspace_bytes(1)), name="group workspace")
    grp = L.ConvGroup()
    L.call("fcn_conv2d_group_prepare_fused", (L.ConvDesc * 1)(d), 1, (L.PoolDesc * 1)(pl), 1, ws.ptr, cfg, C.byref(grp))
    L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), None)
    L.call("fcn_conv2d_group_release", ws.ptr)
    pooled, full = pd.read((n, h, w, 32)), yd.read((n, h, w, 40))
    assert np.array_equal(nchw(pooled, c, 4), ry) and slice_untouched(pooled, 4, c)
    assert np.array_equal(idd.read((n, h, w, c), np.int32).transpose(0, 3, 1, 2), ridx)
    y = nchw(full, 36, 4)
    assert poison_free(y, "huge") and slice_untouched(full, 4, 36)
    within(y, np.maximum(ref64.conv2d(x, wt, b, 0, 1), 0), ref64.dot_bound_rms(c, ref64.conv2d_mag(x, wt, b, 0, 1)), "conv beside the pool")


# ---- pooling / LRN, float32 -----------------------------------------------------------------------------------------
POOL_CASES = [
    # k, s, p, h, w, c, x_cstride, xo, y_cstride, yo, with_idx
    (3, 1, 1, 5, 4, 4, 12, 4, 12, 4, True),           # C = 4: no neighbour group either side; VEC4 + idx
    (3, 2, 0, 6, 7, 8, 16, 4, 8, 0, False),           # last window clipped in y only (6 -> rows 4..5), VEC4 without idx
    (3, 2, 1, 7, 6, 5, 9, 3, 7, 1, True),             # scalar form (C = 5, offsets not multiples of 4) + idx
    (2, 2, 0, 5, 8, 6, 8, 1, 6, 0, False),            # scalar form without idx; last window clipped in y only
    (3, 1, 1, 1, 9, 4, 8, 4, 4, 0, True),             # one row
    (5, 3, 2, 9, 1, 4, 4, 0, 8, 4, True),             # one column, generic window loop of the vector form
]


@pytest.mark.parametrize("case", POOL_CASES)
def test_maxpool_all_negative_in_huge_poison(g, case):
    k, s, p, h, w, c, xcs, xo, ycs, yo, with_idx = case
    rng = np.random.default_rng(9)
    x = -np.abs(rng.standard_normal((2, c, h, w))).astype(np.float32) - 0.25
    x[0, :, 0, 0] = x[0, :, 0, min(1, w - 1)]                  # a tie: the first maximum wins
    ry, ridx = ref64.max_pool(x, k, s, p)
    oh, ow = ry.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison="huge"), at_end=True, poison="huge", name="x")
    yd = g.put(poisoned((2, oh, ow, ycs)), name="y")
    idd = g.put(poisoned((2, oh, ow, c), dtype=np.int32), name="argmax") if with_idx else None
    L.call("fcn_maxpool_fwd_f32", xd.ptr + 4 * xo, yd.ptr, idd.ptr if idd else None, 2, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, None)
    full = yd.read((2, oh, ow, ycs))
    assert np.array_equal(nchw(full, c, yo), ry) and slice_untouched(full, yo, c)
    if with_idx:
        assert np.array_equal(idd.read((2, oh, ow, c), np.int32).transpose(0, 3, 1, 2), ridx)


@pytest.mark.parametrize("k,s,p,h,w", [(3, 2, 1, 7, 6), (3, 1, 1, 4, 5), (7, 7, 0, 7, 7), (2, 2, 0, 5, 3), (3, 2, 1, 1, 1)])
def test_avepool_divisor_counts_the_padding(g, k, s, p, h, w):
    rng = np.random.default_rng(10)
    c, xcs, xo, ycs, yo = 6, 11, 3, 9, 2
    x = rng.standard_normal((2, c, h, w)).astype(np.float32) + 3      # a mean far from zero: a wrong divisor shows
    want = ref64.ave_pool(x, k, s, p)
    oh, ow = want.shape[2:]
    xd, yd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x"), g.put(poisoned((2, oh, ow, ycs)), name="y")
    L.call("fcn_avepool_fwd_f32", xd.ptr + 4 * xo, yd.ptr, 2, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, None)
    full = yd.read((2, oh, ow, ycs))
    y = nchw(full, c, yo)
    assert poison_free(y) and slice_untouched(full, yo, c)
    within(y, want, ref64.dot_bound_rms(k * k, ref64.ave_pool(np.abs(x), k, s, p)) + ref64.U32 * np.abs(want), "avepool")


def lrn_allow(x, y64, scale64, ls, alpha, beta):
    """|dy| of y = x s^-beta with s a float32 sum of `ls` squares (each rounded) and s^-beta from two square roots and a division
    (a few ulp): (ls + 2) u relative on s -> beta (ls + 2) u on the factor, plus 6 u for the power, the product and the store."""
    return (beta * (ls + 2) + 6) * ref64.U32 * np.abs(y64) + 1e-37


@pytest.mark.parametrize("c,ls,xcs,xo,ycs", [(4, 5, 12, 4, 8), (8, 5, 16, 8, 8), (64, 5, 72, 4, 64), (10, 5, 13, 2, 11), (16, 3, 24, 4, 16), (4, 7, 8, 4, 4)])
def test_lrn_of_a_slice_between_poisoned_neighbours(g, c, ls, xcs, xo, ycs):
    """lrn5_kernel (16-byte groups; C = 4 has no neighbour group on either side - the groups beside it belong to OTHER blobs) and
    lrn_generic_kernel; values up to a few hundred, where scale leaves 1."""
    rng = np.random.default_rng(11)
    n, h, w = 2, 3, 5
    x = (rng.standard_normal((n, c, h, w)) * 150).astype(np.float32)
    y64, s64 = ref64.lrn(x, ls, 1e-4, 0.75, 1.0)
    xd, yd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x"), g.put(poisoned((n, h, w, ycs)), name="y")
    sd = g.put(poisoned((n, h, w, c)), at_end=True, name="scale")
    L.call("fcn_lrn_fwd_f32", xd.ptr + 4 * xo, yd.ptr, sd.ptr, n * h * w, c, xcs, ycs, ls, 1e-4, 0.75, 1.0, None)
    full = yd.read((n, h, w, ycs))
    y, sc = nchw(full, c), nchw(sd.read((n, h, w, c)), c)
    assert poison_free(y) and poison_free(sc) and slice_untouched(full, 0, c)
    within(sc, s64, (ls + 2) * ref64.U32 * s64, "lrn scale")
    within(y, y64, lrn_allow(x, y64, s64, ls, 1e-4, 0.75), "lrn")


@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("lrn_first", [0, 1])
@pytest.mark.parametrize("k,s,p,h,w,c,xcs,xo", [(3, 2, 0, 6, 7, 4, 12, 4), (3, 1, 1, 5, 4, 8, 16, 4), (3, 2, 0, 37, 41, 192, 200, 4), (3, 2, 1, 9, 1, 40, 48, 8)])
def test_pool_lrn_single_pass(g, monkeypatch, k, s, p, h, w, c, xcs, xo, lrn_first, lds):
    """fcn_maxpool_lrn5_fwd_f32, both orders, and the opt-in LDS-patch form (FCN_LRN_POOL_LDS=1: taken by the 37 x 41 x 192 case with the LRN
    first).  All-negative inputs in huge poison when the pooling reads x; NaN poison when the LRN does."""
    if lds and not (lrn_first and h * w * c >= 1 << 18):
        pytest.skip("the LDS-patch form takes large LRN-first 3x3/2 problems only")
    set_cfg(monkeypatch, "FCN_LRN_POOL_LDS", 1 if lds else None)
    rng = np.random.default_rng(13)
    n = 2
    x = (-np.abs(rng.standard_normal((n, c, h, w))) * 60 - 1).astype(np.float32)
    poison = "nan" if lrn_first else "huge"
    want = ref64.max_pool(ref64.lrn(x, 5, 1e-4, 0.75)[0], k, s, p)[0] if lrn_first else ref64.lrn(ref64.max_pool(x, k, s, p)[0], 5, 1e-4, 0.75)[0]
    oh, ow = want.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison=poison), at_end=True, poison=poison, name="x")
    yd = g.put(poisoned((n, oh, ow, c + 4)), name="y")
    L.call("fcn_maxpool_lrn5_fwd_f32", xd.ptr + 4 * xo, yd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, c + 4, lrn_first, 1e-4, 0.75, 1.0, None)
    full = yd.read((n, oh, ow, c + 4))
    y = nchw(full, c)
    assert poison_free(y, poison) and slice_untouched(full, 0, c)
    within(y, want, lrn_allow(x, want, None, 5, 1e-4, 0.75), "pool+lrn first=%d lds=%d" % (lrn_first, lds))


@pytest.mark.parametrize("s,p,h,w,ycs,yo,relu", [(2, 0, 6, 7, 72, 4, 0), (1, 1, 5, 4, 64, 0, 1), (2, 1, 9, 1, 80, 16, 0), (2, 0, 17, 37, 64, 0, 1)])
def test_pool_lrn_conv1x1_single_pass(g, s, p, h, w, ycs, yo, relu):
    rng = np.random.default_rng(29)
    n, c, xcs, xo = 2, 64, 80, 12
    x = (-np.abs(rng.standard_normal((n, c, h, w))) * 40 - 1).astype(np.float32)
    wt = (rng.standard_normal((64, c, 1, 1)) * 0.1).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    mid = ref64.lrn(ref64.max_pool(x, 3, s, p)[0], 5, 1e-4, 0.75)[0]
    oh, ow = mid.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison="huge"), at_end=True, poison="huge", name="x")
    wd, bd = g.put(np.ascontiguousarray(wt.reshape(64, c))), g.put(b)
    yd = g.put(poisoned((n, oh, ow, ycs)), name="y")
    L.call("fcn_maxpool_lrn5_conv1x1_fwd_f32", xd.ptr + 4 * xo, n, h, w, c, xcs, 3, s, p, oh, ow, 1e-4, 0.75, 1.0, wd.ptr, bd.ptr, 64, relu, yd.ptr, ycs, yo, None)
    full = yd.read((n, oh, ow, ycs))
    y = nchw(full, 64, yo)
    want, mag = ref64.conv2d(mid, wt, b, 0, 1), ref64.conv2d_mag(mid, wt, b, 0, 1)
    assert poison_free(y, "huge") and slice_untouched(full, yo, 64)
    # the normalised activations carry the LRN's own rounding (lrn_allow, relative) into every product
    within(y, np.maximum(want, 0) if relu else want, ref64.dot_bound_rms(c, mag) + 12 * ref64.U32 * mag, "pool+lrn+conv1x1")


# ---- element-wise ---------------------------------------------------------------------------------------------------
COUNTS = [1, 3, 4, 5, 1003]


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "plus4bytes"])
@pytest.mark.parametrize("count", COUNTS)
def test_unary_kernels(g, count, shift):
    """unary_kernel (16-byte aligned pointers) and unary_scalar_kernel (pointer + 4 bytes); the poison starts at the payload's last byte, so a
    vector tail that rounds the count up is caught on either side."""
    rng = np.random.default_rng(count)
    a = (rng.standard_normal(count + 1) * 3).astype(np.float32)
    a[shift // 4:][:2] = (100.0, -100.0)[:count]
    n = count
    x = a[shift // 4:][:n]

    def run(name, *args):
        xd = g.put(a if shift else x, name="x")
        yd = g.put(poisoned(count + shift // 4), name="y")
        L.call(name, xd.ptr + shift, yd.ptr + shift, n, *args, None)
        full = yd.read((count + shift // 4,))
        assert slice_untouched(full[None], shift // 4, n)
        return full[shift // 4:]

    assert np.array_equal(run("fcn_relu_fwd_f32", 0.0), np.maximum(x, 0))
    within(run("fcn_relu_fwd_f32", 0.1), np.where(x > 0, x, np.float64(np.float32(0.1)) * x), ref64.U32 * np.abs(x) + 1e-37, "leaky relu")
    sg = run("fcn_sigmoid_fwd_f32")
    within(sg, ref64.sigmoid(x), 4 * ref64.U32 * ref64.sigmoid(x) + 1e-37, "sigmoid")      # relative: sigmoid(-100) = 3.7e-44 is held to its own size
    assert np.array_equal(run("fcn_power_fwd_f32", 1.0, 2.0, -127.0), x * np.float32(2) + np.float32(-127))
    pw = run("fcn_power_fwd_f32", 2.0, 0.5, 1.0)
    t = 1.0 + 0.5 * x.astype(np.float64)
    within(pw, t * t, 8 * ref64.U32 * t * t + 1e-37, "power 2")


@pytest.mark.parametrize("count", COUNTS)
def test_eltwise(g, count):
    rng = np.random.default_rng(count + 50)
    a, b = rng.standard_normal((2, count)).astype(np.float32)
    for op, want in [(L.ELT_PROD, a.astype(np.float64) * b), (L.ELT_SUM, 0.5 * a.astype(np.float64) + 2.0 * b), (L.ELT_MAX, np.maximum(a, b))]:
        ad, bd, yd = g.put(a, at_end=True), g.put(b, at_end=True), g.put(poisoned(count), at_end=True, name="y")
        L.call("fcn_eltwise_fwd_f32", ad.ptr, bd.ptr, yd.ptr, count, op, 0.5, 2.0, None)
        within(yd.read((count,)), want, 2 * ref64.U32 * (np.abs(want) + np.abs(0.5 * a) + np.abs(2.0 * b)), "eltwise %d" % op)


@pytest.mark.parametrize("pixels,c,scs,sco,dcs,dco", [(1, 1, 3, 2, 2, 1), (10, 5, 12, 3, 20, 9), (33, 7, 7, 0, 9, 2), (5, 4, 8, 4, 4, 0)])
def test_copy_channels(g, pixels, c, scs, sco, dcs, dco):
    rng = np.random.default_rng(14)
    src = rng.standard_normal((pixels, c)).astype(np.float32)
    wide = poisoned((pixels, scs))
    wide[:, sco:sco + c] = src
    sd, dd = g.put(wide, at_end=True), g.put(poisoned((pixels, dcs)), at_end=True, name="dst")
    L.call("fcn_copy_channels_f32", sd.ptr, dd.ptr, pixels, c, scs, sco, dcs, dco, None)
    out = dd.read((pixels, dcs))
    assert np.array_equal(out[:, dco:dco + c], src) and slice_untouched(out, dco, c)


@pytest.mark.parametrize("pixels,c,xcs,ycs", [(1, 1, 1, 1), (3, 5, 8, 5), (1003, 2, 3, 4), (5, 21, 21, 24)])
def test_softmax_with_large_logits(g, pixels, c, xcs, ycs):
    """Logits in +-90 (exp overflows float32 beyond 88: a kernel that drops the max subtraction returns inf / NaN) and one pixel of
    equal logits; every probability is held to its own size."""
    rng = np.random.default_rng(15)
    x = (rng.random((pixels, c)) * 180 - 90).astype(np.float32)
    x[0] = 37.5
    x[-1, :] = np.linspace(88.5, 90, c)
    wide = poisoned((pixels, xcs))
    wide[:, :c] = x
    xd, yd = g.put(wide, at_end=True), g.put(poisoned((pixels, ycs)), at_end=True, name="y")
    L.call("fcn_softmax_fwd_f32", xd.ptr, yd.ptr, pixels, c, xcs, ycs, None)
    out = yd.read((pixels, ycs))
    y = out[:, :c]
    want = ref64.softmax(x)
    assert poison_free(y) and slice_untouched(out, 0, c)
    assert np.all(y[0] == y[0, 0]) and abs(float(y[0, 0]) * c - 1) < 1e-6
    # exp of a float32 difference of up to 180 carries the difference's rounding (180 u) into the probability
    within(y, want, (200 + c) * ref64.U32 * want + 1e-44, "softmax")


@pytest.mark.parametrize("c,k,s,p,h,w,xcs,xo,ycs,yo", [(5, 4, 2, 1, 3, 4, 7, 1, 9, 3), (4, 8, 4, 2, 2, 5, 8, 4, 8, 4), (3, 3, 1, 1, 1, 1, 3, 0, 3, 0)])
def test_depthwise_deconv(g, c, k, s, p, h, w, xcs, xo, ycs, yo):
    rng = np.random.default_rng(16)
    n = 2
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    wt = rng.standard_normal((c, k, k)).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    want = ref64.deconv_depthwise(x, wt, b, k, s, p)
    mag = ref64.deconv_depthwise(np.abs(x), np.abs(wt), np.abs(b), k, s, p)
    oh, ow = want.shape[2:]
    xd, wd, bd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x"), g.put(wt, at_end=True), g.put(b, at_end=True)
    yd = g.put(poisoned((n, oh, ow, ycs)), name="y")
    L.call("fcn_deconv_depthwise_fwd_f32", xd.ptr + 4 * xo, wd.ptr, bd.ptr, yd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, None)
    full = yd.read((n, oh, ow, ycs))
    y = nchw(full, c, yo)
    assert poison_free(y) and slice_untouched(full, yo, c)
    within(y, want, ref64.dot_bound_rms((k // s + 1) ** 2, mag), "depthwise deconv")


@pytest.mark.parametrize("n,c,h,w,cs,co", [(2, 37, 3, 5, 45, 7), (1, 3, 17, 23, 4, 0), (3, 1, 1, 1, 2, 1), (1, 33, 1, 33, 33, 0)])
def test_layout_kernels(g, n, c, h, w, cs, co):
    """nchw_to_nhwc_kernel / nchw_to_nhwc4_kernel / nhwc_to_nchw_kernel / nhwc_to_nchw_multi_kernel: channel offsets that are not
    multiples of 4, pixel and channel counts that are not multiples of the 32 x 32 transpose tile."""
    rng = np.random.default_rng(17)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    xd, yd = g.put(x, at_end=True, name="nchw"), g.put(poisoned((n, h, w, cs)), at_end=True, name="nhwc")
    L.call("fcn_nchw_to_nhwc_f32", xd.ptr, yd.ptr, n, c, h, w, cs, co, -127.0, None)
    full = yd.read((n, h, w, cs))
    assert np.array_equal(nchw(full, c, co), x + np.float32(-127.0))
    if cs == 4 and co == 0:      # the image form owns the whole 4-channel pixel: its pad channels are zeroed
        assert np.all(full[..., c:] == 0)
    else:
        assert slice_untouched(full, co, c)
    src = g.put(poisoned_nhwc(x, cs, co), at_end=True, name="nhwc src")
    for multi in (False, True):
        back = g.put(poisoned((n, c, h, w)), at_end=True, name="nchw dst")
        if multi:
            d = L.LayoutDesc()
            d.src, d.dst, d.N, d.C, d.H, d.W, d.src_cstride, d.src_coffset = src.ptr, back.ptr, n, c, h, w, cs, co
            L.call("fcn_nhwc_to_nchw_multi_f32", (L.LayoutDesc * 1)(d), 1, None)
        else:
            L.call("fcn_nhwc_to_nchw_f32", src.ptr, back.ptr, n, c, h, w, cs, co, None)
        assert np.array_equal(back.read((n, c, h, w)), x)


# ---- training -------------------------------------------------------------------------------------------------------
WG_CASES = [  # cin, cout, k, stride, pad, h, w, n, x_cstride, xo, dy_cstride, dyo
    (24, 36, 5, 1, 2, 3, 11, 2, 40, 8, 48, 4),
    (40, 33, 3, 1, 1, 13, 5, 1, 64, 16, 40, 4),
    (4, 64, 7, 2, 3, 21, 17, 2, 4, 0, 72, 8),
    (96, 4, 1, 1, 0, 7, 9, 2, 128, 32, 8, 4),
]


@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])
@pytest.mark.parametrize("case", WG_CASES)
def test_wgrad_in_a_guarded_workspace(g, case, cfg):
    """fcn_conv2d_wgrad_cfg_f32, every configuration (4 = the role-split kernel): x and dY are slices of poisoned pixels, the workspace
    has exactly the size the library asks for with red zones on both sides, dw and db end on the last byte."""
    cin, cout, k, s, p, h, w, n, xcs, xo, dcs, dyo = case
    lib = L.load()
    rng = np.random.default_rng(WG_CASES.index(case))
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    oh, ow = ref64.conv_out(h, k, p, s), ref64.conv_out(w, k, p, s)
    dy = rng.standard_normal((n, cout, oh, ow)).astype(np.float32)
    xd, dyd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x"), g.put(poisoned_nhwc(dy, dcs, dyo), at_end=True, name="dY")
    d = conv_desc(xd, xd, None, dyd, n, h, w, cin, xcs, cout, k, p, s, oh, ow, dcs, dyo)
    d.x = xd.ptr + 4 * xo
    splits = C.c_int(0)
    nfl = int(lib.fcn_conv2d_wgrad_workspace_floats_cfg(C.byref(d), cfg, C.byref(splits)))
    ws = g.put(max(nfl, 1) * 4, name="wgrad workspace")
    dwd, dbd = g.put(poisoned((cout, k, k, cin)), at_end=True, name="dw"), g.put(poisoned(cout), at_end=True, name="db")
    L.call("fcn_conv2d_wgrad_cfg_f32", C.byref(d), dwd.ptr, dbd.ptr, ws.ptr, cfg, None)
    dw, db = dwd.read((cout, k, k, cin)).transpose(0, 3, 1, 2), dbd.read((cout,))
    dw64, db64 = ref64.conv2d_wgrad(x, dy, k, p, s)
    mw, mb = ref64.conv2d_wgrad(np.abs(x), np.abs(dy), k, p, s)
    assert poison_free(dw) and poison_free(db)
    within(dw, dw64, ref64.dot_bound_rms(n * oh * ow, mw), "wgrad cfg %d dw" % cfg)
    within(db, db64, ref64.dot_bound_rms(n * oh * ow, mb), "wgrad cfg %d db" % cfg)


def test_wgrad_group_in_a_guarded_workspace(g):
    lib = L.load()
    rng = np.random.default_rng(41)
    n, h, w, cin, xcs, xo = 2, 6, 5, 24, 32, 4
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    xd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x")
    geo = [(36, 1, 0), (4, 3, 1), (33, 5, 2)]
    total = sum((co + 3) // 4 * 4 + 4 for co, _, _ in geo)
    dys = [rng.standard_normal((n, co, h, w)).astype(np.float32) for co, _, _ in geo]
    wide = poisoned((n, h, w, total))
    descs, offs, off = [], [], 4
    for (co, k, p), dy in zip(geo, dys):
        wide[..., off:off + co] = dy.transpose(0, 2, 3, 1)
        offs.append(off)
        off += (co + 3) // 4 * 4 + 4
    dyd = g.put(wide, at_end=True, name="dY")
    for (co, k, p), o in zip(geo, offs):
        d = conv_desc(xd, xd, None, dyd, n, h, w, cin, xcs, co, k, p, 1, h, w, total, o)
        d.x = xd.ptr + 4 * xo
        descs.append(d)
    arr = (L.ConvDesc * 3)(*descs)
    ws = g.put(max(int(lib.fcn_conv2d_wgrad_group_workspace_floats(arr, 3)), 1) * 4, name="wgrad group workspace")
    dws = [g.put(poisoned((co, k, k, cin)), at_end=True, name="dw") for co, k, _ in geo]
    dbs = [g.put(poisoned(co), at_end=True, name="db") for co, _, _ in geo]
    L.call("fcn_conv2d_wgrad_group_f32", arr, (C.c_void_p * 3)(*[b.ptr for b in dws]), (C.c_void_p * 3)(*[b.ptr for b in dbs]), 3, ws.ptr, None)
    for (co, k, p), dy, dwd, dbd in zip(geo, dys, dws, dbs):
        dw64, db64 = ref64.conv2d_wgrad(x, dy, k, p, 1)
        mw, mb = ref64.conv2d_wgrad(np.abs(x), np.abs(dy), k, p, 1)
        within(dwd.read((co, k, k, cin)).transpose(0, 3, 1, 2), dw64, ref64.dot_bound_rms(n * h * w, mw), "wgrad group dw")
        within(dbd.read((co,)), db64, ref64.dot_bound_rms(n * h * w, mb), "wgrad group db")


@pytest.mark.parametrize("cout,cin,k", [(36, 24, 3), (4, 5, 1), (33, 3, 7)])
def test_weights_flip(g, cout, cin, k):
    rng = np.random.default_rng(42)
    cin4, co4 = (cin + 3) // 4 * 4, (cout + 3) // 4 * 4
    wt = rng.standard_normal((cout, cin, k, k)).astype(np.float32)
    w = np.zeros((cout, k, k, cin4), np.float32)
    w[..., :cin] = wt.transpose(0, 2, 3, 1)
    wd, wtd = g.put(w, at_end=True, name="w"), g.put(poisoned((cin, k, k, co4)), at_end=True, name="wt")
    L.call("fcn_conv_weights_flip_f32", wd.ptr, wtd.ptr, cout, k, k, cin, cin4, co4, None)
    got = wtd.read((cin, k, k, co4))
    assert np.array_equal(got[..., :cout], wt[:, :, ::-1, ::-1].transpose(1, 2, 3, 0)) and np.all(got[..., cout:] == 0)


def test_relu_and_sigmoid_backward(g):
    rng = np.random.default_rng(43)
    n, c, h, w, cs = 2, 10, 3, 5, 12
    y = np.maximum(rng.standard_normal((n, c, h, w)), 0).astype(np.float32)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    yd, dyd = g.put(poisoned_nhwc(y, cs), at_end=True, name="y"), g.put(poisoned_nhwc(dy, cs), at_end=True, name="dy")
    L.call("fcn_relu_bwd_f32", dyd.ptr, yd.ptr, dyd.ptr, n * h * w, c, cs, None)
    full = dyd.read((n, h, w, cs))
    assert np.array_equal(nchw(full, c), dy * (y > 0)) and slice_untouched(full, 0, c)
    for count in COUNTS:
        sg = ref64.sigmoid(rng.standard_normal(count) * 4).astype(np.float32)
        gr = rng.standard_normal(count).astype(np.float32)
        for acc in (0, 1):
            base = rng.standard_normal(count).astype(np.float32)
            sd, gd, od = g.put(sg, at_end=True), g.put(gr, at_end=True), g.put(base if acc else poisoned(count), at_end=True, name="dx")
            L.call("fcn_sigmoid_bwd_f32", sd.ptr, gd.ptr, od.ptr, count, acc, None)
            want = gr.astype(np.float64) * sg * (1.0 - sg) + (base if acc else 0)
            within(od.read((count,)), want, 4 * ref64.U32 * (np.abs(want) + np.abs(base) * acc + np.abs(gr)), "sigmoid bwd")


@pytest.mark.parametrize("slope", [0.0, 0.1])
@pytest.mark.parametrize("acc", [0, 1])
def test_relu_backward_with_slope_and_accumulate(g, acc, slope):
    """fcn_relu_bwd_slope_f32, dx (+)= y > 0 ? dy : slope * dy: the packed form (cstride == C) at every count, the channel-stride view
    (10 channels in pixels of 12: the pad channels of dx keep their poison), and in place on dy without accumulate.  y is what the
    forward stores: slope * x on the negative side, so its sign is the input's; some outputs are exact zeros."""
    rng = np.random.default_rng(44 + acc)
    sl = np.float32(slope)

    def case(shape):
        x = rng.standard_normal(shape).astype(np.float32)
        x.flat[::7] = 0.0
        y = np.where(x > 0, x, sl * x).astype(np.float32)
        dy, base = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
        want = np.where(y > 0, dy.astype(np.float64), float(sl) * dy) + (base if acc else 0)
        return y, dy, base, want, 2 * ref64.U32 * (np.abs(want) + np.abs(base) * acc + np.abs(dy))

    for count in COUNTS:
        y, dy, base, want, allow = case((count,))
        yd, dyd = g.put(y, at_end=True, name="y"), g.put(dy, at_end=True, name="dy")
        dxd = g.put(base if acc else poisoned(count), at_end=True, name="dx")
        L.call("fcn_relu_bwd_slope_f32", dyd.ptr, yd.ptr, dxd.ptr, count, 1, 1, float(sl), acc, None)
        within(dxd.read((count,)), want, allow, "relu bwd packed %d" % count)
    n, c, h, w, cs = 2, 10, 3, 5, 12
    y, dy, base, want, allow = case((n, c, h, w))
    yd, dyd = g.put(poisoned_nhwc(y, cs), at_end=True, name="y"), g.put(poisoned_nhwc(dy, cs), at_end=True, name="dy")
    dxd = g.put(poisoned_nhwc(base, cs) if acc else poisoned((n, h, w, cs)), at_end=True, name="dx")
    L.call("fcn_relu_bwd_slope_f32", dyd.ptr, yd.ptr, dxd.ptr, n * h * w, c, cs, float(sl), acc, None)
    full = dxd.read((n, h, w, cs))
    assert poison_free(nchw(full, c)) and slice_untouched(full, 0, c)
    within(nchw(full, c), want, allow, "relu bwd view")
    if not acc:
        L.call("fcn_relu_bwd_slope_f32", dyd.ptr, yd.ptr, dyd.ptr, n * h * w, c, cs, float(sl), 0, None)
        full = dyd.read((n, h, w, cs))
        assert slice_untouched(full, 0, c)
        within(nchw(full, c), want, allow, "relu bwd in place")
    else:      # `+=` into its own dY would be dY + f(dY): refused, like a slope below 0
        lib = L.load()
        assert lib.fcn_relu_bwd_slope_f32(dyd.ptr, yd.ptr, dyd.ptr, n * h * w, c, cs, float(sl), 1, None) == 1
        assert lib.fcn_relu_bwd_slope_f32(dyd.ptr, yd.ptr, dxd.ptr, n * h * w, c, cs, -0.1, 0, None) == 1


@pytest.mark.parametrize("c,cs_dy,co_dy,cs_dx,co_dx", [(8, 16, 8, 12, 4), (6, 9, 2, 7, 1)])
@pytest.mark.parametrize("k,s,p,h,w", [(3, 2, 0, 7, 6), (3, 1, 1, 4, 5), (2, 2, 0, 5, 3), (3, 3, 0, 7, 7)])
def test_maxpool_backward(g, k, s, p, h, w, c, cs_dy, co_dy, cs_dx, co_dx):
    """The three maxpool_bwd kernels (overwrite, accumulate, with the ReLU mask).  With 3 x 3 / stride 3 windows on 7 x 7 and 2 x 2 / stride 2
    on 5 x 3 every input position lies in at most one window: positions no window maps to must come out as exact zeros (overwrite) or keep
    their old value (accumulate)."""
    rng = np.random.default_rng(2)
    n = 2
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    x[0, :, 1, 1] = x[0, :, 1, 2]
    ry, idx = ref64.max_pool(x, k, s, p)
    oh, ow = ry.shape[2:]
    dy = rng.standard_normal(ry.shape).astype(np.float32)
    want = np.zeros(x.shape)
    for (a, ch, i, j), flat in np.ndenumerate(idx):
        want[a, ch, flat // w, flat % w] += dy[a, ch, i, j]
    dyd = g.put(poisoned_nhwc(dy, cs_dy, co_dy), at_end=True, name="dy")
    idd = g.put(np.ascontiguousarray(idx.transpose(0, 2, 3, 1)).astype(np.int32), at_end=True, name="argmax")
    base = rng.standard_normal(x.shape).astype(np.float32)
    act = np.maximum(rng.standard_normal(x.shape), 0).astype(np.float32)
    actd = g.put(poisoned_nhwc(act, cs_dx, co_dx), at_end=True, name="activation")
    args = (n, h, w, c, cs_dx, co_dx, k, s, p, oh, ow, cs_dy, co_dy)
    for acc, mask in ((0, False), (1, False), (1, True), (0, True)):
        dxd = g.put(poisoned_nhwc(base, cs_dx, co_dx) if acc else poisoned((n, h, w, cs_dx)), at_end=True, name="dx")
        if mask:
            L.call("fcn_maxpool_bwd_mask_f32", dyd.ptr, idd.ptr, dxd.ptr, *args, acc, actd.ptr, cs_dx, co_dx, None)
        else:
            L.call("fcn_maxpool_bwd_f32", dyd.ptr, idd.ptr, dxd.ptr, *args, acc, None)
        full = dxd.read((n, h, w, cs_dx))
        got = nchw(full, c, co_dx)
        ref = (want + base * acc) * ((act > 0) if mask else 1)
        assert poison_free(got) and slice_untouched(full, co_dx, c)
        within(got, ref, 8 * ref64.U32 * (np.abs(want) + np.abs(base) + 1), "maxpool bwd acc=%d mask=%d" % (acc, mask))
        if not acc:
            assert np.all(got[want == 0] == 0)


@pytest.mark.parametrize("c,ls,beta,cs", [(64, 5, 0.75, 72), (4, 5, 0.75, 8), (6, 3, 0.75, 7), (10, 5, 0.6, 12)])
def test_lrn_backward(g, c, ls, beta, cs):
    rng = np.random.default_rng(3)
    n, h, w, alpha = 2, 3, 4, 1e-4
    x = (rng.standard_normal((n, c, h, w)) * 60).astype(np.float32)
    y64, s64 = ref64.lrn(x, ls, alpha, beta)
    y, sc = y64.astype(np.float32), s64.astype(np.float32)
    dy = rng.standard_normal(x.shape).astype(np.float32)
    # dx = dy s^-beta - 2 alpha beta / n * x * sum_{window} (dy y / s)
    ratio = dy.astype(np.float64) * y / sc
    half = (ls - 1) // 2
    acc = np.zeros_like(ratio)
    mag = np.zeros_like(ratio)
    for d in range(-half, half + 1):
        lo, hi = max(0, -d), min(c, c - d)
        acc[:, lo:hi] += ratio[:, lo + d:hi + d]
        mag[:, lo:hi] += np.abs(ratio[:, lo + d:hi + d])
    t1 = dy * sc.astype(np.float64) ** -beta
    want = t1 - 2 * alpha * beta / ls * x * acc
    allow = 16 * ref64.U32 * (np.abs(t1) + 2 * alpha * beta / ls * np.abs(x) * mag)
    xd, yd, dyd = (g.put(poisoned_nhwc(a, cs), at_end=True) for a in (x, y, dy))
    sd = g.put(np.ascontiguousarray(sc.transpose(0, 2, 3, 1)), at_end=True, name="scale")
    base = rng.standard_normal(x.shape).astype(np.float32)
    for accum in (0, 1):
        dxd = g.put(poisoned_nhwc(base, cs) if accum else poisoned((n, h, w, cs)), at_end=True, name="dx")
        L.call("fcn_lrn_bwd_f32", xd.ptr, yd.ptr, sd.ptr, dyd.ptr, dxd.ptr, n * h * w, c, cs, cs, ls, alpha, beta, accum, None)
        full = dxd.read((n, h, w, cs))
        got = nchw(full, c)
        assert poison_free(got) and slice_untouched(full, 0, c)
        within(got, want + base * accum, allow + 2 * ref64.U32 * np.abs(base) * accum, "lrn bwd accum=%d" % accum)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("pixels,c,cs", [(1, 1, 1), (7, 4, 4), (35, 5, 8), (1003, 3, 4)])
def test_l1_and_euclidean_loss(g, kind, pixels, c, cs):
    rng = np.random.default_rng(44)
    a, b = rng.standard_normal((2, pixels, c)).astype(np.float32)
    b[0] = a[0]                                                # sign(0) = 0
    wa, wb = poisoned((pixels, cs)), poisoned((pixels, cs))
    wa[:, :c], wb[:, :c] = a, b
    ad, bd = g.put(wa, at_end=True, name="a"), g.put(wb, at_end=True, name="b")
    dad, ld = g.put(poisoned((pixels, cs)), at_end=True, name="da"), g.put(poisoned(1), at_end=True, name="loss")
    L.call("fcn_loss_f32", kind, ad.ptr, bd.ptr, dad.ptr, ld.ptr, pixels, c, cs, 2, 0.5, None)
    loss64, da64 = (ref64.l1_loss if kind == 0 else ref64.euclidean_loss)(a, b, 2, 0.5)
    d = np.abs(a.astype(np.float64) - b)
    mag = (d if kind == 0 else d * d / 2).sum() / 2
    within(ld.read((1,)), np.array([loss64]), ref64.dot_bound_rms(pixels * c, mag) + 1e-30, "loss kind %d" % kind)
    full = dad.read((pixels, cs))
    assert poison_free(full[:, :c]) and slice_untouched(full, 0, c)
    within(full[:, :c], da64, 4 * ref64.U32 * (np.abs(da64) + np.abs(a) / 4 + np.abs(b) / 4) + 1e-37, "loss gradient kind %d" % kind)


def solver_layout(rng):
    """Three segments with two poisoned padding words between them; the middle one has lr_mult = 0."""
    counts, gaps = [5, 1003, 4], 2
    total = sum(counts) + gaps * (len(counts) - 1)
    segs = (L.SolverSeg * 3)()
    live = np.zeros(total, bool)
    off = 0
    for i, cnt in enumerate(counts):
        segs[i].offset, segs[i].count, segs[i].lr_mult, segs[i].decay_mult = off, cnt, (1.0, 0.0, 2.0)[i], (1.0, 1.0, 0.0)[i]
        live[off:off + cnt] = True
        off += cnt + gaps
    return segs, live, total


def flat(rng, live, scale=1.0, positive=False):
    a = poisoned(live.size)
    v = rng.standard_normal(int(live.sum())) * scale
    a[live] = np.abs(v) if positive else v
    return a


def per_element(segs, live, field):
    out = np.zeros(live.size)
    for s in segs:
        out[s.offset:s.offset + s.count] = getattr(s, field)
    return out


def test_sgd_update_segments(g):
    rng = np.random.default_rng(45)
    segs, live, total = solver_layout(rng)
    w, gr, hist = flat(rng, live), flat(rng, live), flat(rng, live, 0.1)
    frozen = slice(segs[1].offset, segs[1].offset + segs[1].count)
    hist[frozen] = 0                                           # no old momentum: the lr_mult = 0 segment must not move at all
    wd, gd, hd = g.put(w, at_end=True, name="w"), g.put(gr, at_end=True, name="g"), g.put(hist, at_end=True, name="hist")
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    L.call("fcn_sgd_update_f32", wd.ptr, gd.ptr, hd.ptr, sd.ptr, 3, 0.01, 0.9, 5e-4, 0.5, None)
    w2, h2 = wd.read((total,)), hd.read((total,))
    lr, dm = per_element(segs, live, "lr_mult"), per_element(segs, live, "decay_mult")
    ww, hh = ref64.sgd_update(np.where(live, w, 0), np.where(live, gr, 0), np.where(live, hist, 0), 0.01, 0.9, 5e-4, lr, dm, 0.5)
    assert np.array_equal(w2.view(np.uint32)[~live], w.view(np.uint32)[~live]) and np.array_equal(h2.view(np.uint32)[~live], hist.view(np.uint32)[~live])
    assert np.array_equal(gd.read((total,)).view(np.uint32), gr.view(np.uint32))
    within(h2[live], hh[live], 8 * ref64.U32 * (np.abs(hh[live]) + np.abs(hist[live])) + 1e-37, "sgd history")
    within(w2[live], ww[live], 8 * ref64.U32 * (np.abs(ww[live]) + np.abs(hh[live])) + 1e-37, "sgd weights")
    assert np.array_equal(w2[frozen], w[frozen]) and not h2[frozen].any()      # lr_mult = 0: bit-identical


@pytest.mark.parametrize("t", [1, 1000])
def test_adam_update_segments(g, t):
    rng = np.random.default_rng(46 + t)
    segs, live, total = solver_layout(rng)
    w, gr, m, v = flat(rng, live), flat(rng, live), flat(rng, live, 0.1), flat(rng, live, 0.01, positive=True)
    if t == 1:
        m[live], v[live] = 0, 0
    wd, gd, md, vd = (g.put(a, at_end=True, name=nm) for a, nm in ((w, "w"), (gr, "g"), (m, "m"), (v, "v")))
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    L.call("fcn_adam_update_f32", wd.ptr, gd.ptr, md.ptr, vd.ptr, sd.ptr, 3, 0.001, 0.9, 0.999, 1e-8, 5e-4, t, 1.0, None)
    w2, m2, v2 = wd.read((total,)), md.read((total,)), vd.read((total,))
    lr, dm = per_element(segs, live, "lr_mult"), per_element(segs, live, "decay_mult")
    z = lambda a: np.where(live, a, 0)
    f = lambda v_: float(np.float32(v_))                      # the ABI takes float32 scalars: 1 - beta2 of the ROUNDED beta2 is what both sides subtract
    ww, mm, vv = ref64.adam_update(z(w), z(gr), z(m), z(v), f(0.001), f(0.9), f(0.999), f(1e-8), f(5e-4), lr, dm, t)
    for got, old in ((w2, w), (m2, m), (v2, v)):
        assert np.array_equal(got.view(np.uint32)[~live], old.view(np.uint32)[~live])
    frozen = slice(segs[1].offset, segs[1].offset + segs[1].count)
    moves = live.copy()
    moves[frozen] = False                                      # (the moments of an lr_mult = 0 segment are not specified: nothing ever reads them)
    within(m2[moves], mm[moves], 8 * ref64.U32 * (np.abs(mm[moves]) + np.abs(m[moves]) + 1e-30), "adam m t=%d" % t)
    within(v2[moves], vv[moves], 8 * ref64.U32 * (np.abs(vv[moves]) + 1e-30), "adam v t=%d" % t)
    step = np.abs(ww - z(w))[live]
    # sqrt(1 - 0.999^t) in float32 loses digits to the subtraction at t = 1 (1 - 0.999 carries 2^-24 / 1e-3 relative): 1e-4 of the step
    within(w2[live], ww[live], 2 * ref64.U32 * np.abs(ww[live]) + 2e-4 * step + 1e-37, "adam w t=%d" % t)
    assert np.array_equal(w2[frozen], w[frozen])               # lr_mult = 0: bit-identical


@pytest.mark.parametrize("c,k,s,p,h,w,cs_dx,cs_dy,co_dy", [(5, 4, 2, 1, 3, 4, 7, 9, 3), (4, 8, 4, 2, 2, 5, 4, 8, 4)])
def test_depthwise_deconv_backward(g, c, k, s, p, h, w, cs_dx, cs_dy, co_dy):
    rng = np.random.default_rng(47)
    n = 2
    oh, ow = s * (h - 1) + k - 2 * p, s * (w - 1) + k - 2 * p
    dy = rng.standard_normal((n, c, oh, ow)).astype(np.float32)
    wt = rng.standard_normal((c, k, k)).astype(np.float32)
    want = ref64.deconv_depthwise_bwd(dy, wt, k, s, p, h, w)
    mag = ref64.deconv_depthwise_bwd(np.abs(dy), np.abs(wt), k, s, p, h, w)
    dyd, wd = g.put(poisoned_nhwc(dy, cs_dy, co_dy), at_end=True, name="dy"), g.put(wt, at_end=True)
    base = rng.standard_normal((n, c, h, w)).astype(np.float32)
    for acc in (0, 1):
        dxd = g.put(poisoned_nhwc(base, cs_dx) if acc else poisoned((n, h, w, cs_dx)), at_end=True, name="dx")
        L.call("fcn_deconv_depthwise_bwd_f32", dyd.ptr, wd.ptr, dxd.ptr, n, h, w, c, cs_dx, k, s, p, oh, ow, cs_dy, co_dy, acc, None)
        full = dxd.read((n, h, w, cs_dx))
        got = nchw(full, c)
        assert poison_free(got) and slice_untouched(full, 0, c)
        within(got, want + base * acc, ref64.dot_bound_rms(k * k, mag + np.abs(base) * acc), "deconv bwd")


@pytest.mark.parametrize("normalize,ignore", [(1, True), (0, False)])
def test_softmax_loss(g, normalize, ignore):
    lib = L.load()
    rng = np.random.default_rng(48)
    n, c, h, w, xcs = 2, 5, 3, 7, 8
    x = (rng.random((n, c, h, w)) * 60 - 30).astype(np.float32)
    lab = rng.integers(0, c, (n, h, w)).astype(np.float32)
    if ignore:
        lab[0, 0, :3] = 255
    xd = g.put(poisoned_nhwc(x, xcs), at_end=True, name="x")
    wide_lab = poisoned((n, h, w, 2))
    wide_lab[..., 0] = lab
    labd = g.put(wide_lab, at_end=True, name="label")
    dxd, ld = g.put(poisoned((n, h, w, xcs)), at_end=True, name="dx"), g.put(poisoned(1), at_end=True, name="loss")
    ws = g.put(int(lib.fcn_softmax_loss_workspace_bytes()), name="softmax loss workspace")
    L.call("fcn_softmax_loss_f32", xd.ptr, labd.ptr, dxd.ptr, ld.ptr, n, n * h * w, c, xcs, 2, normalize, int(ignore), 255, 0.5, ws.ptr, None)
    loss64, dx64 = ref64.softmax_loss(x, lab, bool(normalize), 255 if ignore else None, 0.5)
    full = dxd.read((n, h, w, xcs))
    got = nchw(full, c)
    assert poison_free(got) and slice_untouched(full, 0, c)
    within(ld.read((1,)), np.array([loss64]), 1e-5 * abs(loss64), "softmax loss")
    within(got, dx64, 100 * ref64.U32 * (np.abs(dx64) + 0.5 / (n * h * w)), "softmax loss gradient")


def test_dropout_of_a_slice(g):
    rng = np.random.default_rng(49)
    n, c, h, w, xcs, xo, ycs, yo = 2, 5, 3, 4, 9, 3, 7, 1
    x = rng.standard_normal((n, c, h, w)).astype(np.float32) + 3
    xd, yd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x"), g.put(poisoned((n, h, w, ycs)), at_end=True, name="y")
    L.call("fcn_dropout_f32", xd.ptr, yd.ptr, n, c, h, w, xcs, xo, ycs, yo, 0.4, 5, 0, None)
    full = yd.read((n, h, w, ycs))
    y = nchw(full, c, yo)
    assert poison_free(y) and slice_untouched(full, yo, c)
    kept = y != 0
    assert 0.3 < kept.mean() < 0.9
    within(y[kept], x[kept].astype(np.float64) / 0.6, 4 * ref64.U32 * np.abs(x[kept]) / 0.6, "dropout")


# ---- byte kernels ---------------------------------------------------------------------------------------------------
def test_preprocess_frame_ending_on_the_last_byte(g):
    """fcn_preprocess_bgr8: a 7 x 9 frame (189 bytes, not a multiple of 4) that ends on the last byte in front of the red zone; the
    red zone's bytes (0xC0 / 0x7F) lie above every pixel and would become the frame's maximum if a vector load ran over."""
    rng = np.random.default_rng(50)
    h, w, H, W, cs = 7, 9, 5, 6, 4
    frame = rng.integers(10, 100, (h, w, 3)).astype(np.uint8)      # all below 0x7F: an over-read changes the maximum
    fd = g.put(frame, at_end=True, name="frame")
    dd, mm = g.put(poisoned((H, W, cs)), at_end=True, name="blob"), g.put(32, name="minmax")
    L.call("fcn_preprocess_bgr8", fd.ptr, h, w, dd.ptr, H, W, cs, 0.0, mm.ptr, None)
    out = dd.read((H, W, cs))
    from oracle import detect_ref as D
    want = D.preprocess_frame(frame, W, H).transpose(1, 2, 0)
    assert poison_free(out[..., :3]) and np.abs(out[..., :3] - want).max() < 1e-5
