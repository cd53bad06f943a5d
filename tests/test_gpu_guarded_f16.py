"""Guard-banded, poisoned-buffer parity of the HALF-FLOAT hot path against the float64 reference (tests/ref64.py), -m gpu.

The rules of tests/test_gpu_guarded.py, applied to the kernels that carry batched f16 inference: the streaming convolution
(conv_stream.hip, every configuration), the f16 first-layer kernels, the f16 pooling / LRN family, the f16 layout and image kernels,
the fused head tail, and two training leftovers.  Every device tensor lives in a guarded allocation; an input is a channel slice of
wider pixels whose other channels hold poison, with the data pointer moved; an output starts as poison and everything outside its
slice must be bit-identical afterwards; the red zones are read back when the `g` block ends.  The reference is computed in float64
from the SAME f16-rounded operands and the bound is per element (ref64.dot_bound_f16, or half an f16 ulp plus the float32 term).

Contract of the half kernels (include/fcnhip.h): Cin and x_cstride are multiples of 8 and the channels between a blob's real count and
the next multiple of 8 are the CALLER'S zeros - so the poison lies outside the Cin slice, except where the header says a pad is not
read (the constant-channel first layer), where it lies in the pad too.

Every line `BOUND <what> <ratio>` printed (pytest -s) is the worst |y - y64| / allowance of that check."""
import ctypes as C
import functools

import numpy as np
import pytest

import ref64
from conftest import CFG_FIRST7
from fcn_object_detector_amd import lib as L
from gpu_util import GUARD_BYTES, Guards, channels_untouched, conv_desc, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched
from test_gpu_f16 import _STREAM_SHAPE, STREAM_CFGS, _stream_takes

pytestmark = pytest.mark.gpu
F16 = np.float16


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def within(y, y64, allow, what=""):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)
    return ratio


def halves(a):
    """Rounded to half, held as float32: the operand both sides see."""
    return np.asarray(a).astype(F16).astype(np.float32)


def ohwi(w, dtype=F16):
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1)).astype(dtype)


# ---- a. streaming convolution ---------------------------------------------------------------------------------------------------
# conv_stream_f16 stages, per filter row and 64-channel chunk, a SLAB of `rows` consecutive padded-raster entries (an entry = one
# pixel of x_cstride halves) that starts `pad` entries and `pad` image rows in front of the tile's first pixel, and a weight chunk of
# BN bank rows of K halves.  Both go through buffer descriptors bounded by the operand's last byte, so nothing outside is fetched -
# which is what these cases establish; they are nevertheless SIZED so that a loader without that bound would stay inside the red zones:
#   x, in front of image 0:   (pad W + pad) x_cstride 2 bytes                                 (worst here: 2 x 25 x 384 bytes = 19 KiB)
#   x, behind the last image: the last tile's slab runs rows_max entries from its base and `pad` image rows below:
#                             ((t1 + pad + 1) W - N H W) x_cstride 2 bytes, t1 = the padded-raster row of the slab's last entry
#                             (worst here: the 1x1 group on 288-channel pixels, 160 pixels behind the blob = 90 KiB)
#   w, behind row Cout - 1:   (ceil(Cout / BN) BN - Cout) K 2 bytes, BN = 64 / 128 / 192      (worst here: 120 rows of 864 halves = 202 KiB)
# `stream_reach` computes them per case and configuration and the test asserts them against GUARD_BYTES before anything is launched.
_STREAM_BN = dict(zip(STREAM_CFGS, [128, 64, 128, 64, 128, 64, 64, 192, 192, 128, 64]))


def S(cin, cout, k, h, w, n, xcs=None, xo=0, ycs=None, yo=0, relu=False, bias=True, at_end=True):
    """One problem on one input."""
    return dict(n=n, h=h, w=w, xcs=xcs or cin, inputs=[(cin, xo)], probs=[(0, cout, k, relu, bias, yo)], ycs=ycs or cout + yo, at_end=at_end)


STREAM_CASES = [
    # x as a slice of a wider poisoned blob (x_cstride 1.5x .. 4x Cin, offsets 8 and 24 halves): 1x1, 3x3, 5x5
    S(64, 72, 1, 12, 20, 2, xcs=96, xo=8, ycs=88, yo=8),                  # 0: ragged 64- and 128-channel tiles
    S(32, 24, 3, 9, 14, 2, xcs=128, xo=24, ycs=32, yo=8, at_end=False),   # 1: W + 2 pad == 16, the smallest accepted; unpacked (a slice)
    S(16, 16, 5, 7, 24, 3, xcs=48, xo=8, ycs=24, yo=8),                   # 2: W = 24, the narrowest 5x5 rows a 256-pixel tile's slab holds
    S(48, 120, 5, 6, 19, 2),                                               # 3: five filter rows of one short chunk; W = 19: 128-pixel tiles only
    S(32, 8, 3, 1, 40, 2),                                                 # 4: H = 1: every slab row above and below is padding; packed taps 2 + 1
    S(16, 16, 5, 2, 30, 5, at_end=False),                                  # 5: H = 2 under 5x5; packed taps 4 + 1; batch 5
    S(16, 8, 5, 1, 27, 1, xcs=32, xo=8),                                   # 6: H = 1 under 5x5, M = 27, Cout = 8
    S(96, 136, 3, 2, 28, 3, relu=True),                                    # 7: H = 2, Cin = 64 + 32, Cout 136: two ragged tile widths; ReLU
    S(32, 24, 3, 11, 15, 5, xcs=48, xo=8, at_end=False),                   # 8: 825 pixels in 5 images: tiles straddle image boundaries
    S(32, 24, 3, 11, 15, 5, xcs=48, xo=8),                                 # 9: ... and the last tile's slab runs into the red zone
    S(64, 16, 1, 16, 16, 1),                                               # 10: M = 256: exactly one tile
    S(64, 16, 1, 8, 16, 1, bias=False),                                    # 11: M = 128
    S(64, 16, 1, 1, 257, 1, relu=True),                                    # 12: M = 257: one more than a tile
    S(64, 16, 1, 3, 43, 1),                                                # 13: M = 129
    S(192, 16, 1, 6, 17, 1),                                               # 14: M = 102 < one tile
    S(480, 208, 1, 12, 20, 1, bias=False),                                 # 15: a long 1x1 walk (8 chunks, the last one 32 channels), Cout 208
    S(192, 16, 1, 9, 11, 1),                                               # 16: image rows of 11: refused by every configuration
    S(64, 64, 3, 20, 8, 1),                                                # 17: image rows of 8 + 2: refused
    # groups: slices of ONE poisoned input blob (the shared *_reduce buffer) in, slices of ONE poisoned output blob out
    dict(n=2, h=10, w=20, xcs=288, inputs=[(192, 8)], ycs=256, at_end=True,                       # 18: 1x1 x 3 on one input
         probs=[(0, 48, 1, True, True, 8), (0, 96, 1, False, False, 64), (0, 16, 1, False, True, 200)]),
    dict(n=3, h=8, w=24, xcs=128, inputs=[(96, 8), (16, 104)], ycs=256, at_end=True,             # 19: 3x3 + 5x5
         probs=[(0, 128, 3, False, True, 64), (1, 32, 5, True, True, 200)]),
    dict(n=3, h=8, w=24, xcs=192, inputs=[(96, 8), (16, 104), (64, 120)], ycs=320, at_end=False,  # 20: the whole inception level
         probs=[(0, 136, 3, False, True, 8), (1, 48, 5, False, False, 200), (2, 64, 1, True, True, 256)]),
]


@functools.lru_cache(maxsize=None)
def stream_data(ci):
    """Host operands and float64 references of a case: built once, run under every configuration."""
    c = STREAM_CASES[ci]
    rng = np.random.default_rng(1000 + ci)
    n, h, w = c["n"], c["h"], c["w"]
    xs = [halves(rng.standard_normal((n, cin, h, w))) for cin, _ in c["inputs"]]
    wide = poisoned((n, h, w, c["xcs"]), dtype=F16)
    for x, (cin, xo) in zip(xs, c["inputs"]):
        wide[..., xo:xo + cin] = x.transpose(0, 2, 3, 1)
    probs = []
    for xi, cout, k, relu, bias, yo in c["probs"]:
        cin = c["inputs"][xi][0]
        wt = halves(rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k))
        b = rng.standard_normal(cout).astype(np.float32) if bias else None
        y64, mag = ref64.conv2d(xs[xi], wt, b, (k - 1) // 2, 1), ref64.conv2d_mag(xs[xi], wt, b, (k - 1) // 2, 1)
        probs.append(dict(wt=wt, b=b, y64=np.maximum(y64, 0) if relu else y64, allow=ref64.dot_bound_f16(cin * k * k, mag, y64)))
    return wide, probs


def stream_reach(cfg, c):
    """(bytes a slab could reach in front of x, behind x, bytes a weight chunk could reach behind w): see the comment above."""
    rows_max, _, bm = _STREAM_SHAPE[cfg]
    n, h, w, xcs = c["n"], c["h"], c["w"], c["xcs"]
    front = back = wback = 0
    for xi, cout, k, _, _, _ in c["probs"]:
        pad, cin = (k - 1) // 2, c["inputs"][xi][0]
        pw, M = w + 2 * pad, n * h * w
        m0 = (-(-M // bm) - 1) * bm
        t1 = ((m0 // w) * pw + m0 % w + rows_max - 1) // pw
        front = max(front, (pad * w + pad) * xcs * 2)
        back = max(back, max((t1 + pad + 1) * w - M, 0) * xcs * 2)
        bn = _STREAM_BN[cfg]
        wback = max(wback, (-(-cout // bn) * bn - cout) * cin * k * k * 2)
    return front, back, wback


@pytest.mark.parametrize("cfg", STREAM_CFGS)
@pytest.mark.parametrize("ci", range(len(STREAM_CASES)))
def test_stream_conv_every_configuration(g, ci, cfg):
    c = STREAM_CASES[ci]
    assert max(stream_reach(cfg, c)) <= GUARD_BYTES, "case %d would let an unbounded loader leave the allocation" % ci
    lib = L.load()
    wide, probs = stream_data(ci)
    n, h, w, xcs, ycs = c["n"], c["h"], c["w"], c["xcs"], c["ycs"]
    xd = g.put(wide, at_end=c["at_end"], name="x")
    yd = g.put(poisoned((n, h, w, ycs), dtype=F16), name="y")
    descs = []
    for (xi, cout, k, relu, bias, yo), q in zip(c["probs"], probs):
        cin, xo = c["inputs"][xi]
        wd = g.put(ohwi(q["wt"]), at_end=True, name="w of problem %d" % len(descs))
        bd = g.put(q["b"], name="bias") if bias else None
        d = conv_desc(xd, wd, bd, yd, n, h, w, cin, xcs, cout, k, (k - 1) // 2, 1, h, w, ycs, yo, L.CONV_F16 | (L.CONV_RELU if relu else 0))
        d.x = xd.ptr + 2 * xo
        descs.append(d)
    ws = g.put(int(lib.fcn_conv2d_group_workspace_bytes(len(descs))), name="group workspace")
    grp = L.ConvGroup()
    rc = lib.fcn_conv2d_group_prepare((L.ConvDesc * len(descs))(*descs), len(descs), ws.ptr, cfg, C.byref(grp))
    if not all(_stream_takes(cfg, k, w) for _, _, k, _, _, _ in c["probs"]):
        assert rc != 0, "configuration %d must refuse case %d in prepare" % (cfg, ci)
        assert all(b.unchanged() for b in g.bufs), "a refused prepare wrote device memory"
        return
    assert rc == 0 and grp.cfg == cfg and grp.total_tiles >= 1
    L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), None)
    L.call("fcn_conv2d_group_release", ws.ptr)
    full = yd.read((n, h, w, ycs), F16)
    written = np.zeros(ycs, bool)
    for (xi, cout, k, relu, bias, yo), q in zip(c["probs"], probs):
        y = nchw(full.astype(np.float32), cout, yo)
        assert poison_free(y), "case %d cfg %d: the poison around x / w reached the result" % (ci, cfg)
        within(y, q["y64"], q["allow"], "stream cfg %d case %d k %d" % (cfg, ci, k))
        written[yo:yo + cout] = True
    assert channels_untouched(full, written), "case %d cfg %d: channels of y outside the slices were written" % (ci, cfg)


# ---- b. first-layer kernels -----------------------------------------------------------------------------------------------------
FIRST_SIZES = [(1, 9, 9, 64), (2, 7, 45, 40), (1, 5, 201, 64), (3, 17, 33, 48), (2, 13, 9, 40)]      # n, h, w, cout


def run_first7(g, xh, wh, b, n, h, w, cout, flags, expect_refusal=False):
    lib = L.load()
    oh, ow = ref64.conv_out(h, 7, 3, 2), ref64.conv_out(w, 7, 3, 2)
    ycs, yo = cout + 16, 8
    xd, wd, bd = g.put(xh, at_end=True, name="image"), g.put(wh, at_end=True, name="w"), g.put(b, name="bias")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=F16), name="y")
    ws = g.put(int(lib.fcn_conv2d_group_workspace_bytes(1)), name="group workspace")
    d = conv_desc(xd, wd, bd, yd, n, h, w, 8, 8, cout, 7, 3, 2, oh, ow, ycs, yo, L.CONV_F16 | flags)
    grp = L.ConvGroup()
    rc = lib.fcn_conv2d_group_prepare((L.ConvDesc * 1)(d), 1, ws.ptr, CFG_FIRST7, C.byref(grp))
    if expect_refusal:
        assert rc != 0 and all(buf.unchanged() for buf in g.bufs)
        return None
    assert rc == 0 and grp.cfg == CFG_FIRST7
    L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), None)
    L.call("fcn_conv2d_group_release", ws.ptr)
    full = yd.read((n, oh, ow, ycs), F16)
    assert slice_untouched(full, yo, cout), "first layer: channels of y outside the slice were written"
    return nchw(full.astype(np.float32), cout, yo)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n,h,w,cout", FIRST_SIZES)
def test_first_layer_f16_eight_half_pixels(g, n, h, w, cout, relu):
    """conv_first7_f16_kernel (no FCN_CONV_IMAGE_ONES): it loads the whole 16-byte pixel and the whole 16-byte filter tap and multiplies
    all eight halves - so there is no unread pad to poison, and all eight channels carry data here (a channel mix-up shows).  The
    image ends on the last byte in front of its red zone, so does the bank; odd extents, W in {9, 45, 201}, a partial last tile."""
    rng = np.random.default_rng(n * 1000 + w + relu)
    x = halves(rng.standard_normal((n, 8, h, w)))
    wt = halves(rng.standard_normal((cout, 8, 7, 7)) / np.sqrt(8 * 49))
    b = rng.standard_normal(cout).astype(np.float32)
    y = run_first7(g, np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(F16), ohwi(wt), b, n, h, w, cout, L.CONV_RELU if relu else 0)
    y64, mag = ref64.conv2d(x, wt, b, 3, 2), ref64.conv2d_mag(x, wt, b, 3, 2)
    assert poison_free(y)
    within(y, np.maximum(y64, 0) if relu else y64, ref64.dot_bound_f16(8 * 49, mag, y64), "first7 f16")


def test_first_layer_f16_refuses_cout_36(g):
    """Cout must be a multiple of 8 in 40 .. 64 for the half first-layer kernels: 36 is refused in prepare, nothing is written."""
    rng = np.random.default_rng(5)
    x, wt = halves(rng.standard_normal((1, 9, 9, 8))).astype(F16), halves(rng.standard_normal((36, 7, 7, 8))).astype(F16)
    assert run_first7(g, x, wt, np.zeros(36, np.float32), 1, 9, 9, 36, 0, expect_refusal=True) is None


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n,h,w,cout", FIRST_SIZES)
def test_first_layer_f16_constant_channels(g, n, h, w, cout, relu):
    """conv_first7_f16x4_kernel (FCN_CONV_IMAGE_ONES).  It fetches halves 0..3 of a pixel (b, g, r and the first constant 1, whose filter
    half is masked to zero) and halves 0..4 of a filter tap (three filters + the two shift terms); halves 4..7 of a pixel and 5..7 of a
    tap are NOT READ (include/fcnhip.h).  So channels 5..7 of every pixel and of every tap hold poison here, channels 3 and 4 of the
    image hold the promised 1.  The constant channels count only over the taps inside the image: the border pixels (some tap outside)
    are held to their own allowance and reported separately."""
    rng = np.random.default_rng(n * 1000 + h + relu)
    x3 = halves(rng.random((n, 3, h, w)))
    wt = np.zeros((cout, 5, 7, 7), np.float32)
    wt[:, :3] = halves(rng.standard_normal((cout, 3, 7, 7)) / np.sqrt(147))
    term = -127.0 * wt[:, :3].astype(np.float64).sum(1)                      # the folded Power(-127): hi + lo halves
    wt[:, 3] = halves(term)
    wt[:, 4] = halves(term - wt[:, 3].astype(np.float64))
    b = rng.standard_normal(cout).astype(np.float32)
    xh = poisoned((n, h, w, 8), dtype=F16)
    xh[..., :3] = x3.transpose(0, 2, 3, 1)
    xh[..., 3:5] = 1.0
    wh = poisoned((cout, 7, 7, 8), dtype=F16)
    wh[..., :5] = wt.transpose(0, 2, 3, 1)
    y = run_first7(g, xh, wh, b, n, h, w, cout, L.CONV_IMAGE_ONES | (L.CONV_RELU if relu else 0))
    y64, mag, border = ref64.conv2d_image_ones(x3, wt, b, 3, 2)
    allow = ref64.dot_bound_f16(5 * 49, mag, y64)
    want = np.maximum(y64, 0) if relu else y64
    assert poison_free(y), "the poison in channels 5..7 reached the result"
    within(y[..., border], want[..., border], allow[..., border], "first7 IMAGE_ONES border")
    if (~border).any():
        within(y[..., ~border], want[..., ~border], allow[..., ~border], "first7 IMAGE_ONES interior")


@pytest.mark.parametrize("n,h,w,cout", [(1, 9, 9, 36), (2, 7, 45, 40), (1, 5, 201, 64), (2, 13, 9, 36)])
def test_first_layer_f32_in_halves_out(g, monkeypatch, n, h, w, cout):
    """FCN_CONV_OUT_F16 (conv1_1 / conv1 of an f16 engine that keeps its image in float32): float32 x as a slice of poisoned pixels,
    float32 filters, y stored as halves at channel offset 8 of poisoned half pixels."""
    monkeypatch.delenv("FCN_CONV_CFG", raising=False)
    rng = np.random.default_rng(n * 100 + w)
    x = rng.standard_normal((n, 4, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, 4, 7, 7)) / 14).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    oh, ow = ref64.conv_out(h, 7, 3, 2), ref64.conv_out(w, 7, 3, 2)
    ycs, yo = (cout + 7) // 8 * 8 + 16, 8
    xd = g.put(poisoned_nhwc(x, 8, 4), at_end=True, name="x")
    wd, bd = g.put(ohwi(wt, np.float32), at_end=True, name="w"), g.put(b, name="bias")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=F16), name="y")
    d = conv_desc(xd, wd, bd, yd, n, h, w, 4, 8, cout, 7, 3, 2, oh, ow, ycs, yo, L.CONV_OUT_F16)
    d.x = xd.ptr + 16
    L.call("fcn_conv2d_fwd_f32", C.byref(d), None)
    full = yd.read((n, oh, ow, ycs), F16)
    y = nchw(full.astype(np.float32), cout, yo)
    y64, mag = ref64.conv2d(x, wt, b, 3, 2), ref64.conv2d_mag(x, wt, b, 3, 2)
    assert poison_free(y) and slice_untouched(full, yo, cout)
    within(y, y64, ref64.dot_bound_f16(4 * 49, mag, y64), "first layer OUT_F16")


# ---- c. pooling / LRN -----------------------------------------------------------------------------------------------------------
# A pooling / LRN kernel reads whole 16-byte channel groups of the pixels under one output tile: the farthest a tile-granular form could
# reach is one LDS patch ((2 TH + 1) x (2 TW + 1) pixels of x_cstride halves: 17 x 33 x 208 x 2 = 228 KiB for the widest case here).
POOL16_CASES = [  # k, s, p, n, h, w, c, x_cstride, xo, y_cstride, yo
    (3, 1, 1, 2, 5, 4, 8, 24, 8, 24, 8),
    (3, 2, 0, 2, 6, 7, 8, 16, 8, 8, 0),              # last window clipped in y only
    (3, 2, 1, 2, 7, 6, 16, 32, 8, 24, 8),
    (2, 2, 0, 2, 5, 8, 8, 8, 0, 16, 8),              # the generic kernel (k = 2)
    (3, 1, 1, 2, 1, 9, 8, 16, 8, 8, 0),              # one row
    (5, 3, 2, 2, 9, 1, 8, 8, 0, 16, 8),              # one column, 5 x 5 windows
    (3, 1, 1, 3, 56, 56, 16, 32, 8, 40, 16),         # N H W >= 8192: the LDS 3x3 / stride 1 kernel, 8 x 28 tiles
    (3, 1, 1, 2, 72, 61, 72, 80, 8, 72, 0),          # ... extents that do not divide into tiles, C not a multiple of 64
    (3, 1, 1, 9, 37, 29, 8, 8, 0, 8, 0),             # ... dense, W < 32
]


@pytest.mark.parametrize("at_end", [True, False], ids=["at_end", "at_front"])
@pytest.mark.parametrize("case", POOL16_CASES)
def test_maxpool_f16_all_negative_in_huge_poison(g, case, at_end):
    """fcn_maxpool_fwd_f16 (generic, quad and LDS forms): all-negative halves between channels / red zones of +65504 - a kernel that
    takes anything from outside its blob, or pads with zeros, returns a larger maximum.  Exact equality: the maximum is a selection."""
    k, s, p, n, h, w, c, xcs, xo, ycs, yo = case
    rng = np.random.default_rng(k * 100 + h)
    x = halves(-np.abs(rng.standard_normal((n, c, h, w))) * 3 - 0.25)
    x[0, :, 0, 0] = x[0, :, 0, min(1, w - 1)]
    want = ref64.max_pool_values(x, k, s, p)
    oh, ow = want.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison="huge", dtype=F16), at_end=at_end, poison="huge", name="x")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=F16), name="y")
    L.call("fcn_maxpool_fwd_f16", xd.ptr + 2 * xo, yd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, None)
    full = yd.read((n, oh, ow, ycs), F16)
    assert np.array_equal(nchw(full.astype(np.float64), c, yo), want) and slice_untouched(full, yo, c)


@pytest.mark.parametrize("c,xcs,xo,ycs", [(8, 24, 8, 16), (64, 80, 8, 64), (192, 208, 8, 200), (8, 8, 0, 8)])
def test_lrn_f16_of_a_slice_between_poisoned_neighbours(g, c, xcs, xo, ycs):
    """lrn5_f16_kernel: the channel groups beside the slice belong to OTHER blobs (poison); values up to a few hundred, where scale
    leaves 1.  Held to the definition: half an f16 ulp of the float64 value plus the float32 arithmetic (ref64.lrn_f16_allow)."""
    rng = np.random.default_rng(c)
    n, h, w = 2, 3, 5
    x = halves(rng.standard_normal((n, c, h, w)) * 150)
    y64 = ref64.lrn_f16(x, 5, 1e-4, 0.75, round_out=False)
    xd = g.put(poisoned_nhwc(x, xcs, xo, dtype=F16), at_end=True, name="x")
    yd = g.put(poisoned((n, h, w, ycs), dtype=F16), name="y")
    L.call("fcn_lrn_fwd_f16", xd.ptr + 2 * xo, yd.ptr, n * h * w, c, xcs, ycs, 5, 1e-4, 0.75, 1.0, None)
    full = yd.read((n, h, w, ycs), F16)
    y = nchw(full.astype(np.float32), c)
    assert poison_free(y) and slice_untouched(full, 0, c)
    within(y, y64, ref64.lrn_f16_allow(y64, 5, 0.75), "lrn f16")
    print("BOUND lrn f16 differs from the rounded float64 value on %.3g of the elements" % (y != ref64.to_f16_then_f64(y64)).mean())


def test_lrn_f16_refuses_local_size_3(g):
    """The half LRN implements local_size 5 only: 3 is FCN_E_UNSUPPORTED, decided before anything is launched."""
    x = poisoned((15, 16), dtype=F16)
    xd, yd = g.put(x, name="x"), g.put(poisoned((15, 16), dtype=F16), name="y")
    assert L.load().fcn_lrn_fwd_f16(xd.ptr, yd.ptr, 15, 16, 16, 16, 3, 1e-4, 0.75, 1.0, None) == 3
    assert xd.unchanged() and yd.unchanged()


POOL_LRN16_CASES = [  # k, s, p, n, h, w, c, x_cstride, xo
    (3, 2, 0, 2, 6, 7, 8, 24, 8),
    (3, 1, 1, 2, 5, 4, 16, 32, 8),
    (3, 2, 1, 2, 9, 1, 40, 48, 8),                   # one-column images
    (3, 2, 0, 2, 15, 21, 64, 64, 0),                 # odd extents, dense
    (3, 2, 0, 8, 57, 61, 192, 208, 8),               # N H W C >= 2^22: the LDS-patch kernel, 8-column tiles (OW = 30), odd extents
    (3, 2, 0, 6, 113, 111, 64, 72, 8),               # ... 16-column tiles
]


@pytest.mark.parametrize("lrn_first", [0, 1])
@pytest.mark.parametrize("case", POOL_LRN16_CASES)
def test_pool_lrn_f16_single_pass(g, case, lrn_first):
    """fcn_maxpool_lrn5_fwd_f16, both orders, generic and LDS-patch kernels, each against the DEFINITION (not against the two stand-alone
    launches).  All-negative inputs in huge poison when the pooling reads x; NaN poison when the LRN does."""
    k, s, p, n, h, w, c, xcs, xo = case
    rng = np.random.default_rng(h * 10 + c + lrn_first)
    x = halves(-np.abs(rng.standard_normal((n, c, h, w))) * 60 - 1)
    poison = "nan" if lrn_first else "huge"
    y64 = ref64.pool_lrn_f16(x, k, s, p, lrn_first, 1e-4, 0.75, round_out=False)
    oh, ow = y64.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison=poison, dtype=F16), at_end=True, poison=poison, name="x")
    yd = g.put(poisoned((n, oh, ow, c + 8), dtype=F16), name="y")
    L.call("fcn_maxpool_lrn5_fwd_f16", xd.ptr + 2 * xo, yd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, c + 8, lrn_first, 1e-4, 0.75, 1.0, None)
    full = yd.read((n, oh, ow, c + 8), F16)
    y = nchw(full.astype(np.float32), c)
    assert poison_free(y, poison) and slice_untouched(full, 0, c)
    within(y, y64, ref64.lrn_f16_allow(y64, 5, 0.75), "pool+lrn f16 first=%d %dx%dx%d" % (lrn_first, h, w, c))


@pytest.mark.parametrize("n,h,w,ycs,yo,relu", [(2, 6, 7, 72, 8, 0), (2, 17, 37, 64, 0, 1), (1, 9, 3, 88, 16, 0), (3, 45, 52, 96, 32, 1)])
def test_pool_lrn_conv1x1_f16_single_pass(g, n, h, w, ycs, yo, relu):
    """fcn_maxpool_lrn5_conv1x1_fwd_f16 against pool -> LRN -> (rounded to half, as the kernel stores the normalised tile) -> 1x1
    convolution in float64; allowance derived in ref64.pool_lrn_conv1x1_f16.  x between huge poison (the pooling reads it), the filter
    bank ending on the last byte, y a slice of poisoned pixels."""
    rng = np.random.default_rng(n * h + w)
    c, xcs, xo = 64, 80, 8
    x = halves(-np.abs(rng.standard_normal((n, c, h, w))) * 40 - 1)
    wt = halves(rng.standard_normal((64, c)) * 0.1)
    b = rng.standard_normal(64).astype(np.float32)
    want, allow = ref64.pool_lrn_conv1x1_f16(x, wt, b, 3, 2, 0, 1e-4, 0.75, 1.0, relu=bool(relu))
    oh, ow = want.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison="huge", dtype=F16), at_end=True, poison="huge", name="x")
    wd, bd = g.put(wt.astype(F16), at_end=True, name="w"), g.put(b, name="bias")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=F16), name="y")
    L.call("fcn_maxpool_lrn5_conv1x1_fwd_f16", xd.ptr + 2 * xo, n, h, w, c, xcs, 3, 2, 0, oh, ow, 1e-4, 0.75, 1.0, wd.ptr, bd.ptr, 64, relu, yd.ptr,
           ycs, yo, None)
    full = yd.read((n, oh, ow, ycs), F16)
    y = nchw(full.astype(np.float32), 64, yo)
    assert poison_free(y, "huge") and slice_untouched(full, yo, 64)
    within(y, want, allow, "pool+lrn+conv1x1 f16")


# ---- d. layout and image kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,h,w,cs,co", [(2, 1, 3, 5, 8, 0), (1, 3, 17, 23, 8, 0), (2, 33, 1, 33, 40, 0), (2, 37, 3, 5, 48, 8), (3, 3, 1, 1, 16, 8)])
def test_layout_kernels_f16(g, n, c, h, w, cs, co):
    """fcn_nchw_f32_to_nhwc_f16 (+ shift, rounded once) and fcn_nhwc_f16_to_nchw_f32: moves - exact; channel counts that are not multiples
    of 8 or of the 32 x 32 transpose tile; the slice's neighbours and the blob's pad channels stay poison."""
    rng = np.random.default_rng(c)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    xd, yd = g.put(x, at_end=True, name="nchw"), g.put(poisoned((n, h, w, cs), dtype=F16), at_end=True, name="nhwc")
    L.call("fcn_nchw_f32_to_nhwc_f16", xd.ptr, yd.ptr, n, c, h, w, cs, co, -0.5, None)
    full = yd.read((n, h, w, cs), F16)
    assert np.array_equal(nchw(full, c, co), (x + np.float32(-0.5)).astype(F16)) and slice_untouched(full, co, c)
    src = g.put(poisoned_nhwc(halves(x), cs, co, dtype=F16), at_end=True, name="nhwc src")
    back = g.put(poisoned((n, c, h, w)), at_end=True, name="nchw dst")
    L.call("fcn_nhwc_f16_to_nchw_f32", src.ptr, back.ptr, n, c, h, w, cs, co, None)
    assert np.array_equal(back.read((n, c, h, w)), halves(x))


def _pixels_ok(out, want, mode):
    """Per mode exactly which elements of a pixel are written: 0 = float32 channels 0..2; 1 = halves 0..2 and nothing else; 3 = the whole
    16-byte pixel (b, g, r, 1, 1, 0, 0, 0)."""
    if mode == 0:
        return poison_free(out[..., :3]) and np.abs(out[..., :3] - want).max() < 1e-6 and slice_untouched(out, 0, 3)
    ok = np.array_equal(out[..., :3], want.astype(F16))
    if mode == 1:
        return ok and slice_untouched(out, 0, 3)
    return ok and np.all(out[..., 3:5] == F16(1)) and np.all(out[..., 5:].view(np.uint16) == 0)


def _frames(rng, n, h, w):
    return rng.integers(10, 100, (n, h, w, 3)).astype(np.uint8)      # all below 0x7F: an over-read of the red zone changes the maximum


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_preprocess_batch_of_unaligned_frames(g, mode):
    """fcn_preprocess_bgr8_batch (and, for one frame, fcn_preprocess_bgr8_f16): three frames of 7 x 9 x 3 = 189 bytes, so frames 1 and 2
    start unaligned and the last one ends on the last byte in front of the red zone; d_minmax is exactly 32 bytes per frame."""
    from oracle import detect_ref as D
    rng = np.random.default_rng(60 + mode)
    n, h, w, H, W, cs = 3, 7, 9, 5, 6, 8
    frames = _frames(rng, n, h, w)
    dt = np.float32 if mode == 0 else F16
    fd, mm = g.put(frames, at_end=True, name="frames"), g.put(32 * n, name="minmax")
    dd = g.put(poisoned((n, H, W, cs), dtype=dt), at_end=True, name="blob")
    L.call("fcn_preprocess_bgr8_batch", fd.ptr, n, h, w, dd.ptr, mode, H, W, cs, 0.0, mm.ptr, None)
    out = dd.read((n, H, W, cs), dt)
    for i in range(n):
        assert _pixels_ok(out[i], D.preprocess_frame(frames[i], W, H).transpose(1, 2, 0), mode), "frame %d" % i
    if mode == 1:
        one = g.put(poisoned((H, W, cs), dtype=F16), at_end=True, name="blob of one frame")
        f2 = g.put(frames[2], at_end=True, name="frame 2")
        L.call("fcn_preprocess_bgr8_f16", f2.ptr, h, w, one.ptr, H, W, cs, 0.0, mm.ptr, None)
        assert _pixels_ok(one.read((H, W, cs), F16), D.preprocess_frame(frames[2], W, H).transpose(1, 2, 0), 1)


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_preprocess_windows_touching_every_border(g, mode):
    """fcn_preprocess_bgr8_rois: windows in the four corners (each touches two frame borders), one covering the whole frame and one
    inside; the frame (11 x 13 x 3 = 429 bytes) ends on the last byte.  Every window is normalised with the WHOLE frame's min / max."""
    from oracle import detect_ref as D
    rng = np.random.default_rng(70 + mode)
    h, w, H, W, cs = 11, 13, 5, 6, 8
    frame = _frames(rng, 1, h, w)[0]
    rois = np.asarray([[0, 0, 6, 5], [7, 0, 6, 5], [0, 6, 6, 5], [7, 6, 6, 5], [0, 0, 13, 11], [3, 2, 6, 5]], np.int32)
    n = len(rois)
    dt = np.float32 if mode == 0 else F16
    fd, mm = g.put(frame, at_end=True, name="frame"), g.put(32, name="minmax")
    dd = g.put(poisoned((n, H, W, cs), dtype=dt), at_end=True, name="blob")
    L.call("fcn_preprocess_bgr8_rois", fd.ptr, h, w, rois.ctypes.data, n, dd.ptr, mode, H, W, cs, 0.0, mm.ptr, None)
    out = dd.read((n, H, W, cs), dt)
    im = D.demean_rgb_image(frame, np.float64)
    for i, (rx, ry, rw, rh) in enumerate(rois):
        want = D.resize_bilinear_cv(im[ry:ry + rh, rx:rx + rw], W, H).astype(np.float32)
        assert _pixels_ok(out[i], want, mode), "window %d" % i


# ---- e. fused head tail ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["one_launch", "contribute_then_finalise"])
@pytest.mark.parametrize("hw", [(28, 28), (9, 7)])
@pytest.mark.parametrize("cfg", [23, 24, 25, 27])
def test_head_tail_in_exactly_sized_buffers(g, cfg, hw, split):
    """fcn_conv2d_group_attach_tail: three branches of a concat blob produce the input of two narrow heads, which the producing launches
    evaluate.  scratch, arrive, the group workspaces and the heads' outputs are guarded and exactly as large as the library asks; the
    heads are slices of poisoned pixels; arrive reads back all zero.  ONE run per case: a bounds-and-value test, not a race hunt."""
    lib = L.load()
    rng = np.random.default_rng(31)
    h, w = hw
    n, cin = 1, 64
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    xd = g.put(poisoned_nhwc(x, cin + 8, 4), at_end=True, name="x")
    couts, ks = [64, 96, 32], [1, 3, 1]
    K = sum(couts)
    ws_ = [(rng.standard_normal((co, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32) for co, k in zip(couts, ks)]
    bs = [rng.standard_normal(co).astype(np.float32) * 0.1 for co in couts]
    blob = g.put(poisoned((n, h, w, K)), name="concat blob")
    descs, off = [], 0
    for wt, b, co, k in zip(ws_, bs, couts, ks):
        d = conv_desc(xd, g.put(ohwi(wt, np.float32), at_end=True, name="w"), g.put(b, name="bias"), blob, n, h, w, cin, cin + 8, co, k, k // 2, 1, h, w,
                      K, off, L.CONV_RELU)
        d.x = xd.ptr + 16
        descs.append(d)
        off += co
    hws = [(rng.standard_normal((co, K, 1, 1)) / np.sqrt(K)).astype(np.float32) for co in (4, 16)]
    hbs = [rng.standard_normal(co).astype(np.float32) for co in (4, 16)]
    cvg, sig, box = (g.put(poisoned((n, h, w, cs)), name=nm) for cs, nm in ((12, "cvg"), (8, "sigmoid"), (24, "bbox")))
    tail = L.ConvTail()
    tail.n = 2
    hd = [g.put(np.ascontiguousarray(hw_.reshape(hw_.shape[0], K)), at_end=True, name="head w") for hw_ in hws]
    hb = [g.put(b, name="head bias") for b in hbs]
    tail.heads[0] = conv_desc(blob, hd[0], hb[0], cvg, n, h, w, K, K, 4, 1, 0, 1, h, w, 12, 4, L.CONV_SIGMOID2, 0.0, sig, 8, 4)
    tail.heads[1] = conv_desc(blob, hd[1], hb[1], box, n, h, w, K, K, 16, 1, 0, 1, h, w, 24, 4, 0)
    sb, ab = int(lib.fcn_conv2d_tail_scratch_bytes(C.byref(tail))), int(lib.fcn_conv2d_tail_arrive_bytes(C.byref(tail)))
    scratch = g.put(sb, name="tail scratch")                      # poison: every slot of a pixel is written before it is read
    arrive = g.put(np.zeros(ab, np.uint8), name="tail arrive")
    tail.scratch, tail.arrive = scratch.ptr, arrive.ptr
    launches = [([0], 0), ([1, 2], 1)] if split else [([0, 1, 2], 1)]
    groups = []
    for idx, fin in launches:
        arr = (L.ConvDesc * len(idx))(*[descs[i] for i in idx])
        wsd = g.put(int(lib.fcn_conv2d_group_workspace_bytes(len(idx))), name="group workspace")
        tail.finalize = fin
        L.call("fcn_conv2d_group_attach_tail", wsd.ptr, C.byref(tail))
        grp = L.ConvGroup()
        L.call("fcn_conv2d_group_prepare", arr, len(idx), wsd.ptr, cfg, C.byref(grp))
        assert grp.cfg == cfg
        groups.append((arr, wsd, grp))
    for _, _, grp in groups:
        L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), None)
    L.call("fcn_device_sync")
    for _, wsd, _ in groups:
        L.call("fcn_conv2d_group_release", wsd.ptr)
    assert not arrive.read((ab,), np.uint8).any(), "the arrival words are not left zero"
    yb = nchw(blob.read((n, h, w, K)), K)
    want = [np.maximum(ref64.conv2d(x, wt, b, k // 2, 1), 0) for wt, b, k in zip(ws_, bs, ks)]
    mags = [ref64.conv2d_mag(x, wt, b, k // 2, 1) for wt, b, k in zip(ws_, bs, ks)]
    off = 0
    assert poison_free(yb)
    for y64, mag, co, k in zip(want, mags, couts, ks):
        within(yb[:, off:off + co], y64, ref64.dot_bound_rms(cin * k * k, mag), "tail producer k %d cfg %d" % (k, cfg))
        off += co
    blob64 = np.concatenate(want, axis=1)
    fc, fs, fx = cvg.read((n, h, w, 12)), sig.read((n, h, w, 8)), box.read((n, h, w, 24))
    for full, cs, co, hw_, hb_, what in ((fc, 12, 4, hws[0], hbs[0], "cvg"), (fx, 24, 16, hws[1], hbs[1], "bbox")):
        y = nchw(full, co, 4)
        y64, mag = ref64.conv2d(blob64, hw_, hb_, 0, 1), ref64.conv2d_mag(blob64, hw_, hb_, 0, 1)
        assert poison_free(y) and slice_untouched(full, 4, co)
        # the heads multiply the float32 blob the producers STORED: its own rounding (dot_bound_rms of the producers, <= 4 sqrt(578) u of
        # the blob's magnitude terms ~ 1e-5 relative) rides into every product - 100 u of the head's magnitude term covers it
        within(y, y64, ref64.dot_bound_rms(K, mag) + 100 * ref64.U32 * mag, "tail head %s cfg %d" % (what, cfg))
    rc = ref64.conv2d(blob64, hws[0], hbs[0], 0, 1)
    assert slice_untouched(fs, 4, 4) and np.abs(nchw(fs, 4, 4) - ref64.sigmoid(rc)).max() < 1e-5


# ---- f. training leftovers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])
def test_wgrad_group_every_configuration_in_a_guarded_workspace(g, cfg):
    """fcn_conv2d_wgrad_group_cfg_f32 with the workspace (where the partial-slab reduction runs) sized by
    fcn_conv2d_wgrad_group_workspace_floats_cfg of the SAME configuration; three problems of different K on one poisoned input."""
    lib = L.load()
    assert cfg < lib.fcn_conv2d_wgrad_num_configs() == 5
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
    ws = g.put(max(int(lib.fcn_conv2d_wgrad_group_workspace_floats_cfg(arr, 3, cfg)), 1) * 4, name="wgrad group workspace")
    dws = [g.put(poisoned((co, k, k, cin)), at_end=True, name="dw") for co, k, _ in geo]
    dbs = [g.put(poisoned(co), at_end=True, name="db") for co, _, _ in geo]
    L.call("fcn_conv2d_wgrad_group_cfg_f32", arr, (C.c_void_p * 3)(*[b.ptr for b in dws]), (C.c_void_p * 3)(*[b.ptr for b in dbs]), 3, ws.ptr, cfg, None)
    for (co, k, p), dy, dwd, dbd in zip(geo, dys, dws, dbs):
        dw64, db64 = ref64.conv2d_wgrad(x, dy, k, p, 1)
        mw, mb = ref64.conv2d_wgrad(np.abs(x), np.abs(dy), k, p, 1)
        dw, db = dwd.read((co, k, k, cin)).transpose(0, 3, 1, 2), dbd.read((co,))
        assert poison_free(dw) and poison_free(db)
        within(dw, dw64, ref64.dot_bound_rms(n * h * w, mw), "wgrad group cfg %d dw k %d" % (cfg, k))
        within(db, db64, ref64.dot_bound_rms(n * h * w, mb), "wgrad group cfg %d db k %d" % (cfg, k))


def test_wgrad_plain_entry_point_in_its_own_workspace(g):
    """fcn_conv2d_wgrad_f32 + fcn_conv2d_wgrad_workspace_floats (the built-in heuristic under its own name): the workspace is exactly
    what the size query of the SAME entry-point pair asks for."""
    lib = L.load()
    rng = np.random.default_rng(40)
    cin, cout, k, p, h, w, n, xcs, xo, dcs, dyo = 24, 36, 5, 2, 3, 11, 2, 40, 8, 48, 4
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    dy = rng.standard_normal((n, cout, h, w)).astype(np.float32)
    xd, dyd = g.put(poisoned_nhwc(x, xcs, xo), at_end=True, name="x"), g.put(poisoned_nhwc(dy, dcs, dyo), at_end=True, name="dY")
    d = conv_desc(xd, xd, None, dyd, n, h, w, cin, xcs, cout, k, p, 1, h, w, dcs, dyo)
    d.x = xd.ptr + 4 * xo
    ws = g.put(max(int(lib.fcn_conv2d_wgrad_workspace_floats(C.byref(d), C.byref(C.c_int(0)))), 1) * 4, name="wgrad workspace")
    dwd, dbd = g.put(poisoned((cout, k, k, cin)), at_end=True, name="dw"), g.put(poisoned(cout), at_end=True, name="db")
    L.call("fcn_conv2d_wgrad_f32", C.byref(d), dwd.ptr, dbd.ptr, ws.ptr, None)
    dw, db = dwd.read((cout, k, k, cin)).transpose(0, 3, 1, 2), dbd.read((cout,))
    dw64, db64 = ref64.conv2d_wgrad(x, dy, k, p, 1)
    mw, mb = ref64.conv2d_wgrad(np.abs(x), np.abs(dy), k, p, 1)
    assert poison_free(dw) and poison_free(db)
    within(dw, dw64, ref64.dot_bound_rms(n * h * w, mw), "wgrad dw")
    within(db, db64, ref64.dot_bound_rms(n * h * w, mb), "wgrad db")


def test_weights_flip_batch_between_poisoned_gaps(g):
    """fcn_conv_weights_flip_batch_f32: three segments separated by poisoned gaps in both w_base and wt_base; the gaps are bit-identical
    afterwards, the pad channels of wt are zeros."""
    rng = np.random.default_rng(42)
    geo = [(36, 24, 3), (4, 5, 1), (33, 3, 7)]      # cout, cin, k
    segs = (L.FlipSeg * 3)()
    woff = toff = 3 * 4                              # gaps of 12 floats (48 bytes) in front, between and behind
    wts, wlive, tlive = [], [], []
    for i, (co, ci, k) in enumerate(geo):
        ci4, co4 = (ci + 3) // 4 * 4, (co + 3) // 4 * 4
        segs[i].w_offset, segs[i].wt_offset, segs[i].Cout, segs[i].kh, segs[i].kw, segs[i].Cin, segs[i].Cin4, segs[i].Cout4 = woff, toff, co, k, k, ci, ci4, co4
        wts.append(rng.standard_normal((co, ci, k, k)).astype(np.float32))
        wlive.append((woff, co * k * k * ci4))
        tlive.append((toff, ci * k * k * co4))
        woff += co * k * k * ci4 + 12
        toff += ci * k * k * co4 + 12
    wbase, tbase = poisoned(woff), poisoned(toff)
    for (o, cnt), wt, (co, ci, k) in zip(wlive, wts, geo):
        ci4 = (ci + 3) // 4 * 4
        packed = np.zeros((co, k, k, ci4), np.float32)
        packed[..., :ci] = wt.transpose(0, 2, 3, 1)
        wbase[o:o + cnt] = packed.ravel()
    wd, td = g.put(wbase, at_end=True, name="w_base"), g.put(tbase, at_end=True, name="wt_base")
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    L.call("fcn_conv_weights_flip_batch_f32", wd.ptr, td.ptr, sd.ptr, 3, None)
    got = td.read((toff,))
    gap = np.ones(toff, bool)
    for (o, cnt), wt, (co, ci, k) in zip(tlive, wts, geo):
        co4 = (co + 3) // 4 * 4
        seg = got[o:o + cnt].reshape(ci, k, k, co4)
        assert np.array_equal(seg[..., :co], wt[:, :, ::-1, ::-1].transpose(1, 2, 3, 0)) and np.all(seg[..., co:] == 0)
        gap[o:o + cnt] = False
    assert np.all(got.view(np.uint32)[gap] == poisoned(1).view(np.uint32)[0]), "a gap of wt_base was written"
    assert np.array_equal(wd.read((woff,)).view(np.uint32), wbase.view(np.uint32)), "w_base was written"
