"""Guard-banded, poisoned-buffer parity of the half-float rectangular and dilated convolution (fcn_rconv2d_prepare_f16 /
fcn_rconv2d_f16, csrc/rconv.hip) against the float64 reference (tests/ref_rconv64.py) evaluated on the operands after rounding to
half, -m gpu.  The twin of tests/test_gpu_guarded_rconv.py: every tensor lives in a guarded allocation placed at its end, x is a
channel window of wider pixels whose other halves (the pad channels Cin .. round8(Cin)-1 included) hold NaN, y is a slice of a
poison-filled buffer.  A case passes when the result meets ref64.dot_bound_f16 per element (ref64.dot_bound_rms where the result is
float32), carries no poison, the channels outside the slice and the red zones are bit-identical afterwards - the half that shares a
32-bit word with the slice's first or last half among them -, the inputs are unchanged and a second launch gives the same bits.
Every case runs under the built-in choice and under every configuration 0 .. fcn_rconv2d_num_configs_f16() - 1."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_rconv64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched
from test_gpu_guarded_rconv import GEOMETRIES, IDS, SQUARE_GEOMETRIES, rconv_desc, within

pytestmark = pytest.mark.gpu
F16 = np.float16


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def r8(c):
    return (c + 7) // 8 * 8


def configs():
    return [-1] + list(range(int(L.load().fcn_rconv2d_num_configs_f16())))


def halves(a):
    """float32 values that are halves: what the device holds, exactly."""
    return np.asarray(a, np.float32).astype(F16)


def pack_ohwi8(w):
    """(Cout, Cin, kh, kw) halves -> the bank [Cout][kh][kw][round8(Cin)] as the engine keeps it (pad columns zero)."""
    co, ci, kh, kw = w.shape
    out = np.zeros((co, kh, kw, r8(ci)), F16)
    out[..., :ci] = w.transpose(0, 2, 3, 1)
    return out


def launch(g, descs, cfg=-1, twice=None):
    """prepare + launch; with twice = (buffer, shape, dtype): a second launch of the same plan must give the same bits."""
    lib = L.load()
    n = len(descs)
    arr = (L.RConvDesc * n)(*descs)
    wsb = int(lib.fcn_rconv2d_workspace_bytes(arr, n))
    assert wsb > 0
    ws = g.put(wsb, name="workspace")
    plan = L.RConvPlan()
    L.call("fcn_rconv2d_prepare_f16", arr, n, ws.ptr, cfg, C.byref(plan))
    assert plan.n == n and plan.total_tiles > 0 and plan.cfg >= 256 and (cfg < 0 or plan.cfg == 256 + cfg)
    L.call("fcn_rconv2d_f16", C.byref(plan), None)
    L.call("fcn_device_sync")
    if twice is not None:
        buf, shape, dt = twice
        first = buf.read(shape, dt).view(np.uint16).copy()
        L.call("fcn_rconv2d_f16", C.byref(plan), None)
        L.call("fcn_device_sync")
        assert np.array_equal(first, buf.read(shape, dt).view(np.uint16)), "two launches on the same inputs differ"
    return plan


def allowance(K, mag, y64, out32):
    return ref64.dot_bound_rms(K, mag) if out32 else ref64.dot_bound_f16(K, mag, y64)


def run_fwd(g, seed, n, ci, co, h, w, k, s, pad, dil, relu=False, out32=False, xcs=None, xco=0, ycs=None, yco=0, bias=True, ref=None):
    """x: channels xco .. xco + ci - 1 of pixels of xcs halves (everything else NaN); y: channels yco .. of pixels of ycs elements.
    The reference is computed once and every configuration is held to it on fresh poisoned outputs."""
    rng = np.random.default_rng(seed)
    x = halves(rng.standard_normal((n, ci, h, w)))
    wt = halves(rng.standard_normal((co, ci) + tuple(k)) / np.sqrt(ci))
    b = rng.standard_normal(co).astype(np.float32) if bias else None
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
    xcs = xcs or r8(ci) + xco
    ycs = ycs or co + yco
    assert xco % 8 == 0 and xcs % 8 == 0 and xco + r8(ci) <= xcs and yco + co <= ycs
    x64, w64 = ref64.to_f16_then_f64(x), ref64.to_f16_then_f64(wt)
    y64 = R.conv2d(x64, w64, b, pad, s, dil) if ref is None else ref(x64, w64, b)
    mag = R.conv2d_mag(x64, w64, b, pad, s, dil)
    if relu:
        y64 = np.maximum(y64, 0)
    ydt, ysz = (np.float32, 4) if out32 else (F16, 2)
    xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=F16), at_end=True, name="x")
    wd = g.put(pack_ohwi8(wt), at_end=True, name="bank")
    bd = g.put(b, at_end=True, name="bias") if bias else None
    fl = (L.CONV_RELU if relu else 0) | (L.CONV_OUT_F32 if out32 else 0)
    for cfg in configs():
        yd = g.put(poisoned((n, oh, ow, ycs), dtype=ydt), at_end=True, name="y")
        d = rconv_desc(xd.ptr + 2 * xco, wd.ptr, bd.ptr if bias else None, yd.ptr, n, h, w, ci, xcs, co, k, pad, s, dil, oh, ow, ycs, yco, fl)
        launch(g, [d], cfg, twice=(yd, (n, oh, ow, ycs), ydt))
        full = yd.read((n, oh, ow, ycs), ydt)
        y = nchw(full, co, yco)
        what = "rconv f16 cfg%d k%dx%d d%d s%dx%d p%dx%d %dx%d %d->%d y%d+%d/%d%s%s" % (
            cfg, k[0], k[1], dil, s[0], s[1], pad[0], pad[1], h, w, ci, co, yco, co, ycs, " relu" if relu else "", " f32" if out32 else "")
        assert poison_free(y), "%s: poison (a pad channel, a neighbouring channel or a red zone) reached the result" % what
        within(y, y64, allowance(k[0] * k[1] * ci, mag, y64, out32), what)
        assert slice_untouched(full, yco, co), "%s: channels of y outside the slice were written" % what
        assert xd.unchanged() and wd.unchanged() and (bd is None or bd.unchanged()), "%s: an input was written" % what


@pytest.mark.parametrize("k,pad,s,dil,hw", GEOMETRIES, ids=IDS)
def test_forward_geometries(g, k, pad, s, dil, hw):
    """Cin 5 (three pad halves of NaN), Cout 7 (a scalar tail); then both as channel windows of wider pixels."""
    run_fwd(g, 7 * k[0] + k[1] + dil, 1, 5, 7, hw[0], hw[1], k, s, pad, dil)
    run_fwd(g, 9 * k[0] + k[1] + dil, 1, 5, 7, hw[0], hw[1], k, s, pad, dil, xcs=16, xco=8, ycs=24, yco=8)


@pytest.mark.parametrize("k,dil,pad,s,hw", SQUARE_GEOMETRIES)
def test_square_dilated_forward_geometries(g, k, dil, pad, s, hw):
    """The far taps of d12 lie in the padding for most pixels."""
    run_fwd(g, 7 * k + dil, 1, 5, 7, hw[0], hw[1], (k, k), (s, s), (pad, pad), dil)
    run_fwd(g, 9 * k + dil, 1, 5, 7, hw[0], hw[1], (k, k), (s, s), (pad, pad), dil, xcs=16, xco=8, ycs=24, yco=8)


def test_equal_axes_with_dilation_one_equal_the_dense_convolution(g):
    run_fwd(g, 1, 2, 5, 7, 7, 9, (3, 3), (1, 1), (1, 1), 1, ref=lambda x, w, b: ref64.conv2d(x, w, b, 1, 1))
    run_fwd(g, 2, 1, 4, 8, 9, 8, (3, 3), (2, 2), (0, 0), 1, ref=lambda x, w, b: ref64.conv2d(x, w, b, 0, 2))


@pytest.mark.parametrize("relu", [False, True])
def test_tile_crosses_a_row_end_and_the_image_boundary(g, relu):
    """N = 2 on 9 x 11: 99 pixels per image, so the second 64-pixel tile holds the end of image 0 and the start of image 1."""
    run_fwd(g, 3, 2, 5, 7, 9, 11, (1, 7), (1, 1), (0, 3), 1, relu=relu)
    run_fwd(g, 4, 2, 8, 4, 9, 11, (7, 1), (1, 1), (3, 0), 1, relu=relu)


@pytest.mark.parametrize("ci,co", [(1, 1), (33, 65), (40, 7), (72, 40), (130, 70)])
def test_channel_counts_across_tiles_and_chunks(g, ci, co):
    """1 channel; one channel into a second 32-channel chunk and one into a second 64-channel block; whole 16-byte segments that end
    inside a chunk; several chunks and blocks."""
    run_fwd(g, ci + co, 2, ci, co, 9, 11, (1, 7), (1, 1), (0, 3), 1)
    run_fwd(g, ci * co, 1, ci, co, 5, 6, (3, 3), (1, 1), (4, 4), 4, relu=True)


@pytest.mark.parametrize("ycs,yco,out32", [(24, 8, False), (20, 4, False), (13, 3, False), (16, 4, True), (12, 1, True)],
                         ids=["16-byte-runs", "8-byte-runs", "2-byte-stores", "f32-at-4", "f32-at-1"])
def test_store_forms(g, ycs, yco, out32):
    """Cout 10: two whole runs of four and a tail of two.  At yco 3 of 13 every pixel's slice starts and ends inside a 32-bit word
    whose other half must stay poison."""
    run_fwd(g, 5 + yco, 2, 6, 10, 7, 9, (1, 7), (1, 1), (0, 3), 1, out32=out32, xcs=16, xco=8, ycs=ycs, yco=yco)
    run_fwd(g, 6 + yco, 1, 6, 10, 7, 9, (3, 3), (1, 1), (2, 2), 2, relu=True, out32=out32, ycs=ycs, yco=yco)


@pytest.mark.parametrize("out32", [False, True])
def test_without_bias(g, out32):
    run_fwd(g, 8, 1, 4, 3, 5, 4, (3, 1), (1, 1), (1, 0), 1, out32=out32, ycs=8, yco=4, bias=False)
    run_fwd(g, 9, 1, 9, 12, 6, 5, (3, 3), (1, 1), (2, 2), 2, out32=out32, bias=False)


def shared_launch(g, x, problems, n_expected):
    """`problems`: (k, pad, s, dil, co) reading the one blob x in one launch; every result a slice at channel 8 of its own buffer."""
    rng = np.random.default_rng(9)
    n, ci, h, w = x.shape
    xd = g.put(poisoned_nhwc(x, r8(ci), 0, dtype=F16), at_end=True, name="x")
    x64 = ref64.to_f16_then_f64(x)
    banks = []
    for k, pad, s, dil, co in problems:
        wt = halves(rng.standard_normal((co, ci) + k) / np.sqrt(ci))
        b = rng.standard_normal(co).astype(np.float32)
        banks.append((wt, b, g.put(pack_ohwi8(wt), at_end=True), g.put(b, at_end=True)))
    for cfg in configs():
        descs, outs = [], []
        for (k, pad, s, dil, co), (wt, b, wd, bd) in zip(problems, banks):
            ycs = co + 8 + 3
            oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
            yd = g.put(poisoned((n, oh, ow, ycs), dtype=F16), at_end=True)
            descs.append(rconv_desc(xd.ptr, wd.ptr, bd.ptr, yd.ptr, n, h, w, ci, r8(ci), co, k, pad, s, dil, oh, ow, ycs, 8))
            outs.append((yd, ycs, oh, ow))
        plan = launch(g, descs, cfg)
        assert plan.n == n_expected and plan.grid_y == 1
        for (k, pad, s, dil, co), (wt, b, _wd, _bd), (yd, ycs, oh, ow) in zip(problems, banks, outs):
            full = yd.read((n, oh, ow, ycs), F16)
            y = nchw(full, co, 8)
            assert poison_free(y) and slice_untouched(full, 8, co)
            w64 = ref64.to_f16_then_f64(wt)
            y64 = R.conv2d(x64, w64, b, pad, s, dil)
            within(y, y64, ref64.dot_bound_f16(k[0] * k[1] * ci, R.conv2d_mag(x64, w64, b, pad, s, dil), y64), "shared k%dx%d d%d" % (k + (dil,)))
    assert xd.unchanged()


def test_four_dilations_of_one_input_in_one_launch(g):
    """The ASPP head: four problems read the same 17 x 19 blob with dilations 2, 4, 6, 8 (pad == dilation) in one launch."""
    x = halves(np.random.default_rng(10).standard_normal((1, 6, 17, 19)))
    shared_launch(g, x, [((3, 3), (d, d), (1, 1), d, co) for d, co in zip((2, 4, 6, 8), (7, 70, 4, 9))], 4)


def test_two_geometries_of_one_input_in_one_launch(g):
    """The 8-grid module of Inception-v3: a 1x3 and a 3x1 problem read one blob in one launch - and a strided 3x5 one with them, so that
    the problems of the plan differ in their pixel counts too."""
    x = halves(np.random.default_rng(11).standard_normal((2, 6, 8, 7)))
    shared_launch(g, x, [((1, 3), (0, 1), (1, 1), 1, 7), ((3, 1), (1, 0), (1, 1), 1, 70), ((3, 5), (0, 2), (2, 1), 1, 9)], 3)
