"""Guard-banded, poisoned-buffer parity of the half-float depthwise forward (fcn_dwconv2d_fwd_f16) against the float64 reference
computed from the f16-rounded input, -m gpu.  The harness of tests/test_gpu_guarded_dwconv.py with halves: 8 channels per lane, a
float32 bank of round8(C) channels per tap and a float32 bias, float32 accumulation, y as halves or as float32 (FCN_CONV_OUT_F32).
The bound is the one tests/test_gpu_guarded_f16.py uses for a sum of that length: ref64.dot_bound_f16(kh*kw, magnitude, y64)."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_dwconv64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched
from test_gpu_guarded_dwconv import E_UNSUPPORTED, GEOMETRIES, IDS, configs, dw_desc, g, launch, strip_takes, within      # noqa: F401 (g: the fixture)

pytestmark = pytest.mark.gpu


def r8(c):
    return (c + 7) // 8 * 8


def run_f16(g, seed, n, c, h, w, k, s, pad, dil, relu=False, out_f32=False, xcs=None, xco=0, ycs=None, yco=0, bias=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c, h, w)).astype(np.float16)
    wt = (rng.standard_normal((c, 1) + tuple(k)) / np.sqrt(k[0] * k[1])).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32) if bias else None
    oh, ow = R.out_hw(h, w, k[0], k[1], pad, s, dil)
    xcs, ycs = xcs or r8(c) + xco, ycs or r8(c) + yco
    assert xco % 8 == 0 and xco + r8(c) <= xcs and xcs % 8 == 0 and yco + c <= ycs
    x64 = x.astype(np.float64)
    y64, mag = R.conv2d(x64, wt, b, pad, s, dil), R.conv2d_mag(x64, wt, b, pad, s, dil)
    if relu:
        y64 = np.maximum(y64, 0)
    ydt = np.float32 if out_f32 else np.float16
    xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=np.float16), at_end=True, name="x")
    wd = g.put(R.pack_bank(wt, 8), at_end=True, name="bank")
    bd = g.put(b, at_end=True, name="bias") if bias else None
    fl = (L.CONV_RELU if relu else 0) | (L.CONV_OUT_F32 if out_f32 else 0)
    for cfg in configs():
        y0 = poisoned((n, oh, ow, ycs), dtype=ydt)
        yd = g.put(y0, at_end=True, name="y")
        d = dw_desc(xd.ptr + 2 * xco, wd.ptr, bd.ptr if bias else None, yd.ptr, n, h, w, c, xcs, k, pad, s, dil, ycs, yco, fl)
        what = "dwconv f16 cfg%d k%dx%d d%d s%dx%d p%dx%d %dx%dx%d c%d%s%s" % (cfg, k[0], k[1], dil, s[0], s[1], pad[0], pad[1], n, h, w, c,
                                                                              " RELU" if relu else "", " OUT_F32" if out_f32 else "")
        if cfg == 1 and not strip_takes(k, s, dil):
            assert L.load().fcn_dwconv2d_fwd_f16(C.byref(d), cfg, None) == E_UNSUPPORTED, what
            assert np.array_equal(yd.read((n, oh, ow, ycs), ydt).view(np.uint8), y0.view(np.uint8)), "%s: a refused call wrote y" % what
            continue
        launch("fcn_dwconv2d_fwd_f16", d, cfg, yd, (n, oh, ow, ycs), ydt)
        full = yd.read((n, oh, ow, ycs), ydt)
        y = nchw(full, c, yco)
        assert poison_free(y), "%s: poison (a pad channel, a neighbouring channel or a red zone) reached the result" % what
        within(y, y64, ref64.dot_bound_f16(k[0] * k[1], mag, y64), what)
        assert slice_untouched(full, yco, c), "%s: channels of y outside the slice were written" % what
        assert xd.unchanged() and wd.unchanged(), "%s: an input was written" % what


@pytest.mark.parametrize("k,pad,s,dil,hw", GEOMETRIES, ids=IDS)
def test_half_forward_geometries(g, k, pad, s, dil, hw):
    """C 6 (a partial segment of eight: two pad channels of NaN, a scalar tail); then C 20 as a channel window of wider pixels, ReLU."""
    run_f16(g, 7 * k[0] + k[1] + dil, 1, 6, hw[0], hw[1], k, s, pad, dil)
    run_f16(g, 9 * k[0] + k[1] + dil, 1, 20, hw[0], hw[1], k, s, pad, dil, relu=True, xcs=40, xco=8, ycs=40, yco=8)


def test_half_forward_channels_outputs_and_block_boundaries(g):
    """C 8: one whole segment; float32 output, whole and as an unaligned slice; halves at channel offset 2 (scalar stores); N = 2 on
    9 x 11 with C 40 (a block of lanes holds the end of one image and the start of the next); W = 13 (a tail strip); no bias."""
    run_f16(g, 1, 1, 8, 7, 9, (3, 3), (1, 1), (1, 1), 1)
    run_f16(g, 2, 1, 8, 7, 9, (3, 3), (2, 2), (1, 1), 1, out_f32=True, relu=True)
    run_f16(g, 3, 1, 12, 7, 9, (3, 3), (1, 1), (1, 1), 1, out_f32=True, ycs=20, yco=4)
    run_f16(g, 4, 1, 6, 7, 9, (3, 3), (1, 1), (1, 1), 1, out_f32=True, ycs=9, yco=2)
    run_f16(g, 5, 1, 8, 7, 9, (3, 3), (1, 1), (1, 1), 1, ycs=12, yco=2, relu=True)
    run_f16(g, 6, 2, 40, 9, 11, (3, 3), (2, 2), (1, 1), 1, relu=True)
    run_f16(g, 7, 2, 6, 5, 13, (3, 3), (1, 1), (1, 1), 1, bias=False)
    run_f16(g, 8, 1, 6, 5, 13, (5, 5), (2, 2), (2, 2), 1, bias=False, out_f32=True)
