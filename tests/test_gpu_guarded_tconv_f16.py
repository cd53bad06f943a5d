"""Guard-banded, poisoned-buffer parity of the half-float transposed convolution (fcn_tconv2d_prepare_f16 / fcn_tconv2d_f16,
csrc/tconv.hip), of its bank packing (fcn_tconv_bank_pack_f16) and of the converting crop (fcn_crop_fwd_f16_f32, csrc/crop.hip)
against the float64 scatter reference (tests/ref_tconv64.py) evaluated on the operands after rounding to half, -m gpu.  The twin of
tests/test_gpu_guarded_tconv.py with the harness of tests/test_gpu_guarded_rconv_f16.py: every tensor lives in a guarded allocation
placed at its end, `a` is a channel window of wider pixels whose other halves (the pad channels Ca .. round8(Ca)-1 included) hold NaN,
`b` is a slice of a poison-filled buffer.  A case passes when the result meets ref64.dot_bound_f16 per element (ref64.dot_bound_rms
where the result is float32) with K = taps per output pixel x Ca, carries no poison, the channels outside the slice and the red zones
are bit-identical afterwards - the half that shares a 32-bit word with the slice's first or last half among them -, the inputs are
unchanged and a second launch gives the same bits.  Every case runs under the built-in choice and under every configuration
0 .. fcn_tconv2d_num_configs_f16() - 1."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_tconv64 as T
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched
from test_gpu_guarded_tconv import within

pytestmark = pytest.mark.gpu
F16 = np.float16
CFG_F16 = 256      # FCN_TCONV_CFG_F16


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def r8(c):
    return (c + 7) // 8 * 8


def configs():
    return [-1] + list(range(int(L.load().fcn_tconv2d_num_configs_f16())))


def halves(a):
    """float32 values that are halves: what the device holds, exactly."""
    return np.asarray(a, np.float32).astype(F16)


def device_blob8(w):
    """(Ca, Cb, kh, kw) halves -> [Ca][kh][kw][round8(Cb)]: a group-1 Deconvolution blob as a half-float engine keeps it."""
    ca, cb, kh, kw = w.shape
    out = np.zeros((ca, kh, kw, r8(cb)), F16)
    out[..., :cb] = w.transpose(0, 2, 3, 1)
    return out


def pack_bank8(w):
    """The host statement of fcn_tconv_bank_pack_f16: [kh][kw][Cb][round8(Ca)], pad columns zero."""
    ca, cb, kh, kw = w.shape
    out = np.zeros((kh, kw, cb, r8(ca)), F16)
    out[..., :ca] = w.transpose(2, 3, 1, 0)
    return out


def packed_bank(g, w):
    """The kernel's bank, packed ON THE DEVICE from the engine's blob layout and held to the host statement bit for bit."""
    ca, cb, kh, kw = w.shape
    src = g.put(device_blob8(w), at_end=True, name="blob")
    n = int(L.load().fcn_tconv_bank_halves(ca, cb, kh, kw))
    assert n == kh * kw * cb * r8(ca)
    dst = g.put(n * 2, name="bank")
    L.call("fcn_tconv_bank_pack_f16", src.ptr, dst.ptr, ca, cb, r8(cb), kh, kw, None)
    L.call("fcn_device_sync")
    assert np.array_equal(dst.read((kh, kw, cb, r8(ca)), F16).view(np.uint16), pack_bank8(w).view(np.uint16)), "bank packing differs from the host statement"
    assert src.unchanged()
    return dst


def bank_intact(wd, w):
    """The packed bank (written once by the packing launch, so not `unchanged()` against its poison) still holds the host statement,
    and its red zones their pattern."""
    ca, cb, kh, kw = w.shape
    return wd.modified() is None and np.array_equal(wd.read((kh, kw, cb, r8(ca)), F16).view(np.uint16), pack_bank8(w).view(np.uint16))


def tconv_desc(a_ptr, w_ptr, b_ptr, y_ptr, n, h, w, ca, acs, cb, kh, kw, pad, s, oh, ow, bcs, bco, flags=0):
    d = L.TConvDesc()
    d.a, d.w, d.bias, d.b, d.y2 = a_ptr, w_ptr, b_ptr, y_ptr, None
    d.N, d.H, d.W, d.Ca, d.a_cstride = n, h, w, ca, acs
    d.Cb, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = cb, kh, kw, pad, s, oh, ow
    d.b_cstride, d.b_coffset, d.y2_cstride, d.y2_coffset, d.flags = bcs, bco, 0, 0, flags
    return d


def launch(g, descs, cfg=-1, twice=None):
    """prepare + launch; with twice = (buffer, shape, dtype): a second launch of the same plan must give the same bits."""
    lib = L.load()
    n = len(descs)
    arr = (L.TConvDesc * n)(*descs)
    wsb = int(lib.fcn_tconv2d_workspace_bytes(arr, n))
    assert wsb > 0
    ws = g.put(wsb, name="workspace")
    plan = L.TConvPlan()
    L.call("fcn_tconv2d_prepare_f16", arr, n, ws.ptr, cfg, C.byref(plan))
    assert plan.n == n and plan.total_tiles > 0 and plan.cfg >= CFG_F16 and (cfg < 0 or plan.cfg == CFG_F16 + cfg)
    L.call("fcn_tconv2d_f16", C.byref(plan), None)
    L.call("fcn_device_sync")
    if twice is not None:
        buf, shape, dt = twice
        first = buf.read(shape, dt).view(np.uint16).copy()
        L.call("fcn_tconv2d_f16", C.byref(plan), None)
        L.call("fcn_device_sync")
        assert np.array_equal(first, buf.read(shape, dt).view(np.uint16)), "two launches on the same inputs differ"
    return plan


def allowance(K, mag, y64, out32):
    return ref64.dot_bound_rms(K, mag) if out32 else ref64.dot_bound_f16(K, mag, y64)


def run_case(g, seed, n, ca, cb, h, w, kh, kw, s, pad, extra=(0, 0), relu=False, out32=False, acs=None, aco=0, bcs=None, bco=0, bias=True):
    """a: channels aco .. aco + ca - 1 of pixels of acs halves (everything else NaN); b: channels bco .. of pixels of bcs elements.
    The reference is computed once and every configuration is held to it on fresh poisoned outputs."""
    rng = np.random.default_rng(seed)
    a = halves(rng.standard_normal((n, ca, h, w)))
    wt = halves(rng.standard_normal((ca, cb, kh, kw)) / np.sqrt(ca))
    b = rng.standard_normal(cb).astype(np.float32) if bias else None
    oh, ow = T.out_size(h, kh, s, pad) + extra[0], T.out_size(w, kw, s, pad) + extra[1]
    acs = acs or r8(ca) + aco
    bcs = bcs or cb + bco
    assert aco % 8 == 0 and acs % 8 == 0 and aco + r8(ca) <= acs and bco + cb <= bcs
    a64, w64 = ref64.to_f16_then_f64(a), ref64.to_f16_then_f64(wt)
    y64, mag = T.tconv2d(a64, w64, b, pad, s, (oh, ow)), T.tconv2d_mag(a64, w64, b, pad, s, (oh, ow))
    if relu:
        y64 = np.maximum(y64, 0)
    ydt = np.float32 if out32 else F16
    ad = g.put(poisoned_nhwc(a, acs, aco, dtype=F16), at_end=True, name="a")
    wd = packed_bank(g, wt)
    bd = g.put(b, at_end=True, name="bias") if bias else None
    fl = (L.CONV_RELU if relu else 0) | (L.CONV_OUT_F32 if out32 else 0)
    taps = -(-kh // s) * -(-kw // s)
    y = None
    for cfg in configs():
        yd = g.put(poisoned((n, oh, ow, bcs), dtype=ydt), at_end=True, name="b")
        d = tconv_desc(ad.ptr + 2 * aco, wd.ptr, bd.ptr if bias else None, yd.ptr, n, h, w, ca, acs, cb, kh, kw, pad, s, oh, ow, bcs, bco, fl)
        launch(g, [d], cfg, twice=(yd, (n, oh, ow, bcs), ydt))
        full = yd.read((n, oh, ow, bcs), ydt)
        y = nchw(full, cb, bco)
        what = "tconv f16 cfg%d k%dx%d s%d p%d %dx%d %d->%d b%d+%d/%d%s%s" % (
            cfg, kh, kw, s, pad, h, w, ca, cb, bco, cb, bcs, " relu" if relu else "", " f32" if out32 else "")
        assert poison_free(y), "%s: poison (a pad channel, a neighbouring channel or a red zone) reached the result" % what
        within(y, y64, allowance(taps * ca, mag, y64, out32), what)
        assert slice_untouched(full, bco, cb), "%s: channels of b outside the slice were written" % what
        assert ad.unchanged() and bank_intact(wd, wt) and (bd is None or bd.unchanged()), "%s: an input was written" % what
    return y, y64, b


# k, stride: the shape list of the issue; (2, 4) has phases without a tap
KS = [(1, 2), (2, 2), (3, 2), (4, 2), (16, 8), (32, 16), (64, 32), (2, 4)]


@pytest.mark.parametrize("k,s", KS)
def test_shape_list_every_pad_class(g, k, s):
    """N = 2, Ca 5 (three pad halves of NaN), Cb 7 (a scalar tail); pads 0, k // 2, k - 1 (a pad that leaves no output on the input's
    shorter side has no problem to run: k64 s32 p63 on 2 rows); then the largest legal output size, `a` a window at channel 8 of pixels
    of 16 halves and `b` a slice at channel 8 of pixels of 24."""
    h, w = (2, 3) if k >= 64 else (3, 5) if k >= 16 else (7, 9)
    ran = 0
    for i, pad in enumerate(sorted({0, k // 2, k - 1})):
        if T.out_size(h, k, s, pad) <= 0:
            continue
        run_case(g, 10 * k + s + i, 2, 5, 7, h, w, k, k, s, pad)
        run_case(g, 11 * k + s + i, 2, 5, 7, h, w, k, k, s, pad, extra=(s - 1, s - 1), acs=16, aco=8, bcs=24, bco=8)
        ran += 1
    assert ran >= min(2, len({0, k // 2, k - 1}))


def test_phases_without_a_tap_are_the_bias_alone(g):
    """k2 s4 p0: the outputs with (oy mod 4, ox mod 4) outside [0, 2) x [0, 2) lie under no tap."""
    y, _, b = run_case(g, 3, 1, 5, 7, 4, 3, 2, 2, 4, 0)
    want = b.astype(F16).astype(np.float32)[None, :, None, None]
    assert np.array_equal(y[:, :, 2::4, :], np.broadcast_to(want, y[:, :, 2::4, :].shape))
    assert np.array_equal(y[:, :, :, 3::4], np.broadcast_to(want, y[:, :, :, 3::4].shape))


@pytest.mark.parametrize("out32", [False, True], ids=["halves", "f32"])
@pytest.mark.parametrize("cb,bcs,bco", [(8, 24, 8), (4, 12, 4), (3, 7, 1)], ids=["16-byte-runs", "8-byte-runs", "2-byte-stores"])
def test_store_forms(g, cb, bcs, bco, out32):
    """At offset 1 of 7 every pixel's slice starts and ends inside a 32-bit word whose other half must stay poison."""
    run_case(g, 5 + bco, 2, 6, cb, 5, 7, 4, 4, 2, 1, out32=out32, acs=16, aco=8, bcs=bcs, bco=bco)
    run_case(g, 6 + bco, 1, 6, cb, 3, 4, 3, 3, 2, 0, relu=True, out32=out32, bcs=bcs, bco=bco)


@pytest.mark.parametrize("ca,cb", [(1, 1), (2, 3), (33, 65), (72, 40), (21, 21)])
def test_channel_counts_across_tiles_and_chunks(g, ca, cb):
    """1 channel; one channel into a second 32-channel chunk and one into a second 64-channel block (a third 32-channel one); whole
    16-byte segments that end inside a chunk; the score layers' 21.  9 x 11 at k3 s2 p1 with N = 2: 198 lattice pixels in the largest
    phase, so a tile of either configuration holds the end of image 0 and the start of image 1."""
    run_case(g, ca + cb, 2, ca, cb, 9, 11, 3, 3, 2, 1)


def test_rectangular_kernels(g):
    run_case(g, 1, 2, 5, 6, 5, 7, 3, 5, 2, 1)
    run_case(g, 2, 1, 4, 4, 6, 5, 4, 2, 2, 0, extra=(1, 1), relu=True)
    run_case(g, 3, 1, 4, 8, 4, 5, 1, 3, 3, 0)


def test_stride_one_equals_the_flipped_correlation(g):
    """One phase, every tap: the dense correlation with the flipped, transposed bank (that the scatter reference is that correlation
    at stride 1 is asserted on the host first)."""
    rng = np.random.default_rng(5)
    a, wt = rng.standard_normal((1, 4, 6, 7)), rng.standard_normal((4, 3, 3, 3))
    flipped = wt[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)
    assert np.allclose(T.tconv2d(a, wt, None, 1, 1), ref64.conv2d(a, flipped, None, 1, 1), rtol=1e-12, atol=1e-12)
    y, _, _ = run_case(g, 4, 1, 8, 8, 6, 7, 3, 3, 1, 1)
    assert y.shape == (1, 8, 6, 7)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("relu,out32", [(True, False), (False, True), (True, True)], ids=["relu", "f32", "relu+f32"])
def test_epilogue_flags(g, relu, out32, bias):
    run_case(g, 7, 2, 6, 10, 5, 7, 4, 4, 2, 1, extra=(1, 0), relu=relu, out32=out32, acs=16, aco=8, bcs=24, bco=8, bias=bias)
    run_case(g, 8, 1, 4, 3, 5, 4, 2, 2, 4, 0, relu=relu, out32=out32, bcs=8, bco=4, bias=bias)


def test_several_problems_in_one_launch(g):
    """Problems of different stride, size and Cb in one plan, two with Cb <= 32 and one above: grid rows / columns past a smaller
    problem's phases and tiles return, and one configuration serves them all."""
    rng = np.random.default_rng(9)
    specs = [(2, 5, 7, 7, 9, 3, 2, 1), (1, 8, 4, 3, 4, 16, 8, 4), (1, 3, 70, 5, 5, 2, 4, 0)]
    ins = []
    for n, ca, cb, h, w, k, s, pad in specs:
        a = halves(rng.standard_normal((n, ca, h, w)))
        wt = halves(rng.standard_normal((ca, cb, k, k)) / np.sqrt(ca))
        b = rng.standard_normal(cb).astype(np.float32)
        ins.append((a, wt, b, g.put(poisoned_nhwc(a, r8(ca), 0, dtype=F16), at_end=True), packed_bank(g, wt), g.put(b, at_end=True)))
    for cfg in configs():
        descs, outs = [], []
        for (n, ca, cb, h, w, k, s, pad), (a, wt, b, ad, wd, bd) in zip(specs, ins):
            oh, ow = T.out_size(h, k, s, pad), T.out_size(w, k, s, pad)
            bcs = cb + 8 + 3
            yd = g.put(poisoned((n, oh, ow, bcs), dtype=F16), at_end=True)
            descs.append(tconv_desc(ad.ptr, wd.ptr, bd.ptr, yd.ptr, n, h, w, ca, r8(ca), cb, k, k, pad, s, oh, ow, bcs, 8))
            outs.append((yd, (n, oh, ow, bcs)))
        plan = launch(g, descs, cfg)
        assert plan.grid_y == 64 and (cfg >= 0 or plan.cfg == CFG_F16)      # (a problem above 32 channels: the square tile)
        for (n, ca, cb, h, w, k, s, pad), (a, wt, b, ad, wd, bd), (yd, shape) in zip(specs, ins, outs):
            full = yd.read(shape, F16)
            y = nchw(full, cb, 8)
            assert poison_free(y) and slice_untouched(full, 8, cb)
            a64, w64 = ref64.to_f16_then_f64(a), ref64.to_f16_then_f64(wt)
            y64 = T.tconv2d(a64, w64, b, pad, s)
            taps = (-(-k // s)) ** 2
            within(y, y64, ref64.dot_bound_f16(taps * ca, T.tconv2d_mag(a64, w64, b, pad, s), y64), "grouped tconv f16 cfg%d" % cfg)
            assert ad.unchanged() and bank_intact(wd, wt) and bd.unchanged()


def test_the_built_in_choice_takes_the_narrow_tile_up_to_32_channels(g):
    lib = L.load()
    ws = g.put(int(lib.fcn_tconv2d_workspace_bytes(None, 1)), name="workspace")
    a, wt, y = g.put(poisoned((1, 2, 2, 8), dtype=F16)), g.put(1 * 40 * 8 * 2), g.put(poisoned((1, 2, 2, 40), dtype=F16))
    for cb, want in ((21, 1), (32, 1), (33, 0)):
        plan = L.TConvPlan()
        d = tconv_desc(a.ptr, wt.ptr, None, y.ptr, 1, 2, 2, 5, 8, cb, 1, 1, 0, 1, 2, 2, 40, 0)
        L.call("fcn_tconv2d_prepare_f16", C.byref(d), 1, ws.ptr, -1, C.byref(plan))
        assert plan.cfg == CFG_F16 + want


@pytest.mark.parametrize("ca,cb,kh,kw", [(5, 7, 4, 4), (1, 1, 1, 1), (21, 21, 16, 16), (9, 33, 3, 5), (16, 8, 2, 2)])
def test_bank_packing_bit_for_bit(g, ca, cb, kh, kw):
    """Ca / Cb off 8 (and on it): every pad column of the packed bank is a zero, every other half the blob's, moved."""
    wt = halves(np.random.default_rng(ca * cb).standard_normal((ca, cb, kh, kw)))
    packed_bank(g, wt)
    # the blob as a window of wider rows: w_cstride above round8(Cb), the halves behind Cb poison
    src = np.full((ca, kh, kw, r8(cb) + 8), np.nan, F16)
    src[..., :cb] = wt.transpose(0, 2, 3, 1)
    sd = g.put(src, at_end=True, name="wide blob")
    dst = g.put(kh * kw * cb * r8(ca) * 2, name="bank")
    L.call("fcn_tconv_bank_pack_f16", sd.ptr, dst.ptr, ca, cb, r8(cb) + 8, kh, kw, None)
    L.call("fcn_device_sync")
    assert np.array_equal(dst.read((kh, kw, cb, r8(ca)), F16).view(np.uint16), pack_bank8(wt).view(np.uint16))


@pytest.mark.parametrize("c,xcs,xco,ycs,yco,oy,ox", [(21, 24, 0, 24, 0, 3, 5), (5, 16, 8, 8, 0, 1, 2), (7, 16, 3, 12, 1, 0, 3), (13, 24, 8, 20, 4, 2, 0),
                                                     (3, 8, 5, 4, 1, 1, 1)])
def test_crop_to_float32_is_exact(g, c, xcs, xco, ycs, yco, oy, ox):
    """Windows at odd offsets, C off 8, y a slice of wider float32 pixels: conversion from half to float32 is exact, so every element
    of the window equals its source bit for bit, nothing outside the slice is written and x stays as it was."""
    n, h, w, oh, ow = 2, 9, 11, 5, 6
    x = halves(np.random.default_rng(c + xco).standard_normal((n, c, h, w)))
    xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=F16), at_end=True, name="x")
    yd = g.put(poisoned((n, oh, ow, ycs)), at_end=True, name="y")
    for _ in range(2):
        L.call("fcn_crop_fwd_f16_f32", xd.ptr, yd.ptr, n, h, w, c, xcs, xco, oy, ox, oh, ow, ycs, yco, None)
        L.call("fcn_device_sync")
    full = yd.read((n, oh, ow, ycs))
    y = nchw(full, c, yco)
    assert poison_free(y) and slice_untouched(full, yco, c) and xd.unchanged()
    assert np.array_equal(y, x[:, :, oy:oy + oh, ox:ox + ow].astype(np.float32))
