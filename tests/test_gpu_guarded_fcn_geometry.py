"""Geometry the published FCN nets bring with them, guard-banded against the float64 reference (-m gpu): conv1_1's pad far above
its kernel size (k3 / pad 100 / stride 1) through EVERY tile configuration - each either meets the float32 bound or is refused by
prepare with FCN_E_UNSUPPORTED, which is what makes the tuner skip it - forward and weight gradient; and 2 x 2 / stride 2 MAX
pooling over odd extents (Caffe's ceil rule: the last window is clipped), forward with argmax and backward."""
import ctypes as C

import numpy as np
import pytest

import ref64
from conftest import N_TILE_CFGS
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, conv_desc, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched
from test_gpu_guarded import ohwi, within

pytestmark = pytest.mark.gpu
E_UNSUPPORTED = 3


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


# cin, cout, h, w, n, x_cstride, x channel offset, y_cstride, y channel offset - all k3 / pad 100 / stride 1
PAD100 = [(3, 8, 6, 5, 1, 4, 0, 8, 0),          # the image of conv1_1: three channels in a pixel of four, almost every tile wholly in the pad band
          (4, 36, 3, 7, 2, 12, 4, 40, 4)]       # a slice of a wider pixel, batch 2, Cout beyond one 32-wide tile


@pytest.mark.parametrize("cfg", [-1] + list(range(N_TILE_CFGS)))
@pytest.mark.parametrize("case", PAD100)
def test_pad_far_above_the_kernel_forward(g, case, cfg):
    cin, cout, h, w, n, xcs, xo, ycs, yo = case
    k, s, p = 3, 1, 100
    rng = np.random.default_rng(PAD100.index(case))
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    oh, ow = ref64.conv_out(h, k, p, s), ref64.conv_out(w, k, p, s)
    cin4 = (cin + 3) // 4 * 4
    w4 = np.zeros((cout, k, k, cin4), np.float32)
    w4[..., :cin] = ohwi(wt)
    xd = g.put(poisoned_nhwc(x, xcs, xo) if cin == cin4 else np.ascontiguousarray(np.pad(x.transpose(0, 2, 3, 1), ((0, 0),) * 3 + ((0, cin4 - cin),))),
               at_end=True, name="x")
    wd, bd = g.put(w4, name="w"), g.put(b, name="bias")
    yd = g.put(poisoned((n, oh, ow, ycs)), name="y")
    d = conv_desc(xd, wd, bd, yd, n, h, w, cin4, xcs, cout, k, p, s, oh, ow, ycs, yo)
    d.x = xd.ptr + 4 * xo
    lib = L.load()
    ws = g.put(int(lib.fcn_conv2d_group_workspace_bytes(1)), name="workspace")
    grp = L.ConvGroup()
    rc = lib.fcn_conv2d_group_prepare(C.byref(d), 1, ws.ptr, cfg, C.byref(grp))
    if rc == E_UNSUPPORTED and cfg >= 0:
        print("REFUSED cfg %d: %s" % (cfg, lib.fcn_last_error_string().decode()))
        return
    L.check(rc)
    L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), None)
    L.call("fcn_device_sync")
    L.call("fcn_conv2d_group_release", ws.ptr)
    full = yd.read((n, oh, ow, ycs))
    y = nchw(full, cout, yo)
    y64, mag = ref64.conv2d(x, wt, b, p, s), ref64.conv2d_mag(x, wt, b, p, s)
    assert poison_free(y), "cfg %d: poison reached the result" % cfg
    within(y, y64, ref64.dot_bound_rms(cin * k * k, mag), "pad 100 conv cfg %d" % cfg)
    assert slice_untouched(full, yo, cout)
    # far from the image the output is the bias, exactly
    assert np.array_equal(y[:, :, :90, :], np.broadcast_to(b[None, :, None, None], y[:, :, :90, :].shape))


@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])
@pytest.mark.parametrize("case", PAD100)
def test_pad_far_above_the_kernel_weight_gradient(g, case, cfg):
    cin, cout, h, w, n, xcs, xo, dcs, dyo = case
    k, s, p = 3, 1, 100
    lib = L.load()
    if cfg >= int(lib.fcn_conv2d_wgrad_num_configs()):
        pytest.fail("the library has fewer weight-gradient configurations than this test walks")
    rng = np.random.default_rng(10 + PAD100.index(case))
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    oh, ow = ref64.conv_out(h, k, p, s), ref64.conv_out(w, k, p, s)
    dy = rng.standard_normal((n, cout, oh, ow)).astype(np.float32)
    cin4 = (cin + 3) // 4 * 4
    xd = g.put(poisoned_nhwc(x, xcs, xo) if cin == cin4 else np.ascontiguousarray(np.pad(x.transpose(0, 2, 3, 1), ((0, 0),) * 3 + ((0, cin4 - cin),))),
               at_end=True, name="x")
    dyd = g.put(poisoned_nhwc(dy, dcs, dyo), at_end=True, name="dY")
    d = conv_desc(xd, xd, None, dyd, n, h, w, cin4, xcs, cout, k, p, s, oh, ow, dcs, dyo)
    d.x = xd.ptr + 4 * xo
    splits = C.c_int(0)
    nfl = int(lib.fcn_conv2d_wgrad_workspace_floats_cfg(C.byref(d), cfg, C.byref(splits)))
    ws = g.put(max(nfl, 1) * 4, name="wgrad workspace")
    dwd, dbd = g.put(poisoned((cout, k, k, cin4)), at_end=True, name="dw"), g.put(poisoned(cout), at_end=True, name="db")
    rc = lib.fcn_conv2d_wgrad_cfg_f32(C.byref(d), dwd.ptr, dbd.ptr, ws.ptr, cfg, None)
    if rc == E_UNSUPPORTED and cfg >= 0:
        print("REFUSED wgrad cfg %d: %s" % (cfg, lib.fcn_last_error_string().decode()))
        return
    L.check(rc)
    L.call("fcn_device_sync")
    dw, db = dwd.read((cout, k, k, cin4))[..., :cin].transpose(0, 3, 1, 2), dbd.read((cout,))
    dw64, db64 = ref64.conv2d_wgrad(x, dy, k, p, s)
    mw, mb = ref64.conv2d_wgrad(np.abs(x), np.abs(dy), k, p, s)
    assert poison_free(dw) and poison_free(db)
    # (each dW element sums only the n * h * w products whose tap lies in the image; the bound counts those)
    within(dw, dw64, ref64.dot_bound_rms(n * h * w, mw), "pad 100 wgrad cfg %d dw" % cfg)
    within(db, db64, ref64.dot_bound_rms(n * oh * ow, mb), "pad 100 wgrad cfg %d db" % cfg)


# h, w, c, x_cstride, x channel offset, y_cstride, y channel offset
ODD = [(7, 9, 4, 8, 4, 4, 0), (7, 9, 5, 9, 3, 7, 1), (131, 123, 8, 8, 0, 8, 0), (131, 123, 3, 4, 0, 4, 0), (1, 1, 4, 4, 0, 4, 0), (2, 3, 6, 8, 1, 8, 2)]


@pytest.mark.parametrize("case", ODD)
def test_pool_2x2_s2_over_odd_extents(g, case):
    """The last window of an odd extent holds one row / column only (ceil rule): forward value and argmax, then backward in its
    three forms.  Every input pixel lies in exactly one window, so backward has no sums: exact equality."""
    h, w, c, xcs, xo, ycs, yo = case
    k, s, p, n = 2, 2, 0, 2
    rng = np.random.default_rng(ODD.index(case))
    x = -np.abs(rng.standard_normal((n, c, h, w))).astype(np.float32) - 0.25      # all negative: a window padded with zeros would win
    ry, ridx = ref64.max_pool(x, k, s, p)
    oh, ow = ry.shape[2:]
    assert (oh, ow) == ((h + 1) // 2, (w + 1) // 2)
    xd = g.put(poisoned_nhwc(x, xcs, xo, poison="huge"), at_end=True, poison="huge", name="x")
    yd = g.put(poisoned((n, oh, ow, ycs)), name="y")
    idd = g.put(poisoned((n, oh, ow, c), dtype=np.int32), name="argmax")
    L.call("fcn_maxpool_fwd_f32", xd.ptr + 4 * xo, yd.ptr, idd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, None)
    full = yd.read((n, oh, ow, ycs))
    assert np.array_equal(nchw(full, c, yo), ry) and slice_untouched(full, yo, c)
    idx = idd.read((n, oh, ow, c), np.int32)
    assert np.array_equal(idx.transpose(0, 3, 1, 2), ridx)
    dy = rng.standard_normal(ry.shape).astype(np.float32)
    want = np.zeros(x.shape, np.float32)
    for (a, ch, i, j), flat in np.ndenumerate(ridx):
        want[a, ch, flat // w, flat % w] += dy[a, ch, i, j]
    base = rng.standard_normal(x.shape).astype(np.float32)
    act = np.maximum(rng.standard_normal(x.shape), 0).astype(np.float32)
    dyd = g.put(poisoned_nhwc(dy, ycs, yo), at_end=True, name="dy")
    actd = g.put(poisoned_nhwc(act, xcs, xo), at_end=True, name="activation")
    args = (n, h, w, c, xcs, xo, k, s, p, oh, ow, ycs, yo)
    for acc, mask in ((0, False), (1, False), (0, True), (1, True)):
        dxd = g.put(poisoned_nhwc(base, xcs, xo) if acc else poisoned((n, h, w, xcs)), at_end=True, name="dx")
        if mask:
            L.call("fcn_maxpool_bwd_mask_f32", dyd.ptr, idd.ptr, dxd.ptr, *args, acc, actd.ptr, xcs, xo, None)
        else:
            L.call("fcn_maxpool_bwd_f32", dyd.ptr, idd.ptr, dxd.ptr, *args, acc, None)
        fulld = dxd.read((n, h, w, xcs))
        got = nchw(fulld, c, xo)
        ref = ((want + base * np.float32(acc)) * ((act > 0) if mask else 1)).astype(np.float32)
        assert poison_free(got) and slice_untouched(fulld, xo, c)
        assert np.array_equal(got, ref), "maxpool bwd acc=%d mask=%d over %d x %d" % (acc, mask, h, w)
