#!/usr/bin/env python
"""GPU micro-benchmark: the transposed-convolution launch (csrc/tconv.hip) over the shape list of its contract, and - for the
stride-2 3x3 data gradient - the stride-1 data gradient of the same FLOP count through the tiled forward kernel beside it.
Events around repeated launches on one stream; the median of five rounds of `reps` launches each is printed.
usage: python tools/tconv_sweep.py [name ...]   (run on the GPU box)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402
from gpu_util import conv_desc, dev_from  # noqa: E402

# (name, N, Ca, Cb, H, W, k, stride, pad): a = (N, Ca, H, W) -> b = (N, Cb, s(H-1)+k-2p, ...)
SHAPES = [
    ("dgrad3x3s2", 8, 256, 256, 28, 28, 3, 2, 1),      # dX of a 3x3 / stride 2 convolution on (8, 256, 56, 56)
    ("k1s2", 8, 256, 256, 28, 28, 1, 2, 0),
    ("k2s2", 8, 256, 256, 28, 28, 2, 2, 0),
    ("k4s2", 8, 256, 256, 28, 28, 4, 2, 1),
    ("k5s2", 8, 128, 128, 28, 28, 5, 2, 2),
    ("k7s2", 8, 64, 64, 28, 28, 7, 2, 3),
    ("k3s3", 8, 256, 256, 19, 19, 3, 3, 0),
    ("k2s4", 8, 256, 256, 14, 14, 2, 4, 0),
    ("fcn16s_up2", 1, 21, 21, 16, 16, 4, 2, 0),        # FCN-16s upscore2 (num_output x num_output, group 1)
    ("fcn8s_up8", 1, 21, 21, 70, 70, 16, 8, 0),        # FCN-8s upscore8
    ("fcn32s_up32", 1, 21, 21, 16, 16, 32, 16, 8),
    ("up_wide", 4, 512, 128, 28, 28, 4, 2, 1),
]


def timed(fn, st, e0, e1, reps=20):
    for _ in range(3):
        fn()
    rounds = []
    for _ in range(5):
        L.call("fcn_event_record", e0, st)
        for _ in range(reps):
            fn()
        L.call("fcn_event_record", e1, st)
        L.call("fcn_event_sync", e1)
        ms = C.c_float()
        L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
        rounds.append(ms.value / reps * 1e3)
    return float(np.median(rounds))


def main():
    want = sys.argv[1:] or None
    L.call("fcn_init", 0)
    lib = L.load()
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))
    rng = np.random.default_rng(0)
    for name, n, ca, cb, h, w, k, s, pad in SHAPES:
        if want and name not in want:
            continue
        ca4, cb4 = (ca + 3) // 4 * 4, (cb + 3) // 4 * 4
        oh, ow = s * (h - 1) + k - 2 * pad, s * (w - 1) + k - 2 * pad
        a = dev_from(rng.standard_normal((n, h, w, ca4)).astype(np.float32))
        blob = dev_from((rng.standard_normal((ca, k, k, cb4)) * 0.05).astype(np.float32))
        bank = DeviceBuffer(int(lib.fcn_tconv_bank_floats(ca, cb, k, k)) * 4, zero=True)
        L.call("fcn_tconv_bank_pack_f32", blob.ptr, bank.ptr, ca, cb, cb4, k, k, st)
        b = dev_from(np.zeros((n, oh, ow, cb4), np.float32))
        d = L.TConvDesc()
        d.a, d.w, d.bias, d.b = a.ptr, bank.ptr, None, b.ptr
        d.N, d.H, d.W, d.Ca, d.a_cstride = n, h, w, ca, ca4
        d.Cb, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = cb, k, k, pad, s, oh, ow
        d.b_cstride, d.b_coffset, d.flags = cb4, 0, 0
        ws = DeviceBuffer(int(lib.fcn_tconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
        flops = 2.0 * n * h * w * ca * cb * k * k
        line = "%-12s N%d %dx%dx%d -> %dx%dx%d k%d s%d p%d %7.3f GFLOP |" % (name, n, ca, h, w, cb, oh, ow, k, s, pad, flops / 1e9)
        for cfg in range(int(lib.fcn_tconv2d_num_configs())):
            plan = L.TConvPlan()
            L.call("fcn_tconv2d_prepare", C.byref(d), 1, ws.ptr, cfg, C.byref(plan))
            us = timed(lambda: L.call("fcn_tconv2d_f32", C.byref(plan), st), st, e0, e1)
            line += " c%d/%dwg %7.1fus %5.1fTF |" % (cfg, plan.total_tiles, us, flops / us / 1e6)
        us = timed(lambda: L.call("fcn_tconv_bank_pack_f32", blob.ptr, bank.ptr, ca, cb, cb4, k, k, st), st, e0, e1)
        line += " pack %5.1fus |" % us
        if name == "dgrad3x3s2":
            # the yardstick: a stride-1 3x3 data gradient (the forward kernel on dY) with the same FLOP count: (8, 256, 28, 28) -> same size
            x = dev_from(rng.standard_normal((n, h, w, ca4)).astype(np.float32))
            wt = dev_from((rng.standard_normal((cb, 3, 3, ca4)) * 0.05).astype(np.float32))
            y = dev_from(np.zeros((n, h, w, cb4), np.float32))
            cd = conv_desc(x, wt, None, y, n, h, w, ca4, ca4, cb, 3, 1, 1, h, w, cb4, 0, 0)
            arr = (L.ConvDesc * 1)(cd)
            gws = DeviceBuffer(int(lib.fcn_conv2d_group_workspace_bytes(1)), zero=False)
            best = None
            for cfg in [-1] + list(range(int(lib.fcn_conv2d_first_layer_config()))):
                grp = L.ConvGroup()
                if lib.fcn_conv2d_group_prepare(arr, 1, gws.ptr, cfg, C.byref(grp)) != 0:
                    continue
                t = timed(lambda: L.call("fcn_conv2d_fwd_group_f32", C.byref(grp), st), st, e0, e1, reps=10)
                if cfg == -1:
                    line += " stride-1 dgrad, same FLOPs: auto c%d %7.1fus" % (grp.cfg, t)
                if best is None or t < best[0]:
                    best = (t, grp.cfg)
            line += ", best c%d %7.1fus %5.1fTF |" % (best[1], best[0], flops / best[0] / 1e6)
        print(line, flush=True)


if __name__ == "__main__":
    main()
