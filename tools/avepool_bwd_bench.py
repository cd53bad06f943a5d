#!/usr/bin/env python3
"""Times fcn_avepool_bwd_f32 alone on the GPU (not imported by the package), and a grouped convolution against the same groups
launched as separate problems.

AVE pooling backward on the two auxiliary-head shapes of BVLC GoogLeNet (5x5 / s3 on 14x14, 512 and 528 channels) and on pool5
(7x7 on 7x7, 1024 channels) at batch 8: `--runs` windows of `--reps` launches back to back, the median and the range of the
per-launch time, beside the byte floor (dY + dX bytes at 6.0 TB/s; arithmetic, not a measurement).  Then CaffeNet's conv2 at batch 10
(27x27, 96 -> 256, 5x5, pad 2, group 2): one grouped launch of the two per-group descriptors against two launches of one descriptor
each.  Buffers hold zeros: the kernels' time does not depend on the values.

    python tools/avepool_bwd_bench.py [--runs 7] [--reps 200]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402

HBM = 6.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    lib = L.load()
    L.call("fcn_init", 0)
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))

    def window(fn):
        L.call("fcn_event_record", e0, st)
        for _ in range(a.reps):
            fn()
        L.call("fcn_event_record", e1, st)
        L.call("fcn_event_sync", e1)
        ms = C.c_float()
        L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
        return 1e3 * ms.value / a.reps

    def measure(fn):
        fn()
        L.call("fcn_stream_sync", st)
        us = [window(fn) for _ in range(a.runs)]
        return statistics.median(us), min(us), max(us)

    print("%d windows of %d launches each: median (min .. max) per launch" % (a.runs, a.reps))
    n = 8
    for name, c, h, k, s in (("loss1/ave_pool", 512, 14, 5, 3), ("loss2/ave_pool", 528, 14, 5, 3), ("pool5/7x7_s1", 1024, 7, 7, 1)):
        oh = -(-(h - k) // s) + 1
        dy, dx = DeviceBuffer(4 * n * oh * oh * c), DeviceBuffer(4 * n * h * h * c)
        med, lo, hi = measure(lambda: L.check(lib.fcn_avepool_bwd_f32(dy.ptr, dx.ptr, n, h, h, c, c, 0, k, s, 0, oh, oh, c, 0, 0, st)))
        floor = 1e6 * (dy.nbytes + dx.nbytes) / HBM
        print("avepool_bwd %-15s batch %d  %7.2f us (%.2f .. %.2f)  floor %.2f us  x%.1f" % (name, n, med, lo, hi, floor, med / floor))
        dy.free()
        dx.free()

    # CaffeNet conv2, batch 10: two groups of 48 -> 128 channels
    N, H, cin, cout, k, pad, g = 10, 27, 96, 256, 5, 2, 2
    cg, og = cin // g, cout // g
    x, y = DeviceBuffer(4 * N * H * H * cin), DeviceBuffer(4 * N * H * H * cout)
    w, b = DeviceBuffer(4 * cout * k * k * cg), DeviceBuffer(4 * cout)
    descs = []
    for i in range(g):
        d = L.ConvDesc()
        d.x, d.w, d.bias, d.y = x.ptr + 4 * i * cg, w.ptr + 4 * i * og * k * k * cg, b.ptr + 4 * i * og, y.ptr
        d.N, d.H, d.W, d.Cin, d.x_cstride = N, H, H, cg, cin
        d.Cout, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = og, k, k, pad, 1, H, H
        d.y_cstride, d.y_coffset, d.flags = cout, i * og, L.CONV_RELU
        descs.append(d)
    keep = []

    def prepared(ds):
        arr = (L.ConvDesc * len(ds))(*ds)
        ws = DeviceBuffer(int(lib.fcn_conv2d_group_workspace_bytes(len(ds))), zero=False)
        grp = L.ConvGroup()
        L.call("fcn_conv2d_group_prepare", arr, len(ds), ws.ptr, -1, C.byref(grp))
        keep.extend([arr, ws, grp])
        return grp
    both, one = prepared(descs), [prepared([d]) for d in descs]
    med, lo, hi = measure(lambda: L.check(lib.fcn_conv2d_fwd_group_f32(C.byref(both), st)))
    print("conv2 group 2, one grouped launch of 2 descriptors (cfg %d): %7.2f us (%.2f .. %.2f)" % (both.cfg, med, lo, hi))
    med, lo, hi = measure(lambda: [L.check(lib.fcn_conv2d_fwd_group_f32(C.byref(p), st)) for p in one])
    print("conv2 as two launches of 1 descriptor each (cfg %d, %d):           %7.2f us (%.2f .. %.2f)" % (one[0].cfg, one[1].cfg, med, lo, hi))
    for ws in keep:
        if isinstance(ws, DeviceBuffer):
            lib.fcn_conv2d_group_release(ws.ptr)


if __name__ == "__main__":
    main()
