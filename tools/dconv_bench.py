#!/usr/bin/env python3
"""Times the dilated-convolution kernels alone on the GPU (not imported by the package).

fc6 (512 -> 1024, 3x3, dilation 12, pad 12) and conv5_1 (512 -> 512, 3x3, dilation 2, pad 2) of DeepLab-LargeFOV on their 41 x 41
blobs at batch 1 and 8: the forward launch (fcn_dconv2d_f32), the data gradient (the same kernel on dY with a flipped bank: the channel
counts trade places, pad' = dil (k-1) - pad) and the weight gradient (fcn_dconv2d_wgrad_f32 with db).  Beside each, as a yardstick, the
existing dense kernel on the same shape with dilation 1 and pad 1 - fcn_conv2d_fwd_f32 / fcn_conv2d_wgrad_f32 in their default
configuration - which runs the same FLOPs.  `--runs` windows of `--reps` launches back to back: the median and the range of the
per-launch time, TF/s from 2 N OH OW Cin Cout k k, and the ratio to the dense kernel.  Buffers hold zeros: the kernels' time does not
depend on the values.

    python tools/dconv_bench.py [--runs 7] [--reps 200]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402


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

    def geometry(d, n, hw, cin, cout, pad):
        d.N, d.H, d.W, d.Cin, d.x_cstride = n, hw, hw, cin, cin
        d.Cout, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = cout, 3, 3, pad, 1, hw, hw
        d.y_cstride, d.y_coffset, d.flags = cout, 0, 0

    print("%d windows of %d launches each: median (min .. max) per launch" % (a.runs, a.reps))
    hw, k = 41, 3
    keep = []
    for name, cin, cout, dil in (("fc6", 512, 1024, 12), ("conv5_1", 512, 512, 2)):
        for n in (1, 8):
            flops = 2.0 * n * hw * hw * cin * cout * k * k
            x, dx = (DeviceBuffer(4 * n * hw * hw * cin) for _ in range(2))
            y = DeviceBuffer(4 * n * hw * hw * cout)
            w, wt, dw = (DeviceBuffer(4 * cout * k * k * cin) for _ in range(3))
            b, db = DeviceBuffer(4 * cout), DeviceBuffer(4 * cout)

            def dilated(xb, wb, yb, ci, co, bias=None):
                d = L.DConvDesc()
                d.x, d.w, d.bias, d.y = xb.ptr, wb.ptr, bias, yb.ptr
                geometry(d, n, hw, ci, co, dil)
                d.dilation = dil
                ws = DeviceBuffer(int(lib.fcn_dconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
                plan = L.DConvPlan()
                L.call("fcn_dconv2d_prepare", C.byref(d), 1, ws.ptr, -1, C.byref(plan))
                keep.extend([d, ws, plan])
                return d, (lambda: L.check(lib.fcn_dconv2d_f32(C.byref(plan), st)))

            def dense(xb, wb, yb, ci, co, bias=None):
                d = L.ConvDesc()
                d.x, d.w, d.bias, d.y = xb.ptr, wb.ptr, bias, yb.ptr
                geometry(d, n, hw, ci, co, 1)
                keep.append(d)
                return d, (lambda: L.check(lib.fcn_conv2d_fwd_f32(C.byref(d), st)))

            dd, fwd = dilated(x, w, y, cin, cout, b.ptr)
            cd, fwd_dense = dense(x, w, y, cin, cout, b.ptr)
            _, dgrad = dilated(y, wt, dx, cout, cin)          # pad' = dil (k-1) - pad = dil
            _, dgrad_dense = dense(y, wt, dx, cout, cin)
            wsf = int(lib.fcn_dconv2d_wgrad_workspace_floats(C.byref(dd)))
            wws = DeviceBuffer(max(4 * wsf, 16), zero=False)
            dsf = int(lib.fcn_conv2d_wgrad_workspace_floats(C.byref(cd), None))
            dws = DeviceBuffer(max(4 * dsf, 16), zero=False)
            cases = [
                ("forward", fwd, fwd_dense),
                ("data gradient", dgrad, dgrad_dense),
                ("weight gradient", lambda: L.check(lib.fcn_dconv2d_wgrad_f32(C.byref(dd), dw.ptr, db.ptr, wws.ptr, st)),
                 lambda: L.check(lib.fcn_conv2d_wgrad_f32(C.byref(cd), dw.ptr, db.ptr, dws.ptr, st))),
            ]
            for kname, fn, fn_dense in cases:
                med, lo, hi = measure(fn)
                dmed, dlo, dhi = measure(fn_dense)
                print("%-8s d%-2d batch %d %-15s %9.1f us (%.1f .. %.1f) %6.2f TF/s | dense d1 %9.1f us (%.1f .. %.1f) %6.2f TF/s | x%.2f" % (
                    name, dil, n, kname, med, lo, hi, flops / med * 1e-6, dmed, dlo, dhi, flops / dmed * 1e-6, med / dmed), flush=True)
            for buf in (x, dx, y, w, wt, dw, b, db, wws, dws):
                buf.free()


if __name__ == "__main__":
    main()
