#!/usr/bin/env python3
"""Times the rectangular-convolution kernels alone on the GPU (not imported by the package).

The 17-grid shapes of Inception-v3 at full width: 1x7 (pad 0, 3) and 7x1 (pad 3, 0) on 17 x 17 blobs, 128 -> 128 and 160 -> 192 channels,
at batch 1 and 8: the forward launch (fcn_rconv2d_f32), the data gradient (the same kernel on dY with a flipped bank: the channel counts
trade places, the pads stay) and the weight gradient (fcn_rconv2d_wgrad_f32 with db).  Beside each, as a yardstick, the existing dense
kernel - fcn_conv2d_fwd_f32 / fcn_conv2d_wgrad_f32 in their default configuration - on a 1x1 problem with 7 x Cin input channels and
the same output: the same FLOPs and the same GEMM shape, without the taps.  `--runs` windows of `--reps` launches back to back: the
median and the range of the per-launch time, TF/s from 2 N OH OW Cin Cout kh kw, and the ratio to the dense kernel.  Buffers hold zeros:
the kernels' time does not depend on the values.

    python tools/rconv_bench.py [--runs 7] [--reps 200]
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

    print("%d windows of %d launches each: median (min .. max) per launch" % (a.runs, a.reps))
    hw, taps = 17, 7
    keep = []
    for cin, cout in ((128, 128), (160, 192)):
        for kh, kw in ((1, 7), (7, 1)):
            for n in (1, 8):
                flops = 2.0 * n * hw * hw * cin * cout * taps
                big = max(cin, cout)
                x, dx = (DeviceBuffer(4 * n * hw * hw * taps * big) for _ in range(2))      # (wide enough for the 1x1 yardstick's 7 x C pixels)
                y = DeviceBuffer(4 * n * hw * hw * taps * big)
                w, wt, dw = (DeviceBuffer(4 * cout * taps * cin) for _ in range(3))
                b, db = DeviceBuffer(4 * big), DeviceBuffer(4 * big)

                def rect(xb, wb, yb, ci, co, bias=None):
                    d = L.RConvDesc()
                    d.x, d.w, d.bias, d.y = xb.ptr, wb.ptr, bias, yb.ptr
                    d.N, d.H, d.W, d.Cin, d.x_cstride = n, hw, hw, ci, ci
                    d.Cout, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = co, kh, kw, kh // 2, kw // 2, 1, 1, hw, hw
                    d.y_cstride, d.y_coffset, d.flags, d.dilation = co, 0, 0, 1
                    ws = DeviceBuffer(int(lib.fcn_rconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
                    plan = L.RConvPlan()
                    L.call("fcn_rconv2d_prepare", C.byref(d), 1, ws.ptr, -1, C.byref(plan))
                    keep.extend([d, ws, plan])
                    return d, (lambda: L.check(lib.fcn_rconv2d_f32(C.byref(plan), st)))

                def dense(xb, wb, yb, ci, co, bias=None):
                    d = L.ConvDesc()
                    d.x, d.w, d.bias, d.y = xb.ptr, wb.ptr, bias, yb.ptr
                    d.N, d.H, d.W, d.Cin, d.x_cstride = n, hw, hw, taps * ci, taps * ci
                    d.Cout, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = co, 1, 1, 0, 1, hw, hw
                    d.y_cstride, d.y_coffset, d.flags = co, 0, 0
                    keep.append(d)
                    return d, (lambda: L.check(lib.fcn_conv2d_fwd_f32(C.byref(d), st)))

                rd, fwd = rect(x, w, y, cin, cout, b.ptr)
                cd, fwd_dense = dense(x, w, y, cin, cout, b.ptr)
                _, dgrad = rect(y, wt, dx, cout, cin)             # pad' = (k - 1) - pad = pad for an odd kernel with pad (k - 1) / 2
                _, dgrad_dense = dense(y, wt, dx, cout, cin)
                wsf = int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(rd)))
                wws = DeviceBuffer(max(4 * wsf, 16), zero=False)
                dsf = int(lib.fcn_conv2d_wgrad_workspace_floats(C.byref(cd), None))
                dws = DeviceBuffer(max(4 * dsf, 16), zero=False)
                cases = [
                    ("forward", fwd, fwd_dense),
                    ("data gradient", dgrad, dgrad_dense),
                    ("weight gradient", lambda: L.check(lib.fcn_rconv2d_wgrad_f32(C.byref(rd), dw.ptr, db.ptr, wws.ptr, st)),
                     lambda: L.check(lib.fcn_conv2d_wgrad_f32(C.byref(cd), dw.ptr, db.ptr, dws.ptr, st))),
                ]
                for kname, fn, fn_dense in cases:
                    med, lo, hi = measure(fn)
                    dmed, dlo, dhi = measure(fn_dense)
                    print("%dx%d %3d->%-3d batch %d %-15s %8.1f us (%.1f .. %.1f) %6.2f TF/s | dense 1x1 %4d->%-3d %8.1f us (%.1f .. %.1f) %6.2f TF/s | x%.2f" % (
                        kh, kw, cin, cout, n, kname, med, lo, hi, flops / med * 1e-6, taps * (cout if kname == "data gradient" else cin),
                        cin if kname == "data gradient" else cout, dmed, dlo, dhi, flops / dmed * 1e-6, med / dmed), flush=True)
                for buf in (x, dx, y, w, wt, dw, b, db, wws, dws):
                    buf.free()


if __name__ == "__main__":
    main()
