#!/usr/bin/env python3
"""Times the rectangular / dilated convolution kernels (csrc/rconv.hip) alone on the GPU (not imported by the package).

Two shape sets, each at batch 1 and 8:

  inception  the 17-grid shapes of Inception-v3 at full width: 1x7 (pad 0, 3) and 7x1 (pad 3, 0) on 17 x 17 blobs, 128 -> 128 and
             160 -> 192 channels.  Yardstick: the dense kernel on a 1x1 problem with 7 x Cin input channels and the same output - the
             same FLOPs and the same GEMM shape, without the taps.
  deeplab    fc6 (512 -> 1024, 3x3, dilation 12, pad 12) and conv5_1 (512 -> 512, 3x3, dilation 2, pad 2) of DeepLab-LargeFOV on their
             41 x 41 blobs: square dilated layers, the problem with equal axes.  Yardstick: the dense kernel on the same shape with
             dilation 1 and pad 1, which runs the same FLOPs.

For each: the forward launch (fcn_rconv2d_f32), the data gradient (the same kernel on dY with a flipped bank: the channel counts trade
places, pad' = dil (k-1) - pad = pad) and the weight gradient (fcn_rconv2d_wgrad_f32 with db).  The yardstick is fcn_conv2d_fwd_f32 /
fcn_conv2d_wgrad_f32 in their default configuration.  `--runs` windows of `--reps` launches back to back: the median and the range of
the per-launch time, TF/s from 2 N OH OW Cin Cout kh kw, and the ratio to the dense kernel.  Buffers hold zeros: the kernels' time
does not depend on the values.

    python tools/rconv_bench.py [--shapes inception|deeplab|all] [--runs 7] [--reps 200]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402

# set -> (name, H = W, Cin, Cout, (kh, kw), dilation); the pad is dil * (k // 2) per axis: the output is as large as the input
SHAPES = {
    "inception": [("%dx%d" % k, 17, cin, cout, k, 1) for cin, cout in ((128, 128), (160, 192)) for k in ((1, 7), (7, 1))],
    "deeplab": [("fc6", 41, 512, 1024, (3, 3), 12), ("conv5_1", 41, 512, 512, (3, 3), 2)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", choices=sorted(SHAPES) + ["all"], default="all")
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
    keep = []
    for which in sorted(SHAPES) if a.shapes == "all" else [a.shapes]:
        for name, hw, cin, cout, (kh, kw), dil in SHAPES[which]:
            for n in (1, 8):
                taps = kh * kw
                flops = 2.0 * n * hw * hw * cin * cout * taps
                square = kh == kw      # yardstick: the same kernel at dilation 1 (square) or a 1x1 problem over taps x C channels
                big = max(cin, cout) * (1 if square else taps)
                x, dx, y = (DeviceBuffer(4 * n * hw * hw * big) for _ in range(3))
                w, wt, dw = (DeviceBuffer(4 * cout * taps * cin) for _ in range(3))
                b, db = DeviceBuffer(4 * max(cin, cout)), DeviceBuffer(4 * max(cin, cout))

                def rconv(xb, wb, yb, ci, co, bias=None):
                    d = L.RConvDesc()
                    d.x, d.w, d.bias, d.y = xb.ptr, wb.ptr, bias, yb.ptr
                    d.N, d.H, d.W, d.Cin, d.x_cstride = n, hw, hw, ci, ci
                    d.Cout, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = co, kh, kw, dil * (kh // 2), dil * (kw // 2), 1, 1, hw, hw
                    d.y_cstride, d.y_coffset, d.flags, d.dilation = co, 0, 0, dil
                    ws = DeviceBuffer(int(lib.fcn_rconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
                    plan = L.RConvPlan()
                    L.call("fcn_rconv2d_prepare", C.byref(d), 1, ws.ptr, -1, C.byref(plan))
                    keep.extend([d, ws, plan])
                    return d, (lambda: L.check(lib.fcn_rconv2d_f32(C.byref(plan), st)))

                def dense(xb, wb, yb, ci, co, bias=None):
                    d = L.ConvDesc()
                    d.x, d.w, d.bias, d.y = xb.ptr, wb.ptr, bias, yb.ptr
                    dci, dk = (ci, kh) if square else (taps * ci, 1)
                    d.N, d.H, d.W, d.Cin, d.x_cstride = n, hw, hw, dci, dci
                    d.Cout, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = co, dk, dk, dk // 2, 1, hw, hw
                    d.y_cstride, d.y_coffset, d.flags = co, 0, 0
                    keep.append(d)
                    return d, (lambda: L.check(lib.fcn_conv2d_fwd_f32(C.byref(d), st)))

                rd, fwd = rconv(x, w, y, cin, cout, b.ptr)
                cd, fwd_dense = dense(x, w, y, cin, cout, b.ptr)
                _, dgrad = rconv(y, wt, dx, cout, cin)            # pad' = dil (k - 1) - pad = pad for an odd kernel with pad dil (k - 1) / 2
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
                    print("%-8s d%-2d %4d->%-4d batch %d %-15s %9.1f us (%.1f .. %.1f) %6.2f TF/s | dense %s %9.1f us (%.1f .. %.1f) %6.2f TF/s | x%.2f" % (
                        name, dil, cin, cout, n, kname, med, lo, hi, flops / med * 1e-6, "d1" if square else "1x1", dmed, dlo, dhi,
                        flops / dmed * 1e-6, med / dmed), flush=True)
                for buf in (x, dx, y, w, wt, dw, b, db, wws, dws):
                    buf.free()


if __name__ == "__main__":
    main()
