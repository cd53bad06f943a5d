#!/usr/bin/env python3
"""Times the half-float forward of the rectangular / dilated convolution (fcn_rconv2d_f16, csrc/rconv.hip) beside the float32 kernel
(fcn_rconv2d_f32) on the same shapes, each kernel alone on the GPU (not imported by the package).

Shapes, each at batch 1 and 8:

  deeplab    fc6 (512 -> 1024, 3x3, dilation 12, pad 12) and conv5_1 (512 -> 512, 3x3, dilation 2, pad 2) of DeepLab-LargeFOV on their
             41 x 41 blobs.
  inception  the 17-grid layers of Inception-v3: 1x7 (pad 0, 3) and 7x1 (pad 3, 0) on 17 x 17 blobs, 128 -> 128 and 192 -> 192 channels.

`--runs` windows of `--reps` launches back to back, the two element types taking turns window by window: the median and the range of
the per-launch time, TF/s from 2 N OH OW Cin Cout kh kw, and the ratio half / float32.  Inputs and filters are seeded normal values
(the same values in both element types, rounded to halves for the half kernel); every launch has a bias and no ReLU.

    python tools/rconv_f16_bench.py [--shapes inception|deeplab|all] [--runs 7] [--reps 200]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402

# set -> (name, H = W, Cin, Cout, (kh, kw), dilation); the pad is dil * (k // 2) per axis: the output is as large as the input
SHAPES = {
    "deeplab": [("fc6", 41, 512, 1024, (3, 3), 12), ("conv5_1", 41, 512, 512, (3, 3), 2)],
    "inception": [("%dx%d" % k, 17, c, c, k, 1) for c in (128, 192) for k in ((1, 7), (7, 1))],
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

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(arr.nbytes, zero=False)
        L.call("fcn_memcpy_h2d_async", buf.ptr, arr.ctypes.data, arr.nbytes, st)
        L.call("fcn_stream_sync", st)
        return buf

    print("%d windows of %d launches each, float32 and half taking turns: median (min .. max) per launch" % (a.runs, a.reps))
    rng = np.random.default_rng(0)
    for which in sorted(SHAPES) if a.shapes == "all" else [a.shapes]:
        for name, hw, cin, cout, (kh, kw), dil in SHAPES[which]:
            for n in (1, 8):
                flops = 2.0 * n * hw * hw * cin * cout * kh * kw
                x = rng.standard_normal((n, hw, hw, cin)).astype(np.float32)
                w = (rng.standard_normal((cout, kh, kw, cin)) / np.sqrt(cin * kh * kw)).astype(np.float32)
                b = upload(rng.standard_normal(cout).astype(np.float32))
                keep, fns = [b], {}
                for dt, prepare, launch in ((np.float32, "fcn_rconv2d_prepare", lib.fcn_rconv2d_f32), (np.float16, "fcn_rconv2d_prepare_f16", lib.fcn_rconv2d_f16)):
                    xb, wb = upload(x.astype(dt)), upload(w.astype(dt))
                    yb = DeviceBuffer(np.dtype(dt).itemsize * n * hw * hw * cout)
                    d = L.RConvDesc()
                    d.x, d.w, d.bias, d.y = xb.ptr, wb.ptr, b.ptr, yb.ptr
                    d.N, d.H, d.W, d.Cin, d.x_cstride = n, hw, hw, cin, cin
                    d.Cout, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = cout, kh, kw, dil * (kh // 2), dil * (kw // 2), 1, 1, hw, hw
                    d.y_cstride, d.y_coffset, d.flags, d.dilation = cout, 0, 0, dil
                    ws = DeviceBuffer(int(lib.fcn_rconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
                    plan = L.RConvPlan()
                    L.call(prepare, C.byref(d), 1, ws.ptr, -1, C.byref(plan))
                    keep.extend([xb, wb, yb, d, ws, plan])
                    fns[dt] = lambda plan=plan, launch=launch: L.check(launch(C.byref(plan), st))
                us = {dt: [] for dt in fns}
                for fn in fns.values():      # warm up both
                    fn()
                L.call("fcn_stream_sync", st)
                for _ in range(a.runs):
                    for dt, fn in fns.items():
                        us[dt].append(window(fn))
                m32, m16 = statistics.median(us[np.float32]), statistics.median(us[np.float16])
                print("%-8s d%-2d %4d->%-4d batch %d  f32 %8.1f us (%.1f .. %.1f) %6.1f TF/s | f16 %8.1f us (%.1f .. %.1f) %6.1f TF/s | x%.2f" % (
                    name, dil, cin, cout, n, m32, min(us[np.float32]), max(us[np.float32]), flops / m32 * 1e-6,
                    m16, min(us[np.float16]), max(us[np.float16]), flops / m16 * 1e-6, m16 / m32), flush=True)
                for buf in keep:
                    if isinstance(buf, DeviceBuffer):
                        buf.free()


if __name__ == "__main__":
    main()
