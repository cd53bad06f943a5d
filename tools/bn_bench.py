#!/usr/bin/env python3
"""Times the BatchNorm / Scale kernels alone on the GPU (not imported by the package).

Each of fcn_batchnorm_stats_f32, fcn_batchnorm_apply_f32 (fused BatchNorm + Scale + ReLU, in place, x-hat kept),
fcn_batchnorm_apply_f16 (inference), fcn_batchnorm_bwd_reduce_f32 and fcn_batchnorm_bwd_apply_f32 on the blobs of bn_conv1
(112 x 112 x 64), bn2a_branch2c (56 x 56 x 256) and bn5c_branch2c (7 x 7 x 2048) of ResNet-50 at batch 8: `--runs` windows of `--reps`
launches back to back, the median and the range of the per-launch time, beside the byte floor at 6.0 TB/s (arithmetic, not a
measurement): statistics read x once (the second, centring pass over a slab comes from the caches); apply reads x and writes y and
x-hat; the half twin reads and writes halves; the backward reduce reads dy, x-hat and y; the backward apply reads the three and
writes dx.  Buffers hold zeros: the kernels' time does not depend on the values.

    python tools/bn_bench.py [--runs 7] [--reps 200]
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
    for name, c, h in (("bn_conv1", 64, 112), ("bn2a_branch2c", 256, 56), ("bn5c_branch2c", 2048, 7)):
        pix = n * h * h
        blob = 4 * pix * c
        x, hat, dy, dx, xh = (DeviceBuffer(blob) for _ in range(5))
        bm, bv, bf, save, ga, be, s1, s2 = (DeviceBuffer(4 * 2 * c) for _ in range(8))
        ws = DeviceBuffer(int(lib.fcn_batchnorm_workspace_bytes(pix, c)), zero=False)
        cases = [
            ("stats_f32", blob, lambda: L.check(lib.fcn_batchnorm_stats_f32(x.ptr, pix, c, c, 0, bm.ptr, bv.ptr, bf.ptr, 0.999, 1e-5, save.ptr, ws.ptr, st))),
            ("apply_f32", 3 * blob, lambda: L.check(lib.fcn_batchnorm_apply_f32(x.ptr, x.ptr, hat.ptr, pix, c, c, 0, c, 0, c, save.ptr, None, None, None,
                                                                               1e-5, ga.ptr, be.ptr, 1, st))),
            ("apply_f16", blob, lambda: L.check(lib.fcn_batchnorm_apply_f16(xh.ptr, xh.ptr, pix, c, c, 0, c, 0, bm.ptr, bv.ptr, bf.ptr, 1e-5, ga.ptr,
                                                                            be.ptr, 1, st))),
            ("bwd_reduce_f32", 3 * blob, lambda: L.check(lib.fcn_batchnorm_bwd_reduce_f32(dy.ptr, hat.ptr, x.ptr, pix, c, c, 0, c, 0, c, 0, s1.ptr, s2.ptr,
                                                                                         ws.ptr, st))),
            ("bwd_apply_f32", 4 * blob, lambda: L.check(lib.fcn_batchnorm_bwd_apply_f32(dy.ptr, hat.ptr, x.ptr, dx.ptr, pix, c, c, 0, c, 0, c, 0, c, 0,
                                                                                       save.ptr, None, None, 1e-5, ga.ptr, s1.ptr, s2.ptr, 0, st))),
        ]
        for kname, nbytes, fn in cases:
            med, lo, hi = measure(fn)
            floor = 1e6 * nbytes / HBM
            print("%-15s %-14s batch %d  %7.2f us (%.2f .. %.2f)  floor %.2f us  x%.1f" % (kname, name, n, med, lo, hi, floor, med / floor))
        for b in (x, hat, dy, dx, xh, bm, bv, bf, save, ga, be, s1, s2, ws):
            b.free()


if __name__ == "__main__":
    main()
