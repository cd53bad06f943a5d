#!/usr/bin/env python3
"""Times the depthwise-convolution kernels alone on the GPU (not imported by the package).

The depthwise layers of MobileNet v1 at full width - 3x3 pad 1 on 112x112x32 (stride 1), 112x112x64 (stride 2), 56x56x128, 28x28x256,
14x14x512 (stride 1 and 2 each) and 7x7x1024 - at batch 1 and 8: the forward launch in float32 and in halves, the data gradient and the
weight gradient.  Beside each, as a yardstick, an existing kernel of the same traffic, timed in the same run in windows that alternate
with the new kernel's: fcn_maxpool_fwd_f32 / _f16, 3x3 at the same stride and pad on the same blob, for the forward and the data
gradient (the gradient reads the small blob and writes the large one: the same bytes the other way round); fcn_batchnorm_bwd_reduce_f32
on the same two activations (it reads both and writes per-channel sums) for the weight gradient.  `--runs` windows of `--reps` launches
back to back: the median and the range of the per-launch time, bytes/s from 4 (N H W C + N OH OW C + kh kw C + C) (2 bytes per activation
in halves) and its share of the 6.3 TB/s this chip streams, and the ratio to the yardstick.  Buffers hold zeros: the kernels' time does
not depend on the values.  `--nets` adds MobileNet v1 at full width, batch 1 and 8: milliseconds per forward in both engines and per
training step.

    python tools/dwconv_bench.py [--runs 7] [--reps 200] [--nets]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402
from fcn_object_detector_amd.netspec import pool_out  # noqa: E402

STREAM_TBS = 6.3
SHAPES = ((112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1), (14, 512, 2), (7, 1024, 1))


def nets(batches=(1, 8)):
    import numpy as np
    from fcn_object_detector_amd import models, proto
    from fcn_object_detector_amd.engine import Engine
    from fcn_object_detector_amd.netspec import NetSpec, fill_params
    from fcn_object_detector_amd.train import SolverParams, TrainEngine
    for batch in batches:
        msg = proto.parse_text(models.mobilenet_v1("DEPLOY", batch=batch))
        spec = NetSpec(msg, "TEST", depthwise=True)
        spec.infer()
        for dtype in ("f32", "f16"):
            eng = Engine(NetSpec(msg, "TEST", depthwise=True), params=fill_params(spec, seed=1), device=0, dtype=dtype)
            eng.host_array("data")[...] = np.random.default_rng(0).random((batch, 3, 224, 224), dtype=np.float32)
            eng.upload_inputs()
            eng.forward_resident(5)
            runs = sorted(eng.forward_resident(20) / 20 for _ in range(3))
            dw = sum(t for kind, _n, t, _f, _b in eng.time_ops(5) if kind == "dwconv")
            print("MobileNet-v1 224x224 batch %d %s: %.3f ms/forward (min %.3f max %.3f of 3 x 20), the 13 depthwise launches %.3f ms" % (
                batch, dtype, runs[1], runs[0], runs[2], dw), flush=True)
            eng.close()
        msg = proto.parse_text(models.mobilenet_v1("TRAIN", batch=batch))
        spec = NetSpec(msg, "TRAIN", depthwise=True)
        spec.infer()
        te = TrainEngine(NetSpec(msg, "TRAIN", depthwise=True), dict(spec.input_shapes), params=fill_params(spec, seed=2), device=0,
                         solver=SolverParams(base_lr=1e-10, momentum=0.9, weight_decay=1e-7))
        te.host_array("data")[...] = np.random.default_rng(1).random((batch, 3, 224, 224), dtype=np.float32)
        te.upload_inputs()
        for it in range(3):
            te.step(seed=it, upload=False)
        L.call("fcn_device_sync")
        t0 = time.perf_counter()
        for it in range(10):
            te.step(seed=10 + it, upload=False)
        L.call("fcn_device_sync")
        print("MobileNet-v1 224x224 batch %d training: %.3f ms/step (10 steps)" % (batch, (time.perf_counter() - t0) / 10 * 1e3), flush=True)
        te.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--nets", action="store_true")
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

    def measure(fn, yard):
        """Windows of the new kernel and of its yardstick, alternating."""
        fn()
        yard()
        L.call("fcn_stream_sync", st)
        us, yus = [], []
        for _ in range(a.runs):
            us.append(window(fn))
            yus.append(window(yard))
        return (statistics.median(us), min(us), max(us)), (statistics.median(yus), min(yus), max(yus))

    print("%d windows of %d launches each, alternating with the yardstick: median (min .. max) per launch" % (a.runs, a.reps))
    for n in (1, 8):
        for hw, c, s in SHAPES:
            oh = (hw + 2 - 3) // s + 1
            poh = pool_out(hw, 3, s, 1)
            x, dx = DeviceBuffer(4 * n * hw * hw * c), DeviceBuffer(4 * n * hw * hw * c)
            y = DeviceBuffer(4 * n * max(oh, poh) ** 2 * c)
            w, dw, b, db = DeviceBuffer(4 * 9 * c), DeviceBuffer(4 * 9 * c), DeviceBuffer(4 * c), DeviceBuffer(4 * c)
            d = L.dwconv_desc(x.ptr, w.ptr, b.ptr, y.ptr, n, hw, hw, c, c, 3, 3, 1, 1, s, s, 1, c, 0)
            dd = L.dwconv_desc(dx.ptr, w.ptr, None, y.ptr, n, hw, hw, c, c, 3, 3, 1, 1, s, s, 1, c, 0)
            wsf = int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(d), 0))
            wws = DeviceBuffer(max(4 * wsf, 16), zero=False)
            bnws = DeviceBuffer(max(int(lib.fcn_batchnorm_workspace_bytes(n * oh * oh, c)), 16), zero=False)
            s1, s2 = DeviceBuffer(4 * c), DeviceBuffer(4 * c)
            pool32 = lambda: L.check(lib.fcn_maxpool_fwd_f32(x.ptr, y.ptr, None, n, hw, hw, c, c, 3, s, 1, poh, poh, c, 0, st))
            pool16 = lambda: L.check(lib.fcn_maxpool_fwd_f16(x.ptr, y.ptr, n, hw, hw, c, c, 3, s, 1, poh, poh, c, 0, st))
            # (the yardstick of the weight gradient reads two blobs of the OUTPUT's size: the layer's dY and, in x's place, as many pixels of x)
            bnred = lambda: L.check(lib.fcn_batchnorm_bwd_reduce_f32(y.ptr, x.ptr, None, n * oh * oh, c, c, 0, c, 0, c, 0, s1.ptr, s2.ptr, bnws.ptr, st))
            byts = 4.0 * (n * hw * hw * c + n * oh * oh * c + 9 * c + c)
            cases = [("forward f32", lambda: L.check(lib.fcn_dwconv2d_fwd_f32(C.byref(d), -1, st)), pool32, "maxpool f32", byts),
                     ("forward f32 cfg0", lambda: L.check(lib.fcn_dwconv2d_fwd_f32(C.byref(d), 0, st)), pool32, "maxpool f32", byts),
                     ("forward f16", lambda: L.check(lib.fcn_dwconv2d_fwd_f16(C.byref(d), -1, st)), pool16, "maxpool f16",
                      byts - 2.0 * (n * hw * hw * c + n * oh * oh * c)),
                     ("data gradient", lambda: L.check(lib.fcn_dwconv2d_dgrad_f32(C.byref(dd), -1, st)), pool32, "maxpool f32", byts),
                     ("weight gradient", lambda: L.check(lib.fcn_dwconv2d_wgrad_f32(C.byref(d), dw.ptr, db.ptr, wws.ptr, 0, st)), bnred, "bn reduce", byts)]
            for kname, fn, yard, yname, nbytes in cases:
                (med, lo, hi), (ymed, ylo, yhi) = measure(fn, yard)
                tbs = nbytes / med * 1e-6
                print("3x3/%d %3dx%-3d x%-4d batch %d %-16s %7.1f us (%.1f .. %.1f) %5.2f TB/s %4.0f%% | %-11s %7.1f us (%.1f .. %.1f) | x%.2f%s" % (
                    s, hw, hw, c, n, kname, med, lo, hi, tbs, 100 * tbs / STREAM_TBS, yname, ymed, ylo, yhi, med / ymed,
                    "  SLOWER than the yardstick's range" if med > yhi and med - ymed > yhi - ylo else ""), flush=True)
            for buf in (x, dx, y, w, dw, b, db, wws, bnws, s1, s2):
                buf.free()
    if a.nets:
        nets()


if __name__ == "__main__":
    main()
