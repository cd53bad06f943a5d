#!/usr/bin/env python3
"""Times the InnerProduct streaming kernels on the GPU (not imported by the package).

Per layer shape of CaffeNet / GOTURN / VGG16 and row count M, both element types and both cache policies of the weight loads:
the forward cold (one launch behind a 512 MiB memset that evicts L2 and the Infinity Cache; median of `--cold` such launches)
and replayed (`--reps` launches back to back: 200 by default, a window of several milliseconds), in microseconds, GB/s of weight bytes, and the ratio to the byte floor at 6.0 TB/s;
then the backward kernels at M = 8 and 32.  Buffers hold zeros: the kernels' time does not depend on the values.

    python tools/ip_bench.py [--quick] [--cold 5] [--reps 200] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402

SHAPES = [("caffenet fc6", 9216, 4096), ("caffenet fc7", 4096, 4096), ("caffenet fc8", 4096, 1000), ("goturn fc6-new", 18432, 4096),
          ("goturn fc8-shapes", 4096, 4), ("vgg16 fc6", 25088, 4096)]
HBM = 6.0e12


class Timer:
    def __init__(self, stream):
        self.stream, self.a, self.b = stream, C.c_void_p(), C.c_void_p()
        L.call("fcn_event_create", C.byref(self.a))
        L.call("fcn_event_create", C.byref(self.b))

    def us(self, fn, reps=1):
        L.call("fcn_event_record", self.a, self.stream)
        for _ in range(reps):
            fn()
        L.call("fcn_event_record", self.b, self.stream)
        L.call("fcn_event_sync", self.b)
        ms = C.c_float()
        L.call("fcn_event_elapsed_ms", self.a, self.b, C.byref(ms))
        return 1e3 * ms.value / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M in {1, 8, 32} only")
    ap.add_argument("--cold", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = L.load()
    L.call("fcn_init", 0)
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    t = Timer(st)
    evict = DeviceBuffer(512 << 20, zero=True)
    rows = []

    def measure(fn):
        fn()
        L.call("fcn_stream_sync", st)
        cold = []
        for _ in range(a.cold):
            L.call("fcn_memset_async", evict.ptr, 0, evict.nbytes, st)
            L.call("fcn_stream_sync", st)
            cold.append(t.us(fn))
        return statistics.median(cold), t.us(fn, a.reps)

    ms = (1, 8, 32) if a.quick else (1, 2, 4, 8, 10, 16, 32)
    print("%-18s %-4s %3s %-3s %9s %9s %8s %8s %6s" % ("layer", "type", "M", "nt", "cold us", "replay us", "cold GB/s", "floor us", "ratio"))
    for name, K, N in SHAPES:
        w = DeviceBuffer(4 * N * K)
        x, y, b = DeviceBuffer(4 * 32 * K), DeviceBuffer(4 * 32 * (N + 8)), DeviceBuffer(4 * (N + 8))
        ycs = (N + 7) // 8 * 8
        for esize, fn in ((4, lib.fcn_inner_product_fwd_f32), (2, lib.fcn_inner_product_fwd_f16)):
            for M in ms:
                nb = int(lib.fcn_inner_product_workspace_bytes(M, K, N))
                ws = DeviceBuffer(nb) if nb else None
                for nt in (0, L.IP_WEIGHTS_NT):
                    call = lambda: L.check(fn(x.ptr, K, w.ptr, b.ptr, y.ptr, ycs, 0, M, K, N, L.CONV_RELU | nt, ws.ptr if ws else None, st))
                    cold, rep = measure(call)
                    floor = 1e6 * esize * N * K / HBM
                    rows.append(dict(layer=name, kernel="fwd", esize=esize, M=M, nt=bool(nt), cold_us=cold, replay_us=rep, floor_us=floor))
                    print("%-18s %-4s %3d %-3s %9.1f %9.1f %8.0f %8.1f %6.2f" % (name, "f32" if esize == 4 else "f16", M, "nt" if nt else "-",
                                                                                 cold, rep, esize * N * K / cold / 1e3, floor, cold / floor))
        for M in (8, 32):
            nb = int(lib.fcn_inner_product_workspace_bytes(M, K, N))
            ws = DeviceBuffer(nb) if nb else None
            for kname, call in (
                    ("bwd_data", lambda: L.check(lib.fcn_inner_product_bwd_data_f32(y.ptr, ycs, 0, w.ptr, x.ptr, K, M, K, N, 0, ws.ptr if ws else None, st))),
                    ("bwd_weights", lambda: L.check(lib.fcn_inner_product_bwd_weights_f32(x.ptr, K, y.ptr, ycs, 0, w.ptr, b.ptr, M, K, N, 0, st)))):
                cold, rep = measure(call)
                floor = 1e6 * 4 * N * K / HBM
                rows.append(dict(layer=name, kernel=kname, esize=4, M=M, nt=False, cold_us=cold, replay_us=rep, floor_us=floor))
                print("%-18s %-11s %3d %9.1f %9.1f %8.0f %8.1f %6.2f" % (name, kname, M, cold, rep, 4 * N * K / cold / 1e3, floor, cold / floor))
        for d in (w, x, y, b):
            d.free()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
