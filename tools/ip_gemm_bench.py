#!/usr/bin/env python3
"""Times the InnerProduct GEMM kernels (csrc/ip_gemm.hip) on the GPU beside the only thing the streaming kernels can do at those row
counts: ceil(M / 32) calls of at most 32 rows each (not imported by the package).  The method is tools/ip_bench.py's.

Per layer shape of CaffeNet and VGG16 and row count M in {33, 64, 128, 256, 300}: the forward in both element types and the two float32
backward kernels, each alone, cold (one launch behind a 512 MiB memset that evicts L2 and the Infinity Cache; median of `--cold` such
launches) and replayed (`--reps` launches back to back), in microseconds, the TF/s of the cold launch, the two floors as arithmetic
(bank bytes at 6.0 TB/s, FLOPs at the float32 MFMA pipe's 143 TF/s - for the half-float forward the same figure times 16), and the chunked
stream in the same run.  Buffers hold zeros: the kernels' time does not depend on the values.

    python tools/ip_gemm_bench.py [--quick] [--cold 5] [--reps 200] [--json out.json]
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

SHAPES = [("caffenet fc6", 9216, 4096), ("caffenet fc7", 4096, 4096), ("caffenet fc8", 4096, 1000), ("vgg16 fc6", 25088, 4096)]
ROWS = (33, 64, 128, 256, 300)
HBM, MFMA_F32 = 6.0e12, 143e12


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
    ap.add_argument("--quick", action="store_true", help="M in {33, 300} only")
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
    out = []

    def measure(fn, reps):
        fn()
        L.call("fcn_stream_sync", st)
        cold = []
        for _ in range(a.cold):
            L.call("fcn_memset_async", evict.ptr, 0, evict.nbytes, st)
            L.call("fcn_stream_sync", st)
            cold.append(t.us(fn))
        return statistics.median(cold), t.us(fn, reps)

    def chunks(M):
        return [(m0, min(32, M - m0)) for m0 in range(0, M, 32)]

    rows = (33, 300) if a.quick else ROWS
    mmax = max(rows)
    print("%-13s %-11s %3s | %9s %9s %6s | %8s %8s | %9s %9s %6s" % ("layer", "kernel", "M", "gemm cold", "replay us", "TF/s", "bytes us", "flops us",
                                                                    "strm cold", "replay us", "ratio"))
    for name, K, N in SHAPES:
        ycs = (N + 7) // 8 * 8
        w, x, y, b = DeviceBuffer(4 * N * K), DeviceBuffer(4 * mmax * K), DeviceBuffer(4 * mmax * ycs), DeviceBuffer(4 * ycs)
        for M in rows:
            flops = 2.0 * M * K * N
            reps = max(min(a.reps, int(a.reps * 64 / M)), 20)      # (a window of some tens of milliseconds at the large shapes)
            cases = []
            for esize, tag in ((4, "f32"), (2, "f16")):
                gemm, stream = getattr(lib, "fcn_ip_gemm_fwd_" + tag), getattr(lib, "fcn_inner_product_fwd_" + tag)
                nb = int(lib.fcn_ip_gemm_workspace_bytes(M, K, N, esize))
                gws = DeviceBuffer(nb) if nb else None
                snb = max(int(lib.fcn_inner_product_fwd_workspace_bytes(m, K, N, esize)) for _m0, m in chunks(M))
                sws = DeviceBuffer(snb) if snb else None

                def gemm_call(gemm=gemm, gws=gws):
                    L.check(gemm(x.ptr, K, w.ptr, b.ptr, y.ptr, ycs, 0, M, K, N, L.CONV_RELU, gws.ptr if gws else None, st))

                def stream_call(stream=stream, sws=sws, esize=esize):
                    for m0, m in chunks(M):
                        L.check(stream(x.ptr + esize * m0 * K, K, w.ptr, b.ptr, y.ptr + esize * m0 * ycs, ycs, 0, m, K, N,
                                       L.CONV_RELU | L.IP_WEIGHTS_NT, sws.ptr if sws else None, st))
                cases.append(("fwd " + tag, esize, gemm_call, stream_call, MFMA_F32 * (16 if esize == 2 else 1)))
            nb = int(lib.fcn_ip_gemm_workspace_bytes(M, K, N, 4))
            ws1, ws2 = (DeviceBuffer(nb), DeviceBuffer(nb)) if nb else (None, None)
            snb = int(lib.fcn_inner_product_workspace_bytes(32, K, N))
            sws = DeviceBuffer(snb) if snb else None

            def bwd_data():
                L.check(lib.fcn_ip_gemm_bwd_data_f32(y.ptr, ycs, 0, w.ptr, x.ptr, K, M, K, N, 0, ws1.ptr if ws1 else None, st))

            def bwd_data_stream():
                for m0, m in chunks(M):
                    L.check(lib.fcn_inner_product_bwd_data_f32(y.ptr + 4 * m0 * ycs, ycs, 0, w.ptr, x.ptr + 4 * m0 * K, K, m, K, N, 0,
                                                               sws.ptr if sws else None, st))

            def bwd_weights():
                L.check(lib.fcn_ip_gemm_bwd_weights_f32(x.ptr, K, y.ptr, ycs, 0, w.ptr, b.ptr, M, K, N, 0, ws2.ptr if ws2 else None, st))

            def bwd_weights_stream():      # the first chunk writes dW, the others add into it
                for i, (m0, m) in enumerate(chunks(M)):
                    L.check(lib.fcn_inner_product_bwd_weights_f32(x.ptr + 4 * m0 * K, K, y.ptr + 4 * m0 * ycs, ycs, 0, w.ptr, b.ptr, m, K, N,
                                                                  1 if i else 0, st))
            cases += [("bwd_data", 4, bwd_data, bwd_data_stream, MFMA_F32), ("bwd_weights", 4, bwd_weights, bwd_weights_stream, MFMA_F32)]
            for kname, esize, gemm_call, stream_call, peak in cases:
                gc, gr = measure(gemm_call, reps)
                sc, sr = measure(stream_call, max(reps // 4, 10))
                bytes_us, flops_us = 1e6 * esize * N * K / HBM, 1e6 * flops / peak
                out.append(dict(layer=name, kernel=kname, M=M, K=K, N=N, gemm_cold_us=gc, gemm_replay_us=gr, tflops_cold=flops / gc / 1e6,
                                bytes_floor_us=bytes_us, flops_floor_us=flops_us, stream_calls=len(chunks(M)), stream_cold_us=sc,
                                stream_replay_us=sr))
                print("%-13s %-11s %3d | %9.1f %9.1f %6.1f | %8.1f %8.1f | %9.1f %9.1f %6.2f" % (name, kname, M, gc, gr, flops / gc / 1e6, bytes_us,
                                                                                                flops_us, sc, sr, sc / gc), flush=True)
        for d in (w, x, y, b):
            d.free()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
