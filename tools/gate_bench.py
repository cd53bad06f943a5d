#!/usr/bin/env python3
"""Times the gated-Scale launches (csrc/gate.hip) on the GPU against their byte floors (not imported by the package).  The method is
tools/ip_gemm_bench.py's.

At SE-ResNet-50's four stage shapes (56 x 56 x 256, 28 x 28 x 512, 14 x 14 x 1024, 7 x 7 x 2048), batch 1 and 8, float32 and halves:
the gate alone (y = x g), the fused launch (y = relu(x g + r)) beside the three launches it replaces (the gate, the Eltwise SUM, the
in-place ReLU - the launches the engines plan without the fusion), and in float32 the two gradients (dx = dy g; dgate = sum dy x, a
launch pair).  Each alone, cold (one call behind a 512 MiB memset that evicts L2 and the Infinity Cache; median of `--cold` such calls)
and replayed (`--reps` calls back to back: at these sizes the operands stay in the Infinity Cache, so a replay is not an HBM figure),
in microseconds, with the bytes the call must move at least (every operand once; the gate and the workspace are not counted) and the
time those bytes take at 6.3 TB/s.  Buffers hold zeros: the kernels' time does not depend on the values.

    python tools/gate_bench.py [--quick] [--cold 5] [--reps 200] [--json out.json]
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

SHAPES = [("conv2_x", 56 * 56, 256), ("conv3_x", 28 * 28, 512), ("conv4_x", 14 * 14, 1024), ("conv5_x", 7 * 7, 2048)]
BATCHES = (1, 8)
HBM = 6.3e12


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
    ap.add_argument("--quick", action="store_true", help="the first and the last stage only")
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

    def measure(fn):
        fn()
        L.call("fcn_stream_sync", st)
        cold = []
        for _ in range(a.cold):
            L.call("fcn_memset_async", evict.ptr, 0, evict.nbytes, st)
            L.call("fcn_stream_sync", st)
            cold.append(t.us(fn))
        return statistics.median(cold), t.us(fn, a.reps)

    print("%-8s %2s %-4s %-16s | %8s %9s | %9s %8s %6s" % ("stage", "N", "type", "launch", "cold us", "replay us", "MB moved", "floor us", "cold/fl"))
    for name, ppi, c in (SHAPES[::3] if a.quick else SHAPES):
        for n in BATCHES:
            pix = n * ppi
            for es, tag in ((4, "f32"), (2, "f16")):
                x, r, y, m = (DeviceBuffer(es * pix * c) for _ in range(4))
                g = DeviceBuffer(4 * n * c)
                ws = DeviceBuffer(max(int(lib.fcn_scale_gate_workspace_bytes(n, ppi, c)), 16))
                fwd = lib.fcn_scale_gate_fwd_f16 if es == 2 else lib.fcn_scale_gate_fwd_f32
                elt = lib.fcn_eltwise_fwd_f16 if es == 2 else lib.fcn_eltwise_fwd_f32

                def gate():
                    L.check(fwd(x.ptr, g.ptr, None, m.ptr, n, ppi, c, c, 0, c, 0, 0, c, 0, 0, st))

                def fused():
                    L.check(fwd(x.ptr, g.ptr, r.ptr, y.ptr, n, ppi, c, c, 0, c, c, 0, c, 0, 1, st))

                def three():
                    gate()
                    L.check(elt(m.ptr, r.ptr, y.ptr, pix * c, L.ELT_SUM, 1.0, 1.0, st))
                    if es == 2:
                        L.check(lib.fcn_batchnorm_apply_f16(y.ptr, y.ptr, pix, c, c, 0, c, 0, None, None, None, 0.0, None, None, 1, st))
                    else:
                        L.check(lib.fcn_relu_fwd_f32(y.ptr, y.ptr, pix * c, 0.0, st))

                def bwd_data():
                    L.check(lib.fcn_scale_gate_bwd_data_f32(y.ptr, g.ptr, x.ptr, n, ppi, c, c, 0, c, c, 0, 0, st))

                def bwd_data_acc():
                    L.check(lib.fcn_scale_gate_bwd_data_f32(y.ptr, g.ptr, x.ptr, n, ppi, c, c, 0, c, c, 0, 1, st))

                def bwd_gate():
                    L.check(lib.fcn_scale_gate_bwd_gate_f32(y.ptr, x.ptr, g.ptr, n, ppi, c, c, 0, c, 0, c, 0, ws.ptr, st))
                # (launch, tensors it must read or write once)
                cases = [("gate", gate, 2), ("fused", fused, 3), ("gate+sum+relu", three, 2 + 3 + 2)]
                if es == 4:
                    cases += [("bwd_data", bwd_data, 2), ("bwd_data accum", bwd_data_acc, 3), ("bwd_gate", bwd_gate, 2)]
                for kname, fn, tensors in cases:
                    cold, replay = measure(fn)
                    nbytes = tensors * es * pix * c
                    floor = 1e6 * nbytes / HBM
                    out.append(dict(stage=name, N=n, ppi=ppi, C=c, type=tag, launch=kname, cold_us=cold, replay_us=replay, bytes=nbytes, floor_us=floor))
                    print("%-8s %2d %-4s %-16s | %8.1f %9.1f | %9.2f %8.2f %6.1f" % (name, n, tag, kname, cold, replay, nbytes / 1e6, floor, cold / floor),
                          flush=True)
                for d in (x, r, y, m, g, ws):
                    d.free()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
