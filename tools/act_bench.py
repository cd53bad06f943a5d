#!/usr/bin/env python3
"""Times the activation launches (csrc/act.hip: PReLU, TanH, Bias) on the GPU against their byte floors (not imported by the package).
The method is tools/gate_bench.py's.

At the PReLU shapes of MTCNN's P-Net (models.mtcnn) on a 12 x 12 crop and on a 480 x 640 image, and of ENet's stages (models.enet at
512 x 1024: the initial block and stage 5, stages 1 and 4, stages 2 and 3) at batches 1 and 8: the forward in float32 (in place, as the
nets write it), the same launch with the kept copy a TRAIN engine asks for, the forward in halves, TanH and Bias in float32, the data
gradient and the slope gradient (a launch pair).  Each alone, cold (one call behind a 512 MiB memset that evicts L2 and the Infinity
Cache; median of `--cold` such calls) and replayed (`--reps` calls back to back: at most of these sizes the operands stay in the
Infinity Cache, so a replay is not an HBM figure), in microseconds, with the bytes the call must move at least (every operand's real
channels once; parameters and the workspace are not counted) and the time those bytes take at 6.3 TB/s.  Buffers hold zeros: the
kernels' time does not depend on the values (tanh included: no branch on the value).

    python tools/act_bench.py [--quick] [--cold 5] [--reps 200] [--json out.json]
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

# (name, pixels per image, channels, batches)
SHAPES = [("pnet12 PReLU1", 10 * 10, 10, (1,)), ("pnet12 PReLU2", 3 * 3, 16, (1,)), ("pnet12 PReLU3", 1, 32, (1,)),
          ("pnet480 PReLU1", 478 * 638, 10, (1,)), ("pnet480 PReLU2", 237 * 317, 16, (1,)), ("pnet480 PReLU3", 235 * 315, 32, (1,)),
          ("enet initial/5", 256 * 512, 16, (1, 8)), ("enet stage 1/4", 128 * 256, 64, (1, 8)), ("enet stage 2/3", 64 * 128, 128, (1, 8))]
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
    ap.add_argument("--quick", action="store_true", help="one P-Net and one ENet shape only")
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

    print("%-16s %2s %-22s | %8s %9s | %9s %8s %6s" % ("shape", "N", "launch", "cold us", "replay us", "MB moved", "floor us", "cold/fl"))
    for name, ppi, c, batches in ([SHAPES[3], SHAPES[7]] if a.quick else SHAPES):
        for n in batches:
            pix = n * ppi
            c4, c8 = (c + 3) // 4 * 4, (c + 7) // 8 * 8
            x, y, keep = (DeviceBuffer(max(4 * pix * c4, 16)) for _ in range(3))
            h = DeviceBuffer(max(2 * pix * c8, 16))
            par, dpar = DeviceBuffer(4 * c4), DeviceBuffer(4 * c4)
            ws = DeviceBuffer(max(int(lib.fcn_act_workspace_bytes(pix, c)), 16))

            def fwd(mode, kp=None):
                return lambda: L.check(lib.fcn_act_fwd_f32(x.ptr, x.ptr, kp, pix, c, c4, 0, c4, 0, c4, mode, None if mode == L.ACT_TANH else par.ptr, 0, st))

            def fwd16():
                L.check(lib.fcn_act_fwd_f16(h.ptr, h.ptr, pix, c, c8, 0, c8, 0, L.ACT_PRELU, par.ptr, 0, st))

            def bwd_data():
                L.check(lib.fcn_act_bwd_data_f32(y.ptr, keep.ptr, y.ptr, pix, c, c4, 0, c4, 0, c4, 0, L.ACT_PRELU, par.ptr, 0, 0, st))

            def bwd_param():
                L.check(lib.fcn_act_bwd_param_f32(y.ptr, keep.ptr, dpar.ptr, pix, c, c4, 0, c4, 0, L.ACT_PRELU, 0, ws.ptr, st))
            # (launch, bytes it must move at least: every operand's real channels once)
            cases = [("prelu f32 in place", fwd(L.ACT_PRELU), 2 * 4), ("prelu f32 + keep", fwd(L.ACT_PRELU, keep.ptr), 3 * 4), ("prelu f16 in place", fwd16, 2 * 2),
                     ("tanh f32 in place", fwd(L.ACT_TANH), 2 * 4), ("bias f32 in place", fwd(L.ACT_BIAS), 2 * 4),
                     ("prelu bwd_data in place", bwd_data, 3 * 4), ("prelu bwd_param", bwd_param, 2 * 4)]
            for kname, fn, per_el in cases:
                cold, replay = measure(fn)
                nbytes = per_el * pix * c
                floor = 1e6 * nbytes / HBM
                out.append(dict(shape=name, N=n, ppi=ppi, C=c, launch=kname, cold_us=cold, replay_us=replay, bytes=nbytes, floor_us=floor))
                print("%-16s %2d %-22s | %8.1f %9.1f | %9.3f %8.2f %6.1f" % (name, n, kname, cold, replay, nbytes / 1e6, floor, cold / floor), flush=True)
            for d in (x, y, keep, h, par, dpar, ws):
                d.free()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
