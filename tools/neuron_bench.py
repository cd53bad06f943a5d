#!/usr/bin/env python3
"""Times the forward launches of csrc/neuron.hip beside fcn_act_fwd_* in TanH mode, at one shape (not imported by the package).

The shape is the expand blob of MobileNet-v2's second stage at batch 1: 112 x 112 pixels of 96 channels, in place, whole buffers, in
float32 (4.8 MB) and in halves (2.4 MB).  The method is tools/launch_floor.py's: 10 launches to warm up, then `--reps` launches back to
back between two events of one stream, microseconds each; the median of `--runs` such measurements.  At this size the operands stay in
the Infinity Cache between launches, so the figure is a launch in a warm cache hierarchy, not an HBM figure.  Buffers hold zeros.

    python tools/neuron_bench.py [--reps 200] [--runs 5] [--json out.json]
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

PIX, CH = 112 * 112, 96


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = L.load()
    L.call("fcn_init", 0)
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))
    x, h = DeviceBuffer(4 * PIX * CH), DeviceBuffer(2 * PIX * CH)
    ms = C.c_float()

    def neuron32(mode, p, q):
        return lambda: L.check(lib.fcn_neuron_fwd_f32(x.ptr, x.ptr, None, PIX, CH, CH, 0, CH, 0, 0, mode, p, q, st))

    def neuron16(mode, p, q):
        return lambda: L.check(lib.fcn_neuron_fwd_f16(h.ptr, h.ptr, PIX, CH, CH, 0, CH, 0, mode, p, q, st))
    cases = [("neuron ReLU6 f32", neuron32(L.NEURON_CLIP, 0.0, 6.0), 4), ("neuron Swish f32", neuron32(L.NEURON_SWISH, 1.0, 0.0), 4),
             ("neuron ELU f32", neuron32(L.NEURON_ELU, 1.0, 0.0), 4), ("neuron BNLL f32", neuron32(L.NEURON_BNLL, 0.0, 0.0), 4),
             ("act TanH f32", lambda: L.check(lib.fcn_act_fwd_f32(x.ptr, x.ptr, None, PIX, CH, CH, 0, CH, 0, 0, L.ACT_TANH, None, 0, st)), 4),
             ("neuron ReLU6 f16", neuron16(L.NEURON_CLIP, 0.0, 6.0), 2), ("neuron Swish f16", neuron16(L.NEURON_SWISH, 1.0, 0.0), 2),
             ("act TanH f16", lambda: L.check(lib.fcn_act_fwd_f16(h.ptr, h.ptr, PIX, CH, CH, 0, CH, 0, L.ACT_TANH, None, 0, st)), 2)]
    out = []
    print("%-18s | %9s | %8s" % ("launch", "us each", "MB moved"))
    for name, fn, esize in cases:
        runs = []
        for _ in range(a.runs):
            for _ in range(10):
                fn()
            L.call("fcn_event_record", e0, st)
            for _ in range(a.reps):
                fn()
            L.call("fcn_event_record", e1, st)
            L.call("fcn_event_sync", e1)
            L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
            runs.append(1e3 * ms.value / a.reps)
        us = statistics.median(runs)
        out.append(dict(launch=name, us=us, runs=runs, bytes=2 * esize * PIX * CH))
        print("%-18s | %9.2f | %8.3f   (runs: %s)" % (name, us, 2 * esize * PIX * CH / 1e6, " ".join("%.2f" % r for r in runs)), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
