#!/usr/bin/env python3
"""Times launches of the kernels on csrc/chan_group.h, one family per run (not imported by the package).

--family neuron (the default): the forward launches of csrc/neuron.hip beside fcn_act_fwd_* in TanH mode.  The shape is the expand blob of MobileNet-v2's second stage at batch 1: 112 x 112 pixels of 96 channels, in place, whole buffers, in
float32 (4.8 MB) and in halves (2.4 MB).  The method is tools/launch_floor.py's: 10 launches to warm up, then `--reps` launches back to
back between two events of one stream, microseconds each; the median of `--runs` such measurements.  At this size the operands stay in
the Infinity Cache between launches, so the figure is a launch in a warm cache hierarchy, not an HBM figure.  Buffers hold zeros.
--family gate: fcn_scale_gate_fwd_f32 at SE-ResNet's first stage, one image of 56 x 56 pixels of 256 channels (3.2 MB a tensor).
--family batchnorm: fcn_batchnorm_apply_f32 / _f16 (statistics from the save area / the blobs, gamma, beta, ReLU),
fcn_batchnorm_bwd_reduce_f32 and fcn_batchnorm_bwd_apply_f32 (under the ReLU's mask) at ResNet's 56 x 56 x 256.

    python tools/neuron_bench.py [--family neuron|gate|batchnorm] [--reps 200] [--runs 5] [--json out.json]
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
RES_PIX, RES_CH = 56 * 56, 256


def neuron_cases(lib, st):
    x, h = DeviceBuffer(4 * PIX * CH), DeviceBuffer(2 * PIX * CH)

    def neuron32(mode, p, q):
        return lambda: L.check(lib.fcn_neuron_fwd_f32(x.ptr, x.ptr, None, PIX, CH, CH, 0, CH, 0, 0, mode, p, q, st))

    def neuron16(mode, p, q):
        return lambda: L.check(lib.fcn_neuron_fwd_f16(h.ptr, h.ptr, PIX, CH, CH, 0, CH, 0, mode, p, q, st))
    return [("neuron ReLU6 f32", neuron32(L.NEURON_CLIP, 0.0, 6.0), 8 * PIX * CH), ("neuron Swish f32", neuron32(L.NEURON_SWISH, 1.0, 0.0), 8 * PIX * CH),
            ("neuron ELU f32", neuron32(L.NEURON_ELU, 1.0, 0.0), 8 * PIX * CH), ("neuron BNLL f32", neuron32(L.NEURON_BNLL, 0.0, 0.0), 8 * PIX * CH),
            ("act TanH f32", lambda: L.check(lib.fcn_act_fwd_f32(x.ptr, x.ptr, None, PIX, CH, CH, 0, CH, 0, 0, L.ACT_TANH, None, 0, st)), 8 * PIX * CH),
            ("neuron ReLU6 f16", neuron16(L.NEURON_CLIP, 0.0, 6.0), 4 * PIX * CH), ("neuron Swish f16", neuron16(L.NEURON_SWISH, 1.0, 0.0), 4 * PIX * CH),
            ("act TanH f16", lambda: L.check(lib.fcn_act_fwd_f16(h.ptr, h.ptr, PIX, CH, CH, 0, CH, 0, L.ACT_TANH, None, 0, st)), 4 * PIX * CH)]


def gate_cases(lib, st):
    p, c = RES_PIX, RES_CH
    x, y, g = DeviceBuffer(4 * p * c), DeviceBuffer(4 * p * c), DeviceBuffer(4 * c)
    return [("gate fwd f32", lambda: L.check(lib.fcn_scale_gate_fwd_f32(x.ptr, g.ptr, None, y.ptr, 1, p, c, c, 0, c, 0, 0, c, 0, 0, st)), 8 * p * c)]


def batchnorm_cases(lib, st):
    p, c = RES_PIX, RES_CH
    x, y, hat, dx = (DeviceBuffer(4 * p * c) for _ in range(4))
    xh, yh = DeviceBuffer(2 * p * c), DeviceBuffer(2 * p * c)
    save, mean, var, fac, gamma, beta, s0, s1 = (DeviceBuffer(4 * n) for n in (2 * c, c, c, 4, c, c, c, c))
    ws = DeviceBuffer(int(lib.fcn_batchnorm_workspace_bytes(p, c)))
    return [("bn apply f32", lambda: L.check(lib.fcn_batchnorm_apply_f32(
                x.ptr, y.ptr, hat.ptr, p, c, c, 0, c, 0, c, save.ptr, None, None, None, 1e-5, gamma.ptr, beta.ptr, 1, st)), 12 * p * c),
            ("bn apply f16", lambda: L.check(lib.fcn_batchnorm_apply_f16(
                xh.ptr, yh.ptr, p, c, c, 0, c, 0, mean.ptr, var.ptr, fac.ptr, 1e-5, gamma.ptr, beta.ptr, 1, st)), 4 * p * c),
            ("bn bwd reduce f32", lambda: L.check(lib.fcn_batchnorm_bwd_reduce_f32(
                x.ptr, hat.ptr, y.ptr, p, c, c, 0, c, 0, c, 0, s0.ptr, s1.ptr, ws.ptr, st)), 12 * p * c),
            ("bn bwd apply f32", lambda: L.check(lib.fcn_batchnorm_bwd_apply_f32(
                x.ptr, hat.ptr, y.ptr, dx.ptr, p, c, c, 0, c, 0, c, 0, c, 0, save.ptr, None, None, 1e-5, gamma.ptr, s0.ptr, s1.ptr, 0, st)),
             16 * p * c)]


FAMILIES = {"neuron": neuron_cases, "gate": gate_cases, "batchnorm": batchnorm_cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=sorted(FAMILIES), default="neuron")
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
    ms = C.c_float()
    cases = FAMILIES[a.family](lib, st)
    out = []
    print("%-18s | %9s | %8s" % ("launch", "us each", "MB moved"))
    for name, fn, nbytes in cases:
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
        out.append(dict(launch=name, us=us, runs=runs, bytes=nbytes))
        print("%-18s | %9.2f | %8.3f   (runs: %s)" % (name, us, nbytes / 1e6, " ".join("%.2f" % r for r in runs)), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
