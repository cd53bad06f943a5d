#!/usr/bin/env python
"""GPU: where a frame's time goes OUTSIDE the kernels in the bench's headline region (ForwardPipeline.run_io: H2D of the frame, layout
change, all kernels, D2H of the two head blobs, several frames in flight).  For the bench's net at 448x448 and for 3 and 4 frames in
flight it prints, per frame:
  * the host time of Engine.forward_begin() / forward_end() and of every library call inside them (time.perf_counter around each call;
    what is left of begin + end is interpreter time),
  * the idle gap of a replica's stream: one HIP event behind the last D2H of a frame, one in front of the H2D of the next frame on the
    same stream, and the elapsed time between them,
  * lib.HW_QUEUES, which replicas' streams are prioritized (fcn_stream_is_prioritized: a hardware queue that plain streams do not
    share) and the depth calibrate() chose.
Host clocks and HIP events only: this region is never put under a kernel-tracing profiler.
usage: python tools/frame_path.py [--frames N] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fcn_object_detector_amd import lib as L, models, proto  # noqa: E402
from fcn_object_detector_amd.engine import ForwardPipeline  # noqa: E402
from fcn_object_detector_amd.netspec import NetSpec, fill_params  # noqa: E402


class TimedLib:
    """Stands in for the loaded library: every entry point called through it is timed (seconds and calls, by name)."""

    def __init__(self, real):
        self._real = real
        self.seconds = defaultdict(float)
        self.calls = defaultdict(int)
        self._wrapped = {}

    def __getattr__(self, name):
        w = self._wrapped.get(name)
        if w is None:
            fn = getattr(self._real, name)

            def w(*a, _fn=fn, _name=name, _pc=time.perf_counter):
                t0 = _pc()
                r = _fn(*a)
                self.seconds[_name] += _pc() - t0
                self.calls[_name] += 1
                return r
            self._wrapped[name] = w
        return w


def host_times(engines, frames):
    """run_io's loop with the library's calls timed: microseconds per frame in forward_begin / forward_end, split by call."""
    timed = TimedLib(L.load())
    t_begin = t_end = 0.0
    pending = []
    real = L.substitute(timed)
    try:
        for i in range(frames):
            e = engines[i % len(engines)]
            if len(pending) == len(engines):
                t0 = time.perf_counter()
                pending.pop(0).forward_end()
                t_end += time.perf_counter() - t0
            t0 = time.perf_counter()
            e.forward_begin()
            t_begin += time.perf_counter() - t0
            pending.append(e)
        while pending:
            t0 = time.perf_counter()
            pending.pop(0).forward_end()
            t_end += time.perf_counter() - t0
    finally:
        L.substitute(real)
    us = 1e6 / frames
    in_calls = sum(timed.seconds.values())
    waits = timed.seconds.get("fcn_stream_sync", 0.0)
    return {
        "forward_begin_us": round(t_begin * us, 2), "forward_end_us": round(t_end * us, 2),
        "calls": {k: {"us_per_frame": round(timed.seconds[k] * us, 2), "calls_per_frame": round(timed.calls[k] / frames, 2)} for k in sorted(timed.seconds)},
        "in_library_us": round(in_calls * us, 2),
        "of_which_waiting_for_the_stream_us": round(waits * us, 2),
        "interpreter_us": round((t_begin + t_end - in_calls) * us, 2),
    }


def idle_gaps(engines, frames):
    """run_io's loop with two events per frame on the frame's stream: [behind the last D2H of frame i] -> [in front of the H2D of the
    next frame on that stream].  Microseconds; the first frame of every replica has no predecessor."""
    def event():
        e = C.c_void_p()
        L.call("fcn_event_create", C.byref(e))
        return e
    front = [event() for _ in range(frames)]
    behind = [event() for _ in range(frames)]
    pending = []
    t0 = time.perf_counter()
    for i in range(frames):
        e = engines[i % len(engines)]
        if len(pending) == len(engines):
            pending.pop(0).forward_end()
        L.call("fcn_event_record", front[i], e.stream)
        e.forward_begin()
        L.call("fcn_event_record", behind[i], e.stream)
        pending.append(e)
    while pending:
        pending.pop(0).forward_end()
    wall = time.perf_counter() - t0
    gaps, busy = [], []
    ms = C.c_float()
    for i in range(frames):
        L.call("fcn_event_elapsed_ms", front[i], behind[i], C.byref(ms))
        busy.append(ms.value * 1e3)
        if i >= len(engines):
            L.call("fcn_event_elapsed_ms", behind[i - len(engines)], front[i], C.byref(ms))
            gaps.append(ms.value * 1e3)
    for ev in front + behind:
        L.call("fcn_event_destroy", ev)
    gaps = np.array(gaps[len(engines):] or gaps)      # (the first round starts from an empty device)
    return {"idle_gap_us": {"median": round(float(np.median(gaps)), 2), "mean": round(float(gaps.mean()), 2),
                            "p10": round(float(np.percentile(gaps, 10)), 2), "p90": round(float(np.percentile(gaps, 90)), 2)},
            "frame_on_stream_us_median": round(float(np.median(busy)), 2),
            "frames_per_s_with_events": round(frames / wall, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    msg = proto.parse_text(models.googlenet_detectnet_deploy(1, 448, 448, 4))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    pipe = ForwardPipeline(lambda: NetSpec(msg, "TEST"), params=fill_params(spec, seed=1234), device=0, depth=4, max_lds_kb=36)
    x = np.random.default_rng(0).random((1, 3, 448, 448), dtype=np.float32)
    for e in pipe.engines:
        e.host_array("data")[...] = x
        e.upload_inputs()
    pipe.run_resident(20)
    chosen = pipe.calibrate((3, 4))
    prioritized = [bool(getattr(e, "stream_prioritized", False)) for e in pipe.engines]
    out = {"hw_queues": L.HW_QUEUES, "replica_streams_prioritized": prioritized, "calibrate_depth": chosen, "frames": args.frames, "depths": {}}
    for depth in (3, 4):
        engines = pipe.engines[:depth]
        pipe.warm_io(depth)
        pipe.run_io(20, depth)
        rates = [args.frames / pipe.run_io(args.frames, depth) for _ in range(3)]
        res = {"frames_per_s_uninstrumented": round(float(np.median(rates)), 1),
               "kernels_only_frames_per_s": round(args.frames / pipe.run_resident(args.frames, depth), 1)}
        res["host"] = host_times(engines, args.frames)
        res.update(idle_gaps(engines, args.frames))
        out["depths"][str(depth)] = res
        h = res["host"]
        print("depth %d: %.0f frames/s with transfers (%.0f kernels only); per frame: forward_begin %.1f us + forward_end %.1f us on the host = "
              "%.1f us in the library (%.1f us of them waiting for the stream) + %.1f us interpreter; stream idle between frames: median %.1f us "
              "(p10 %.1f, p90 %.1f), busy %.1f us"
              % (depth, res["frames_per_s_uninstrumented"], res["kernels_only_frames_per_s"], h["forward_begin_us"], h["forward_end_us"],
                 h["in_library_us"], h["of_which_waiting_for_the_stream_us"], h["interpreter_us"], res["idle_gap_us"]["median"],
                 res["idle_gap_us"]["p10"], res["idle_gap_us"]["p90"], res["frame_on_stream_us_median"]))
        for k, v in h["calls"].items():
            print("    %-28s %8.2f us/frame  %5.2f calls/frame" % (k, v["us_per_frame"], v["calls_per_frame"]))
    print("hw queues: %s; replica streams prioritized: %s; calibrate() chose depth %d" % (json.dumps(L.HW_QUEUES), prioritized, chosen))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    pipe.close()


if __name__ == "__main__":
    main()
