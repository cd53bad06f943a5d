#!/usr/bin/env python3
"""Times the ArgMax launches on the GPU against the Interp launch they replace (not imported by the package).

DeepLab's tail, 21 channels in pixels of 24, 65 x 65 -> 513 x 513, batch 1, both element types.  Per type, in microseconds per launch
from hipEvents around `--reps` launches back to back, `--rounds` times, the three candidates alternating inside every round:
  interp          fcn_interp_fwd_* alone (what the net ended in before; the half form writing float32, a net's output)
  interp+argmax   the unfused pair: that launch (halves out for the half type, as the unfused plan has it) and fcn_argmax_fwd_*
  fused           fcn_interp_argmax_fwd_*: the resampled map is never written
Reported: the median over the rounds and the spread (max - min) of each, so that a difference can be read against the run-to-run
spread of the same launch.  A classifier's rows (64 x 1000, the wave-per-pixel side) and shapes on both sides of the lane / wave
switch follow.  Inputs are seeded noise; the fused labels are compared with the unfused pair's before anything is timed.

    python tools/argmax_bench.py [--reps 1000] [--rounds 7] [--sweep] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402


class Timer:
    def __init__(self, stream):
        self.stream, self.a, self.b = stream, C.c_void_p(), C.c_void_p()
        L.call("fcn_event_create", C.byref(self.a))
        L.call("fcn_event_create", C.byref(self.b))

    def us(self, fn, reps):
        L.call("fcn_event_record", self.a, self.stream)
        for _ in range(reps):
            fn()
        L.call("fcn_event_record", self.b, self.stream)
        L.call("fcn_event_sync", self.b)
        ms = C.c_float()
        L.call("fcn_event_elapsed_ms", self.a, self.b, C.byref(ms))
        return 1e3 * ms.value / reps


def upload(arr):
    d = DeviceBuffer(arr.nbytes, zero=False)
    L.call("fcn_memcpy_h2d_async", d.ptr, arr.ctypes.data, arr.nbytes, None)
    L.call("fcn_device_sync")
    return d


def download(d, shape):
    out = np.empty(shape, np.float32)
    L.call("fcn_memcpy_d2h_async", out.ctypes.data, d.ptr, out.nbytes, None)
    L.call("fcn_device_sync")
    return out


def compare(t, cands, reps, rounds):
    """{name: (median us, spread us)} of the candidates, alternating inside every round."""
    for fn in cands.values():
        fn()
    L.call("fcn_stream_sync", t.stream)
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(t.us(fn, reps))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sweep", action="store_true", help="the plain kernel over channel counts (see the comment in main)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = L.load()
    L.call("fcn_init", 0)
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    t = Timer(st)
    rows = []
    n, c, cs, h, oh = 1, 21, 24, 65, 513
    rng = np.random.default_rng(0)
    print("%-34s %-4s %10s %10s" % ("launch", "type", "median us", "spread us"))
    for half in (False, True):
        dt = np.float16 if half else np.float32
        x = upload(rng.standard_normal((n, h, h, cs)).astype(dt))
        mid32, mid = DeviceBuffer(4 * n * oh * oh * cs), DeviceBuffer((2 if half else 4) * n * oh * oh * cs)
        y0, y1 = DeviceBuffer(4 * n * oh * oh * 4), DeviceBuffer(4 * n * oh * oh * 4)
        if half:
            interp = lambda: L.check(lib.fcn_interp_fwd_f16(x.ptr, mid32.ptr, n, h, h, c, cs, 0, 0, 0, oh, oh, cs, 0, 1, st))
            first = lambda: L.check(lib.fcn_interp_fwd_f16(x.ptr, mid.ptr, n, h, h, c, cs, 0, 0, 0, oh, oh, cs, 0, 0, st))
            second = lambda: L.check(lib.fcn_argmax_fwd_f16(mid.ptr, y0.ptr, n * oh * oh, c, cs, 0, 1, 4, 0, 0, st))
            fused = lambda: L.check(lib.fcn_interp_argmax_fwd_f16(x.ptr, y1.ptr, n, h, h, c, cs, 0, 0, 0, oh, oh, 4, 0, 0, st))
        else:
            interp = lambda: L.check(lib.fcn_interp_fwd_f32(x.ptr, mid32.ptr, n, h, h, c, cs, 0, 0, 0, oh, oh, cs, 0, st))
            first = lambda: L.check(lib.fcn_interp_fwd_f32(x.ptr, mid.ptr, n, h, h, c, cs, 0, 0, 0, oh, oh, cs, 0, st))
            second = lambda: L.check(lib.fcn_argmax_fwd_f32(mid.ptr, y0.ptr, n * oh * oh, c, cs, 0, 1, 4, 0, 0, st))
            fused = lambda: L.check(lib.fcn_interp_argmax_fwd_f32(x.ptr, y1.ptr, n, h, h, c, cs, 0, 0, 0, oh, oh, 4, 0, 0, st))

        def pair():
            first()
            second()
        pair()
        fused()
        L.call("fcn_stream_sync", st)
        a0, a1 = download(y0, (oh * oh, 4))[:, 0], download(y1, (oh * oh, 4))[:, 0]
        differ = int((a0 != a1).sum())
        print("# %s: fused and unfused labels differ at %d of %d pixels%s" % ("f16" if half else "f32", differ, oh * oh,
              " (the unfused half path rounds the blend to a half first)" if half else ""))
        if not half and differ:
            raise SystemExit("float32: the fused launch names other classes than Interp + ArgMax")
        res = compare(t, {"interp": interp, "interp+argmax": pair, "argmax alone": second, "fused": fused}, a.reps, a.rounds)
        for k, (med, spread) in res.items():
            rows.append(dict(case="deeplab tail 21ch 65->513", launch=k, half=half, median_us=med, spread_us=spread))
            print("%-34s %-4s %10.2f %10.2f" % (k, "f16" if half else "f32", med, spread))
        for d in (x, mid32, mid, y0, y1):
            d.free()
    # the plain kernel: a classifier's rows, and both sides of the lane / wave switch at the same pixel count
    P, MC = L.ARGMAX_WAVE_PIXELS, L.ARGMAX_WAVE_MIN_C
    for pixels, ch, k in ((64, 1000, 5), (64, MC - 8, 1), (64, MC, 1), (P, MC, 1), (P + 64, MC, 1), (P, 128, 1), (P + 64, 128, 1), (P + 64, 136, 1)):
        for half in (False, True):
            x = upload(rng.standard_normal((pixels, ch)).astype(np.float16 if half else np.float32))
            y = DeviceBuffer(4 * pixels * 8)
            fn = lib.fcn_argmax_fwd_f16 if half else lib.fcn_argmax_fwd_f32
            res = compare(t, {"argmax": lambda: L.check(fn(x.ptr, y.ptr, pixels, ch, ch, 0, k, 8, 0, 0, st))}, a.reps, a.rounds)
            med, spread = res["argmax"]
            name = "argmax %d x %d top_k %d" % (pixels, ch, k)
            rows.append(dict(case=name, launch="argmax", half=half, median_us=med, spread_us=spread))
            print("%-34s %-4s %10.2f %10.2f" % (name, "f16" if half else "f32", med, spread))
            x.free()
            y.free()
    # --sweep: the plain kernel over channel counts at a segmentation map's and a classifier batch's pixel counts.  Run it against
    # `make exp EXP=-DFCN_EXP_ARGMAX_KERNEL=0 EXPNAME=lane EXPSRC=argmax` and `... =1 EXPNAME=wave ...` (FCN_LIB_PATH) to see where the
    # lane-per-pixel and the wave-per-pixel kernel cross
    for pixels in ((263169, 4096, 64) if a.sweep else ()):
        for ch in (8, 16, 24, 32, 48, 64, 96, 128, 192, 256):
            if pixels * ch > 64 << 20:
                continue
            for half in (False, True):
                x = upload(rng.standard_normal((pixels, ch)).astype(np.float16 if half else np.float32))
                y = DeviceBuffer(4 * pixels * 4)
                fn = lib.fcn_argmax_fwd_f16 if half else lib.fcn_argmax_fwd_f32
                med, spread = compare(t, {"argmax": lambda: L.check(fn(x.ptr, y.ptr, pixels, ch, ch, 0, 1, 4, 0, 0, st))}, a.reps, 3)["argmax"]
                rows.append(dict(case="sweep %d x %d" % (pixels, ch), launch="argmax", half=half, median_us=med, spread_us=spread))
                print("%-34s %-4s %10.2f %10.2f" % ("sweep %d x %d" % (pixels, ch), "f16" if half else "f32", med, spread))
                x.free()
                y.free()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
