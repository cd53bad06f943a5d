#!/usr/bin/env python3
"""Times fcn_shuffle_channel_f32 / _f16 (csrc/shuffle.hip) against fcn_copy_channels_f32 / _f16 over a blob of the same bytes - the same
traffic without the permutation (not imported by the package).

Shapes: the blobs a ShuffleNet shuffles at batch 8 - 28 x 28 pixels of 240 channels in 3 groups (v1, stage 2) and 56 x 56 pixels of 48
channels in 2 groups (v2 0.5x, stage 2) - whole buffers, x and y apart, in float32 and in halves.
Cold: a blob of 2.4 - 6 MB stays in the L2 and the Infinity Cache between launches, so every launch takes the next of a ring of (x, y)
pairs whose bytes together exceed `--ring-mb` (default 640: more than twice the 256 MiB Infinity Cache); a pair is touched again only
after the rest of the ring has gone through the caches.  One pass over the ring warms up, then `--reps` launches back to back between
two events of one stream, microseconds each; the copy and the shuffle alternate, `--runs` such measurements each.  Printed per launch:
the median, the spread (max - min) / median of its runs, and the shuffle's median over the copy's.
Warm (--warm as well): the same on one pair, which stays in the caches: what the launch costs beside its neighbours in a net.
$FCN_LIB_PATH names an experiment build (make exp EXP=-DFCN_SHUFFLE_LDS EXPNAME=shuffle_lds EXPSRC=shuffle: the form that stages pixel
rows through LDS).

    python tools/shuffle_bench.py [--reps 200] [--runs 5] [--ring-mb 640] [--warm] [--json out.json]
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

SHAPES = (("28x28x240 g3", 8 * 28 * 28, 240, 3), ("56x56x48 g2", 8 * 56 * 56, 48, 2))


def launches(lib, st, pix, c, g, esize, pairs):
    """(copy, shuffle): each takes the index of the launch and runs on pair index % len(pairs)."""
    k = len(pairs)
    if esize == 4:
        copy = lambda i: L.check(lib.fcn_copy_channels_f32(pairs[i % k][0].ptr, pairs[i % k][1].ptr, pix, c, c, 0, c, 0, st))
        shuf = lambda i: L.check(lib.fcn_shuffle_channel_f32(pairs[i % k][0].ptr, pairs[i % k][1].ptr, pix, c, g, c, 0, c, 0, 0, st))
    else:
        copy = lambda i: L.check(lib.fcn_copy_channels_f16(pairs[i % k][0].ptr, pairs[i % k][1].ptr, pix, c, c, 0, c, 0, st))
        shuf = lambda i: L.check(lib.fcn_shuffle_channel_f16(pairs[i % k][0].ptr, pairs[i % k][1].ptr, pix, c, g, c, 0, c, 0, st))
    return copy, shuf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ring-mb", type=int, default=640)
    ap.add_argument("--warm", action="store_true")
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

    def timed(fn, warmup):
        for i in range(warmup):
            fn(i)
        L.call("fcn_event_record", e0, st)
        for i in range(a.reps):
            fn(i)
        L.call("fcn_event_record", e1, st)
        L.call("fcn_event_sync", e1)
        L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
        return 1e3 * ms.value / a.reps

    out = []
    print("%-28s | %9s | %7s | %8s | %s" % ("launch", "us each", "spread", "TB/s", "runs"))
    for mode in ("cold",) + (("warm",) if a.warm else ()):
        for shape, pix, c, g in SHAPES:
            for esize in (4, 2):
                blob = esize * pix * c
                k = max(-(-a.ring_mb * (1 << 20) // (2 * blob)), 2) if mode == "cold" else 1
                pairs = [(DeviceBuffer(blob), DeviceBuffer(blob)) for _ in range(k)]
                copy, shuf = launches(lib, st, pix, c, g, esize, pairs)
                runs = {"copy": [], "shuffle": []}
                for _ in range(a.runs):      # alternating
                    runs["copy"].append(timed(copy, max(k, 10)))
                    runs["shuffle"].append(timed(shuf, max(k, 10)))
                med = {n: statistics.median(r) for n, r in runs.items()}
                for n in ("copy", "shuffle"):
                    spread = (max(runs[n]) - min(runs[n])) / med[n]
                    name = "%s %s %s %s" % (mode, n, "f32" if esize == 4 else "f16", shape)
                    out.append(dict(launch=name, us=med[n], runs=runs[n], spread=spread, bytes=2 * blob, ring=k))
                    print("%-28s | %9.2f | %6.1f%% | %8.2f | %s" % (name, med[n], 100 * spread, 2 * blob / med[n] / 1e6, " ".join("%.2f" % r for r in runs[n])),
                          flush=True)
                out.append(dict(launch="%s ratio %s %s" % (mode, "f32" if esize == 4 else "f16", shape), ratio=med["shuffle"] / med["copy"]))
                print("%-28s   shuffle / copy = %.3f" % ("", med["shuffle"] / med["copy"]), flush=True)
                for x, y in pairs:
                    x.free()
                    y.free()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
