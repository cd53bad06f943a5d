#!/usr/bin/env python
"""GPU micro-benchmark: the Interp launches (csrc/interp.hip) - forward, backward plain and accumulating, and the half-float forward -
at fc8_interp of DeepLab on a 513 and a 321 image (65 -> 513 and 41 -> 321 at 21 channels) and at a pyramid-pooling branch (6 -> 60
at 512 channels).  Beside each, in the same run, fcn_crop_fwd_f32 / fcn_crop_bwd_f32 over the whole extent of two buffers of the
OUTPUT's size: Crop is the project's plain copy of this layout, and moving the same output bytes is the floor an upsampling can reach.
Events around repeated launches on one stream; the median of five rounds of `reps` launches each (tools/tconv_sweep.timed).  Every
launch takes the NEXT of several buffer sets whose total size is above 1 GiB, more than the last-level cache holds: a launch finds
nothing of its own operands left there by the launch before it (--resident: one set, reused).
usage: python tools/interp_bench.py [name ...] [--resident]   (run on the GPU box)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fcn_object_detector_amd import lib as L  # noqa: E402
from gpu_util import dev_from  # noqa: E402
from tconv_sweep import timed  # noqa: E402

# (name, N, C, H, OH): x = (N, C, H, H) -> y = (N, C, OH, OH)
SHAPES = [
    ("fc8_interp_513", 1, 21, 65, 513),
    ("fc8_interp_321", 1, 21, 41, 321),
    ("pyramid_6_60", 1, 512, 6, 60),
    ("fc8_interp_513_n8", 8, 21, 65, 513),      # the same layer on a batch of 8: past the launch floor
]


def main():
    resident = "--resident" in sys.argv[1:]
    want = [a for a in sys.argv[1:] if a != "--resident"] or None
    L.call("fcn_init", 0)
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))
    rng = np.random.default_rng(0)
    for name, n, c, h, oh in SHAPES:
        if want and name not in want:
            continue
        cs, hs = (c + 3) // 4 * 4, (c + 7) // 8 * 8
        set_bytes = 4 * n * cs * (h * h + 2 * oh * oh)
        sets = 1 if resident else max(2, min(64, -(-(1 << 30) // set_bytes) + 1))
        x0 = rng.standard_normal((n, h, h, cs)).astype(np.float32)
        x0h = rng.standard_normal((n, h, h, hs)).astype(np.float16)
        xs = [dev_from(x0) for _ in range(sets)]
        xh = [dev_from(x0h) for _ in range(sets)]
        ys = [dev_from(np.zeros((n, oh, oh, cs), np.float32)) for _ in range(sets)]      # y / dY; as halves it needs half of it
        zs = [dev_from(np.zeros((n, oh, oh, cs), np.float32)) for _ in range(sets)]      # the copy's second buffer
        turn = [0]

        def rotating(call):
            def run():
                turn[0] = (turn[0] + 1) % sets
                call(turn[0])
            return run
        ia = (n, h, h, c, cs, 0, 0, 0, oh, oh, cs, 0)
        ih = (n, h, h, c, hs, 0, 0, 0, oh, oh, hs, 0)
        ca = (n, oh, oh, c, cs, 0, 0, 0, oh, oh, cs, 0)
        small, big = 4.0 * n * h * h * c, 4.0 * n * oh * oh * c
        print("%-18s N%d %dx%dx%d -> %dx%d, %d buffer set%s" % (name, n, c, h, h, oh, oh, sets, "" if sets == 1 else "s"), flush=True)
        for label, fn, byts, ref, ref_fn, ref_byts in (
                ("fwd", lambda i: L.call("fcn_interp_fwd_f32", xs[i].ptr, ys[i].ptr, *ia, st), small + big,
                 "crop_fwd", lambda i: L.call("fcn_crop_fwd_f32", zs[i].ptr, ys[i].ptr, *ca, st), 2 * big),
                ("bwd", lambda i: L.call("fcn_interp_bwd_f32", ys[i].ptr, xs[i].ptr, *ia, 0, st), small + big,
                 "crop_bwd", lambda i: L.call("fcn_crop_bwd_f32", ys[i].ptr, zs[i].ptr, *ca, 0, st), 2 * big),
                ("bwd+=", lambda i: L.call("fcn_interp_bwd_f32", ys[i].ptr, xs[i].ptr, *ia, 1, st), 2 * small + big,
                 "crop_bwd+=", lambda i: L.call("fcn_crop_bwd_f32", ys[i].ptr, zs[i].ptr, *ca, 1, st), 3 * big),
                ("fwd_f16", lambda i: L.call("fcn_interp_fwd_f16", xh[i].ptr, ys[i].ptr, *ih, 0, st), (small + big) / 2,
                 "crop_fwd_f16", lambda i: L.call("fcn_crop_fwd_f16", zs[i].ptr, ys[i].ptr, n, oh, oh, c, hs, 0, 0, 0, oh, oh, hs, 0, st), big)):
            us = timed(rotating(fn), st, e0, e1, reps=50)
            ref_us = timed(rotating(ref_fn), st, e0, e1, reps=50)
            print("  %-8s %8.1f us %7.1f GB/s | %-12s %8.1f us %7.1f GB/s | x%.2f" % (
                label, us, byts / us / 1e3, ref, ref_us, ref_byts / ref_us / 1e3, us / ref_us), flush=True)
        for b in xs + xh + ys + zs:
            b.free()


if __name__ == "__main__":
    main()
