#!/usr/bin/env python
"""GPU micro-benchmark: the Upsample launches (csrc/unpool.hip) on a SegNet decoder shape - batch 1, 64 channels, 180 x 240 unpooled to
360 x 480 by the indices of a 2 x 2 / stride 2 pooling - forward in float32 and in halves, backward plain and accumulating.  Beside
each time, its ratio to the byte floor bytes(x + idx + y) / HBM bandwidth at the 8.0 TB/s of the data sheet and at the 6.29 TB/s a
float4 copy reaches on this part.
Events around repeated launches on one stream; the median of five rounds of `reps` launches each (tools/tconv_sweep.timed).  Every
launch takes the NEXT of several buffer sets whose total size is above 1 GiB, more than the last-level cache holds: a launch finds
nothing of its own operands left there by the launch before it (--resident: one set, reused).
usage: python tools/unpool_bench.py [--resident]   (run on the GPU box)"""
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

N, CH, PH, PW, H, W = 1, 64, 180, 240, 360, 480
SPEC_TBS, COPY_TBS = 8.0, 6.29


def main():
    resident = "--resident" in sys.argv[1:]
    L.call("fcn_init", 0)
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))
    rng = np.random.default_rng(0)
    # the argmax of a 2 x 2 / 2 pooling over noise: one pixel of every window, uniformly
    dy_, dx_ = rng.integers(0, 2, (N, PH, PW, CH)), rng.integers(0, 2, (N, PH, PW, CH))
    idx0 = ((2 * np.arange(PH)[None, :, None, None] + dy_) * W + 2 * np.arange(PW)[None, None, :, None] + dx_).astype(np.int32)
    small, big = N * PH * PW * CH, N * H * W * CH
    set_bytes = 4 * (2 * small + big)
    sets = 1 if resident else max(2, min(64, -(-(1 << 30) // set_bytes) + 1))
    x0 = rng.standard_normal((N, PH, PW, CH)).astype(np.float32)
    xs = [dev_from(x0) for _ in range(sets)]
    xh = [dev_from(x0.astype(np.float16)) for _ in range(sets)]
    ids = [dev_from(idx0) for _ in range(sets)]
    ys = [dev_from(np.zeros((N, H, W, CH), np.float32)) for _ in range(sets)]      # y / dY; as halves it needs half of it
    turn = [0]

    def rotating(call):
        def run():
            turn[0] = (turn[0] + 1) % sets
            call(turn[0])
        return run
    geo = (N, PH, PW, CH, CH, 0, 2, 2, 0, H, W, CH, 0)
    print("unpool N%d %dx%dx%d -> %dx%d, %d buffer set%s" % (N, CH, PH, PW, H, W, sets, "" if sets == 1 else "s"), flush=True)
    for label, fn, byts in (
            ("fwd_f32", lambda i: L.call("fcn_unpool_fwd_f32", xs[i].ptr, ids[i].ptr, ys[i].ptr, *geo, st), 4.0 * small + 4.0 * small + 4.0 * big),
            ("fwd_f16", lambda i: L.call("fcn_unpool_fwd_f16", xh[i].ptr, ids[i].ptr, ys[i].ptr, *geo, 0, st), 2.0 * small + 4.0 * small + 2.0 * big),
            ("fwd_f16_out_f32", lambda i: L.call("fcn_unpool_fwd_f16", xh[i].ptr, ids[i].ptr, ys[i].ptr, *geo, 1, st), 2.0 * small + 4.0 * small + 4.0 * big),
            ("bwd", lambda i: L.call("fcn_unpool_bwd_f32", ys[i].ptr, ids[i].ptr, xs[i].ptr, *geo, 0, st), 4.0 * small * 3),
            ("bwd+=", lambda i: L.call("fcn_unpool_bwd_f32", ys[i].ptr, ids[i].ptr, xs[i].ptr, *geo, 1, st), 4.0 * small * 4)):
        us = timed(rotating(fn), st, e0, e1, reps=50)
        print("  %-16s %8.1f us  %6.1f MB  %7.1f GB/s | x%.2f of the floor at %.1f TB/s, x%.2f at %.2f TB/s" % (
            label, us, byts / 1e6, byts / us / 1e3, us / (byts / SPEC_TBS / 1e6), SPEC_TBS, us / (byts / COPY_TBS / 1e6), COPY_TBS), flush=True)
    for b in xs + xh + ids + ys:
        b.free()


if __name__ == "__main__":
    main()
