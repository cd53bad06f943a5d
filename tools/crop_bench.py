#!/usr/bin/env python
"""GPU micro-benchmark: the Crop launches (csrc/crop.hip) at the three crops of FCN-8s on a 500 x 500 image - forward, backward plain
(all of dX: dY inside the window, zeros outside) and backward accumulating (the window only) - and, as the yardstick,
fcn_copy_channels_f32 moving the same number of bytes between two dense buffers.  Events around repeated launches on one stream;
the median of five rounds of `reps` launches each is printed with bytes / time (bytes read + bytes written, pad channels not counted).
Every launch takes the NEXT of several buffer pairs whose total size is above 1 GiB, more than the last-level cache holds: a launch
finds nothing of its own operands left there by the launch before it, whichever variant that was (--resident: one pair, reused).
usage: python tools/crop_bench.py [name ...]   (run on the GPU box)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fcn_object_detector_amd import lib as L  # noqa: E402
from gpu_util import dev_from  # noqa: E402
from tconv_sweep import timed  # noqa: E402

# (name, N, C, H, W, offset, OH, OW): x = (N, C, H, W) -> y = (N, C, OH, OW) at (offset, offset)
SHAPES = [
    ("score_pool4c", 1, 21, 44, 44, 5, 34, 34),
    ("score_pool3c", 1, 21, 88, 88, 9, 70, 70),
    ("score", 1, 21, 568, 568, 31, 500, 500),
    ("score_n8", 8, 21, 568, 568, 31, 500, 500),      # the same crop on a batch of 8: past the launch floor
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
    for name, n, c, h, w, off, oh, ow in SHAPES:
        if want and name not in want:
            continue
        cs = (c + 3) // 4 * 4
        pair_bytes = 4 * n * cs * (h * w + oh * ow)
        pairs = 1 if resident else max(2, min(64, -(-(1 << 30) // pair_bytes) + 1))
        x0 = rng.standard_normal((n, h, w, cs)).astype(np.float32)
        xs = [dev_from(x0) for _ in range(pairs)]
        ys = [dev_from(np.zeros((n, oh, ow, cs), np.float32)) for _ in range(pairs)]
        turn = [0]

        def rotating(call):
            def run():
                i = turn[0] = (turn[0] + 1) % pairs
                call(xs[i], ys[i])
            return run
        args = (n, h, w, c, cs, 0, off, off, oh, ow, cs, 0)
        win, whole = 4.0 * n * oh * ow * c, 4.0 * n * h * w * c
        line = "%-13s N%d %dx%dx%d -> %dx%d, %d pair%s |" % (name, n, c, h, w, oh, ow, pairs, "" if pairs == 1 else "s")
        for label, fn, byts in (
                ("fwd", lambda x, y: L.call("fcn_crop_fwd_f32", x.ptr, y.ptr, *args, st), 2 * win),
                ("bwd", lambda x, y: L.call("fcn_crop_bwd_f32", y.ptr, x.ptr, *args, 0, st), win + whole),
                ("bwd+=", lambda x, y: L.call("fcn_crop_bwd_f32", y.ptr, x.ptr, *args, 1, st), 3 * win),
                # the yardstick moves the bytes of the forward crop: n * oh * ow pixels of c channels, dense to dense
                ("copy_channels", lambda x, y: L.call("fcn_copy_channels_f32", x.ptr, y.ptr, n * oh * ow, c, cs, 0, cs, 0, st), 2 * win)):
            us = timed(rotating(fn), st, e0, e1, reps=50)
            line += " %s %6.1fus %6.1f GB/s |" % (label, us, byts / us / 1e3)
        print(line, flush=True)
        for b in xs + ys:
            b.free()


if __name__ == "__main__":
    main()
