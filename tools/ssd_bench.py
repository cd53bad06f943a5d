#!/usr/bin/env python
"""GPU micro-benchmark: the tail of an SSD deploy net alone (csrc/ssd.hip) at the shapes of MobileNet-SSD (300 x 300: 1917 priors, six
heads, confidence_threshold 0.25, top_k 100, keep_top_k 100) and SSD300-VGG (8732 priors, six heads, 0.01 / 400 / 200), 21 classes, batch 1:
the two gather launches that stand for 24 Permute / Flatten / Concat layers, the row softmax, and DetectionOutput (its four launches) on
synthetic scores with `--cands` candidates per class above the threshold (default 40, a frame with a few objects; 1000 fills every
class's top_k and is the worst case of the NMS sweep).
Events around repeated launches on one stream; the median of five rounds of `reps` launches each (tools/tconv_sweep.timed).  The operands
stay resident: the tail of a net reads what the launches in front of it have just written.
usage: python tools/ssd_bench.py [--cands N]   (run on the GPU box)"""
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

CLASSES = 21
NETS = {   # name -> ((cells per side, priors per cell) per head, confidence_threshold, top_k, keep_top_k)
    "mobilenet_ssd": (((19, 3), (10, 6), (5, 6), (3, 6), (2, 6), (1, 6)), 0.25, 100, 100),
    "ssd300_vgg": (((38, 4), (19, 6), (10, 6), (5, 6), (3, 4), (1, 4)), 0.01, 400, 200),
}


def r4(c):
    return (c + 3) // 4 * 4


def main():
    cands = int(sys.argv[sys.argv.index("--cands") + 1]) if "--cands" in sys.argv else 40
    L.call("fcn_init", 0)
    lib = L.load()
    sp, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))
    st = sp.value
    rng = np.random.default_rng(0)
    for name, (heads, thr, top_k, keep) in NETS.items():
        p = sum(s * s * a for s, a in heads)
        print("%s: %d priors, %d classes, %d candidates per class" % (name, p, CLASSES, min(cands, p)), flush=True)
        keepers = []
        for kind, per in (("loc", 4), ("conf", CLASSES)):
            arr = (L.SsdHead * len(heads))()
            col = 0
            for h, (s, a) in zip(arr, heads):
                c = a * per
                src = dev_from(rng.standard_normal((s * s, r4(c))).astype(np.float32))
                keepers.append(src)
                h.src, h.pixels, h.C, h.cstride, h.coffset, h.dst_col = src.ptr, s * s, c, r4(c), 0, col
                col += s * s * c
            dst = dev_from(np.zeros(r4(col), np.float32))
            us = timed(lambda: L.call("fcn_ssd_gather_f32", arr, len(heads), 1, dst.ptr, r4(col), col, st), st, e0, e1, reps=50)
            print("  gather mbox_%-5s %7.1f us  (%d heads, %d columns, %.2f MB moved)" % (kind, us, len(heads), col, 8.0 * col / 1e6), flush=True)
            keepers.append(dst)
        logits = dev_from(rng.standard_normal((p, CLASSES)).astype(np.float32))
        probs = dev_from(np.zeros((p, CLASSES), np.float32))
        us = timed(lambda: L.call("fcn_softmax_fwd_f32", logits.ptr, probs.ptr, p, CLASSES, CLASSES, CLASSES, st), st, e0, e1, reps=50)
        print("  row softmax       %7.1f us" % us, flush=True)
        # priors on a grid with jitter, scores below the threshold but for `cands` per class
        cxy = rng.uniform(0.05, 0.95, (p, 2))
        wh = rng.uniform(0.05, 0.4, (p, 2))
        priors = np.stack([np.concatenate([cxy - wh / 2, cxy + wh / 2], axis=1).reshape(-1), np.tile([0.1, 0.1, 0.2, 0.2], p)]).astype(np.float32)
        conf = rng.uniform(0, thr * 0.8, (p, CLASSES))
        for c in range(1, CLASSES):
            at = rng.choice(p, min(cands, p), replace=False)
            conf[at, c] = rng.uniform(thr * 1.5, 0.99, at.size)
        par = L.DetOutParams()
        par.N, par.P, par.num_classes, par.background, par.code_type, par.variance_encoded = 1, p, CLASSES, 0, L.CODE_CENTER_SIZE, 0
        par.top_k, par.keep_top_k, par.conf_threshold, par.nms_threshold = top_k, keep, thr, 0.45
        par.loc_rstride, par.conf_rstride, par.capacity = 4 * p, r4(p * CLASSES), keep
        nbytes = int(lib.fcn_detection_output_workspace_bytes(C.byref(par)))
        ld, cd, pd = dev_from(rng.normal(0, 0.3, p * 4).astype(np.float32)), dev_from(conf.astype(np.float32)), dev_from(priors)
        od, ws = dev_from(np.zeros(keep * 7 + 4, np.float32)), dev_from(np.zeros(nbytes, np.uint8))
        us = timed(lambda: L.call("fcn_detection_output_f32", ld.ptr, cd.ptr, pd.ptr, C.byref(par), od.ptr, od.ptr + 28 * keep, ws.ptr, nbytes, st),
                   st, e0, e1, reps=20)
        out = np.empty(keep * 7 + 4, np.float32)
        L.call("fcn_memcpy_d2h_async", out.ctypes.data, od.ptr, out.nbytes, st)
        L.call("fcn_stream_sync", st)
        print("  detection output  %7.1f us  (%d rows out, workspace %.2f MB)" % (us, int(out[keep * 7:keep * 7 + 1].view(np.int32)[0]), nbytes / 1e6), flush=True)
        for b in keepers + [logits, probs, ld, cd, pd, od, ws]:
            b.free()


if __name__ == "__main__":
    main()
