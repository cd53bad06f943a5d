#!/usr/bin/env python
"""GPU micro-benchmark: the region stage of an R-FCN deploy net alone (csrc/region.hip), batch 1: the RPN softmax and Proposal (its four
launches) at the ResNet-101 R-FCN shape (600 x 1000 image: 38 x 63 map, 9 anchors, 21546 candidates, pre / post_nms_topN 6000 / 300) and at
the small shape of the tests (5 x 7 map, 100 / 20), then PSROIPooling (21 x 49 and 8 x 49 channels, group 7) and ROIPooling (1024 channels,
7 x 7) over 300 ROIs of the 38 x 63 map.
The inputs are the cases of tests/region_cases.py (scores 1e-3 apart in random places, deltas of small spread: neighbouring anchors
decode to boxes that overlap, so the sweep has rows to or in); the ROIs of the poolings are the rows that Proposal has just written.
Events around repeated launches on one stream; the median of five rounds of `reps` launches each (tools/tconv_sweep.timed).  The operands
stay resident: the stage reads what the launches in front of it have just written.
usage: python tools/region_bench.py   (run on the GPU box)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import region_cases as RC  # noqa: E402
from fcn_object_detector_amd import lib as L  # noqa: E402
from gpu_util import dev_from, nhwc  # noqa: E402
from tconv_sweep import timed  # noqa: E402


def r4(c):
    return (c + 3) // 4 * 4


def main():
    L.call("fcn_init", 0)
    lib = L.load()
    sp, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))
    st = sp.value
    rng = np.random.default_rng(0)
    rois_full = None
    for name in ("rfcn_full", "m5x7"):
        c, base, scores, deltas, im_info = RC.proposal_inputs(name)
        a, h, w, post = len(base), c["H"], c["W"], c["post"]
        print("%s: %d x %d map, %d anchors, %d candidates, pre / post_nms_topN %d / %d" % (name, h, w, a, h * w * a, c["pre"], post), flush=True)
        s_cs, d_cs = r4(2 * a), r4(4 * a)
        xd, yd = dev_from(nhwc(scores, s_cs)), dev_from(np.zeros((h * w, s_cs), np.float32))
        us = timed(lambda: L.call("fcn_pair_softmax_f32", xd.ptr, yd.ptr, h * w, a, s_cs, 0, s_cs, 0, st), st, e0, e1, reps=50)
        print("  rpn softmax       %7.1f us" % us, flush=True)
        par = L.ProposalParams()
        par.H, par.W, par.A, par.feat_stride, par.pre_nms_topn, par.post_nms_topn = h, w, a, RC.FEAT_STRIDE, c["pre"], post
        par.min_size, par.nms_thresh, par.score_cstride, par.delta_cstride, par.rois_cstride = c["min_size"], c["nms"], s_cs, d_cs, 8
        for i, v in enumerate(np.asarray(base, np.float32).reshape(-1)):
            par.anchors[i] = v
        nbytes = int(lib.fcn_proposal_workspace_bytes(C.byref(par)))
        dd, imd = dev_from(nhwc(deltas, d_cs)), dev_from(im_info)
        rd, cd, ws = dev_from(np.zeros((post, 8), np.float32)), dev_from(np.zeros(4, np.int32)), dev_from(np.zeros(nbytes, np.uint8))
        us = timed(lambda: L.call("fcn_proposal_f32", xd.ptr, dd.ptr, imd.ptr, C.byref(par), rd.ptr, None, cd.ptr, ws.ptr, nbytes, st), st, e0, e1, reps=20)
        cnt = np.empty(4, np.int32)
        L.call("fcn_memcpy_d2h_async", cnt.ctypes.data, cd.ptr, 16, st)
        L.call("fcn_stream_sync", st)
        print("  proposal          %7.1f us  (%d rows out, workspace %.2f MB)" % (us, int(cnt[0]), nbytes / 1e6), flush=True)
        if name == "rfcn_full":
            rois_full = rd
        for b in (xd, yd, dd, imd, cd, ws) + (() if name == "rfcn_full" else (rd,)):
            b.free()
    h, w, r = 38, 63, 300
    for od in (21, 8):
        ch = od * 49
        fd, od_y = dev_from(rng.standard_normal((h * w, r4(ch))).astype(np.float32)), dev_from(np.zeros((r * 49, r4(od)), np.float32))
        us = timed(lambda: L.call("fcn_psroi_pool_fwd_f32", fd.ptr, rois_full.ptr, od_y.ptr, 1, h, w, ch, r4(ch), 0, r, 8, 0, od, 7, 0.0625, r4(od), 0, st),
                   st, e0, e1, reps=50)
        print("  psroi pooling     %7.1f us  (%d ROIs, output_dim %d, group 7, %.2f MB of features)" % (us, r, od, 4.0 * h * w * ch / 1e6), flush=True)
        fd.free()
        od_y.free()
    ch = 1024
    fd, py = dev_from(rng.standard_normal((h * w, ch)).astype(np.float32)), dev_from(np.zeros((r * 49, ch), np.float32))
    us = timed(lambda: L.call("fcn_roi_pool_fwd_f32", fd.ptr, rois_full.ptr, py.ptr, None, 1, h, w, ch, ch, 0, r, 8, 0, 7, 7, 0.0625, ch, 0, st), st, e0, e1, reps=20)
    print("  roi pooling       %7.1f us  (%d ROIs, %d channels, 7 x 7, %.1f MB written)" % (us, r, ch, 4.0 * r * 49 * ch / 1e6), flush=True)
    for b in (fd, py, rois_full):
        b.free()


if __name__ == "__main__":
    main()
