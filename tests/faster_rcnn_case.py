"""The small Faster R-CNN net of tests/test_gpu_ip_gemm_nets.py, its parameters and its float64 reference - shared with the no-GPU margin
check of tests/test_ip_gemm_faster_rcnn_ref.py, which runs the same reference on the CPU.

models.faster_rcnn_vgg16 at width_div 8, fc_div 32, five classes, a 64 x 96 image (conv5_3 is 4 x 6: 216 anchors, few enough
that a seed exists at which no two neighbours of the score order are closer than the margin), pre / post_nms_topn
200 / 48: fc6 runs over 48 rows of roi_pool5 - past the 32 rows of the weight-streaming InnerProduct kernels - whatever the count is.
The reference is tests/region_net_ref.reference (torch float64 for the body, tests/ref_region64.py for the region stage), told this net's
proposal parameters for the length of the call.  As there, the RPN's score bank is scaled down so that the foreground probabilities
spread over (0, 1) and its box bank halved; the seed is one at which no decision of the NMS, no neighbour of the score order and no bin
edge of the pooling lies within region_cases.MARGIN of its threshold, and at which the NMS keeps fewer boxes than post_nms_topn: the
zero rows behind the count are there, and fc6 multiplies them."""
import functools

import numpy as np

import region_net_ref as N
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from torch_dw_ref import random_params

NET = dict(classes=5, size=(64, 96), width_div=8, fc_div=32, post_nms_topn=48, pre_nms_topn=200)
PROPOSAL = dict(scales=(8, 16, 32), pre_nms_topn=200, post_nms_topn=48)      # (the writer's anchors are the published 8 / 16 / 32)
SEED, SCORE_GAIN, BOX_GAIN = 108, 0.2, 0.5
OUTPUTS = ["cls_prob", "bbox_pred"]
BLOBS = ["conv5_3", "rpn_cls_score", "rpn_bbox_pred", "rpn_cls_prob_reshape", "roi_pool5", "fc6", "fc7", "cls_score", "cls_prob", "bbox_pred"]


def build(seed=SEED):
    """(prototxt text, spec, parameters, {input blob: array})"""
    text = models.faster_rcnn_vgg16(**NET)
    spec = NetSpec(proto.parse_text(text), "TEST", ip_gemm=True)
    spec.infer()
    params = random_params(spec, seed)
    params["rpn_cls_score"][0] *= np.float32(SCORE_GAIN)
    params["rpn_bbox_pred"][0] *= np.float32(BOX_GAIN)
    x = np.random.default_rng(seed + 1).standard_normal(spec.input_shapes["data"]).astype(np.float32)
    return text, spec, params, {"data": x, "im_info": np.array([[NET["size"][0], NET["size"][1], 1.0]], np.float32)}


def reference(spec, params, inputs):
    """region_net_ref.reference with this net's proposal parameters: ({blob: float64 array, ROI-axis blobs cut to the count}, margin,
    count, the Proposal's result).  The two Dropout layers are left out of what it walks: in a TEST-phase net they are the identity on
    their in-place blobs, and the interpreter behind the reference has no such layer."""
    saved = dict(N.RFCN)
    N.RFCN.update(PROPOSAL)
    try:
        return N.reference("faster_rcnn", N._Layers(spec, [l for l in spec.layers if l.type != "Dropout"]), params, inputs)
    finally:
        N.RFCN.clear()
        N.RFCN.update(saved)


@functools.lru_cache(maxsize=None)
def case():
    """The net and its reference, computed once and left unchanged."""
    text, spec, params, inputs = build()
    B, margin, count, prop = reference(spec, params, inputs)
    return dict(text=text, spec=spec, params=params, inputs=inputs, ref=B, margin=margin, count=count, prop=prop)
