"""The two region-stage test nets of tests/test_gpu_region_nets.py, their parameters and their float64 reference - shared with the no-GPU
margin check of tests/test_region_ref.py, which runs the same reference on the CPU.

"fast": a Fast-R-CNN-style fragment - a convolution, ROIPooling of rois fed through an Input layer (R = 8, on both images of the batch),
InnerProduct, Softmax.  "rfcn": models.rfcn_resnet(50, width_div=8, size=96, classes=5) with pre / post_nms_topn 60 / 12 and 48 .. 192
pixel anchors (most of them clipped to the 96 x 96 image: boxes that overlap).  The body runs through tests/torch_dw_ref.py layer by
layer, the region stage through tests/ref_region64.py.

Parameters (test inputs): tests/torch_resnet_ref.random_params; the RPN's score bank is scaled down so that the foreground probabilities
spread over (0, 1) without saturating - no two neighbours of the order closer than the margin - and its box bank halved: the NMS keeps
fewer boxes than post_nms_topn and suppresses many (tests/test_region_ref.py asserts both), so the zero rows behind the count are
there.  The margin returned also covers the roundings of PSROIPooling / ROIPooling on the reference's rois: what reaches the poolings
on the device are the float32 net's."""
import numpy as np
import torch

import ref_region64 as R
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from torch_dw_ref import as_torch, random_params, torch_net

FAST = """name: "fast_rcnn_fragment"
layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 3 dim: 24 dim: 32 } } }
layer { name: "rois" type: "Input" top: "rois" input_param { shape { dim: 8 dim: 5 } } }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv" convolution_param { num_output: 10 kernel_size: 3 pad: 1 stride: 2 } }
layer { name: "relu" type: "ReLU" bottom: "conv" top: "conv" }
layer { name: "roi_pool" type: "ROIPooling" bottom: "conv" bottom: "rois" top: "roi_pool" roi_pooling_param { pooled_h: 3 pooled_w: 2 spatial_scale: 0.5 } }
layer { name: "fc" type: "InnerProduct" bottom: "roi_pool" top: "fc" inner_product_param { num_output: 6 } }
layer { name: "prob" type: "Softmax" bottom: "fc" top: "prob" }
"""
FAST_ROIS = np.array([[0, 2.0, 2.0, 21.0, 13.0], [1, 0.0, 0.0, 31.0, 23.0], [1, 9.0, 5.0, 40.0, 30.0], [0, 13.0, 7.0, 13.2, 7.3],
                      [1, -8.0, -6.0, 11.0, 9.0], [0, 4.3, 1.2, 25.8, 20.1], [1, 15.0, 11.0, 27.0, 17.0], [0, 0.0, 6.0, 31.0, 12.0]], np.float32)
RFCN = dict(depth=50, width_div=8, size=96, classes=5, pre_nms_topn=60, post_nms_topn=12, scales=(3, 6, 12))
RFCN_SEED, RFCN_SCORE_GAIN, RFCN_BOX_GAIN = 14, 0.1, 0.5
OUTPUTS = {"fast": ["prob"], "rfcn": ["cls_prob", "bbox_pred"]}


class _Layers:
    """What torch_net reads of a spec, for a run of one layer."""
    def __init__(self, spec, layers):
        self.layers, self.phase, self.blob_shapes = layers, spec.phase, spec.blob_shapes


def build(name):
    """(prototxt text, spec, parameters, {input blob: array}) of a test net."""
    text = FAST if name == "fast" else models.rfcn_resnet(**RFCN)
    spec = NetSpec(proto.parse_text(text), "TEST", depthwise=True)
    spec.infer()
    seed = 31 if name == "fast" else RFCN_SEED
    params = random_params(spec, seed)
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal(spec.input_shapes["data"]).astype(np.float32)
    if name == "fast":
        return text, spec, params, {"data": x, "rois": FAST_ROIS}
    params["rpn_cls_score"][0] *= np.float32(RFCN_SCORE_GAIN)
    params["rpn_bbox_pred"][0] *= np.float32(RFCN_BOX_GAIN)
    return text, spec, params, {"data": x, "im_info": np.array([[96, 96, 1.0]], np.float32)}


def reference(name, spec, params, inputs):
    """({blob: float64 array} with the ROI-axis blobs cut to the count, margin, count, the Proposal's result or None)."""
    P = as_torch(params)
    B = {k: np.asarray(v, np.float64) for k, v in inputs.items()}
    margin, count, prop, cut = np.inf, None, None, set()
    for l in spec.layers:
        t = l.type
        if t == "Input":
            continue
        b0 = B[l.bottoms[0]]
        if t == "Reshape":
            y = b0.reshape(spec.blob_shapes[l.tops[0]])
        elif t == "InnerProduct":
            y = b0.reshape(b0.shape[0], -1) @ np.asarray(params[l.name][0], np.float64).T + np.asarray(params[l.name][1], np.float64)
        elif t == "Softmax" and b0.ndim == 2:
            e = np.exp(b0 - b0.max(axis=1, keepdims=True))
            y = e / e.sum(axis=1, keepdims=True)
        elif t == "Proposal":
            prop = R.proposal(b0, B[l.bottoms[1]], B[l.bottoms[2]], R.anchors(16, (0.5, 1.0, 2.0), RFCN["scales"]), 16, RFCN["pre_nms_topn"],
                              RFCN["post_nms_topn"], 0.7, 16)
            y, count, margin = prop["rois"], prop["count"], min(margin, prop["margin"])
            cut.add(l.tops[0])
        elif t == "ROIPooling":
            p = l.sub("roi_pooling_param")
            y, _arg, m = R.roi_pool(b0, B[l.bottoms[1]], int(p.get("pooled_h")), int(p.get("pooled_w")), float(p.get("spatial_scale")))
            margin = min(margin, m)
        elif t == "PSROIPooling":
            p = l.sub("psroi_pooling_param")
            y, _mag, _largest, m = R.psroi_pool(b0, B[l.bottoms[1]], int(p.get("output_dim")), int(p.get("group_size")), float(p.get("spatial_scale")))
            margin = min(margin, m)
        else:
            with torch.no_grad():
                y = torch_net(_Layers(spec, [l]), P, {b: B[b] for b in l.bottoms})[l.tops[0]].numpy()
        if l.bottoms[1 if t in ("ROIPooling", "PSROIPooling") else 0] in cut:
            cut.add(l.tops[0])
        B[l.tops[0]] = y
    if count is not None:
        for nm in cut:
            B[nm] = B[nm][:count]
    return B, margin, count, prop
