"""The region stage of the two-stage detectors (Faster R-CNN, R-FCN): what the parameters of Proposal, ROIPooling and PSROIPooling mean,
the anchors, and the shapes of their tops.

Pure functions of a layer's prototxt message and of blob shapes: nothing here touches the device.  netspec.py infers shapes from them,
storage.py and engine.py plan from them, and the float64 restatement in tests/ref_region64.py is written without reading them.
Every refusal names its layer: ``layer <name>: ...``.
"""
from __future__ import annotations

import ast
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

Shape = Tuple[int, ...]

# layer types of the region stage: no learnable blob, float32 TEST-phase engine only
REGION_TYPES = ("Proposal", "ROIPooling", "PSROIPooling")
# what training the region stage needs: refused by name, with a text that says so
TRAINING_TYPES = ("AnchorTarget", "ProposalTarget")
# python_param (module, layer) of the published deploy files' spelling of Proposal
PYTHON_PROPOSAL = ("rpn.proposal_layer", "ProposalLayer")
# capacity of fcn_proposal_f32 (include/fcnhip.h)
MAX_ANCHORS, MAX_CANDIDATES, MAX_PRE_NMS = 32, 65536, 6144


def is_python_proposal(l) -> bool:
    """A `type: "Python"` layer that names py-faster-rcnn's rpn.proposal_layer.ProposalLayer: the built-in Proposal, no module is imported."""
    if l.type != "Python":
        return False
    p = l.sub("python_param")
    return (str(p.get("module", "")), str(p.get("layer", ""))) == PYTHON_PROPOSAL


@dataclass(frozen=True)
class ProposalParams:
    feat_stride: int
    base_size: int
    min_size: float
    ratios: Tuple[float, ...]
    scales: Tuple[float, ...]
    pre_nms_topn: int
    post_nms_topn: int
    nms_thresh: float


def proposal_params(l) -> ProposalParams:
    """proposal_param of a `type: "Proposal"` layer, or the param_str (a Python dict body: 'feat_stride': 16, 'scales': [..]) of the Python
    spelling; the defaults are py-faster-rcnn's TEST settings."""
    d = dict(feat_stride=16, base_size=16, min_size=16.0, ratio=[0.5, 1.0, 2.0], scale=[8.0, 16.0, 32.0], pre_nms_topn=6000, post_nms_topn=300,
             nms_thresh=0.7)
    if getattr(l, "python_alias", False):
        s = str(l.sub("python_param").get("param_str", "")).strip()
        try:
            given = ast.literal_eval(s if s.startswith("{") else "{" + s + "}") if s else {}
        except (ValueError, SyntaxError):
            raise ValueError("layer %s: ProposalLayer param_str %r is no dictionary body" % (l.name, s)) from None
        for k, v in given.items():
            key = {"scales": "scale", "ratios": "ratio"}.get(k, k)
            if key not in d:
                raise ValueError("layer %s: ProposalLayer param_str names %r (feat_stride, scales, ratios, base_size, min_size, pre_nms_topn, "
                                 "post_nms_topn, nms_thresh)" % (l.name, k))
            d[key] = v
    else:
        p = l.sub("proposal_param")
        for k in ("feat_stride", "base_size", "min_size", "pre_nms_topn", "post_nms_topn", "nms_thresh"):
            if p.get(k) is not None:
                d[k] = p.get(k)
        for k in ("ratio", "scale"):
            if p.getall(k):
                d[k] = p.getall(k)
    out = ProposalParams(int(d["feat_stride"]), int(d["base_size"]), float(d["min_size"]), tuple(float(v) for v in d["ratio"]),
                         tuple(float(v) for v in d["scale"]), int(d["pre_nms_topn"]), int(d["post_nms_topn"]), float(d["nms_thresh"]))
    if out.feat_stride < 1 or out.base_size < 1 or out.min_size < 0 or out.pre_nms_topn < 1 or out.post_nms_topn < 1:
        raise ValueError("layer %s: Proposal with feat_stride %d, base_size %d, min_size %g, pre_nms_topn %d, post_nms_topn %d (all positive, "
                         "min_size not negative)" % (l.name, out.feat_stride, out.base_size, out.min_size, out.pre_nms_topn, out.post_nms_topn))
    if not out.ratios or not out.scales or any(v <= 0 for v in out.ratios + out.scales):
        raise ValueError("layer %s: Proposal needs positive ratios and scales, got %s / %s" % (l.name, list(out.ratios), list(out.scales)))
    return out


def anchors(base_size: int = 16, ratios: Sequence[float] = (0.5, 1.0, 2.0), scales: Sequence[float] = (8.0, 16.0, 32.0)) -> np.ndarray:
    """py-faster-rcnn's generate_anchors: (len(ratios) * len(scales), 4) float64 corners, ratio-major and scale-minor.  The base box is
    [0, 0, base - 1, base - 1]; per ratio r the width is round(sqrt(base^2 / r)) and the height round(width * r) (numpy's round: halves
    to even); per scale the box of that size times the scale about the base box's centre, as centre -+ 0.5 (size - 1)."""
    w = h = float(base_size)
    c = 0.5 * (base_size - 1)
    out: List[List[float]] = []
    for r in ratios:
        ws = float(np.round(np.sqrt(w * h / r)))
        hs = float(np.round(ws * r))
        for s in scales:
            out.append([c - 0.5 * (ws * s - 1), c - 0.5 * (hs * s - 1), c + 0.5 * (ws * s - 1), c + 0.5 * (hs * s - 1)])
    return np.array(out, np.float64)


def proposal_shapes(l, bots: Sequence[Shape]) -> List[Shape]:
    """The tops of a Proposal: rois (post_nms_topn, 5) and, with a second top, scores (post_nms_topn, 1).  Every refusal that needs
    only shapes is made here."""
    p = proposal_params(l)
    a = len(p.ratios) * len(p.scales)
    if len(bots) != 3 or len(bots[0]) != 4 or len(bots[1]) != 4 or not 1 <= len(l.tops) <= 2:
        raise ValueError("layer %s: Proposal takes three bottoms (scores (1, 2A, H, W), box deltas (1, 4A, H, W), im_info (1, 3)) and has one "
                         "or two tops, got %s" % (l.name, list(bots)))
    sc, dl, im = bots
    if sc[0] != 1 or dl[0] != 1:
        raise NotImplementedError("layer %s: Proposal at a batch of %d (one image a forward, as py-faster-rcnn's layer)" % (l.name, sc[0]))
    if sc[1] != 2 * a or dl[1] != 4 * a or sc[2:] != dl[2:] or int(np.prod(im)) != 3:
        raise ValueError("layer %s: Proposal with %d anchors needs scores (1, %d, H, W), deltas (1, %d, H, W) and im_info (1, 3), got %s"
                         % (l.name, a, 2 * a, 4 * a, list(bots)))
    m = sc[2] * sc[3] * a
    if a > MAX_ANCHORS:
        raise NotImplementedError("layer %s: Proposal with %d anchors (the kernel holds at most %d)" % (l.name, a, MAX_ANCHORS))
    if m > MAX_CANDIDATES:
        raise NotImplementedError("layer %s: Proposal over %d candidates (%d x %d x %d anchors): the kernel ranks at most %d"
                                  % (l.name, m, sc[2], sc[3], a, MAX_CANDIDATES))
    if min(p.pre_nms_topn, m) > MAX_PRE_NMS or p.post_nms_topn > MAX_PRE_NMS:
        raise NotImplementedError("layer %s: Proposal with pre_nms_topn %d / post_nms_topn %d over %d candidates: the NMS kernel holds at "
                                  "most %d boxes" % (l.name, p.pre_nms_topn, p.post_nms_topn, m, MAX_PRE_NMS))
    return [(p.post_nms_topn, 5), (p.post_nms_topn, 1)][:len(l.tops)]


@dataclass(frozen=True)
class RoiPoolParams:
    pooled_h: int
    pooled_w: int
    spatial_scale: float


def roi_pool_params(l) -> RoiPoolParams:
    p = l.sub("roi_pooling_param")
    out = RoiPoolParams(int(p.get("pooled_h", 0)), int(p.get("pooled_w", 0)), float(p.get("spatial_scale", 1.0)))
    if out.pooled_h < 1 or out.pooled_w < 1:
        raise ValueError("layer %s: ROIPooling with pooled_h %d, pooled_w %d (both at least 1)" % (l.name, out.pooled_h, out.pooled_w))
    if not out.spatial_scale > 0:
        raise ValueError("layer %s: ROIPooling with spatial_scale %g (must be positive)" % (l.name, out.spatial_scale))
    return out


def _roi_bottoms(l, bots: Sequence[Shape]) -> Tuple[Shape, Shape]:
    if len(bots) != 2 or len(bots[0]) != 4 or len(bots[1]) not in (2, 4) or int(np.prod(bots[1][1:])) != 5 or len(l.tops) != 1:
        raise ValueError("layer %s: %s takes a 4-d feature blob and rois (R, 5) and has one top, got %s" % (l.name, l.type, list(bots)))
    return bots[0], bots[1]


def roi_pool_shape(l, bots: Sequence[Shape]) -> Shape:
    feat, rois = _roi_bottoms(l, bots)
    p = roi_pool_params(l)
    return (rois[0], feat[1], p.pooled_h, p.pooled_w)


@dataclass(frozen=True)
class PsRoiPoolParams:
    output_dim: int
    group_size: int
    spatial_scale: float


def psroi_pool_params(l) -> PsRoiPoolParams:
    p = l.sub("psroi_pooling_param")
    out = PsRoiPoolParams(int(p.get("output_dim", 0)), int(p.get("group_size", 0)), float(p.get("spatial_scale", 0.0)))
    if out.group_size < 1 or out.output_dim < 1:
        raise ValueError("layer %s: PSROIPooling with output_dim %d, group_size %d (both at least 1)" % (l.name, out.output_dim, out.group_size))
    if not out.spatial_scale > 0:
        raise ValueError("layer %s: PSROIPooling with spatial_scale %g (must be positive)" % (l.name, out.spatial_scale))
    return out


def psroi_pool_shape(l, bots: Sequence[Shape]) -> Shape:
    feat, rois = _roi_bottoms(l, bots)
    p = psroi_pool_params(l)
    if feat[1] != p.output_dim * p.group_size ** 2:
        raise ValueError("layer %s: PSROIPooling with output_dim %d and group_size %d needs a bottom of %d channels, %s has %d"
                         % (l.name, p.output_dim, p.group_size, p.output_dim * p.group_size ** 2, l.bottoms[0], feat[1]))
    return (rois[0], p.output_dim, p.group_size, p.group_size)


def rpn_softmax_anchors(first: Shape, mid: Shape, last: Shape) -> Optional[int]:
    """A for the chain Reshape -> Softmax(axis 1) -> Reshape when it is the RPN's: (N, 2A, H, W) -> (N, 2, A * H, W) -> (N, 2A, H, W);
    None for any other three shapes."""
    if len(first) != 4 or len(mid) != 4 or tuple(last) != tuple(first) or first[1] % 2:
        return None
    n, c2, h, w = first
    return c2 // 2 if tuple(mid) == (n, 2, (c2 // 2) * h, w) else None
