"""The SSD detection head (Caffe-SSD, the weiliu89 fork, as remembered): what its layers' parameters mean and the prior boxes.

Pure functions of a layer's prototxt message and of blob shapes: nothing here touches the device.  netspec.py infers shapes from
them, storage.py and engine.py plan from them, and the float64 restatement in tests/ref_ssd64.py is written without reading them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

Shape = Tuple[int, ...]

# layer types of the head that own no learnable blob and run in a TEST-phase float32 engine only
HEAD_TYPES = ("Permute", "Flatten", "Reshape", "PriorBox", "Normalize", "DetectionOutput")
# SSD's training and evaluation layers: refused by name, with a text that says so
TRAINING_TYPES = ("MultiBoxLoss", "AnnotatedData", "DetectionEvaluate", "VideoData")
CODE_CORNER, CODE_CENTER_SIZE = 1, 2            # PriorBoxParameter.CodeType


def permute_order(l, ndim: int) -> Tuple[int, ...]:
    """permute_param.order with the axes it leaves out appended in order, as Caffe does."""
    order = [int(o) for o in l.sub("permute_param").getall("order")]
    if len(set(order)) != len(order) or any(not 0 <= o < ndim for o in order):
        raise ValueError("layer %s: Permute order %s on a %d-d blob (distinct axes below %d)" % (l.name, order, ndim, ndim))
    return tuple(order + [a for a in range(ndim) if a not in order])


def flatten_shape(l, b: Shape) -> Shape:
    p = l.sub("flatten_param")
    axis, end = int(p.get("axis", 1)), int(p.get("end_axis", -1))
    nd = len(b)
    axis, end = axis + (nd if axis < 0 else 0), end + (nd if end < 0 else 0)
    if not 0 <= axis <= end < nd:
        raise ValueError("layer %s: Flatten of axes %d..%d of a %d-d blob" % (l.name, axis, end, nd))
    if axis != 1 or end != nd - 1:
        raise NotImplementedError("layer %s: Flatten of axes %d..%d of a %d-d blob (only axis 1 to the end)" % (l.name, axis, end, nd))
    return tuple(b[:axis]) + (int(np.prod(b[axis:end + 1])),) + tuple(b[end + 1:])


def reshape_shape(l, b: Shape) -> Shape:
    """Caffe's ReshapeLayer over all axes: dim 0 copies the bottom's extent, one dim -1 is inferred."""
    p = l.sub("reshape_param")
    if int(p.get("axis", 0)) != 0 or int(p.get("num_axes", -1)) != -1:
        raise NotImplementedError("layer %s: Reshape with axis %d, num_axes %d (only the whole shape: axis 0, num_axes -1)"
                                  % (l.name, int(p.get("axis", 0)), int(p.get("num_axes", -1))))
    shp = p.get("shape")
    dims = [int(d) for d in shp.getall("dim")] if shp is not None else []
    if not dims:
        raise ValueError("layer %s: Reshape without reshape_param.shape" % l.name)
    out = []
    for i, d in enumerate(dims):
        if d == 0:
            if i >= len(b):
                raise ValueError("layer %s: Reshape dim %d copies an axis the %d-d bottom lacks" % (l.name, i, len(b)))
            d = b[i]
        out.append(d)
    if out.count(-1) > 1 or any(d < -1 or d == 0 for d in out):
        raise ValueError("layer %s: Reshape to %s (positive extents, 0 to copy, at most one -1)" % (l.name, dims))
    total, known = int(np.prod(b)), int(np.prod([d for d in out if d != -1]))
    if -1 in out:
        if known == 0 or total % known:
            raise ValueError("layer %s: Reshape of %s to %s: the -1 has no whole value" % (l.name, tuple(b), dims))
        out[out.index(-1)] = total // known
    elif known != total:
        raise ValueError("layer %s: Reshape of %s (%d elements) to %s (%d)" % (l.name, tuple(b), total, tuple(out), known))
    return tuple(out)


# ---------------------------------------------------------------------- PriorBox
@dataclass(frozen=True)
class PriorBoxParams:
    min_sizes: Tuple[float, ...]
    max_sizes: Tuple[float, ...]
    ratios: Tuple[float, ...]          # expanded: 1 first, then each aspect_ratio and (flip) its reciprocal, near-duplicates dropped
    clip: bool
    variance: Tuple[float, ...]        # one value or four
    img_h: int                         # 0: the data bottom's
    img_w: int
    step_h: float                      # 0: image extent / map extent
    step_w: float
    offset: float

    @property
    def per_cell(self) -> int:
        return len(self.ratios) * len(self.min_sizes) + len(self.max_sizes)


def priorbox_params(l) -> PriorBoxParams:
    p = l.sub("prior_box_param")
    mins = tuple(float(v) for v in p.getall("min_size"))
    maxs = tuple(float(v) for v in p.getall("max_size"))
    if not mins or any(s <= 0 for s in mins):
        raise ValueError("layer %s: PriorBox needs at least one positive min_size, got %s" % (l.name, list(mins)))
    if maxs and len(maxs) != len(mins):
        raise ValueError("layer %s: PriorBox with %d max_size for %d min_size (none, or one per min_size)" % (l.name, len(maxs), len(mins)))
    for s, m in zip(mins, maxs):
        if m <= s:
            raise ValueError("layer %s: PriorBox max_size %g is not above min_size %g" % (l.name, m, s))
    flip = bool(p.get("flip", True))
    ratios: List[float] = [1.0]
    for v in p.getall("aspect_ratio"):
        for ar in ((float(v), 1.0 / float(v)) if flip else (float(v),)):
            if not any(abs(ar - r) < 1e-6 for r in ratios):
                ratios.append(ar)
    var = tuple(float(v) for v in p.getall("variance"))
    if len(var) not in (0, 1, 4):
        raise ValueError("layer %s: PriorBox with %d variance values (none, one or four)" % (l.name, len(var)))
    if any(v <= 0 for v in var):
        raise ValueError("layer %s: PriorBox variances must be positive, got %s" % (l.name, list(var)))

    def pair(both: str, h: str, w: str, cast):
        vb, vh, vw = p.get(both), p.get(h), p.get(w)
        if vb is not None and (vh is not None or vw is not None):
            raise ValueError("layer %s: PriorBox with both %s and %s / %s (one form or the other)" % (l.name, both, h, w))
        if (vh is None) != (vw is None):
            raise ValueError("layer %s: PriorBox with one of %s / %s alone (both or neither)" % (l.name, h, w))
        out = (cast(vb), cast(vb)) if vb is not None else (cast(vh), cast(vw)) if vh is not None else (cast(0), cast(0))
        if min(out) < 0 or (vb is not None or vh is not None) and min(out) <= 0:
            raise ValueError("layer %s: PriorBox %s must be positive, got %s" % (l.name, both, out))
        return out

    img_h, img_w = pair("img_size", "img_h", "img_w", int)
    step_h, step_w = pair("step", "step_h", "step_w", float)
    return PriorBoxParams(mins, maxs, tuple(ratios), bool(p.get("clip", False)), var or (0.1,), img_h, img_w, step_h, step_w,
                          float(p.get("offset", 0.5)))


def prior_boxes(pp: PriorBoxParams, fh: int, fw: int, data_h: int, data_w: int) -> np.ndarray:
    """The top of a PriorBox layer over an fh x fw map of a data_h x data_w image: float32 (1, 2, fh * fw * A * 4).  Channel 0: per cell
    (rows first) and prior the corners xmin, ymin, xmax, ymax as fractions of the image; channel 1: the variances, four per prior.
    Per cell and min_size s: the s x s box, with a max_size m the sqrt(s m) square, then per expanded ratio ar != 1 the box
    s sqrt(ar) x s / sqrt(ar).  Computed in float32 the way the layer does (a float centre, float half extents)."""
    f = np.float32
    ih, iw = (pp.img_h, pp.img_w) if pp.img_h else (data_h, data_w)
    sh, sw = (f(pp.step_h), f(pp.step_w)) if pp.step_h else (f(ih) / f(fh), f(iw) / f(fw))
    half: List[Tuple[np.float32, np.float32]] = []       # (half width, half height) per prior of a cell
    for i, s in enumerate(pp.min_sizes):
        half.append((f(s) / f(2), f(s) / f(2)))
        if pp.max_sizes:
            q = f(math.sqrt(f(s) * f(pp.max_sizes[i])))
            half.append((q / f(2), q / f(2)))
        for ar in pp.ratios:
            if abs(ar - 1.0) < 1e-6:
                continue
            r = f(math.sqrt(f(ar)))
            half.append((f(s) * r / f(2), f(s) / r / f(2)))
    hw = np.array(half, f)                                                   # (A, 2)
    cx = (np.arange(fw, dtype=f) + f(pp.offset)) * sw                        # (fw,)
    cy = (np.arange(fh, dtype=f) + f(pp.offset)) * sh
    boxes = np.empty((fh, fw, len(half), 4), f)
    boxes[..., 0] = (cx[None, :, None] - hw[None, None, :, 0]) / f(iw)
    boxes[..., 1] = (cy[:, None, None] - hw[None, None, :, 1]) / f(ih)
    boxes[..., 2] = (cx[None, :, None] + hw[None, None, :, 0]) / f(iw)
    boxes[..., 3] = (cy[:, None, None] + hw[None, None, :, 1]) / f(ih)
    if pp.clip:
        np.clip(boxes, 0.0, 1.0, out=boxes)
    out = np.empty((1, 2, boxes.size), f)
    out[0, 0] = boxes.reshape(-1)
    out[0, 1] = np.tile(np.array(pp.variance if len(pp.variance) == 4 else pp.variance * 4, f), boxes.size // 4)
    return out


# ---------------------------------------------------------------------- DetectionOutput
@dataclass(frozen=True)
class DetectionParams:
    num_classes: int
    background: int
    nms_threshold: float
    top_k: int
    code_type: int
    variance_encoded: bool
    keep_top_k: int
    confidence_threshold: float

    @property
    def keep(self) -> int:
        """Rows per image that the top can hold: keep_top_k, or every class's top_k survivors."""
        return self.keep_top_k if self.keep_top_k > -1 else (self.num_classes - 1) * self.top_k


def detection_params(l) -> DetectionParams:
    p = l.sub("detection_output_param")
    if p.get("num_classes") is None or int(p.get("num_classes")) < 1:
        raise ValueError("layer %s: DetectionOutput needs num_classes >= 1" % l.name)
    if not bool(p.get("share_location", True)):
        raise NotImplementedError("layer %s: DetectionOutput with share_location: false (one box set per class)" % l.name)
    nms = p.get("nms_param")
    nms_thr = float(nms.get("nms_threshold", 0.3)) if nms is not None else 0.3
    top_k = int(nms.get("top_k", -1)) if nms is not None else -1
    eta = float(nms.get("eta", 1.0)) if nms is not None else 1.0
    if eta != 1.0:
        raise NotImplementedError("layer %s: DetectionOutput with nms_param.eta %g (adaptive NMS; only eta 1.0)" % (l.name, eta))
    code = str(p.get("code_type", "CORNER"))
    if code not in ("CORNER", "CENTER_SIZE"):
        raise NotImplementedError("layer %s: DetectionOutput with code_type %s (CORNER and CENTER_SIZE only)" % (l.name, code))
    so = p.get("save_output_param")
    if so is not None and str(so.get("output_directory", "")) != "":
        raise NotImplementedError("layer %s: DetectionOutput with save_output_param.output_directory %r (this runtime writes no files)"
                                  % (l.name, str(so.get("output_directory"))))
    keep_top_k = int(p.get("keep_top_k", -1))
    if keep_top_k == -1 and top_k == -1:
        raise NotImplementedError("layer %s: DetectionOutput with neither keep_top_k nor nms_param.top_k (the top's capacity is "
                                  "unbounded)" % l.name)
    if top_k == 0 or top_k < -1 or keep_top_k == 0 or keep_top_k < -1:
        raise ValueError("layer %s: DetectionOutput top_k %d / keep_top_k %d (positive, or -1 for no cut)" % (l.name, top_k, keep_top_k))
    conf = p.get("confidence_threshold")
    return DetectionParams(int(p.get("num_classes")), int(p.get("background_label_id", 0)), nms_thr, top_k,
                           CODE_CORNER if code == "CORNER" else CODE_CENTER_SIZE, bool(p.get("variance_encoded_in_target", False)),
                           keep_top_k, float(conf) if conf is not None else -float(np.finfo(np.float32).max))


def detection_shapes(l, bots: Sequence[Shape]) -> Tuple[Shape, int]:
    """(shape of the top at capacity, number of priors) of a DetectionOutput over loc (N, P*4), conf (N, P*classes), priors (1, 2, P*4)."""
    dp = detection_params(l)
    if len(bots) != 3 or len(bots[0]) != 2 or len(bots[1]) != 2 or len(bots[2]) != 3 or bots[2][:2] != (1, 2):
        raise ValueError("layer %s: DetectionOutput takes loc (N, P*4), conf (N, P*classes) and priors (1, 2, P*4), got %s" % (l.name, list(bots)))
    loc, conf, pri = bots
    if loc[1] % 4 or pri[2] != loc[1] or loc[0] != conf[0]:
        raise ValueError("layer %s: DetectionOutput bottoms disagree: loc %s, priors %s, conf %s (one P, one batch)" % (l.name, loc, pri, conf))
    priors = loc[1] // 4
    if conf[1] != priors * dp.num_classes:
        raise ValueError("layer %s: DetectionOutput conf %s is not %d priors x %d classes wide" % (l.name, conf, priors, dp.num_classes))
    if not 0 <= dp.background < dp.num_classes and dp.background != -1:
        raise ValueError("layer %s: background_label_id %d is outside the %d classes" % (l.name, dp.background, dp.num_classes))
    return (1, 1, loc[0] * dp.keep, 7), priors


def compose_detections(raw_rows: np.ndarray, count: int, batch: int) -> np.ndarray:
    """Caffe's top from the device's rows: (1, 1, K, 7), or with K == 0 the (1, 1, batch, 7) block of -1 with the image index in
    column 0 (what the CPU layer emits when nothing is detected)."""
    if count > 0:
        return np.array(raw_rows[:count * 7], np.float32).reshape(1, 1, count, 7)
    out = np.full((1, 1, batch, 7), -1.0, np.float32)
    out[0, 0, :, 0] = np.arange(batch, dtype=np.float32)
    return out
