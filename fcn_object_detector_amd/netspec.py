"""Network description: layers, blob shapes and parameter fillers from a Caffe prototxt.

This is the host-side "program" the HIP engine executes — the reference's
models/*.prototxt and train/**/*.prototxt are consumed unmodified (reference:
scripts/fcn_object_detector.py:317 ``caffe.Net(proto, weights, caffe.TEST)``).
Shape rules follow the public Caffe layer definitions (conv: floor, pooling:
ceil with the last-window clip, deconvolution: s(H-1)+k-2p).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import proto, region, ssd
from .lib import NEURON_MODES

Shape = Tuple[int, ...]


class Layer:
    __slots__ = ("name", "type", "bottoms", "tops", "msg", "lr_mult", "decay_mult", "loss_weight", "python_alias", "axpy")

    def __init__(self, msg: proto.Msg):
        self.msg = msg
        self.name: str = str(msg.get("name", ""))
        self.type: str = str(msg.get("type", ""))
        self.bottoms: List[str] = [str(b) for b in msg.getall("bottom")]
        self.tops: List[str] = [str(t) for t in msg.getall("top")]
        params = msg.getall("param")
        self.lr_mult = [float(p.get("lr_mult", 1.0)) for p in params]
        self.decay_mult = [float(p.get("decay_mult", 1.0)) for p in params]
        self.loss_weight = [float(w) for w in msg.getall("loss_weight")]
        # the published Faster R-CNN / R-FCN deploy files write Proposal as a Python layer (rpn.proposal_layer.ProposalLayer): the same
        # built-in layer, its parameters in param_str; no module is imported.  Every other Python layer stays a Python layer
        self.python_alias: bool = region.is_python_proposal(self)
        self.axpy: Optional[str] = None      # the Axpy layer of the file this layer stands for (NetSpec scale_gate=True), else None
        if self.python_alias:
            self.type = "Proposal"
        # the ShuffleNet ports (and several MobileNet ones) spell the depthwise layer ConvolutionDepthwise: the same layer, the same
        # convolution_param
        if self.type == "ConvolutionDepthwise":
            self.type = "DepthwiseConvolution"

    def sub(self, key: str) -> proto.Msg:
        m = self.msg.get(key)
        return m if m is not None else proto.Msg()

    def __repr__(self) -> str:
        return "Layer(%s:%s %s->%s)" % (self.type, self.name, self.bottoms, self.tops)


def _phase_included(msg: proto.Msg, phase: str) -> bool:
    inc = msg.getall("include")
    if inc:
        return any(str(m.get("phase", phase)) == phase for m in inc)
    exc = msg.getall("exclude")
    if exc:
        return not any(str(m.get("phase", "")) == phase for m in exc)
    return True


def _axis_pair(p: proto.Msg, what: str, both: str, h: str, w: str, default: Optional[int], least: int) -> Tuple[int, int]:
    """One of Caffe's either/or geometry fields as (h, w): `both` once (both axes) or twice ((h, w), the way Caffe repeats it), or `h`
    AND `w`; `default` when nothing is written (None: the field is required)."""
    vals, vh, vw = p.getall(both), p.getall(h), p.getall(w)
    if vals and (vh or vw):
        raise ValueError("%s: both %s and %s / %s are given (one form or the other)" % (what, both, h, w))
    if bool(vh) != bool(vw):
        raise ValueError("%s: %s without %s (both or neither)" % ((what, h, w) if vh else (what, w, h)))
    if len(vals) > 2 or len(vh) > 1 or len(vw) > 1:
        raise ValueError("%s: %s given %d times (once, or twice as (h, w))" % (what, both if vals else h if len(vh) > 1 else w,
                                                                              max(len(vals), len(vh), len(vw))))
    if vh:
        out = (int(vh[0]), int(vw[0]))
    elif vals:
        out = (int(vals[0]), int(vals[-1]))
    elif default is None:
        raise ValueError("%s without %s" % (what, both))
    else:
        out = (default, default)
    if min(out) < least:
        raise ValueError("%s: %s %s is below %d" % (what, both, "x".join(str(v) for v in out), least))
    return out


def _geometry(p: proto.Msg, what: str) -> Tuple[int, int, int, int, int, int]:
    kh, kw = _axis_pair(p, what, "kernel_size", "kernel_h", "kernel_w", None, 1)
    sh, sw = _axis_pair(p, what, "stride", "stride_h", "stride_w", 1, 1)
    ph, pw = _axis_pair(p, what, "pad", "pad_h", "pad_w", 0, 0)
    return kh, kw, sh, sw, ph, pw


def layer_geometry(l: "Layer") -> Tuple[int, int, int, int, int, int]:
    """(kh, kw, sh, sw, ph, pw) of a Convolution / Deconvolution / Pooling layer by Caffe's rules: the kernel is kernel_size or
    kernel_h AND kernel_w, the stride is stride or stride_h / stride_w (default 1), the pad is pad or pad_h / pad_w (default 0);
    kernel_size / stride / pad written twice mean (h, w).  Both forms of one field, one of an _h / _w pair alone, any other count,
    a kernel or stride below 1 and a pad below 0 are ValueErrors that name the layer."""
    return _geometry(l.sub("pooling_param" if l.type == "Pooling" else "convolution_param"), "layer %s" % l.name)


def is_rectangular(l: "Layer") -> bool:
    """The two spatial axes of the layer differ in kernel extent, stride or pad."""
    kh, kw, sh, sw, ph, pw = layer_geometry(l)
    return (kh, sh, ph) != (kw, sw, pw)


def kernel_stride_pad(p: proto.Msg) -> Tuple[int, int, int]:
    """(kernel, stride, pad) of a layer whose two spatial axes agree, however it is written; a layer whose axes differ has no such
    answer (layer_geometry gives the per-axis values)."""
    kh, kw, sh, sw, ph, pw = _geometry(p, "layer")
    if (kh, sh, ph) != (kw, sw, pw):
        raise NotImplementedError("kernel %dx%d stride %dx%d pad %dx%d: the axes differ (netspec.layer_geometry has the per-axis values)"
                                  % (kh, kw, sh, sw, ph, pw))
    return kh, sh, ph


def layer_dilation(l: "Layer") -> int:
    """convolution_param.dilation of a Convolution / Deconvolution: absent = 1, one value, or two equal ones (both spatial axes);
    anything else is refused by layer name, and so is a dilated Deconvolution."""
    vals = [int(v) for v in l.sub("convolution_param").getall("dilation")]
    if len(vals) > 2 or len(set(vals)) > 1:
        raise NotImplementedError("layer %s: dilation %s (one value, or the same value for both spatial axes)" % (l.name, vals))
    d = vals[0] if vals else 1
    if d < 1:
        raise ValueError("layer %s: dilation %d is below 1" % (l.name, d))
    if d > 1 and l.type == "Deconvolution":
        raise NotImplementedError("layer %s: Deconvolution with dilation %d (dilation is supported for Convolution only)" % (l.name, d))
    return d


def _square(l: "Layer") -> Tuple[int, int, int]:
    """(kernel, stride, pad) of a Pooling / Deconvolution layer; one whose axes differ is refused by layer name (rectangular
    windows are supported for Convolution only)."""
    kh, kw, sh, sw, ph, pw = layer_geometry(l)
    if (kh, sh, ph) != (kw, sw, pw):
        raise NotImplementedError("layer %s: %s with kernel %dx%d stride %dx%d pad %dx%d (axes that differ are supported for Convolution only)"
                                  % (l.name, l.type, kh, kw, sh, sw, ph, pw))
    return kh, sh, ph


def conv_out(h: int, k: int, s: int, p: int, d: int = 1) -> int:
    return (h + 2 * p - (d * (k - 1) + 1)) // s + 1


def pool_out(h: int, k: int, s: int, p: int) -> int:
    o = int(math.ceil((h + 2 * p - k) / float(s))) + 1
    if p > 0 and (o - 1) * s >= h + p:
        o -= 1
    return o


def deconv_out(h: int, k: int, s: int, p: int) -> int:
    return s * (h - 1) + k - 2 * p


def crop_window(l: "Layer", b0: Shape, b1: Shape) -> Tuple[Shape, Tuple[int, ...]]:
    """Caffe's CropLayer: (shape of the top, offset into bottom 0 per axis).  Axes before crop_param.axis (default 2, negative counts
    from the end) keep bottom 0's extent, axes from it on take bottom 1's; no offset means 0, one offset applies to every cropped
    axis, otherwise exactly one per cropped axis.  Bottom 1 only lends its shape."""
    cp = l.sub("crop_param")
    if len(b0) != 4 or len(b1) != 4:
        raise ValueError("layer %s: Crop takes two 4-d blobs, got %s and %s" % (l.name, b0, b1))
    axis = int(cp.get("axis", 2))
    if not -4 <= axis < 4:
        raise ValueError("layer %s: crop axis %d is outside [-4, 4)" % (l.name, axis))
    axis += 4 if axis < 0 else 0
    if axis == 0:
        raise NotImplementedError("layer %s: Crop along the batch axis (axis: 0)" % l.name)
    offs = [int(o) for o in cp.getall("offset")]
    if len(offs) > 1 and len(offs) != 4 - axis:
        raise ValueError("layer %s: %d crop offsets for %d cropped axes (none, one, or one per axis)" % (l.name, len(offs), 4 - axis))
    if b0[0] != b1[0]:
        raise ValueError("layer %s: batch of %d cropped to the shape of a batch of %d" % (l.name, b0[0], b1[0]))
    shape, offset = list(b0), [0, 0, 0, 0]
    for i in range(axis, 4):
        offset[i] = offs[0] if len(offs) == 1 else offs[i - axis] if offs else 0
        shape[i] = b1[i]
        if offset[i] < 0 or offset[i] + b1[i] > b0[i]:
            raise ValueError("layer %s: crop of axis %d at offset %d + size %d leaves the extent %d" % (l.name, i, offset[i], b1[i], b0[i]))
    return tuple(shape), tuple(offset)


def interp_size(l: "Layer", h: int, w: int) -> Tuple[int, int, int, int]:
    """DeepLab-Caffe's InterpLayer: (height of the top, width of the top, pad_beg, pad_end) for an h x w bottom.  pad_beg / pad_end are
    <= 0 and crop: the effective input is rows and columns -pad_beg .. h + pad_end - 1.  Per axis the output extent is (He - 1) //
    shrink_factor + 1, He + (He - 1) (zoom_factor - 1), both (shrink first), or interp_param's height / width; as in Caffe a field counts
    as given when the prototxt writes it, a factor of 1 included.  Everything else is refused by layer name."""
    p = l.sub("interp_param")
    pad_beg, pad_end = int(p.get("pad_beg", 0)), int(p.get("pad_end", 0))
    if pad_beg > 0 or pad_end > 0:
        raise ValueError("layer %s: Interp with pad_beg %d / pad_end %d: only pads <= 0 (they crop)" % (l.name, pad_beg, pad_end))
    he, we = h + pad_beg + pad_end, w + pad_beg + pad_end
    if he < 1 or we < 1:
        raise ValueError("layer %s: pad_beg %d / pad_end %d leave nothing of the %d x %d bottom" % (l.name, pad_beg, pad_end, h, w))
    given = {k: int(p.get(k)) for k in ("height", "width", "zoom_factor", "shrink_factor") if p.get(k) is not None}
    shrink, zoom = given.get("shrink_factor"), given.get("zoom_factor")
    if any(f is not None and f < 1 for f in (shrink, zoom)):
        raise ValueError("layer %s: Interp factors must be at least 1 (zoom_factor %s, shrink_factor %s)" % (l.name, zoom, shrink))
    if shrink is not None or zoom is not None:
        oh, ow = he, we
        if shrink is not None:
            oh, ow = (oh - 1) // shrink + 1, (ow - 1) // shrink + 1
        if zoom is not None:
            oh, ow = oh + (oh - 1) * (zoom - 1), ow + (ow - 1) * (zoom - 1)
    elif "height" in given and "width" in given:
        oh, ow = given["height"], given["width"]
    else:
        raise ValueError("layer %s: Interp needs zoom_factor, shrink_factor or both height and width" % l.name)
    if oh < 1 or ow < 1:
        raise ValueError("layer %s: Interp to %d x %d: the output extents must be at least 1" % (l.name, oh, ow))
    return oh, ow, pad_beg, pad_end


def upsample_size(l: "Layer", h: int, w: int) -> Tuple[int, int]:
    """The SegNet fork's UpsampleLayer: (height, width) of the top for an h x w bottom.  upsample_param's upsample_h AND upsample_w give the
    extents as they are (the way the published nets undo a ceil-mode pooling of an odd extent); otherwise each axis is h * scale -
    pad_out_h / w * scale - pad_out_w, scale defaulting to 2 and the pads to 0.  One of upsample_h / upsample_w alone is refused by
    layer name."""
    p = l.sub("upsample_param")
    uh, uw = p.get("upsample_h"), p.get("upsample_w")
    if (uh is None) != (uw is None):
        raise ValueError("layer %s: Upsample with %s and no %s (both or neither)" % ((l.name, "upsample_h", "upsample_w") if uw is None
                                                                                     else (l.name, "upsample_w", "upsample_h")))
    if uh is not None:
        oh, ow = int(uh), int(uw)
    else:
        scale = int(p.get("scale", 2))
        if scale < 1:
            raise ValueError("layer %s: Upsample scale %d is below 1" % (l.name, scale))
        oh, ow = h * scale - int(p.get("pad_out_h", 0)), w * scale - int(p.get("pad_out_w", 0))
    if oh < 1 or ow < 1:
        raise ValueError("layer %s: Upsample to %d x %d: the output extents must be at least 1" % (l.name, oh, ow))
    return oh, ow


ARGMAX_MAX_TOPK = 32      # FCN_ARGMAX_MAX_TOPK of include/fcnhip.h


def argmax_form(l: "Layer", shape: Shape) -> Tuple[int, bool, bool]:
    """Caffe's ArgMaxLayer on a bottom of `shape`: (top_k, out_max_val, legacy).  With axis 1 (-3 on a 4-d blob) the top is the bottom
    with top_k channels - the indices, or with out_max_val the values.  legacy: no axis, Caffe's form over everything behind the batch
    axis, taken only where that is the channels alone (H * W == 1): the top is (N, 1, top_k), or (N, 2, top_k) with out_max_val - the
    indices, then the values.  Everything else is refused by layer name."""
    p = l.sub("argmax_param")
    if len(l.bottoms) != 1 or len(shape) not in (2, 4) or len(l.tops) != 1:
        raise ValueError("layer %s: ArgMax takes one 4-d or 2-d bottom and has one top, got bottoms %s" % (l.name, l.bottoms))
    if l.tops[0] == l.bottoms[0]:
        raise ValueError("layer %s: ArgMax cannot run in place" % l.name)
    top_k, axis = int(p.get("top_k", 1)), p.get("axis")
    n, c, h, w = as_nchw(shape)
    if axis is not None and int(axis) not in ((1, -3) if len(shape) == 4 else (1, -1)):
        raise NotImplementedError("layer %s: ArgMax over axis %d of a %d-d blob (only the channel axis)" % (l.name, int(axis), len(shape)))
    if axis is None and h * w != 1:
        raise NotImplementedError("layer %s: ArgMax without an axis over the %d x %d x %d blob of an image (Caffe's legacy form ranks C * H * W "
                                  "values; only H * W == 1 - a classifier's scores - or axis: 1)" % (l.name, c, h, w))
    if top_k < 1 or top_k > c:
        raise ValueError("layer %s: top_k %d is outside [1, %d]" % (l.name, top_k, c))
    if top_k > ARGMAX_MAX_TOPK:
        raise NotImplementedError("layer %s: ArgMax with top_k %d (at most %d)" % (l.name, top_k, ARGMAX_MAX_TOPK))
    return top_k, bool(p.get("out_max_val", False)), axis is None


def as_nchw(shape: Shape) -> Optional[Tuple[int, int, int, int]]:
    """A blob's shape as the NHWC machinery sees it: a 4-d blob as it is, an (N, C) blob (the top of an InnerProduct) as N pixels of C
    channels (H = W = 1); None for anything else.  Engine.Blob.nchw and the channel-axis layers (Concat, Slice) share this rule."""
    if len(shape) == 4:
        return tuple(shape)
    if len(shape) == 2:
        return (shape[0], shape[1], 1, 1)
    return None


def _channel_axis_bottoms(l: "Layer", bots: Sequence[Shape]) -> List[Tuple[int, int, int, int]]:
    """The bottoms of a Concat / Slice as NCHW: all 4-d or all 2-d, refused by layer name otherwise."""
    g = [as_nchw(b) for b in bots]
    if not bots or any(x is None for x in g) or len({len(b) for b in bots}) != 1:
        raise ValueError("layer %s: %s takes 4-d blobs or 2-d blobs (not a mix), got %s" % (l.name, l.type, list(bots)))
    return g


def _like(nchw: Tuple[int, int, int, int], model: Shape) -> Shape:
    """An NCHW result in the dimensionality of the layer's bottoms."""
    return tuple(nchw) if len(model) == 4 else (nchw[0], nchw[1])


def bn_global_stats(l: "Layer", phase: str) -> bool:
    """BatchNormLayer's use_global_stats: the moving averages normalise (default: in the TEST phase), not the batch's statistics."""
    v = l.sub("batch_norm_param").get("use_global_stats")
    return phase == "TEST" if v is None else bool(v)


def is_scale_gate(l: "Layer") -> bool:
    """A Scale whose multiplier is a blob of the net (two bottoms): the gated form of csrc/gate.hip, not a link of a BatchNorm chain."""
    return l.type == "Scale" and len(l.bottoms) == 2


def scale_gate_form(l: "Layer", bots: Sequence[Shape], phase: str) -> Tuple[int, int, int]:
    """Caffe's ScaleLayer with two bottoms (x, gate) in the one form taken: x is (N, C, H, W) or (N, C), axis is 0 (or its negative
    equivalent) and the gate's shape equals x.shape[axis : axis + gate.ndim] with two axes - an (N, C) gate; an (N, C, 1, 1) gate is
    legal only where H = W = 1 (Caffe's own rule).  Returns (N, pixels per image, C).  bias_term, any other axis or gate rank and, in
    a TRAIN net, the form in place on x (Caffe keeps a copy of x for the backward pass; nothing here does) are refused by layer name."""
    sp = l.sub("scale_param")
    x, g = tuple(bots[0]), tuple(bots[1])
    if l.axpy is not None and len(g) == 4 and g[2:] == (1, 1):
        g = g[:2]      # (the Axpy layer takes its gate as (N, C, 1, 1): the top of a 1x1 convolution over the pooled blob)
    if len(l.tops) != 1 or len(x) not in (2, 4):
        raise ValueError("layer %s: Scale with two bottoms takes a 4-d or 2-d blob and its multiplier and has one top, got %s" % (l.name, list(bots)))
    if bool(sp.get("bias_term", False)):
        raise NotImplementedError("layer %s: Scale with two bottoms and bias_term: true (a learned bias beside a multiplier from the net)" % l.name)
    axis = int(sp.get("axis", 1))
    if not -len(x) <= axis < len(x):
        raise ValueError("layer %s: Scale axis %d is outside [%d, %d)" % (l.name, axis, -len(x), len(x)))
    axis += len(x) if axis < 0 else 0
    if x[axis:axis + len(g)] != g:
        raise ValueError("layer %s: the multiplier %s %s does not match axes %d.. of %s %s (Caffe: its shape must equal "
                         "x.shape[axis : axis + its rank])" % (l.name, l.bottoms[1], g, axis, l.bottoms[0], x))
    if axis != 0 or not (len(g) == 2 or (len(g) == 4 and x[2:] == (1, 1))):
        raise NotImplementedError("layer %s: Scale with two bottoms over axis %d with the %d-d multiplier %s %s (only a per-image, per-channel "
                                  "gate: axis 0 and an (N, C) multiplier, or (N, C, 1, 1) where H = W = 1)" % (l.name, axis, len(g), l.bottoms[1], g))
    if phase == "TRAIN" and l.tops[0] == l.bottoms[0]:
        raise NotImplementedError("layer %s: Scale with two bottoms in place on %s in a TRAIN net (the gate's gradient needs x as it was; "
                                  "give the layer a top of its own)" % (l.name, l.bottoms[0]))
    if l.tops[0] == l.bottoms[1]:
        raise ValueError("layer %s: Scale with two bottoms cannot write its top over the multiplier %s" % (l.name, l.bottoms[1]))
    n, c, h, w = as_nchw(x)
    return n, h * w, c


def _lower_axpy(m: proto.Msg) -> List["Layer"]:
    """The SENet release's Axpy layer (bottoms: gate, x, residual; top = gate * x + residual, the gate (N, C, 1, 1) or (N, C)) as the two
    layers it stands for: a gated Scale `<name>/scale` of (x, gate) over axis 0 with the top `<top>/scale`, and an Eltwise SUM `<name>`
    of that blob and the residual with the layer's top.  No new layer type reaches the planners."""
    name, bots, tops = str(m.get("name", "")), [str(b) for b in m.getall("bottom")], [str(t) for t in m.getall("top")]
    if len(bots) != 3 or len(tops) != 1:
        raise ValueError("layer %s: Axpy takes three bottoms (the gate, the blob, the residual) and has one top, got %s -> %s" % (name, bots, tops))
    mid = tops[0] + "/scale"
    sc, el, sp = proto.Msg(), proto.Msg(), proto.Msg()
    sp.add("axis", 0)
    for k, v in (("name", name + "/scale"), ("type", "Scale"), ("bottom", bots[1]), ("bottom", bots[0]), ("top", mid), ("scale_param", sp)):
        sc.add(k, v)
    for k, v in (("name", name), ("type", "Eltwise"), ("bottom", mid), ("bottom", bots[2]), ("top", tops[0])):
        el.add(k, v)
    out = [Layer(sc), Layer(el)]
    for l in out:
        l.axpy = name
    return out


ACT_TYPES = ("PReLU", "TanH", "Bias")      # the one-bottom activations of csrc/act.hip (NetSpec activations=True)


def act_param_shape(l: "Layer", bots: Sequence[Shape]) -> Shape:
    """The learned blob of a PReLU (Caffe's PReLULayer: the slopes, (C,), or () - one value - with channel_shared) or of a Bias (Caffe's
    BiasLayer in its one-bottom form over the channel axis: (C,)).  One bottom, 4-d or 2-d, channels on shape[1]; everything else is
    refused by layer name."""
    if len(l.bottoms) == 2 and l.type == "Bias":
        raise NotImplementedError("layer %s: Bias with two bottoms (the bias as a blob of the net)" % l.name)
    if len(bots) != 1 or len(bots[0]) not in (2, 4) or len(l.tops) != 1:
        raise ValueError("layer %s: %s takes one 4-d or 2-d bottom and has one top, got %s" % (l.name, l.type, list(bots)))
    c = bots[0][1]
    if l.type == "PReLU":
        return () if bool(l.sub("prelu_param").get("channel_shared", False)) else (c,)
    bp = l.sub("bias_param")
    if int(bp.get("axis", 1)) != 1 or int(bp.get("num_axes", 1)) != 1:
        raise NotImplementedError("layer %s: Bias over axis %d, num_axes %d (only the channel axis: axis 1, num_axes 1)"
                                  % (l.name, int(bp.get("axis", 1)), int(bp.get("num_axes", 1))))
    return (c,)


# the one-bottom activations of csrc/neuron.hip: no learned blob, no opt-in keyword - every NetSpec takes them
NEURON_TYPES = ("ELU", "ReLU6", "Clip", "AbsVal", "BNLL", "Swish")


def neuron_params(l: "Layer") -> Tuple[int, float, float]:
    """(mode, a, b) of fcn_neuron_*: a is alpha (ELU, elu_param, default 1), beta (Swish, swish_param, default 1) or lo (Clip), b is hi
    (Clip); ReLU6 - the MobileNet forks' type, no parameters - is Clip with 0 and 6; both are 0 where the mode ignores them.  Refused by
    layer name: a second bottom or top, AbsVal in place (Caffe's own CHECK), ELU with a negative alpha (the sign of y would no longer
    tell the sign of x, which the gradient reads from y), Clip without both bounds (required fields of clip_param) or with min >= max."""
    t = l.type
    if len(l.bottoms) != 1 or len(l.tops) != 1:
        raise ValueError("layer %s: %s takes one bottom and has one top, got %d and %d" % (l.name, t, len(l.bottoms), len(l.tops)))
    a = b = 0.0
    if t == "ELU":
        a = float(l.sub("elu_param").get("alpha", 1.0))
        if not a >= 0.0:
            raise NotImplementedError("layer %s: ELU with alpha %g (a negative alpha is not supported: the gradient is read from the top)"
                                      % (l.name, a))
    elif t == "Swish":
        a = float(l.sub("swish_param").get("beta", 1.0))
    elif t == "ReLU6":
        a, b = 0.0, 6.0
    elif t == "Clip":
        cp = l.sub("clip_param")
        if cp.get("min") is None or cp.get("max") is None:
            raise ValueError("layer %s: Clip needs clip_param { min max }, both" % l.name)
        a, b = float(cp.get("min")), float(cp.get("max"))
        if not a < b:
            raise ValueError("layer %s: Clip with min %g >= max %g" % (l.name, a, b))
    elif t == "AbsVal":
        if l.tops[0] == l.bottoms[0]:
            raise ValueError("layer %s: AbsVal does not allow in-place computation (the gradient needs the bottom's sign)" % l.name)
    elif t != "BNLL":
        raise ValueError("layer %s: %s is none of %s" % (l.name, t, list(NEURON_TYPES)))
    return NEURON_MODES[t], a, b


# the channel shuffle of csrc/shuffle.hip (the ShuffleNet ports' layer): no learned blob, no opt-in keyword - every NetSpec takes it
SHUFFLE_TYPES = ("ShuffleChannel",)


def shuffle_group(l: "Layer", bots: Sequence[Shape]) -> int:
    """shuffle_channel_param.group (default 1) of a ShuffleChannel over its bottom shapes: y[j * g + i] = x[i * (C / g) + j].  Refused by
    layer name, as Caffe's own checks do: a second bottom or top, in place, a blob that is neither 4-d nor 2-d, group < 1 and a channel
    count that group does not divide."""
    if len(l.bottoms) != 1 or len(l.tops) != 1 or len(bots) != 1:
        raise ValueError("layer %s: %s takes one bottom and has one top, got %d and %d" % (l.name, l.type, len(l.bottoms), len(l.tops)))
    if l.tops[0] == l.bottoms[0]:
        raise ValueError("layer %s: %s does not allow in-place computation (a permutation of the channels)" % (l.name, l.type))
    if len(bots[0]) not in (2, 4):
        raise ValueError("layer %s: %s takes one 4-d or 2-d bottom, got %s" % (l.name, l.type, list(bots)))
    g, c = int(l.sub("shuffle_channel_param").get("group", 1)), bots[0][1]
    if g < 1 or c % g:
        raise ValueError("layer %s: %s with group %d over %d channels (group must be at least 1 and divide the channels)" % (l.name, l.type, g, c))
    return g


DATA_TYPES = ("Data", "Python", "Input", "DummyData", "MemoryData", "ImageData", "HDF5Data")
LOSS_TYPES = ("L1Loss", "EuclideanLoss", "SoftmaxWithLoss", "SigmoidCrossEntropyLoss")
# the opt-in keywords of NetSpec (each off in a bare NetSpec; NetSpec.public turns them on): a new layer family adds its keyword here
FEATURES = ("depthwise", "ip_gemm", "rconv_f16", "tconv_f16", "scale_gate", "activations")


class NetSpec:
    """Phase-filtered layer list + blob/parameter shapes."""

    def __init__(self, msg: proto.Msg, phase: str = "TEST", depthwise: bool = False, ip_gemm: bool = False, rconv_f16: bool = False,
                 tconv_f16: bool = False, scale_gate: bool = False, *, activations: bool = False):
        """depthwise: a Convolution with group == bottom channels == num_output > 1 is a depthwise convolution (is_depthwise), the
        same thing as a layer of type DepthwiseConvolution - the way the published MobileNet prototxts write it.  Off by default:
        a bare NetSpec keeps refusing such a layer where its parameters are laid out (storage.conv_groups).  The public entry points
        (caffe.Net, caffe.get_solver, `caffe train / test / time`) pass True.
        ip_gemm: an InnerProduct over more than FCN_IP_MAX_ROWS (32) rows runs through the matrix-core kernels of csrc/ip_gemm.hip.
        Off by default for the same reason: a bare NetSpec keeps refusing such a layer by name where it is planned (both engines and the
        backward planner); the same public entry points pass True.  At up to 32 rows the keyword changes nothing.
        rconv_f16: in a half-float engine a dilated or rectangular Convolution runs through the half-float kernel of csrc/rconv.hip
        (fcn_rconv2d_f16).  Off by default, again: a bare NetSpec keeps refusing such a layer by name in a half-float engine; the public
        entry points that build a TEST-phase net pass True.  A float32 engine never looks at the keyword.
        tconv_f16: in a half-float engine a group-1 Deconvolution over a half bottom runs through the half-float kernel of
        csrc/tconv.hip (fcn_tconv2d_f16) and its blob is a bank of halves.  Off by default, passed by the same entry points, never looked
        at by a float32 engine: the rule of rconv_f16.
        scale_gate: a Scale with two bottoms (x, gate) over axis 0 - the multiplier a per-image, per-channel (N, C) blob of the net, the gate of
        a Squeeze-and-Excitation block - is accepted and runs through csrc/gate.hip (scale_gate_form), and the SENet release's Axpy layer
        (gate, x, residual) is read as the two layers it stands for: such a Scale `<name>/scale` with the top `<top>/scale`, and an Eltwise SUM
        `<name>` of that blob and the residual.  Off by default, once more: a bare NetSpec keeps refusing the two-bottom Scale by name (and
        knows no Axpy type); the same public entry points pass True.  A net without such a layer is planned the same either way.
        activations (keyword only): PReLU (prelu_param { filler channel_shared }: one learned blob (C,), or () with channel_shared), Bias
        (bias_param { axis: 1 num_axes: 1 filler }: one learned blob (C,)) and TanH are accepted and run through csrc/act.hip in both
        inference engines and train in float32.  Off by default, as the others are: a bare NetSpec keeps refusing PReLU and Bias by name
        and hands TanH to an engine that refuses it; the same public entry points pass True.  A net without one of the three is planned
        the same either way."""
        if phase not in ("TRAIN", "TEST"):
            raise ValueError("phase must be 'TRAIN' or 'TEST'")
        self.phase = phase
        self.depthwise = bool(depthwise)
        self.ip_gemm = bool(ip_gemm)
        self.rconv_f16 = bool(rconv_f16)
        self.tconv_f16 = bool(tconv_f16)
        self.scale_gate = bool(scale_gate)
        self.activations = bool(activations)
        self.name = str(msg.get("name", ""))
        self.layers: List[Layer] = [l for m in msg.getall("layer") if _phase_included(m, phase)
                                    for l in (_lower_axpy(m) if self.scale_gate and str(m.get("type", "")) == "Axpy" else [Layer(m)])]
        if msg.getall("layers"):
            raise NotImplementedError("V1 'layers' prototxt syntax is not used by the reference")
        self.input_shapes: Dict[str, Shape] = {}
        names = [str(n) for n in msg.getall("input")]
        shapes = msg.getall("input_shape")
        dims = [int(d) for d in msg.getall("input_dim")]
        for i, nm in enumerate(names):
            if shapes:
                self.input_shapes[nm] = tuple(int(d) for d in shapes[i].getall("dim"))
            else:
                self.input_shapes[nm] = tuple(dims[4 * i:4 * i + 4])
        for l in self.layers:
            if l.type == "Input":
                shp = l.sub("input_param").getall("shape")
                for t, s in zip(l.tops, shp):
                    self.input_shapes[t] = tuple(int(d) for d in s.getall("dim"))
        self.blob_shapes: Dict[str, Shape] = {}
        self.param_shapes: Dict[str, List[Shape]] = {}
        # second top of a MAX Pooling (Caffe's mask: the flat iy * W + ix argmax as floats) -> that layer.  A mask has a shape and can be
        # read, but it is no activation blob: on the device it is the pooling's int32 argmax buffer, and only an Upsample may consume it
        self.mask_blobs: Dict[str, Layer] = {}
        # SSD: tops of PriorBox layers and of their Concat(axis 2) -> that layer (constants of the net, computed when it is planned), and the
        # top of a DetectionOutput -> that layer (its shape is a capacity: a forward says how many rows it holds)
        self.prior_blobs: Dict[str, Layer] = {}
        self.detection_blobs: Dict[str, Layer] = {}
        # region stage: blobs whose axis 0 is the ROI axis of a Proposal - its tops and everything downstream that keeps that axis - ->
        # the Proposal layer whose count says how many of the post_nms_topn rows a forward found (rois fed through an Input are not here)
        self.roi_blobs: Dict[str, Layer] = {}

    @classmethod
    def from_file(cls, path: str, phase: str = "TEST", depthwise: bool = False, *, ip_gemm: bool = False, rconv_f16: bool = False,
                  tconv_f16: bool = False, scale_gate: bool = False, activations: bool = False) -> "NetSpec":
        return cls(proto.parse_file(path), phase, depthwise, ip_gemm, rconv_f16, tconv_f16, scale_gate, activations=activations)

    @staticmethod
    def public_features(phase: str) -> Dict[str, bool]:
        """The keywords of FEATURES as the public entry points pass them: everything on, the two half-float ones where the net is a TEST net."""
        return {k: phase == "TEST" if k in ("rconv_f16", "tconv_f16") else True for k in FEATURES}

    @classmethod
    def public(cls, msg: proto.Msg, phase: str = "TEST") -> "NetSpec":
        """The NetSpec of the public entry points (caffe.Net, caffe.get_solver, `caffe train / test / time`): public_features(phase)."""
        return cls(msg, phase, **cls.public_features(phase))

    def is_depthwise(self, l: Layer) -> bool:
        """The layer runs through csrc/dwconv.hip: a DepthwiseConvolution, or - with the `depthwise` keyword - a Convolution whose
        group equals its bottom's channels and its num_output (> 1).  The one predicate storage and both planners ask; it needs
        infer() to have run."""
        if l.type == "DepthwiseConvolution":
            return True
        if l.type != "Convolution" or not self.depthwise:
            return False
        p = l.sub("convolution_param")
        g = int(p.get("group", 1))
        shp = self.blob_shapes.get(l.bottoms[0]) if l.bottoms else None
        return g > 1 and shp is not None and len(shp) == 4 and g == shp[1] == int(p.get("num_output"))

    # ------------------------------------------------------------------
    def data_tops(self) -> List[str]:
        """Blobs that must be fed from outside: net inputs and tops of data / Python layers."""
        out = list(self.input_shapes.keys())
        for l in self.layers:
            if l.type in DATA_TYPES:
                out.extend(t for t in l.tops if t not in out)
        return out

    def infer(self, data_shapes: Optional[Dict[str, Shape]] = None) -> Dict[str, Shape]:
        """Compute every blob's NCHW shape; ``data_shapes`` supplies data-layer tops."""
        shapes: Dict[str, Shape] = dict(self.input_shapes)
        if data_shapes:
            shapes.update({k: tuple(int(d) for d in v) for k, v in data_shapes.items()})
        self.param_shapes = {}
        self.mask_blobs = {}
        self.prior_blobs, self.detection_blobs = {}, {}
        self.roi_blobs = {}
        self.blob_shapes = shapes      # (filled as the layers are walked: is_depthwise reads a layer's bottom)
        for l in self.layers:
            t = l.type
            if t in DATA_TYPES:
                for tp in l.tops:
                    if tp not in shapes:
                        raise KeyError("shape of data blob %r (layer %s) was not provided" % (tp, l.name))
                continue
            try:
                bots = [shapes[b] for b in l.bottoms]
            except KeyError as e:
                raise KeyError("layer %s: unknown bottom blob %s" % (l.name, e)) from None
            for bi, b in enumerate(l.bottoms):
                if b in self.mask_blobs and not (t == "Upsample" and bi == 1):
                    raise NotImplementedError("layer %s: the pooling mask %s (second top of %s) feeds %s (a mask may only be the second "
                                              "bottom of an Upsample)" % (l.name, b, self.mask_blobs[b].name,
                                                                          "the first bottom of an Upsample" if t == "Upsample" else "a layer of type %s" % t))
            # the ROI axis travels with the rois through the poolings (and with the first bottom through every other layer: below)
            governs = self.roi_blobs.get(l.bottoms[1]) if t in ("ROIPooling", "PSROIPooling") and len(l.bottoms) > 1 else None
            if t == "Convolution":
                p = l.sub("convolution_param")
                kh, kw, sh, sw, ph, pw = layer_geometry(l)
                g = int(p.get("group", 1))
                co = int(p.get("num_output"))
                n, c, h, w = bots[0]
                d = layer_dilation(l)
                rect = (kh, sh, ph) != (kw, sw, pw)
                if self.depthwise and g > 1 and g == c and co != c:
                    raise NotImplementedError("layer %s: depthwise Convolution over %d channels with num_output %d (a channel multiplier of "
                                              "%s is not supported: num_output must equal group)" % (l.name, c, co, co // c if co % c == 0 else "%d/%d" % (co, c)))
                if (d > 1 or rect or self.is_depthwise(l)) and (conv_out(h, kh, sh, ph, d) < 1 or conv_out(w, kw, sw, pw, d) < 1):
                    raise ValueError("layer %s: the %dx%d window with dilation %d exceeds the padded %dx%d bottom" % (l.name, kh, kw, d, h + 2 * ph, w + 2 * pw))
                self.param_shapes[l.name] = [(co, c // g, kh, kw)] + ([(co,)] if bool(p.get("bias_term", True)) else [])
                shapes[l.tops[0]] = (n, co, conv_out(h, kh, sh, ph, d), conv_out(w, kw, sw, pw, d))
            elif t == "DepthwiseConvolution":
                # the common forks' DepthwiseConvolutionLayer (MobileNet-SSD deploy files): a convolution_param whose group, if written,
                # equals the bottom's channels and num_output; the blob is Caffe's (C, 1, kh, kw)
                p = l.sub("convolution_param")
                if len(bots) != 1 or len(bots[0]) != 4 or len(l.tops) != 1:
                    raise ValueError("layer %s: DepthwiseConvolution takes one 4-d bottom and has one top, got %s" % (l.name, bots))
                kh, kw, sh, sw, ph, pw = layer_geometry(l)
                n, c, h, w = bots[0]
                if p.get("num_output") is None:
                    raise ValueError("layer %s: DepthwiseConvolution without num_output" % l.name)
                co, g = int(p.get("num_output")), int(p.get("group", c))
                if g == c and co > c and co % c == 0:
                    raise NotImplementedError("layer %s: DepthwiseConvolution over %d channels with num_output %d (a channel multiplier of "
                                              "%d is not supported: num_output must equal the bottom's channels)" % (l.name, c, co, co // c))
                if g != c or co != c:
                    raise ValueError("layer %s: DepthwiseConvolution over %d channels with group %d, num_output %d (group, if written, and "
                                     "num_output must equal the bottom's channels)" % (l.name, c, g, co))
                d = layer_dilation(l)
                if conv_out(h, kh, sh, ph, d) < 1 or conv_out(w, kw, sw, pw, d) < 1:
                    raise ValueError("layer %s: the %dx%d window with dilation %d exceeds the padded %dx%d bottom" % (l.name, kh, kw, d, h + 2 * ph, w + 2 * pw))
                self.param_shapes[l.name] = [(c, 1, kh, kw)] + ([(c,)] if bool(p.get("bias_term", True)) else [])
                shapes[l.tops[0]] = (n, c, conv_out(h, kh, sh, ph, d), conv_out(w, kw, sw, pw, d))
            elif t == "Deconvolution":
                p = l.sub("convolution_param")
                k, s, pad = _square(l)
                g = int(p.get("group", 1))
                co = int(p.get("num_output"))
                n, c, h, w = bots[0]
                layer_dilation(l)      # (refuses a dilated Deconvolution by name)
                self.param_shapes[l.name] = [(c, co // g, k, k)] + ([(co,)] if bool(p.get("bias_term", True)) else [])
                shapes[l.tops[0]] = (n, co, deconv_out(h, k, s, pad), deconv_out(w, k, s, pad))
            elif t == "InnerProduct":
                # Caffe's InnerProductLayer: everything behind the batch axis is one vector of K = C*H*W elements in (c, h, w) order
                p = l.sub("inner_product_param")
                if int(p.get("axis", 1)) != 1:
                    raise NotImplementedError("layer %s: InnerProduct over axis %d (only axis 1)" % (l.name, int(p.get("axis", 1))))
                if bool(p.get("transpose", False)):
                    raise NotImplementedError("layer %s: InnerProduct with transpose: true" % l.name)
                if len(bots) != 1 or len(bots[0]) not in (2, 4):
                    raise ValueError("layer %s: InnerProduct takes one 4-d or 2-d bottom, got %s" % (l.name, bots))
                co = int(p.get("num_output"))
                kk = int(np.prod(bots[0][1:]))
                self.param_shapes[l.name] = [(co, kk)] + ([(co,)] if bool(p.get("bias_term", True)) else [])
                shapes[l.tops[0]] = (bots[0][0], co)
            elif t == "Pooling":
                p = l.sub("pooling_param")
                n, c, h, w = bots[0]
                if len(l.tops) > 2:
                    raise ValueError("layer %s: Pooling has one top, or two (the pooled blob and the mask), got %d" % (l.name, len(l.tops)))
                if len(l.tops) == 2 and (str(p.get("pool", "MAX")) != "MAX" or bool(p.get("global_pooling", False))):
                    raise NotImplementedError("layer %s: a second top (the mask %s) on %s pooling: only pool: MAX without global_pooling writes one"
                                              % (l.name, l.tops[1], "global" if bool(p.get("global_pooling", False)) else str(p.get("pool"))))
                if bool(p.get("global_pooling", False)):
                    shapes[l.tops[0]] = (n, c, 1, 1)
                else:
                    k, s, pad = _square(l)
                    shapes[l.tops[0]] = (n, c, pool_out(h, k, s, pad), pool_out(w, k, s, pad))
                if len(l.tops) == 2:
                    if l.tops[1] in (l.tops[0], l.bottoms[0]):
                        raise ValueError("layer %s: the mask top %s must be a blob of its own" % (l.name, l.tops[1]))
                    shapes[l.tops[1]] = shapes[l.tops[0]]
                    self.mask_blobs[l.tops[1]] = l
            elif t == "Concat":
                axis = int(l.sub("concat_param").get("axis", l.sub("concat_param").get("concat_dim", 1)))
                if axis == 2 and bots and all(len(b) == 3 and b[:2] == (1, 2) for b in bots) and all(b in self.prior_blobs for b in l.bottoms):
                    # SSD's mbox_priorbox: the PriorBox tops side by side, a constant of the net like them
                    shapes[l.tops[0]] = (1, 2, sum(b[2] for b in bots))
                    self.prior_blobs[l.tops[0]] = l
                    continue
                if axis != 1:
                    raise NotImplementedError("Concat along axis %d" % axis)
                g4 = _channel_axis_bottoms(l, bots)
                n, _, h, w = g4[0]
                for b in g4[1:]:
                    if (b[0], b[2], b[3]) != (n, h, w):
                        raise ValueError("layer %s: concat inputs disagree: %s" % (l.name, bots))
                shapes[l.tops[0]] = _like((n, sum(b[1] for b in g4), h, w), bots[0])
            elif t == "Slice":
                sp = l.sub("slice_param")
                axis = int(sp.get("axis", sp.get("slice_dim", 1)))
                if axis != 1:
                    raise NotImplementedError("Slice along axis %d" % axis)
                n, c, h, w = _channel_axis_bottoms(l, bots[:1])[0]
                pts = [int(x) for x in sp.getall("slice_point")]
                if not pts:
                    step = c // len(l.tops)
                    pts = [step * i for i in range(1, len(l.tops))]
                edges = [0] + pts + [c]
                if len(edges) != len(l.tops) + 1 or any(b <= a for a, b in zip(edges[:-1], edges[1:])):
                    raise ValueError("layer %s: bad slice points %s for %d channels" % (l.name, pts, c))
                for tp, a, b in zip(l.tops, edges[:-1], edges[1:]):
                    shapes[tp] = _like((n, b - a, h, w), bots[0])
            elif t in LOSS_TYPES:
                shapes[l.tops[0]] = ()
            elif t == "Accuracy":
                # Caffe's AccuracyLayer over the channel axis: top0 the scalar accuracy, optional top1 the per-class accuracies
                ap = l.sub("accuracy_param")
                if int(ap.get("axis", 1)) != 1:
                    raise NotImplementedError("Accuracy over axis %d (layer %s): only the channel axis" % (int(ap.get("axis", 1)), l.name))
                if len(bots) != 2 or len(bots[0]) not in (2, 4) or not 1 <= len(l.tops) <= 2:
                    raise ValueError("layer %s: Accuracy takes a 4-d or 2-d score blob and a label blob, and has one or two tops" % l.name)
                if int(ap.get("top_k", 1)) < 1 or int(ap.get("top_k", 1)) > bots[0][1]:
                    raise ValueError("layer %s: top_k %d is outside [1, %d]" % (l.name, int(ap.get("top_k", 1)), bots[0][1]))
                shapes[l.tops[0]] = ()
                if len(l.tops) > 1:
                    shapes[l.tops[1]] = (bots[0][1],)
            elif t in ("ReLU", "Sigmoid", "Power", "LRN", "Dropout", "Softmax", "TanH"):
                shapes[l.tops[0]] = bots[0]
            elif t in NEURON_TYPES:
                neuron_params(l)      # (its refusals, by layer name)
                if len(bots) != 1 or len(bots[0]) not in (2, 4):
                    raise ValueError("layer %s: %s takes one 4-d or 2-d bottom, got %s" % (l.name, t, list(bots)))
                shapes[l.tops[0]] = bots[0]
            elif t in SHUFFLE_TYPES:
                shuffle_group(l, bots)      # (its refusals, by layer name)
                shapes[l.tops[0]] = bots[0]
            elif t in ("PReLU", "Bias"):
                if not self.activations:
                    raise NotImplementedError("layer type %r (layer %s): taken by a NetSpec built with activations=True (caffe.Net, the "
                                              "solvers and the caffe tool pass it)" % (t, l.name))
                self.param_shapes[l.name] = [act_param_shape(l, bots)]
                shapes[l.tops[0]] = bots[0]
            elif t == "BatchNorm":
                # Caffe's BatchNormLayer over the channel axis: blobs (C,) mean sum, (C,) variance sum, (1,) scale factor - statistics,
                # not parameters: the layer insists on lr_mult 0 for each ("Cannot configure batch normalization statistics as layer parameters")
                if len(bots) != 1 or len(bots[0]) not in (2, 4) or len(l.tops) != 1:
                    raise ValueError("layer %s: BatchNorm takes one 4-d or 2-d bottom and has one top, got %s" % (l.name, bots))
                if any(m != 0.0 for m in l.lr_mult):
                    raise ValueError("layer %s: BatchNorm blobs are statistics, their lr_mult must be 0 (got %s)" % (l.name, l.lr_mult))
                c = bots[0][1]
                self.param_shapes[l.name] = [(c,), (c,), (1,)]
                shapes[l.tops[0]] = bots[0]
            elif t == "Scale":
                # Caffe's ScaleLayer with the multiplier as a learned blob over the channel axis: (C,) gamma and, with bias_term, (C,) beta
                sp = l.sub("scale_param")
                if len(bots) == 2 and not self.scale_gate:
                    raise NotImplementedError("layer %s: Scale with two bottoms (the multiplier as a blob of the net): a per-image, "
                                              "per-channel gate over axis 0 is taken by a NetSpec built with scale_gate=True (caffe.Net, the "
                                              "solvers and the caffe tool pass it)" % l.name)
                if len(bots) == 2:
                    scale_gate_form(l, bots, self.phase)     # (no parameter blobs: the multiplier is the second bottom)
                    shapes[l.tops[0]] = bots[0]
                    continue
                if len(bots) != 1 or len(bots[0]) not in (2, 4) or len(l.tops) != 1:
                    raise ValueError("layer %s: Scale takes one 4-d or 2-d bottom and has one top, got %s" % (l.name, bots))
                if int(sp.get("axis", 1)) != 1 or int(sp.get("num_axes", 1)) != 1:
                    raise NotImplementedError("layer %s: Scale over axis %d, num_axes %d (only the channel axis: axis 1, num_axes 1)"
                                              % (l.name, int(sp.get("axis", 1)), int(sp.get("num_axes", 1))))
                c = bots[0][1]
                self.param_shapes[l.name] = [(c,)] + ([(c,)] if bool(sp.get("bias_term", False)) else [])
                shapes[l.tops[0]] = bots[0]
            elif t == "Crop":
                if len(bots) != 2 or len(l.tops) != 1:
                    raise ValueError("layer %s: Crop takes two bottoms (the blob and the shape donor) and has one top" % l.name)
                shapes[l.tops[0]] = crop_window(l, bots[0], bots[1])[0]
            elif t == "Interp":
                if len(bots) == 2:
                    raise NotImplementedError("layer %s: Interp with two bottoms (the second one lending its size)" % l.name)
                if len(bots) != 1 or len(bots[0]) != 4 or len(l.tops) != 1:
                    raise ValueError("layer %s: Interp takes one 4-d bottom and has one top, got %s" % (l.name, bots))
                if l.tops[0] == l.bottoms[0]:
                    raise ValueError("layer %s: Interp cannot run in place" % l.name)
                oh, ow, _, _ = interp_size(l, bots[0][2], bots[0][3])
                shapes[l.tops[0]] = (bots[0][0], bots[0][1], oh, ow)
            elif t == "ArgMax":
                if len(bots) != 1:
                    raise ValueError("layer %s: ArgMax takes one bottom, got %d" % (l.name, len(bots)))
                top_k, out_max_val, legacy = argmax_form(l, bots[0])
                if legacy:
                    shapes[l.tops[0]] = (bots[0][0], 2 if out_max_val else 1, top_k)
                else:
                    shapes[l.tops[0]] = (bots[0][0], top_k) + tuple(bots[0][2:])
            elif t == "Upsample":
                if len(bots) != 2 or any(len(b) != 4 for b in bots) or len(l.tops) != 1:
                    raise ValueError("layer %s: Upsample takes two 4-d bottoms (the blob and the pooling mask) and has one top, got %s" % (l.name, bots))
                if bots[0] != bots[1]:
                    raise ValueError("layer %s: Upsample bottoms disagree: %s %s and mask %s %s" % (l.name, l.bottoms[0], bots[0], l.bottoms[1], bots[1]))
                if l.tops[0] in l.bottoms:
                    raise ValueError("layer %s: Upsample cannot run in place" % l.name)
                oh, ow = upsample_size(l, bots[0][2], bots[0][3])
                pool = self.mask_blobs.get(l.bottoms[1])
                if pool is None:
                    raise NotImplementedError("layer %s: the mask %s is not the second top of a MAX Pooling of this net (a mask fed from "
                                              "outside, or computed by other layers, is not supported)" % (l.name, l.bottoms[1]))
                ph, pw = shapes[pool.bottoms[0]][2:]
                if (oh, ow) != (ph, pw):
                    raise NotImplementedError("layer %s: Upsample to %d x %d, but the mask %s indexes the %d x %d bottom of %s: "
                                              "upsample_h: %d upsample_w: %d would match" % (l.name, oh, ow, l.bottoms[1], ph, pw, pool.name, ph, pw))
                shapes[l.tops[0]] = (bots[0][0], bots[0][1], oh, ow)
            elif t == "Permute":
                if len(bots) != 1 or len(l.tops) != 1 or l.tops[0] == l.bottoms[0]:
                    raise ValueError("layer %s: Permute takes one bottom and has one top of its own" % l.name)
                order = ssd.permute_order(l, len(bots[0]))
                shapes[l.tops[0]] = tuple(bots[0][a] for a in order)
            elif t == "Flatten":
                if len(bots) != 1 or len(l.tops) != 1 or l.tops[0] == l.bottoms[0]:
                    raise ValueError("layer %s: Flatten takes one bottom and has one top of its own" % l.name)
                shapes[l.tops[0]] = ssd.flatten_shape(l, bots[0])
            elif t == "Reshape":
                if len(bots) != 1 or len(l.tops) != 1 or l.tops[0] == l.bottoms[0]:
                    raise ValueError("layer %s: Reshape takes one bottom and has one top of its own" % l.name)
                shapes[l.tops[0]] = ssd.reshape_shape(l, bots[0])
            elif t == "PriorBox":
                if len(bots) != 2 or any(len(b) != 4 for b in bots) or len(l.tops) != 1:
                    raise ValueError("layer %s: PriorBox takes two 4-d bottoms (the feature map and the image) and has one top, got %s" % (l.name, bots))
                shapes[l.tops[0]] = (1, 2, bots[0][2] * bots[0][3] * ssd.priorbox_params(l).per_cell * 4)
                self.prior_blobs[l.tops[0]] = l
            elif t == "Normalize":
                np_ = l.sub("norm_param")
                if len(bots) != 1 or len(bots[0]) != 4 or len(l.tops) != 1:
                    raise ValueError("layer %s: Normalize takes one 4-d bottom and has one top, got %s" % (l.name, bots))
                if bool(np_.get("across_spatial", True)):
                    raise NotImplementedError("layer %s: Normalize with across_spatial: true (one norm per image; only the per-pixel form "
                                              "across_spatial: false)" % l.name)
                self.param_shapes[l.name] = [(1,) if bool(np_.get("channel_shared", True)) else (bots[0][1],)]
                shapes[l.tops[0]] = bots[0]
            elif t == "DetectionOutput":
                if len(l.tops) != 1:
                    raise ValueError("layer %s: DetectionOutput has one top" % l.name)
                shapes[l.tops[0]] = ssd.detection_shapes(l, bots)[0]
                self.detection_blobs[l.tops[0]] = l
            elif t == "Proposal":
                for tp, shp in zip(l.tops, region.proposal_shapes(l, bots)):
                    shapes[tp] = shp
                    self.roi_blobs[tp] = l
            elif t == "ROIPooling":
                shapes[l.tops[0]] = region.roi_pool_shape(l, bots)
                if governs is not None:
                    self.roi_blobs[l.tops[0]] = governs
            elif t == "PSROIPooling":
                shapes[l.tops[0]] = region.psroi_pool_shape(l, bots)
                if governs is not None:
                    self.roi_blobs[l.tops[0]] = governs
            elif t in region.TRAINING_TYPES:
                raise NotImplementedError("layer type %r (layer %s): training the region stage (AnchorTarget, ProposalTarget and a backward "
                                          "pass through the ROI poolings) is not built: deploy nets only" % (t, l.name))
            elif t in ssd.TRAINING_TYPES:
                raise NotImplementedError("layer type %r (layer %s): SSD's training and evaluation layers (MultiBoxLoss, AnnotatedData, "
                                          "DetectionEvaluate, VideoData) are not built: deploy nets only" % (t, l.name))
            elif t == "BN":
                raise NotImplementedError("layer type 'BN' (layer %s): the SegNet fork's BN layer is not supported: write BatchNorm + Scale" % l.name)
            elif t == "Eltwise":
                for b in bots[1:]:
                    if b != bots[0]:
                        raise ValueError("layer %s: eltwise inputs disagree: %s" % (l.name, bots))
                shapes[l.tops[0]] = bots[0]
            else:
                raise NotImplementedError("layer type %r (layer %s)" % (t, l.name))
        for l in self.layers:      # downstream of the poolings: a top that keeps its first bottom's axis 0 keeps its count
            src = self.roi_blobs.get(l.bottoms[0]) if l.bottoms and l.type not in region.REGION_TYPES else None
            if src is not None:
                for tp in l.tops:
                    if len(shapes.get(tp, ())) >= 1 and shapes[tp][0] == shapes[l.bottoms[0]][0]:
                        self.roi_blobs[tp] = src
        self.blob_shapes = shapes
        return shapes

    # ------------------------------------------------------------------
    def output_blobs(self) -> List[str]:
        """Tops that no later layer consumes (what ``net.forward()`` returns), in file order."""
        consumed = set()
        for l in self.layers:
            consumed.update(l.bottoms)
        out: List[str] = []
        for l in self.layers:
            for t in l.tops:
                if t not in consumed and t not in out:
                    out.append(t)
        return out

    def param_layers(self) -> List[Layer]:
        return [l for l in self.layers if l.name in self.param_shapes]


# ----------------------------------------------------------------------
# fillers (Caffe filler.hpp semantics)
# ----------------------------------------------------------------------

def bilinear_kernel(k: int) -> np.ndarray:
    f = int(math.ceil(k / 2.0))
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    v = 1.0 - np.abs(np.arange(k) / float(f) - c)
    return np.outer(v, v).astype(np.float32)


def fill_blob(shape: Shape, filler: Optional[proto.Msg], rng: np.random.Generator) -> np.ndarray:
    ftype = str(filler.get("type", "constant")) if filler is not None else "constant"
    if ftype == "constant":
        return np.full(shape, float(filler.get("value", 0.0)) if filler is not None else 0.0, np.float32)
    if ftype == "xavier":
        fan_in = int(np.prod(shape)) // shape[0]
        fan_out = int(np.prod(shape)) // shape[1] if len(shape) > 1 else fan_in
        norm = str(filler.get("variance_norm", "FAN_IN"))
        n = fan_in if norm == "FAN_IN" else fan_out if norm == "FAN_OUT" else (fan_in + fan_out) / 2.0
        scale = math.sqrt(3.0 / n)
        return rng.uniform(-scale, scale, size=shape).astype(np.float32)
    if ftype == "gaussian":
        return (rng.standard_normal(size=shape) * float(filler.get("std", 1.0)) + float(filler.get("mean", 0.0))).astype(np.float32)
    if ftype == "uniform":
        return rng.uniform(float(filler.get("min", 0.0)), float(filler.get("max", 1.0)), size=shape).astype(np.float32)
    if ftype == "bilinear":
        if len(shape) != 4 or shape[2] != shape[3]:
            raise ValueError("bilinear filler needs a square 4-d blob")
        return np.broadcast_to(bilinear_kernel(shape[3]), shape).astype(np.float32).copy()
    raise NotImplementedError("filler type %r" % ftype)


def fill_params(spec: NetSpec, seed: int = 0) -> Dict[str, List[np.ndarray]]:
    """Seeded filler initialisation of every learnable blob, in layer order."""
    rng = np.random.default_rng(seed)
    out: Dict[str, List[np.ndarray]] = {}
    one = proto.parse_text("type: \"constant\" value: 1")
    for l in spec.param_layers():
        shapes = spec.param_shapes[l.name]
        if l.type == "BatchNorm":      # Caffe sets the three blobs to zero, whatever the prototxt says
            out[l.name] = [np.zeros(s, np.float32) for s in shapes]
            continue
        if l.type == "Scale":          # ScaleLayer: filler defaults to constant 1, bias_filler (BiasLayer's) to constant 0
            p = l.sub("scale_param")
            blobs = [fill_blob(shapes[0], p.get("filler") if p.get("filler") is not None else one, rng)]
            if len(shapes) > 1:
                blobs.append(fill_blob(shapes[1], p.get("bias_filler"), rng))
            out[l.name] = blobs
            continue
        if l.type in ("PReLU", "Bias"):      # PReLULayer: filler defaults to constant 0.25; BiasLayer: to constant 0
            f = l.sub("prelu_param" if l.type == "PReLU" else "bias_param").get("filler")
            if f is None and l.type == "PReLU":
                f = proto.parse_text("type: \"constant\" value: 0.25")
            out[l.name] = [fill_blob(shapes[0], f, rng)]
            continue
        if l.type == "Normalize":      # NormalizeLayer: scale_filler defaults to constant 1
            f = l.sub("norm_param").get("scale_filler")
            out[l.name] = [fill_blob(shapes[0], f if f is not None else one, rng)]
            continue
        p = l.sub("inner_product_param" if l.type == "InnerProduct" else "convolution_param")
        blobs = [fill_blob(shapes[0], p.get("weight_filler"), rng)]
        if len(shapes) > 1:
            blobs.append(fill_blob(shapes[1], p.get("bias_filler"), rng))
        out[l.name] = blobs
    return out
