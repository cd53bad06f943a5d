"""Where every byte of a net lives on the device: which blobs own a buffer and which are channel windows of another blob's, and
how each parameter blob is laid out in the flat parameter buffer.

Everything here is a pure function of the NetSpec, the inferred shapes and a few flags: nothing allocates, copies or reads the
environment.  :class:`Engine` does that, from what these functions return.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from . import region, ssd
from .netspec import Layer, NetSpec, as_nchw

F32 = np.float32


def _r4(c: int) -> int:
    return (c + 3) // 4 * 4


def _ra(c: int, esize: int) -> int:
    """Channel count rounded up to whole 16-byte segments of `esize`-byte elements (4 floats / 8 halves)."""
    eps = 16 // esize
    return (c + eps - 1) // eps * eps


def blob_nchw(shape: Sequence[int], rows: bool) -> Optional[Tuple[int, int, int, int]]:
    """A blob as the NHWC machinery sees it: a 4-d blob as it is, an (N, C) blob (the top of an InnerProduct) as N pixels of C
    channels (H = W = 1); an (N,) label that pairs with such score rows (`rows`) as N pixels of one channel, and an (N, P, C) blob of an
    SSD head (`rows` as well) as N pixels of P * C channels - the row of its (N, P * C) twin; None for anything else (scalars, per-class
    vectors, the rows of a DetectionOutput: dense floats outside that machinery).  netspec.as_nchw is the rule."""
    if rows and len(shape) == 1:
        return (shape[0], 1, 1, 1)
    if rows and len(shape) == 3:
        return (shape[0], shape[1] * shape[2], 1, 1)
    return as_nchw(shape)


# ---------------------------------------------------------------------- blobs
@dataclass(frozen=True)
class BlobView:
    """Where one blob lies: `coffset` channels into the pixels of the buffer that `root` owns, `cstride` channels per pixel."""
    shape: Tuple[int, ...]
    esize: int                 # bytes per element: 4 (float32) or 2 (half)
    root: str
    coffset: int
    cstride: int
    upload_shift: float        # value added while the blob is uploaded (device copy = host + upload_shift)
    lazy_shift: float          # value added when the blob is read back (Power layer folded into the upload)
    rows: bool                 # an (N,) label blob of a loss / Accuracy over N score rows: N pixels of one channel; an (N, P, C) blob of
    #                            an SSD head: N pixels of P * C channels

    @property
    def nchw(self) -> Optional[Tuple[int, int, int, int]]:
        return blob_nchw(self.shape, self.rows)


@dataclass(frozen=True)
class BlobPlan:
    views: Dict[str, BlobView]
    root_bytes: Dict[str, int]                    # blob that owns a buffer -> its size
    esize: Dict[str, int]
    alias: Dict[str, Tuple[str, int]]             # child blob -> (parent blob, channel offset in parent)
    shift: Dict[str, float]                       # Power top folded into its bottom's upload -> the shift
    copy_concats: Set[str]                        # Concat / Slice layers that copy (the others are views)
    copy_slices: Set[str]
    half_inputs: Dict[str, Tuple[str, float]]     # data top kept as a half image -> (Power top, shift)
    rows: Set[str]
    producers: Dict[str, List[Layer]]
    consumers: Dict[str, List[Layer]]
    # SSD heads.  permutes: top of a Permute(0, 2, 3, 1) -> its bottom (the top owns no buffer: the bottom's NHWC buffer IS that order).
    # gathers: Concat (or lone Flatten) layer -> (top that receives the columns, [(Flatten top, head blob, first column)]): one launch of
    # fcn_ssd_gather_f32 per 16 heads.  detections: top of a DetectionOutput -> rows of capacity (its buffer: 7 floats a row, then the count)
    permutes: Dict[str, str] = field(default_factory=dict)
    gathers: Dict[str, Tuple[str, List[Tuple[str, str, int]]]] = field(default_factory=dict)
    detections: Dict[str, int] = field(default_factory=dict)
    # region stage.  pair_softmax: Softmax layer of an RPN chain Reshape -> Softmax -> Reshape -> (blob the one launch reads, blob it
    # writes, A).  rpn_views: a middle blob of such a chain (it owns nothing) -> (the neighbour whose NCHW array, reshaped, it is)
    pair_softmax: Dict[str, Tuple[str, str, int]] = field(default_factory=dict)
    rpn_views: Dict[str, str] = field(default_factory=dict)


def plan_blobs(spec: NetSpec, shapes: Dict[str, Tuple[int, ...]], inputs: Sequence[str], outputs: Sequence[str],
               f16: bool, fuse: bool, half_image: bool) -> BlobPlan:
    producers: Dict[str, List[Layer]] = {}
    consumers: Dict[str, List[Layer]] = {}
    for l in spec.layers:
        for t in l.tops:
            producers.setdefault(t, []).append(l)
        for b in l.bottoms:
            consumers.setdefault(b, []).append(l)
    heads = [l for l in spec.layers if l.type in ssd.HEAD_TYPES]
    if f16 and heads:
        raise NotImplementedError("f16 engine: layer type %s (%s) has no half-float kernel" % (heads[0].type, heads[0].name))
    stage = [l for l in spec.layers if l.type in region.REGION_TYPES]
    if f16 and stage:
        raise NotImplementedError("f16 engine: layer type %s (%s) has no half-float kernel" % (stage[0].type, stage[0].name))
    # the RPN's two-class softmax: Reshape(0, 2, -1, 0) -> Softmax(axis 1) -> Reshape(0, 2A, -1, 0).  In Caffe's memory order the middle
    # blobs pair channel a with channel a + A at every pixel; on the NHWC device that is no view, so the chain is ONE launch that reads the
    # first Reshape's bottom and writes the second one's top, and the two middle blobs own nothing
    pair_softmax: Dict[str, Tuple[str, str, int]] = {}
    rpn_views: Dict[str, str] = {}
    chain_reshapes: Set[str] = set()
    for l in spec.layers:
        if l.type != "Softmax" or len(l.bottoms) != 1 or int(l.sub("softmax_param").get("axis", 1)) != 1 or f16:
            continue
        r1, r2 = producers.get(l.bottoms[0], []), consumers.get(l.tops[0], [])
        only = [q.name for q in consumers.get(l.bottoms[0], []) if q is not l]
        if len(r1) != 1 or r1[0].type != "Reshape" or len(r2) != 1 or r2[0].type != "Reshape" or only or l.tops[0] in outputs or l.bottoms[0] in outputs:
            continue
        src, dst = r1[0].bottoms[0], r2[0].tops[0]
        a = region.rpn_softmax_anchors(shapes[src], shapes[l.bottoms[0]], shapes[dst])
        if a is None or len(producers.get(l.tops[0], [])) != 1:
            continue
        pair_softmax[l.name] = (src, dst, a)
        rpn_views[l.bottoms[0]] = src
        rpn_views[l.tops[0]] = dst
        chain_reshapes.update((r1[0].name, r2[0].name))
    # the top of a Permute(0, 2, 3, 1) owns nothing: its bottom's NHWC buffer, minus the pad channels, is Caffe's memory order of it
    permutes: Dict[str, str] = {}
    for l in spec.layers:
        if l.type == "Permute":
            order = ssd.permute_order(l, len(shapes[l.bottoms[0]]))
            if len(shapes[l.bottoms[0]]) != 4 or order != (0, 2, 3, 1):
                raise NotImplementedError("layer %s: Permute of a %d-d blob to order %s (only order 0 2 3 1 of a 4-d blob: channels last, "
                                          "the layout the device keeps)" % (l.name, len(shapes[l.bottoms[0]]), list(order)))
            bad = [q.name for q in consumers.get(l.tops[0], []) if q.type != "Flatten"]
            if bad or l.tops[0] in outputs:
                raise NotImplementedError("layer %s: the Permute top %s %s (only Flatten layers may read it)"
                                          % (l.name, l.tops[0], "feeds %s" % bad if bad else "is an output of the net"))
            permutes[l.tops[0]] = l.bottoms[0]
    # the top of a DetectionOutput is dense floats: `capacity` rows of 7, then the int32 count in a 16-byte tail
    detections: Dict[str, int] = {name: int(shapes[name][2]) for name in spec.detection_blobs}
    # a pooling mask is no activation blob: it is the pooling's argmax buffer, which the engine allocates (no view, no buffer here)
    shapes = {name: ((detections[name] * 7 + 4,) if name in detections else shp) for name, shp in shapes.items()
              if name not in spec.mask_blobs and name not in permutes and name not in rpn_views}
    data_tops = set(inputs)
    # f16 mode: everything is stored as halves except what leaves the net towards the f32 decode kernel - the output
    # blobs and the input / output of a Sigmoid head (written by the convolution epilogue in f32)
    # f16 mode, the image itself: the nets shift a [0,1] image by -127 (Power layer), which leaves 16 half-float levels
    # for the whole input range - but a convolution is linear, conv(x + s) = conv(x) + s * conv(indicator), and the
    # indicator of "inside the image" is what zero padding makes of a constant-1 channel.  The half image therefore
    # holds the UN-shifted pixels in channels 0..2 and the constant 1 in channels 3 and 4 of its 8-channel segment
    # (written once), and the first convolution's filters carry s * sum_c(w_c) per tap in those two channels, split
    # into a half and its rounding remainder (pack): exact to 2^-22 of the shift term.
    half_inputs: Dict[str, Tuple[str, float]] = {}
    if f16 and fuse and half_image:
        for d in data_tops:
            cons = consumers.get(d, [])
            if len(shapes[d]) != 4 or shapes[d][1] > 3 or len(cons) != 1 or cons[0].type != "Power":
                continue
            pw = cons[0].sub("power_param")
            t = cons[0].tops[0]
            if (float(pw.get("power", 1.0)) != 1.0 or float(pw.get("scale", 1.0)) != 1.0 or t == d or t in outputs
                    or [q.type for q in consumers.get(t, [])] != ["Convolution"] or spec.is_depthwise(consumers[t][0])):
                continue
            half_inputs[d] = (t, float(pw.get("shift", 0.0)))
    halves = set(half_inputs) | {t for t, _s in half_inputs.values()}
    esize: Dict[str, int] = {}
    for name, shp in shapes.items():
        if name in halves:
            esize[name] = 2
            continue
        wide = (not f16 or len(shp) not in (2, 4) or name in outputs or name in data_tops      # inputs stay float32 (Power(-127) quirk)
                or any(q.type == "Power" and q.bottoms[0] in data_tops for q in producers.get(name, []))
                or any(q.type == "Sigmoid" for q in consumers.get(name, [])) or any(q.type in ("Sigmoid", "ArgMax") for q in producers.get(name, [])))
        esize[name] = 4 if wide else 2
    if f16:
        for l in spec.layers:      # labels and ranks are float32: nothing of the half-float path reads them
            if l.type == "ArgMax" and consumers.get(l.tops[0]):
                q = consumers[l.tops[0]][0]
                raise NotImplementedError("f16 engine: layer %s (%s) reads %s, the float32 top of ArgMax %s" % (q.name, q.type, l.tops[0], l.name))
        for name in shapes:
            if esize[name] == 4 and len(shapes[name]) in (2, 4) and name not in data_tops:
                # (Softmax, Deconvolution, Interp, Upsample and Crop read halves and store float32: the out_f32 forms of their half kernels;
                # the top of an ArgMax is float32 in both engines, as Caffe's is)
                bad = [q.type for q in producers.get(name, []) if q.type not in ("Convolution", "Sigmoid", "Power", "Softmax", "Deconvolution", "InnerProduct",
                                                                                 "Interp", "DepthwiseConvolution", "Upsample", "ArgMax", "Crop")]
                if bad:
                    raise NotImplementedError("f16 engine: float32 blob %s is produced by %s" % (name, bad))

    alias: Dict[str, Tuple[str, int]] = {}
    shift: Dict[str, float] = {}
    copy_concats: Set[str] = set()
    copy_slices: Set[str] = set()
    gathers: Dict[str, Tuple[str, List[Tuple[str, str, int]]]] = {}
    for l in spec.layers:
        if l.type == "Concat" and l.tops[0] in spec.prior_blobs:
            continue      # SSD's mbox_priorbox: a constant with a buffer of its own, like the PriorBox tops beside it
        if l.type == "Flatten":
            top, bot = l.tops[0], l.bottoms[0]
            bshape = spec.blob_shapes[bot]
            if bot in permutes:
                # Caffe's memory order of the Permute top, per image: the head's pixels x real channels.  One Concat(axis 1) that is the only
                # reader of all its Flatten bottoms receives them directly (below); any other Flatten of this kind is a gather of one head
                gathers[l.name] = (top, [(top, permutes[bot], 0)])
            elif len(bshape) == 3 or (len(bshape) == 4 and bshape[2] == bshape[3] == 1):
                alias[top] = (bot, 0)      # the same floats per image, at the same row stride
            else:
                raise NotImplementedError("layer %s: Flatten of the %s blob %s (Caffe's C x H x W order of a row is not the device's: Flatten "
                                          "the top of a Permute(0, 2, 3, 1), an (N, P, C) blob or a blob with H = W = 1)" % (l.name, tuple(bshape), bot))
        elif l.type == "Reshape" and l.name in chain_reshapes:
            pass      # the RPN softmax chain: its Softmax layer launches for all three
        elif l.type == "Reshape":
            top, bot = l.tops[0], l.bottoms[0]
            a, b = spec.blob_shapes[bot], spec.blob_shapes[top]
            if not ((len(a), len(b)) in ((2, 3), (3, 2)) and a[0] == b[0]) or bot in data_tops:
                raise NotImplementedError("layer %s: Reshape of %s to %s (only between (N, K) and (N, P, C) with P * C == K, or the RPN's chain "
                                          "Reshape(0, 2, -1, 0) -> Softmax -> Reshape(0, 2A, -1, 0) whose middle blobs nothing else reads)"
                                          % (l.name, tuple(a), tuple(b)))
            alias[top] = (bot, 0)
        if l.type == "Concat" and l.bottoms and all(
                len(producers.get(b, [])) == 1 and producers[b][0].name in gathers and [q.name for q in consumers.get(b, [])] == [l.name]
                and b not in outputs for b in l.bottoms) and len(set(l.bottoms)) == len(l.bottoms):
            # the mbox_loc / mbox_conf form: every bottom is the Flatten of a Permute top and nothing else reads it
            off, cols = 0, []
            for b in l.bottoms:
                cols.append((b, gathers.pop(producers[b][0].name)[1][0][1], off))
                alias[b] = (l.tops[0], off)
                off += shapes[b][1]
            gathers[l.name] = (l.tops[0], cols)
            continue
        if l.type == "Concat":
            off = 0
            ok = True
            plan = []
            for b in l.bottoms:
                c = shapes[b][1]
                prods = [p for p in producers.get(b, []) if not (p.type in ("ReLU", "Dropout") and p.bottoms == p.tops)]
                good = (fuse and b not in data_tops and b not in alias and c % (16 // esize[b]) == 0 and len(prods) == 1
                        and esize[b] == esize[l.tops[0]]
                        and prods[0].type in ("Convolution", "Pooling", "InnerProduct")
                        and [q.type for q in consumers.get(b, []) if not (q.type in ("ReLU", "Dropout") and q.bottoms == q.tops)] == ["Concat"])
                ok = ok and good
                plan.append((b, off))
                off += c
            if ok:
                for b, o in plan:
                    alias[b] = (l.tops[0], o)
            else:
                copy_concats.add(l.name)
        elif l.type == "Dropout" and spec.phase == "TEST" and l.tops[0] != l.bottoms[0]:
            alias[l.tops[0]] = (l.bottoms[0], 0)       # identity at test time: share the view
        elif l.type == "Power" and fuse and l.tops[0] != l.bottoms[0]:
            # Power(shift) directly on a net input that nothing else reads: the upload adds the shift, the
            # device buffer holds the transformed blob and both names share it
            p = l.sub("power_param")
            bot = l.bottoms[0]
            if (float(p.get("power", 1.0)) == 1.0 and float(p.get("scale", 1.0)) == 1.0 and bot in data_tops
                    and bot not in alias and len(consumers.get(bot, [])) == 1 and len(shapes[bot]) == 4):
                alias[l.tops[0]] = (bot, 0)
                shift[l.tops[0]] = float(p.get("shift", 0.0))
        elif l.type == "Slice":
            # tops are views of the bottom when every consumer can read a channel slice at a 16-byte aligned offset;
            # otherwise (models/train_val.prototxt slices a 17-channel label record at 1, 5, 9, 13 for Eltwise layers)
            # the slices are materialised by copies
            offs, off = [], 0
            for t in l.tops:
                offs.append(off)
                off += shapes[t][1]
            viewable = all(o % (16 // esize[l.bottoms[0]]) == 0 for o in offs) and all(
                q.type in ("Convolution", "Pooling", "Concat") for t in l.tops for q in consumers.get(t, []))
            if viewable:
                for t, o in zip(l.tops, offs):
                    alias[t] = (l.bottoms[0], o)
            else:
                copy_slices.add(l.name)

    rows: Set[str] = set()
    for l in spec.layers:      # Caffe's data layers emit (N,) labels: beside N score rows such a blob is N pixels of one channel
        if l.type in ("SoftmaxWithLoss", "Accuracy") and len(l.bottoms) == 2:
            score, lab = shapes[l.bottoms[0]], shapes[l.bottoms[1]]
            if len(score) == 2 and tuple(lab) == (score[0],):
                rows.add(l.bottoms[1])
        # an SSD head's 3-d blobs - (N, P, C) scores, (1, 2, P * 4) priors - are rows of P * C floats per image, like their 2-d twins
        if (l.type in ("Reshape", "PriorBox") or l.tops[:1] and l.tops[0] in spec.prior_blobs
                or l.type == "Softmax" and l.bottoms[0] in rows) and len(shapes.get(l.tops[0], ())) == 3:
            rows.add(l.tops[0])
        # the legacy ArgMax top (N, 1 or 2, top_k) is a row per image: the indices, then - with out_max_val - the values
        if l.type == "ArgMax" and len(shapes.get(l.tops[0], ())) == 3:
            rows.add(l.tops[0])

    # roots own a buffer; every other blob resolves through its chain of parents to a channel window of one
    cstride: Dict[str, int] = {}
    root_bytes: Dict[str, int] = {}
    for name, shp in shapes.items():
        if name in alias:
            continue
        g = blob_nchw(shp, name in rows)
        if g is not None:
            cstride[name] = _ra(g[1], esize[name])
            root_bytes[name] = g[0] * g[2] * g[3] * cstride[name] * esize[name]
        else:
            cstride[name] = 1
            root_bytes[name] = max(16, 4 * int(np.prod(shp)) if shp else 16)
    window: Dict[str, Tuple[str, int]] = {name: (name, 0) for name in root_bytes}
    upload_shift: Dict[str, float] = {}
    lazy_shift: Dict[str, float] = {}
    for name in alias:
        root, off = name, 0
        total_shift = 0.0
        seen = 0
        while root in alias:
            total_shift += shift.get(root, 0.0)
            root, o = alias[root]
            off += o
            seen += 1
            if seen > 64:
                raise RuntimeError("alias cycle at blob %s" % name)
        if esize[name] != esize[root]:
            raise NotImplementedError("f16 engine: blob %s (%d-byte elements) is a view of %s (%d-byte)" % (name, esize[name], root, esize[root]))
        window[name] = (root, off)
        if total_shift and root in half_inputs:
            lazy_shift[name] = total_shift        # the device keeps the un-shifted half image: reading the Power top adds the shift
        elif total_shift:
            upload_shift[root] = total_shift      # device copy of the input = host value + shift
            lazy_shift[root] = -total_shift       # reading the input back undoes it
    views = {name: BlobView(tuple(shp), esize[name], window[name][0], window[name][1], cstride[window[name][0]],
                            upload_shift.get(name, 0.0), lazy_shift.get(name, 0.0), name in rows)
             for name, shp in shapes.items()}
    return BlobPlan(views, root_bytes, esize, alias, shift, copy_concats, copy_slices, half_inputs, rows, producers, consumers,
                    permutes, gathers, detections, pair_softmax, rpn_views)


# ---------------------------------------------------------------------- parameters
CONV, INNER_PRODUCT, DECONV, PLAIN, DEPTHWISE = "conv", "inner_product", "deconv", "plain", "depthwise"


@dataclass(frozen=True)
class ParamSeg:
    """One parameter blob's segment of the flat parameter buffer."""
    layer: str
    index: int
    kind: str                            # CONV: OHWI, Cin padded to whole 16-byte segments of the bottom's elements
    #                                      INNER_PRODUCT: [num_output][H*W*cstride], the columns in the order of a row of the NHWC bottom
    #                                      DECONV (group 1): [Cin][kh][kw][Cout padded to 4], an OHWI bank of Cin outputs over Cout inputs
    #                                      (halves, Cout padded to 8, in a half-float engine whose NetSpec has tconv_f16)
    #                                      DEPTHWISE: [kh][kw][C padded to whole 16-byte segments of the bottom's elements], always float32
    #                                      PLAIN: as it is (biases, the depthwise Deconvolution's filters)
    offset: int                          # in 4-byte words (= floats in the f32 engine, where the solver and RCCL index the buffer)
    count: int                           # elements on the device
    shape: Tuple[int, ...]               # on the device
    host_shape: Tuple[int, ...]          # Caffe's
    lr_mult: float
    decay_mult: float
    nbytes: int
    esize: int                           # 4, or 2: a bank of halves (half-float engine, CONV / INNER_PRODUCT / DECONV over a half bottom)
    bottom: Optional[Tuple[int, int, int, int]] = None      # INNER_PRODUCT: c, h, w, cstride of the bottom


def param_layout(spec: NetSpec, views, f16: bool, skip: Sequence[str] = ()) -> Tuple[List[ParamSeg], int]:
    """All learnable blobs live in ONE flat device buffer in the kernels' layout: the segments of every parameter layer not in
    `skip`, in layer order, and the buffer's length in words.  `views`: blob name -> its view (esize, coffset, cstride, nchw)."""
    segs: List[ParamSeg] = []
    off = 0
    for l in spec.param_layers():
        if l.name in skip:
            continue
        for i, host_shape in enumerate(tuple(int(v) for v in s) for s in spec.param_shapes[l.name]):
            kind, shape, esize, bottom = PLAIN, host_shape, 4, None
            if i == 0 and spec.is_depthwise(l):
                # tap-major, channel-contiguous, float32 whatever the bottom holds: a lane that owns a 16-byte channel segment of the
                # bottom fetches a tap's weights with one 16-byte load (csrc/dwconv.hip); conv_groups is not asked
                c, _one, kh, kw = host_shape
                kind, shape = DEPTHWISE, (kh, kw, _ra(c, views[l.bottoms[0]].esize))
            elif i == 0 and l.type == "Convolution":
                esize = views[l.bottoms[0]].esize          # element type of the layer's input: 16-byte segments of it
                co, ci, kh, kw = host_shape
                conv_groups(l, co, ci, esize)
                kind, shape = CONV, (co, kh, kw, _ra(ci, esize))
            elif i == 0 and l.type == "InnerProduct":
                # the bottom must be a whole buffer: a row of it is then the layer's input vector as it lies in memory
                xb = views[l.bottoms[0]]
                if xb.nchw is None or xb.coffset or xb.cstride != _ra(xb.nchw[1], xb.esize):
                    raise NotImplementedError("InnerProduct %s: the bottom %s is a channel window of a wider buffer (or no 4-d / 2-d blob)"
                                              % (l.name, l.bottoms[0]))
                _n, c, h, w = xb.nchw
                kind, shape, esize, bottom = INNER_PRODUCT, (host_shape[0], h * w * xb.cstride), xb.esize, (c, h, w, xb.cstride)
            elif i == 0 and l.type == "Deconvolution":
                # group == channels == num_output: the depthwise kernels, filters as they are; group 1: the transposed-convolution kernel
                # and its bank.  Every other grouping is refused, by name.
                c, cog, kh, kw = host_shape
                p = l.sub("convolution_param")
                g, co = int(p.get("group", 1)), int(p.get("num_output"))
                if g == c and co == c:
                    shape = (c, kh, kw)
                elif g != 1:
                    raise NotImplementedError("Deconvolution %s: group %d with %d -> %d channels (only group 1 and group == channels == num_output)"
                                              % (l.name, g, c, co))
                elif f16 and not spec.tconv_f16:
                    raise NotImplementedError("f16 engine: layer type Deconvolution with group 1 (%s) has no half-float kernel" % l.name)
                elif f16:
                    # the half-float transposed convolution (csrc/tconv.hip, fcn_tconv2d_f16): inference over a half bottom, a bank of halves
                    if spec.phase == "TRAIN":
                        raise NotImplementedError("f16 engine: Deconvolution %s with group 1 in a TRAIN net (half-float training)" % l.name)
                    if views[l.bottoms[0]].esize != 2:
                        raise NotImplementedError("f16 engine: Deconvolution %s reads the float32 blob %s" % (l.name, l.bottoms[0]))
                    kind, shape, esize = DECONV, (c, kh, kw, _ra(cog, 2)), 2
                else:
                    kind, shape = DECONV, (c, kh, kw, _r4(cog))
            elif i == 0 and l.type not in ("BatchNorm", "Scale", "Normalize", "PReLU", "Bias"):      # (their blobs are per-channel vectors as they are: PLAIN)
                raise NotImplementedError(l.type)
            count = int(np.prod(shape))
            lr, decay = float(l.lr_mult[i] if i < len(l.lr_mult) else 1.0), float(l.decay_mult[i] if i < len(l.decay_mult) else 1.0)
            if l.type == "BatchNorm":
                lr = decay = 0.0      # statistics, written by the forward pass alone: the solver never moves them, whatever the prototxt says
            segs.append(ParamSeg(l.name, i, kind, off, count, shape, host_shape, lr, decay, count * esize, esize, bottom))
            off += _r4((count * esize + 3) // 4)
    return segs, off


def conv_groups(l: Layer, cout: int, cin_g: int, esize: int) -> int:
    """`group` of a Convolution whose blob is (cout, cin_g, k, k).  A (Cout, Cin/g, k, k) blob lies as [Cout][kh][kw][ra(Cin/g)]: group i's
    bank is the contiguous run of rows i*Cout/g .. (i+1)*Cout/g, an ordinary OHWI bank, PROVIDED the group's channels start on a
    16-byte segment of the bottom and of the top - Cin/g and Cout/g whole numbers of segments (4 floats / 8 halves).  Anything else
    is refused here, by layer name (depthwise convolution among them)."""
    g = int(l.sub("convolution_param").get("group", 1))
    if g == 1:
        return 1
    eps = 16 // esize
    if g < 1 or cout % g:
        raise ValueError("Convolution %s: group %d does not divide num_output %d" % (l.name, g, cout))
    if cin_g % eps or (cout // g) % eps:
        raise NotImplementedError("grouped Convolution %s: group %d leaves %d input and %d output channels per group, not whole 16-byte "
                                  "segments (%d %s)%s" % (l.name, g, cin_g, cout // g, eps, "floats" if esize == 4 else "halves",
                                                          ": depthwise convolution has no kernel here for a NetSpec built without "
                                                          "depthwise=True (caffe.Net and the solvers pass it; type DepthwiseConvolution "
                                                          "needs no keyword)" if cin_g == 1 else ""))
    return g


def ip_pack_bank(w: np.ndarray, c: int, h: int, wd: int, cstride: int, dtype=F32) -> np.ndarray:
    """Caffe's (num_output, C*H*W) InnerProduct bank -> (num_output, H*W*cstride) in the memory order of a row of the NHWC bottom:
    column p * cstride + ch holds Caffe's column ch * H*W + p, the pad channels' columns are zero."""
    n = w.shape[0]
    out = np.zeros((n, h * wd, cstride), dtype)
    out[:, :, :c] = w.reshape(n, c, h * wd).transpose(0, 2, 1)
    return out.reshape(n, h * wd * cstride)


def ip_unpack_bank(packed: np.ndarray, c: int, h: int, wd: int, cstride: int) -> np.ndarray:
    """The inverse of ip_pack_bank, as float32 and always a copy: what read_param and snapshots return."""
    n = packed.shape[0]
    return np.array(packed.reshape(n, h * wd, cstride)[:, :, :c].transpose(0, 2, 1), dtype=F32, order="C").reshape(n, c * h * wd)


def pack(seg: ParamSeg, host_blob: np.ndarray, folded_shift: float = 0.0) -> np.ndarray:
    """A Caffe-layout blob as the device holds it (pad channels zero).  folded_shift: the Power shift of a half image, carried by
    channels 3 and 4 of the first convolution's filters."""
    a = np.asarray(host_blob, F32).reshape(seg.host_shape)
    dtype = np.float16 if seg.esize == 2 else F32
    if seg.kind == INNER_PRODUCT:
        return ip_pack_bank(a, *seg.bottom, dtype)
    if seg.kind == PLAIN:
        return np.ascontiguousarray(a.reshape(seg.shape))
    if seg.kind == DEPTHWISE:               # Caffe's (C, 1, kh, kw) -> [kh][kw][C padded]
        out = np.zeros(seg.shape, F32)
        out[..., :seg.host_shape[0]] = a[:, 0].transpose(1, 2, 0)
        return out
    n = seg.host_shape[1]                   # CONV: Cin; DECONV: Cout, which its data gradient (a forward convolution of dY) reads as Cin
    out = np.zeros(seg.shape, dtype)
    out[..., :n] = a.transpose(0, 2, 3, 1)
    if folded_shift:
        # channels 3 and 4 see the constant 1 (zero in the padding, like the shifted image)
        term = np.float64(folded_shift) * out[..., :n].astype(np.float64).sum(-1)      # of the ROUNDED filters: what the device multiplies
        hi = term.astype(np.float16)
        out[..., 3] = hi
        out[..., 4] = (term - hi.astype(np.float64)).astype(np.float16)
    return out


def unpack(seg: ParamSeg, raw: np.ndarray) -> np.ndarray:
    """The inverse of pack: the segment's words (or bytes) as read from the device -> float32 in Caffe's layout, a copy.  Pad
    channels are dropped, the folded-shift channels of a half first layer among them."""
    a = raw.reshape(-1).view(np.float16 if seg.esize == 2 else F32)[:seg.count].reshape(seg.shape)
    if seg.kind == INNER_PRODUCT:
        return ip_unpack_bank(a, *seg.bottom)
    if seg.kind in (CONV, DECONV):
        a = a[..., :seg.host_shape[1]].transpose(0, 3, 1, 2)
    if seg.kind == DEPTHWISE:
        a = a[..., :seg.host_shape[0]].transpose(2, 0, 1)
    return np.array(a.reshape(seg.host_shape), dtype=F32, order="C")
