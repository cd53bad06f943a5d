"""Programmatic builders for the detector networks the reference ships as prototxt.

The engine consumes the reference's prototxt files unmodified (``caffe.Net(path, ...)``).  These
builders exist because /root/reference is not available on the GPU box: bench.py, smoke() and the
GPU tests need the same networks without carrying the reference's files.  They emit prototxt TEXT
that parses to the same layer graph (names, types, bottoms/tops, kernel geometry, fillers,
lr/decay multipliers) as

  * ``googlenet_detectnet_deploy``  <->  reference models/deploy.prototxt
  * ``googlenet_detectnet_train``   <->  reference models/train_val.prototxt with the LMDB Data +
                                         Slice front replaced by the Python data layer's tops, as the
                                         reference README (:57-76) instructs
  * ``vgg16_fcn_bbox``              <->  reference train/fcn_bbox/train_val.prototxt (bbox branch + seg branch)

tests/test_models.py checks that equivalence layer by layer whenever /root/reference is present.

``caffenet`` / ``goturn_tracker`` / ``bvlc_googlenet`` are not files of the reference either: they emit the structure of the published
BVLC reference CaffeNet, of the GOTURN tracker (Held, Thrun, Savarese: "Learning to Track at 100 FPS with Deep Regression Networks")
and of BVLC GoogLeNet with its auxiliary heads - the nets the reference's curation scripts run through pycaffe and the net its
detector body is fine-tuned from.

``voc_fcn32s`` / ``voc_fcn16s`` / ``voc_fcn8s`` are not reference nets: they emit the structure of the published FCN nets for
PASCAL VOC (Long, Shelhamer, Darrell: "Fully Convolutional Networks for Semantic Segmentation") - VGG16 with ``pad: 100`` on
conv1_1, convolutional fc6 / fc7, group-1 Deconvolution upsampling and ``Crop`` layers aligning the skip connections and the
score map - as test and tool material.

``deeplab_largefov`` / ``deeplab_aspp`` emit the structure of DeepLab-LargeFOV and of the DeepLab-v2 ASPP head on VGG16 (Chen et al.):
the stride-8 VGG16 body with dilated conv5_* and a dilated 3x3 fc6 (one per rate in the ASPP head); ``interp=True`` adds the
published ``Interp`` layers (fc8_interp, label_shrink).  The published ImageSegData layer is not emitted.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

# (module, 1x1, 3x3_reduce, 3x3, 5x5_reduce, 5x5, pool_proj) — GoogLeNet v1 widths
INCEPTION = [
    ("inception_3a", 64, 96, 128, 16, 32, 32),
    ("inception_3b", 128, 128, 192, 32, 96, 64),
    ("inception_4a", 192, 96, 208, 16, 48, 64),
    ("inception_4b", 160, 112, 224, 24, 64, 64),
    ("inception_4c", 128, 128, 256, 24, 64, 64),
    ("inception_4d", 112, 144, 288, 32, 64, 64),
    ("inception_4e", 256, 160, 320, 32, 128, 128),
    ("inception_5a", 256, 160, 320, 32, 128, 128),
    ("inception_5b", 384, 192, 384, 48, 128, 128),
]


# the reference gives this one bias lr_mult 1 instead of 2 (models/deploy.prototxt:1926-1957); reproduced, not fixed
BIAS_LR_QUIRK = {"inception_5b/3x3_reduce": (1.0, 1.0)}


class _Writer:
    def __init__(self) -> None:
        self.lines: List[str] = []

    def raw(self, s: str) -> None:
        self.lines.append(s)

    def layer(self, name: str, type_: str, bottoms: Sequence[str], tops: Sequence[str], body: str = "",
              quote: str = '"', extra: str = "") -> None:
        s = ["layer {", '  name: "%s"' % name, "  type: %s%s%s" % (quote, type_, quote)]
        s += ['  bottom: "%s"' % b for b in bottoms]
        s += ['  top: "%s"' % t for t in tops]
        if extra:
            s.append(extra)
        if body:
            s.append(body)
        s.append("}")
        self.lines.append("\n".join(s))

    def text(self) -> str:
        return "\n".join(self.lines) + "\n"


def _conv_body(num_output: int, k: int, pad: int = 0, stride: int = 1, bias_value: float = 0.2,
               lr: Tuple[float, float] = (1.0, 2.0), decay: Tuple[float, float] = (1.0, 0.0), explicit: bool = False) -> str:
    s = ["  param { lr_mult: %g decay_mult: %g }" % (lr[0], decay[0]),
         "  param { lr_mult: %g decay_mult: %g }" % (lr[1], decay[1]),
         "  convolution_param {", "    num_output: %d" % num_output]
    if pad or explicit:                      # explicit: True = write pad and stride even at their defaults, "pad" = pad only
        s.append("    pad: %d" % pad)
    s.append("    kernel_size: %d" % k)
    if stride != 1 or explicit is True:
        s.append("    stride: %d" % stride)
    s += ['    weight_filler { type: "xavier" }', '    bias_filler { type: "constant" value: %g }' % bias_value, "  }"]
    return "\n".join(s)


def _conv_relu(w: _Writer, name: str, relu_name: str, bottom: str, num_output: int, k: int, pad: int = 0, stride: int = 1) -> None:
    w.layer(name, "Convolution", [bottom], [name], _conv_body(num_output, k, pad, stride, lr=BIAS_LR_QUIRK.get(name, (1.0, 2.0))))
    w.layer(relu_name, "ReLU", [name], [name])


def _pool(w: _Writer, name: str, bottom: str, k: int, stride: int, pad: int = 0) -> None:
    body = "  pooling_param { pool: MAX kernel_size: %d stride: %d%s }" % (k, stride, " pad: %d" % pad if pad else "")
    w.layer(name, "Pooling", [bottom], [name], body)


def _lrn(w: _Writer, name: str, bottom: str) -> None:
    w.layer(name, "LRN", [bottom], [name], "  lrn_param { local_size: 5 alpha: 0.0001 beta: 0.75 }")


def _googlenet_body(w: _Writer, data_blob: str, bvlc_div: int = 0):
    """GoogLeNet v1 to the last inception module.  bvlc_div 0: the DetectNet body (input shift, no pool4, Dropout behind inception_5b),
    returns its last blob.  bvlc_div d > 0: the body of BVLC GoogLeNet at widths / d - no input shift, pool4/3x3_s2 behind
    inception_4e, no Dropout - returns (last blob, the taps of the auxiliary heads behind inception_4a and inception_4d)."""
    wd = (lambda c: max(c // bvlc_div, 1)) if bvlc_div else (lambda c: c)
    taps: List[str] = []
    if not bvlc_div:
        w.layer("deploy_transform", "Power", [data_blob], ["transformed_data"], "  power_param { shift: -127.0 }")
        data_blob = "transformed_data"
    _conv_relu(w, "conv1/7x7_s2", "conv1/relu_7x7", data_blob, wd(64), 7, 3, 2)
    _pool(w, "pool1/3x3_s2", "conv1/7x7_s2", 3, 2)
    _lrn(w, "pool1/norm1", "pool1/3x3_s2")
    _conv_relu(w, "conv2/3x3_reduce", "conv2/relu_3x3_reduce", "pool1/norm1", wd(64), 1)
    _conv_relu(w, "conv2/3x3", "conv2/relu_3x3", "conv2/3x3_reduce", wd(192), 3, 1)
    _lrn(w, "conv2/norm2", "conv2/3x3")
    _pool(w, "pool2/3x3_s2", "conv2/norm2", 3, 2)
    prev = "pool2/3x3_s2"
    for mod, c1, c3r, c3, c5r, c5, cp in INCEPTION:
        _conv_relu(w, mod + "/1x1", mod + "/relu_1x1", prev, wd(c1), 1)
        _conv_relu(w, mod + "/3x3_reduce", mod + "/relu_3x3_reduce", prev, wd(c3r), 1)
        _conv_relu(w, mod + "/3x3", mod + "/relu_3x3", mod + "/3x3_reduce", wd(c3), 3, 1)
        _conv_relu(w, mod + "/5x5_reduce", mod + "/relu_5x5_reduce", prev, wd(c5r), 1)
        _conv_relu(w, mod + "/5x5", mod + "/relu_5x5", mod + "/5x5_reduce", wd(c5), 5, 2)
        _pool(w, mod + "/pool", prev, 3, 1, 1)
        _conv_relu(w, mod + "/pool_proj", mod + "/relu_pool_proj", mod + "/pool", wd(cp), 1)
        w.layer(mod + "/output", "Concat", [mod + "/1x1", mod + "/3x3", mod + "/5x5", mod + "/pool_proj"], [mod + "/output"])
        prev = mod + "/output"
        if mod == "inception_3b":
            _pool(w, "pool3/3x3_s2", prev, 3, 2)
            prev = "pool3/3x3_s2"
        if bvlc_div and mod in ("inception_4a", "inception_4d"):
            taps.append(prev)
        if bvlc_div and mod == "inception_4e":
            _pool(w, "pool4/3x3_s2", prev, 3, 2)
            prev = "pool4/3x3_s2"
    if bvlc_div:
        return prev, taps
    w.layer("pool5/drop_s1", "Dropout", [prev], ["pool5/drop_s1"], "  dropout_param { dropout_ratio: 0.4 }")
    return "pool5/drop_s1"


def _heads(w: _Writer, feat: str, num_classes: int) -> None:
    w.layer("cvg/classifier", "Convolution", [feat], ["cvg/classifier"], _conv_body(num_classes, 1, bias_value=0.0))
    w.layer("coverage/sig", "Sigmoid", ["cvg/classifier"], ["coverage"])
    w.layer("bbox/regressor", "Convolution", [feat], ["bboxes"], _conv_body(4 * num_classes, 1, bias_value=0.0))


def googlenet_detectnet_deploy(batch: int = 1, height: int = 448, width: int = 448, num_classes: int = 4) -> str:
    """Inference net: input ``data`` -> ``coverage`` (C x H/16 x W/16) and ``bboxes`` (4C x H/16 x W/16)."""
    w = _Writer()
    w.raw('input: "data"\ninput_shape {\n  dim: %d\n  dim: 3\n  dim: %d\n  dim: %d\n}' % (batch, height, width))
    feat = _googlenet_body(w, "data")
    _heads(w, feat, num_classes)
    return w.text()


def _python_data_layers(w: _Writer, name: str, tops: List[str], module: str, layer: str, param_str: str,
                        test_param_str: Optional[str]) -> None:
    """The Python data layer; with test_param_str twice, `include { phase: TRAIN }` with param_str and `include { phase: TEST }`
    with test_param_str - the validation copy with its own geometry of train/bounding_box/train_val.prototxt lines 1-36."""
    body = "  python_param {\n    module: '%s'\n    layer: '%s'\n    param_str: '%s'\n  }"
    if test_param_str is None:
        w.layer(name, "Python", [], tops, body % (module, layer, param_str), quote="'")
        return
    for phase, ps in (("TRAIN", param_str), ("TEST", test_param_str)):
        w.layer(name, "Python", [], tops, body % (module, layer, ps) + "\n  include { phase: %s }" % phase, quote="'")


def googlenet_detectnet_train(module: str, layer: str, param_str: str, num_classes: int = 1, test_param_str: Optional[str] = None) -> str:
    """Training net: Python data layer (6 tops) -> GoogLeNet body -> masked/normalised L1 + Euclidean losses.  test_param_str adds a
    TEST-phase copy of the data layer (the solver's test net)."""
    w = _Writer()
    tops = ["data", "coverage-label", "bbox-label", "size-block", "obj-block", "coverage-block"]
    _python_data_layers(w, "data", tops, module, layer, param_str, test_param_str)
    prod = "  eltwise_param { operation: PROD }"
    w.layer("bb-label-norm", "Eltwise", ["bbox-label", "size-block"], ["bbox-label-norm"], prod)
    w.layer("bb-obj-norm", "Eltwise", ["bbox-label-norm", "obj-block"], ["bbox-obj-label-norm"], prod)
    feat = _googlenet_body(w, "data")
    _heads(w, feat, num_classes)
    w.layer("bbox_mask", "Eltwise", ["bboxes", "coverage-block"], ["bboxes-masked"], prod)
    w.layer("bbox-norm", "Eltwise", ["bboxes-masked", "size-block"], ["bboxes-masked-norm"], prod)
    w.layer("bbox-obj-norm", "Eltwise", ["bboxes-masked-norm", "obj-block"], ["bboxes-obj-masked-norm"], prod)
    w.layer("bbox_loss", "L1Loss", ["bboxes-obj-masked-norm", "bbox-obj-label-norm"], ["loss_bbox"], extra="  loss_weight: 2.0")
    w.layer("coverage_loss", "EuclideanLoss", ["coverage", "coverage-label"], ["loss_coverage"])
    return w.text()


def googlenet_detectnet_train_lmdb(features_db: str = "/home/krishneel/Desktop/lmdb/features", labels_db: str = "/home/krishneel/Desktop/lmdb/labels",
                                   batch: int = 1, num_classes: int = 1, head_classes: Optional[int] = None) -> str:
    """The reference's models/train_val.prototxt as it stands (models/train_val2.prototxt = head_classes 3 over the SAME
    1-class slice points: the reference's own inconsistency, reproduced when asked for): two LMDB `Data` layers (image, 17-channel label record), a
    `Slice` that cuts the record into coverage-label / bbox-label / size-block / obj-block / coverage-block, then the same
    body and loss tail as googlenet_detectnet_train.  LMDB reading is out of scope: with this engine the two
    Data tops are input blobs the caller fills (pycaffe `net.blobs['data'].data[...] = ...`)."""
    w = _Writer()
    for name, top, src in (("train_data", "data", features_db), ("train_label", "label", labels_db)):
        body = "  include { phase: TRAIN }\n  data_param {\n    source: \"%s\"\n    batch_size: %d\n    backend: LMDB\n  }" % (src, batch)
        w.layer(name, "Data", [], [top], body)
    c = num_classes
    pts = (c, 5 * c, 9 * c, 13 * c)
    slice_tops = ["coverage-label", "bbox-label", "size-block", "obj-block", "coverage-block"]
    slice_body = "  slice_param {\n    slice_dim: 1\n" + "".join("    slice_point: %d\n" % p for p in pts) + "  }"
    prod = "  eltwise_param { operation: PROD }"
    feat_w = _Writer()
    feat = _googlenet_body(feat_w, "data")
    body_layers = feat_w.lines
    w.lines.append(body_layers[0])                                   # deploy_transform (Power) sits in front of the Slice
    w.layer("slice-label", "Slice", ["label"], slice_tops, slice_body)
    w.layer("bb-label-norm", "Eltwise", ["bbox-label", "size-block"], ["bbox-label-norm"], prod)
    w.layer("bb-obj-norm", "Eltwise", ["bbox-label-norm", "obj-block"], ["bbox-obj-label-norm"], prod)
    w.lines.extend(body_layers[1:])
    _heads(w, feat, head_classes or num_classes)
    w.layer("bbox_mask", "Eltwise", ["bboxes", "coverage-block"], ["bboxes-masked"], prod)
    w.layer("bbox-norm", "Eltwise", ["bboxes-masked", "size-block"], ["bboxes-masked-norm"], prod)
    w.layer("bbox-obj-norm", "Eltwise", ["bboxes-masked-norm", "obj-block"], ["bboxes-obj-masked-norm"], prod)
    w.layer("bbox_loss", "L1Loss", ["bboxes-obj-masked-norm", "bbox-obj-label-norm"], ["loss_bbox"], extra="  loss_weight: 2.0")
    w.layer("coverage_loss", "EuclideanLoss", ["coverage", "coverage-label"], ["loss_coverage"])
    return w.text()


# VGG16 conv stack: (block, number of convs, width)
VGG16 = [(1, 2, 64), (2, 2, 128), (3, 3, 256), (4, 3, 512), (5, 3, 512)]


def _vgg16_body(w: _Writer, data_blob: str) -> None:
    prev = data_blob
    for blk, n, width_ in VGG16:
        for i in range(1, n + 1):
            nm = "conv%d_%d" % (blk, i)
            w.layer(nm, "Convolution", [prev], [nm], _conv_body(width_, 3, 1, explicit=True))
            w.layer("relu%d_%d" % (blk, i), "ReLU", [nm], [nm])
            prev = nm
        body = "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }"
        w.layer("pool%d" % blk, "Pooling", [prev], ["pool%d" % blk], body)
        prev = "pool%d" % blk
    w.layer("dropout5", "Dropout", ["pool5"], ["dropout5"], "  dropout_param { dropout_ratio: 0.5 }")


def _frozen_bilinear_deconv(w: _Writer, name: str, bottom: str, ch: int, k: int, s: int, p: int) -> None:
    body = ("  convolution_param {\n    kernel_size: %d\n    stride: %d\n    num_output: %d\n    group: %d\n    pad: %d\n"
            "    weight_filler { type: \"bilinear\" }\n    bias_term: false\n  }\n  param { lr_mult: 0 decay_mult: 0 }") % (k, s, ch, ch, p)
    w.layer(name, "Deconvolution", [bottom], [name], body)


def _fcn_bbox_heads(w: _Writer, num_classes: int) -> None:
    """bbox branch (stride 8 after a x4 bilinear deconvolution) and the FCN-8s style score branch of train/fcn_bbox."""
    c4 = 4 * num_classes
    w.layer("score_conv5_bbox", "Convolution", ["dropout5"], ["score_conv5_bbox"], _conv_body(c4, 1, explicit=True))
    _frozen_bilinear_deconv(w, "upscore_pool5_bbox", "score_conv5_bbox", c4, 8, 4, 2)


def _fcn_bbox_scores(w: _Writer, num_classes: int) -> None:
    w.layer("score_conv5", "Convolution", ["dropout5"], ["score_conv5"], _conv_body(num_classes, 1, explicit=True))
    _frozen_bilinear_deconv(w, "upscore_pool5", "score_conv5", num_classes, 4, 2, 1)
    w.layer("score_pool4", "Convolution", ["pool4"], ["score_pool4"], _conv_body(num_classes, 1, explicit=True))
    w.layer("fuse_pool4", "Eltwise", ["upscore_pool5", "score_pool4"], ["fuse_pool4"], "  eltwise_param { operation: SUM }")
    _frozen_bilinear_deconv(w, "upscore_pool4", "fuse_pool4", num_classes, 4, 2, 1)
    w.layer("score_pool3", "Convolution", ["pool3"], ["score_pool3"], _conv_body(num_classes, 1, explicit=True))
    w.layer("fuse_pool3", "Eltwise", ["upscore_pool4", "score_pool3"], ["fuse_pool3"], "  eltwise_param { operation: SUM }")
    _frozen_bilinear_deconv(w, "upscore_pool3", "fuse_pool3", num_classes, 16, 8, 4)


def vgg16_fcn_bbox_train(module: str, layer: str, param_str: str, num_classes: int = 11) -> str:
    """The reference's train/fcn_bbox/train_val.prototxt (the net HEAD's Python layer and the ROS node match): VGG16 ->
    masked / normalised L1 loss on the x4-upsampled bbox map (stride 8) + SoftmaxWithLoss on the FCN-8s score map against
    the full-resolution class mask the data layer emits as top[1]."""
    w = _Writer()
    tops = ["data", "label", "bbox-label", "size-block", "obj-block", "coverage-block"]
    body = "  python_param {\n    module: '%s'\n    layer: '%s'\n    param_str: '%s'\n  }" % (module, layer, param_str)
    w.layer("Argumentation", "Python", [], tops, body, quote="'")
    _vgg16_body(w, "data")
    _fcn_bbox_heads(w, num_classes)
    prod = "  eltwise_param { operation: PROD }"
    w.layer("bb-label-norm", "Eltwise", ["bbox-label", "size-block"], ["bbox-label-norm"], prod)
    w.layer("bb-obj-norm", "Eltwise", ["bbox-label-norm", "obj-block"], ["bbox-obj-label-norm"], prod)
    w.layer("bbox_mask", "Eltwise", ["upscore_pool5_bbox", "coverage-block"], ["bboxes-masked"], prod)
    w.layer("bbox-norm", "Eltwise", ["bboxes-masked", "size-block"], ["bboxes-masked-norm"], prod)
    w.layer("bbox-obj-norm", "Eltwise", ["bboxes-masked-norm", "obj-block"], ["bboxes-obj-masked-norm"], prod)
    w.layer("bbox_loss", "L1Loss", ["bboxes-obj-masked-norm", "bbox-obj-label-norm"], ["loss_bbox"], extra="  loss_weight: 2.0")
    _fcn_bbox_scores(w, num_classes)
    w.layer("loss", "SoftmaxWithLoss", ["upscore_pool3", "label"], ["loss"], "  loss_param { normalize: false }")
    return w.text()


def vgg16_fcn_bbox_deploy(batch: int = 1, height: int = 448, width: int = 448, num_classes: int = 11) -> str:
    """Inference form of train/fcn_bbox: the node (scripts/fcn_object_detector.py:89-90) reads ``pool_score`` (class
    probabilities at stride 8: Softmax of ``fuse_pool3``) and ``upscore_pool5_bbox``."""
    w = _Writer()
    w.raw('input: "data"\ninput_shape {\n  dim: %d\n  dim: 3\n  dim: %d\n  dim: %d\n}' % (batch, height, width))
    _vgg16_body(w, "data")
    _fcn_bbox_heads(w, num_classes)
    _fcn_bbox_scores(w, num_classes)
    w.layer("pool_score", "Softmax", ["fuse_pool3"], ["pool_score"])
    return w.text()


def vgg16_bounding_box_train(module: str, layer: str, param_str: str, num_classes: int = 11, test_param_str: Optional[str] = None) -> str:
    """The reference's train/bounding_box/train_val.prototxt (solver: ADAM, step policy): VGG16 with conv1_1..conv3_3
    frozen (lr_mult 0), no ReLU after conv5_3, a frozen x2 bilinear deconvolution back to stride 8, dropout, the
    DetectNet coverage / bbox heads and their L1 + Euclidean losses.  test_param_str adds the TEST-phase copy of the data
    layer (the reference's reads val.txt at 448 x 448, stride 16, batch 10)."""
    w = _Writer()
    tops = ["data", "coverage-label", "bbox-label", "size-block", "obj-block", "coverage-block"]
    _python_data_layers(w, "Argumentation", tops, module, layer, param_str, test_param_str)
    prod = "  eltwise_param { operation: PROD }"
    w.layer("bb-label-norm", "Eltwise", ["bbox-label", "size-block"], ["bbox-label-norm"], prod)
    w.layer("bb-obj-norm", "Eltwise", ["bbox-label-norm", "obj-block"], ["bbox-obj-label-norm"], prod)
    prev = "data"
    for blk, n, width_ in VGG16:
        frozen = blk <= 3
        for i in range(1, n + 1):
            nm = "conv%d_%d" % (blk, i)
            w.layer(nm, "Convolution", [prev], [nm], _conv_body(width_, 3, 1, bias_value=0.0, lr=(0.0, 0.0) if frozen else (1.0, 2.0),
                                                                decay=(0.0, 0.0) if frozen else (1.0, 0.0)))
            if (blk, i) != (5, 3):
                w.layer("relu%d_%d" % (blk, i), "ReLU", [nm], [nm])
            prev = nm
        if blk < 5:
            w.layer("pool%d" % blk, "Pooling", [prev], ["pool%d" % blk], "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }")
            prev = "pool%d" % blk
    _frozen_bilinear_deconv(w, "conv5_3/upsample", "conv5_3", 512, 4, 2, 1)
    w.layer("dropout5", "Dropout", ["conv5_3/upsample"], ["dropout5"], "  dropout_param { dropout_ratio: 0.5 }")
    w.layer("cvg/classifier", "Convolution", ["dropout5"], ["cvg/classifier"], _conv_body(num_classes, 1, bias_value=0.0))
    w.layer("coverage/sig", "Sigmoid", ["cvg/classifier"], ["coverage"])
    w.layer("bbox/regressor", "Convolution", ["dropout5"], ["bboxes"], _conv_body(4 * num_classes, 1, bias_value=0.0))
    w.layer("bbox_mask", "Eltwise", ["bboxes", "coverage-block"], ["bboxes-masked"], prod)
    w.layer("bbox-norm", "Eltwise", ["bboxes-masked", "size-block"], ["bboxes-masked-norm"], prod)
    w.layer("bbox-obj-norm", "Eltwise", ["bboxes-masked-norm", "obj-block"], ["bboxes-obj-masked-norm"], prod)
    w.layer("bbox_loss", "L1Loss", ["bboxes-obj-masked-norm", "bbox-obj-label-norm"], ["loss_bbox"], extra="  loss_weight: 2.0")
    w.layer("coverage_loss", "EuclideanLoss", ["coverage", "coverage-label"], ["loss_coverage"])
    return w.text()


def vgg16_bounding_box_deploy(batch: int = 10, height: int = 448, width: int = 448, num_classes: int = 20) -> str:
    """The reference's train/bounding_box/deploy.prototxt: VGG16 to conv5_3 (stride 16), a pyramid-pooling context branch on
    conv4_3 (AVE pools to 1x1 / 2x2 / 4x4 / 7x7, 1x1 convolutions to 128 channels, frozen bilinear deconvolutions back to
    28x28), concatenated with conv5_3 and pool4 (1536 channels), dropout, the DetectNet coverage / bbox heads."""
    w = _Writer()
    w.layer("data", "Input", [], ["data"], "  input_param { shape { dim: %d dim: 3 dim: %d dim: %d } }" % (batch, height, width))
    prev = "data"
    for blk, n, width_ in VGG16[:4]:
        for i in range(1, n + 1):
            nm = "conv%d_%d" % (blk, i)
            w.layer(nm, "Convolution", [prev], [nm], _conv_body(width_, 3, 1, bias_value=0.0))
            w.layer("relu%d_%d" % (blk, i), "ReLU", [nm], [nm])
            prev = nm
        w.layer("pool%d" % blk, "Pooling", [prev], ["pool%d" % blk], "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }")
        prev = "pool%d" % blk
    ups = []
    for tag, pk, dk, ds, dp in (("1x1", 56, 56, 28, 14), ("2x2", 28, 28, 14, 7), ("4x4", 14, 13, 7, 3), ("7x7", 8, 8, 4, 2)):
        w.layer("pool4/" + tag, "Pooling", ["conv4_3"], ["pool4/" + tag], "  pooling_param { pool: AVE kernel_size: %d stride: %d }" % (pk, pk))
        cn = "conv4_3/" + tag
        w.layer(cn, "Convolution", ["pool4/" + tag], [cn], _conv_body(128, 1, 0, bias_value=0.0, lr=(10.0, 2.0), explicit="pad"))
        w.layer("act_4_3/" + tag, "ReLU", [cn], [cn])
        _frozen_bilinear_deconv(w, cn + "/upsample", cn, 128, dk, ds, dp)
        ups.append(cn + "/upsample")
    prev = "pool4"
    for i in range(1, 4):
        nm = "conv5_%d" % i
        w.layer(nm, "Convolution", [prev], [nm], _conv_body(512, 3, 1, bias_value=0.0))
        if i < 3:
            w.layer("relu5_%d" % i, "ReLU", [nm], [nm])
        prev = nm
    w.layer("conv4_3/conv5_3/concat", "Concat", ["conv5_3", "pool4"] + ups, ["conv4_3/conv5_3/concat"])
    w.layer("dropout5", "Dropout", ["conv4_3/conv5_3/concat"], ["dropout5"], "  dropout_param { dropout_ratio: 0.5 }")
    w.layer("cvg/classifier", "Convolution", ["dropout5"], ["cvg/classifier"], _conv_body(num_classes, 1, bias_value=0.0))
    w.layer("coverage/sig", "Sigmoid", ["cvg/classifier"], ["coverage"])
    w.layer("bbox/regressor", "Convolution", ["dropout5"], ["bboxes"], _conv_body(4 * num_classes, 1, bias_value=0.0))
    return w.text()


# ----------------------------------------------------------------------
# the published FCN-32s / 16s / 8s nets (PASCAL VOC)
# ----------------------------------------------------------------------

def _voc_conv(w: _Writer, name: str, bottom: str, num_output: int, k: int, pad: int, fillers: bool, relu: Optional[str] = None) -> None:
    fill = '    weight_filler { type: "xavier" }\n    bias_filler { type: "constant" value: 0.1 }\n' if fillers else ""
    body = ("  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }\n"
            "  convolution_param {\n    num_output: %d\n    pad: %d\n    kernel_size: %d\n    stride: 1\n%s  }") % (num_output, pad, k, fill)
    w.layer(name, "Convolution", [bottom], [name], body)
    if relu:
        w.layer(relu, "ReLU", [name], [name])


def _voc_upscore(w: _Writer, name: str, bottom: str, num_output: int, k: int, s: int, fillers: bool) -> None:
    fill = '    weight_filler { type: "bilinear" }\n' if fillers else ""
    body = ("  param { lr_mult: 0 }\n  convolution_param {\n    num_output: %d\n    bias_term: false\n    kernel_size: %d\n"
            "    stride: %d\n%s  }") % (num_output, k, s, fill)
    w.layer(name, "Deconvolution", [bottom], [name], body)


def _voc_crop(w: _Writer, name: str, bottom: str, like: str, offset: int) -> None:
    w.layer(name, "Crop", [bottom, like], [name], "  crop_param {\n    axis: 2\n    offset: %d\n  }" % offset)


def _label_map(w: _Writer, score: str) -> None:
    """The label map behind a deploy net's scores or probabilities, as SegNet's web-demo prototxt ends: ArgMax over the channel axis."""
    w.layer("argmax", "ArgMax", [score], ["argmax"], "  argmax_param {\n    axis: 1\n  }")


def _voc_fcn(variant: int, phase: str, num_classes: int, shape: Sequence[int], width_div: int, fc_div: Optional[int], fillers: bool,
             argmax: bool = False) -> str:
    if phase not in ("TRAIN", "TEST"):
        raise ValueError("phase must be 'TRAIN' or 'TEST'")
    n, c, h, wd = (int(v) for v in shape)
    w = _Writer()
    w.raw('name: "voc-fcn%ds"' % variant)
    w.layer("data", "Input", [], ["data"], "  input_param { shape { dim: %d dim: %d dim: %d dim: %d } }" % (n, c, h, wd))
    if phase == "TRAIN":
        w.layer("label", "Input", [], ["label"], "  input_param { shape { dim: %d dim: 1 dim: %d dim: %d } }" % (n, h, wd))
    prev = "data"
    for blk, convs, width_ in VGG16:
        for i in range(1, convs + 1):
            nm = "conv%d_%d" % (blk, i)
            _voc_conv(w, nm, prev, max(width_ // width_div, 1), 3, 100 if (blk, i) == (1, 1) else 1, fillers, "relu%d_%d" % (blk, i))
            prev = nm
        w.layer("pool%d" % blk, "Pooling", [prev], ["pool%d" % blk], "  pooling_param {\n    pool: MAX\n    kernel_size: 2\n    stride: 2\n  }")
        prev = "pool%d" % blk
    fc = max(4096 // (fc_div or width_div), 1)
    for nm, k, tag in (("fc6", 7, "6"), ("fc7", 1, "7")):
        _voc_conv(w, nm, prev, fc, k, 0, fillers, "relu" + tag)
        w.layer("drop" + tag, "Dropout", [nm], [nm], "  dropout_param {\n    dropout_ratio: 0.5\n  }")
        prev = nm
    nc = num_classes
    _voc_conv(w, "score_fr", "fc7", nc, 1, 0, fillers)
    if variant == 32:
        _voc_upscore(w, "upscore", "score_fr", nc, 64, 32, fillers)
        _voc_crop(w, "score", "upscore", "data", 19)
    else:
        _voc_upscore(w, "upscore2", "score_fr", nc, 4, 2, fillers)
        _voc_conv(w, "score_pool4", "pool4", nc, 1, 0, fillers)
        _voc_crop(w, "score_pool4c", "score_pool4", "upscore2", 5)
        w.layer("fuse_pool4", "Eltwise", ["upscore2", "score_pool4c"], ["fuse_pool4"], "  eltwise_param {\n    operation: SUM\n  }")
        if variant == 16:
            _voc_upscore(w, "upscore16", "fuse_pool4", nc, 32, 16, fillers)
            _voc_crop(w, "score", "upscore16", "data", 27)
        else:
            _voc_upscore(w, "upscore_pool4", "fuse_pool4", nc, 4, 2, fillers)
            _voc_conv(w, "score_pool3", "pool3", nc, 1, 0, fillers)
            _voc_crop(w, "score_pool3c", "score_pool3", "upscore_pool4", 9)
            w.layer("fuse_pool3", "Eltwise", ["upscore_pool4", "score_pool3c"], ["fuse_pool3"], "  eltwise_param {\n    operation: SUM\n  }")
            _voc_upscore(w, "upscore8", "fuse_pool3", nc, 16, 8, fillers)
            _voc_crop(w, "score", "upscore8", "data", 31)
    if phase == "TRAIN":
        w.layer("loss", "SoftmaxWithLoss", ["score", "label"], ["loss"], "  loss_param {\n    ignore_label: 255\n    normalize: false\n  }")
    elif argmax:
        _label_map(w, "score")
    return w.text()


def voc_fcn32s(phase: str = "TEST", num_classes: int = 21, shape: Sequence[int] = (1, 3, 500, 500), width_div: int = 1,
               fc_div: Optional[int] = None, fillers: bool = False, argmax: bool = False) -> str:
    """The published FCN-32s: VGG16 (conv1_1 with pad 100) to pool5, fc6 (k7) / fc7 (k1) as convolutions with ReLU and Dropout,
    score_fr, a x32 Deconvolution (k64 s32, no bias, lr_mult 0) and score = Crop(upscore, data) at offset 19.  TRAIN adds the label
    input and SoftmaxWithLoss (normalize: false, ignore_label: 255); TEST ends at `score`.  width_div / fc_div divide the VGG widths
    and the 4096 of fc6 / fc7 (tests).  argmax=True ends the TEST net in the label map `argmax` (ArgMax, axis 1) behind `score`; the
    other two variants take it alike.  The published files carry no fillers (the nets are initialised by net surgery);
    fillers=True writes xavier / constant 0.1 into the convolutions and the bilinear filler into the upsampling layers."""
    return _voc_fcn(32, phase, num_classes, shape, width_div, fc_div, fillers, argmax)


def voc_fcn16s(phase: str = "TEST", num_classes: int = 21, shape: Sequence[int] = (1, 3, 500, 500), width_div: int = 1,
               fc_div: Optional[int] = None, fillers: bool = False, argmax: bool = False) -> str:
    """The published FCN-16s: as voc_fcn32s to score_fr, then upscore2 (k4 s2), score_pool4 on pool4 cropped to it at offset 5, their
    sum, upscore16 (k32 s16) and score = Crop(upscore16, data) at offset 27."""
    return _voc_fcn(16, phase, num_classes, shape, width_div, fc_div, fillers, argmax)


def voc_fcn8s(phase: str = "TEST", num_classes: int = 21, shape: Sequence[int] = (1, 3, 500, 500), width_div: int = 1,
              fc_div: Optional[int] = None, fillers: bool = False, argmax: bool = False) -> str:
    """The published FCN-8s: as voc_fcn16s to fuse_pool4, then upscore_pool4 (k4 s2), score_pool3 on pool3 cropped to it at offset 9,
    their sum, upscore8 (k16 s8) and score = Crop(upscore8, data) at offset 31."""
    return _voc_fcn(8, phase, num_classes, shape, width_div, fc_div, fillers, argmax)


# ----------------------------------------------------------------------
# BVLC reference CaffeNet, the GOTURN tracker, BVLC GoogLeNet
# ----------------------------------------------------------------------

def _strip_fillers(text: str) -> str:
    return "\n".join(ln for ln in text.split("\n") if "_filler" not in ln) + ("\n" if text.endswith("\n") else "")


def _inputs(w: _Writer, phase: str, batch: int, images: Sequence[str], size: int, label: Optional[Tuple[str, Sequence[int]]]) -> None:
    for nm in images:
        w.layer(nm, "Input", [], [nm], "  input_param { shape { dim: %d dim: 3 dim: %d dim: %d } }" % (batch, size, size))
    if label is not None and phase != "DEPLOY":
        w.layer(label[0], "Input", [], [label[0]], "  input_param { shape { %s } }" % " ".join("dim: %d" % d for d in label[1]))


def _cn_conv(w: _Writer, name: str, relu: str, bottom: str, num_output: int, k: int, pad: int, stride: int, group: int, bias: float,
             frozen: bool) -> None:
    mult = ("  param { lr_mult: 0 decay_mult: 0 }\n  param { lr_mult: 0 decay_mult: 0 }" if frozen
            else "  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }")
    geo = ["    num_output: %d" % num_output] + (["    pad: %d" % pad] if pad else []) + ["    kernel_size: %d" % k] + \
          (["    group: %d" % group] if group != 1 else []) + (["    stride: %d" % stride] if stride != 1 else [])
    body = "%s\n  convolution_param {\n%s\n    weight_filler { type: \"gaussian\" std: 0.01 }\n    bias_filler { type: \"constant\" value: %g }\n  }" % (
        mult, "\n".join(geo), bias)
    w.layer(name, "Convolution", [bottom], [name], body)
    w.layer(relu, "ReLU", [name], [name])


def _cn_fc(w: _Writer, name: str, bottom: str, num_output: int, std: float, bias: float, relu: Optional[str] = None, drop: Optional[str] = None,
           ratio: float = 0.5, filler: str = "gaussian") -> None:
    fill = '    weight_filler { type: "xavier" }' if filler == "xavier" else '    weight_filler { type: "gaussian" std: %g }' % std
    w.layer(name, "InnerProduct", [bottom], [name], "  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }\n"
            "  inner_product_param {\n    num_output: %d\n%s\n    bias_filler { type: \"constant\" value: %g }\n  }" % (num_output, fill, bias))
    if relu:
        w.layer(relu, "ReLU", [name], [name])
    if drop:
        w.layer(drop, "Dropout", [name], [name], "  dropout_param { dropout_ratio: %g }" % ratio)


def _caffenet_tower(w: _Writer, data_blob: str, suffix: str, width_div: int, frozen: bool) -> str:
    """conv1 .. pool5 of CaffeNet (pooling before normalisation, conv2 / conv4 / conv5 in two groups); layer and blob names + suffix."""
    wd = lambda c: max(c // width_div, 1)
    n = lambda nm: nm + suffix
    lrn = "  lrn_param { local_size: 5 alpha: 0.0001 beta: 0.75 }"
    pool = "  pooling_param { pool: MAX kernel_size: 3 stride: 2 }"
    _cn_conv(w, n("conv1"), n("relu1"), data_blob, wd(96), 11, 0, 4, 1, 0.0, frozen)
    w.layer(n("pool1"), "Pooling", [n("conv1")], [n("pool1")], pool)
    w.layer(n("norm1"), "LRN", [n("pool1")], [n("norm1")], lrn)
    _cn_conv(w, n("conv2"), n("relu2"), n("norm1"), wd(256), 5, 2, 1, 2, 1.0, frozen)
    w.layer(n("pool2"), "Pooling", [n("conv2")], [n("pool2")], pool)
    w.layer(n("norm2"), "LRN", [n("pool2")], [n("norm2")], lrn)
    _cn_conv(w, n("conv3"), n("relu3"), n("norm2"), wd(384), 3, 1, 1, 1, 0.0, frozen)
    _cn_conv(w, n("conv4"), n("relu4"), n("conv3"), wd(384), 3, 1, 1, 2, 1.0, frozen)
    _cn_conv(w, n("conv5"), n("relu5"), n("conv4"), wd(256), 3, 1, 1, 2, 1.0, frozen)
    w.layer(n("pool5"), "Pooling", [n("conv5")], [n("pool5")], pool)
    return n("pool5")


def _check_phase(phase: str) -> None:
    if phase not in ("TRAIN", "TEST", "DEPLOY"):
        raise ValueError("phase must be 'TRAIN', 'TEST' or 'DEPLOY'")


def caffenet(phase: str = "DEPLOY", batch: int = 10, num_classes: int = 1000, width_div: int = 1, fc_div: Optional[int] = None,
             size: int = 227, fillers: bool = True) -> str:
    """BVLC reference CaffeNet: conv1 11x11 / s4, pool1, norm1, conv2 (group 2), pool2, norm2, conv3, conv4 (group 2), conv5 (group 2), pool5,
    fc6, fc7 (ReLU, Dropout 0.5), fc8.  TRAIN ends in SoftmaxWithLoss over an (N,) `label`, TEST adds Accuracy, DEPLOY takes `data`
    alone and ends in Softmax `prob`.  width_div / fc_div divide the convolution widths and the 4096 of fc6 / fc7, size is the image
    edge (tests); fillers=False leaves the fillers out."""
    _check_phase(phase)
    w = _Writer()
    w.raw('name: "CaffeNet"')
    _inputs(w, phase, batch, ["data"], size, ("label", (batch,)))
    feat = _caffenet_tower(w, "data", "", width_div, False)
    fc = max(4096 // (fc_div or width_div), 1)
    _cn_fc(w, "fc6", feat, fc, 0.005, 1.0, "relu6", "drop6")
    _cn_fc(w, "fc7", "fc6", fc, 0.005, 1.0, "relu7", "drop7")
    _cn_fc(w, "fc8", "fc7", num_classes, 0.01, 0.0)
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", ["fc8"], ["prob"])
    else:
        if phase == "TEST":
            w.layer("accuracy", "Accuracy", ["fc8", "label"], ["accuracy"])
        w.layer("loss", "SoftmaxWithLoss", ["fc8", "label"], ["loss"])
    return w.text() if fillers else _strip_fillers(w.text())


def goturn_tracker(phase: str = "DEPLOY", batch: int = 1, width_div: int = 1, fc_div: Optional[int] = None, size: int = 227,
                   fillers: bool = True) -> str:
    """The GOTURN tracker: two frozen CaffeNet towers, conv1 .. pool5 on `image` (the search region) and conv1_p .. pool5_p on `target`,
    their Concat, fc6-new, fc7-new, fc7-newb (ReLU, Dropout 0.5) and fc8-shapes: the 4 corner coordinates.  TRAIN and TEST add the
    (N, 4) `bbox` input and L1Loss against it."""
    _check_phase(phase)
    w = _Writer()
    w.raw('name: "GOTURN"')
    _inputs(w, phase, batch, ["image", "target"], size, ("bbox", (batch, 4)))
    a = _caffenet_tower(w, "image", "", width_div, True)
    b = _caffenet_tower(w, "target", "_p", width_div, True)
    w.layer("concat", "Concat", [a, b], ["pool5_concat"], "  concat_param { axis: 1 }")
    fc = max(4096 // (fc_div or width_div), 1)
    _cn_fc(w, "fc6-new", "pool5_concat", fc, 0.005, 1.0, "relu6", "drop6")
    _cn_fc(w, "fc7-new", "fc6-new", fc, 0.005, 1.0, "relu7", "drop7")
    _cn_fc(w, "fc7-newb", "fc7-new", fc, 0.005, 1.0, "relu7b", "drop7b")
    _cn_fc(w, "fc8-shapes", "fc7-newb", 4, 0.01, 0.0)
    if phase != "DEPLOY":
        w.layer("loss", "L1Loss", ["fc8-shapes", "bbox"], ["loss"])
    return w.text() if fillers else _strip_fillers(w.text())


def _googlenet_aux_head(w: _Writer, tag: str, tap: str, num_classes: int, div: int, fc_div: int) -> None:
    """loss1/* / loss2/*: AVE 5x5 / s3, 1x1 convolution to 128, fc 1024 (ReLU, Dropout 0.7), classifier, SoftmaxWithLoss at weight 0.3."""
    n = lambda nm: "%s/%s" % (tag, nm)
    w.layer(n("ave_pool"), "Pooling", [tap], [n("ave_pool")], "  pooling_param { pool: AVE kernel_size: 5 stride: 3 }")
    _conv_relu(w, n("conv"), n("relu_conv"), n("ave_pool"), max(128 // div, 1), 1)
    _cn_fc(w, n("fc"), n("conv"), max(1024 // fc_div, 1), 0.0, 0.2, n("relu_fc"), n("drop_fc"), 0.7, filler="xavier")
    _cn_fc(w, n("classifier"), n("fc"), num_classes, 0.0, 0.0, filler="xavier")
    w.layer(n("loss"), "SoftmaxWithLoss", [n("classifier"), "label"], [n(tag)], extra="  loss_weight: 0.3")


def bvlc_googlenet(phase: str = "DEPLOY", batch: int = 10, num_classes: int = 1000, aux: bool = True, width_div: int = 1,
                   fc_div: Optional[int] = None, size: int = 224, fillers: bool = True) -> str:
    """BVLC GoogLeNet, the net the detector body (googlenet_detectnet_*) is fine-tuned from: the same inception stack with pool4/3x3_s2
    behind inception_4e, then pool5/7x7_s1 (AVE), Dropout 0.4 and loss3/classifier.  TRAIN adds (aux=True) the auxiliary heads
    loss1/* behind inception_4a and loss2/* behind inception_4d, each a SoftmaxWithLoss at loss_weight 0.3, and loss3/loss3; TEST adds
    loss3/top-1 and loss3/top-5 Accuracy; DEPLOY takes `data` alone and ends in Softmax `prob`.  width_div divides every convolution
    width, fc_div (default: width_div) the 1024 of the auxiliary fc layers."""
    _check_phase(phase)
    w = _Writer()
    w.raw('name: "GoogleNet"')
    _inputs(w, phase, batch, ["data"], size, ("label", (batch,)))
    feat, taps = _googlenet_body(w, "data", bvlc_div=width_div)
    if phase == "TRAIN" and aux:
        _googlenet_aux_head(w, "loss1", taps[0], num_classes, width_div, fc_div or width_div)
        _googlenet_aux_head(w, "loss2", taps[1], num_classes, width_div, fc_div or width_div)
    w.layer("pool5/7x7_s1", "Pooling", [feat], ["pool5/7x7_s1"], "  pooling_param { pool: AVE kernel_size: 7 stride: 1 }")
    w.layer("pool5/drop_7x7_s1", "Dropout", ["pool5/7x7_s1"], ["pool5/7x7_s1"], "  dropout_param { dropout_ratio: 0.4 }")
    _cn_fc(w, "loss3/classifier", "pool5/7x7_s1", num_classes, 0.0, 0.0, filler="xavier")
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", ["loss3/classifier"], ["prob"])
    else:
        w.layer("loss3/loss3", "SoftmaxWithLoss", ["loss3/classifier", "label"], ["loss3/loss3"], extra="  loss_weight: 1")
        if phase == "TEST":
            w.layer("loss3/top-1", "Accuracy", ["loss3/classifier", "label"], ["loss3/top-1"])
            w.layer("loss3/top-5", "Accuracy", ["loss3/classifier", "label"], ["loss3/top-5"], "  accuracy_param { top_k: 5 }")
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# ResNet-50 / 101 / 152 (He et al., "Deep Residual Learning for Image Recognition"; the published Caffe prototxts' names)
# ----------------------------------------------------------------------

RESNET_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}


def _resnet_block_names(count: int, numbered: bool) -> List[str]:
    """Block letters of one stage as published: a, b, c ..., or a, b1, b2 ... in stages 3 and 4 of ResNet-101 / 152."""
    if not numbered:
        return [chr(ord("a") + i) for i in range(count)]
    return ["a"] + ["b%d" % i for i in range(1, count)]


def _rn_conv_bn(w: _Writer, tag: str, bottom: str, num_output: int, k: int, pad: int, stride: int, phase: str, relu: bool,
                conv_name: Optional[str] = None, bias: bool = False, dilation: int = 1) -> str:
    """Convolution `res<tag>` (bias_term: false but for conv1) with BatchNorm `bn<tag>`, Scale `scale<tag>` (bias_term: true) and ReLU
    `res<tag>_relu` in place on its top; returns the top."""
    name = conv_name or "res" + tag
    sfx = tag if conv_name is None else "_" + conv_name
    geo = "    num_output: %d\n    kernel_size: %d\n    pad: %d\n    stride: %d\n" % (num_output, k, pad, stride)
    if dilation != 1:
        geo += "    dilation: %d\n" % dilation
    fill = "    weight_filler { type: \"gaussian\" std: %g }\n" % (2.0 / (k * k * num_output)) ** 0.5
    if bias:
        fill += "    bias_filler { type: \"constant\" value: 0 }\n"
    else:
        geo += "    bias_term: false\n"
    w.layer(name, "Convolution", [bottom], [name], "  convolution_param {\n%s%s  }" % (geo, fill))
    stats = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3) if phase != "DEPLOY" else "  batch_norm_param { use_global_stats: true }"
    w.layer("bn" + sfx, "BatchNorm", [name], [name], stats)
    w.layer("scale" + sfx, "Scale", [name], [name], "  scale_param { bias_term: true }")
    if relu:
        w.layer(name + "_relu" if conv_name is None else conv_name + "_relu", "ReLU", [name], [name])
    return name


def resnet(phase: str = "DEPLOY", depth: int = 50, batch: int = 1, num_classes: int = 1000, width_div: int = 1, size: int = 224,
           fillers: bool = True) -> str:
    """ResNet-50 / 101 / 152 with the published layer and blob names (a downloaded ResNet-50-model.caffemodel maps by name): conv1 7x7 / 2
    with bias, bn_conv1, scale_conv1, conv1_relu, pool1 MAX 3x3 / 2, the bottleneck stages res2a .. res5c (branch1 on the first block of
    a stage, branch2a / b / c, bias_term: false, BatchNorm and Scale in place, stride 2 on the first 1x1 convolutions of stages 3 - 5),
    pool5 AVE 7 (global pooling at other sizes), fc1000 and prob.  use_global_stats: true only in DEPLOY, as published; TRAIN ends in
    SoftmaxWithLoss over an (N,) `label`, TEST adds Accuracy.  width_div divides every convolution width, size is the image edge (tests)."""
    _check_phase(phase)
    if depth not in RESNET_BLOCKS:
        raise ValueError("depth must be one of %s" % sorted(RESNET_BLOCKS))
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "ResNet-%d"' % depth)
    _inputs(w, phase, batch, ["data"], size, ("label", (batch,)))
    _rn_conv_bn(w, "", "data", wd(64), 7, 3, 2, phase, True, conv_name="conv1", bias=True)
    w.layer("pool1", "Pooling", ["conv1"], ["pool1"], "  pooling_param { pool: MAX kernel_size: 3 stride: 2 }")
    feat = "pool1"
    for stage, count in zip((2, 3, 4, 5), RESNET_BLOCKS[depth]):
        mid, out = wd(64 << (stage - 2)), wd(256 << (stage - 2))
        for bi, letter in enumerate(_resnet_block_names(count, depth > 50 and stage in (3, 4))):
            tag = "%d%s" % (stage, letter)
            stride = 2 if bi == 0 and stage > 2 else 1
            short = feat if bi else _rn_conv_bn(w, tag + "_branch1", feat, out, 1, 0, stride, phase, False)
            x = _rn_conv_bn(w, tag + "_branch2a", feat, mid, 1, 0, stride, phase, True)
            x = _rn_conv_bn(w, tag + "_branch2b", x, mid, 3, 1, 1, phase, True)
            x = _rn_conv_bn(w, tag + "_branch2c", x, out, 1, 0, 1, phase, False)
            feat = "res" + tag
            w.layer(feat, "Eltwise", [short, x], [feat])
            w.layer(feat + "_relu", "ReLU", [feat], [feat])
    pool = "kernel_size: 7 stride: 1" if size == 224 else "global_pooling: true"
    w.layer("pool5", "Pooling", [feat], ["pool5"], "  pooling_param { pool: AVE %s }" % pool)
    _cn_fc(w, "fc1000", "pool5", num_classes, 0.01, 0.0)
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", ["fc1000"], ["prob"])
    else:
        if phase == "TEST":
            w.layer("accuracy", "Accuracy", ["fc1000", "label"], ["accuracy"])
        w.layer("loss", "SoftmaxWithLoss", ["fc1000", "label"], ["loss"])
    return w.text() if fillers else _strip_fillers(w.text())


def resnet50(phase: str = "DEPLOY", **kw) -> str:
    return resnet(phase, depth=50, **kw)


def resnet101(phase: str = "DEPLOY", **kw) -> str:
    return resnet(phase, depth=101, **kw)


def resnet152(phase: str = "DEPLOY", **kw) -> str:
    return resnet(phase, depth=152, **kw)


# ----------------------------------------------------------------------
# SE-ResNet-50 / 101 / 152 (Hu, Shen, Sun: "Squeeze-and-Excitation Networks"; the SENet release's Caffe names where remembered)
# ----------------------------------------------------------------------

def _se_fc(w: _Writer, name: str, bottom: str, num_output: int, form: str) -> str:
    """A squeeze or excite layer over the pooled (N, C, 1, 1) blob, with a bias: an InnerProduct (form "scale") or the release's 1x1
    Convolution (form "axpy").  Their blobs agree up to the trailing 1, 1."""
    fill = "    weight_filler { type: \"gaussian\" std: %g }\n    bias_filler { type: \"constant\" value: 0 }\n" % (2.0 / num_output) ** 0.5
    if form == "scale":
        w.layer(name, "InnerProduct", [bottom], [name], "  inner_product_param {\n    num_output: %d\n%s  }" % (num_output, fill))
    else:
        w.layer(name, "Convolution", [bottom], [name], "  convolution_param {\n    num_output: %d\n    kernel_size: 1\n    stride: 1\n%s  }" % (num_output, fill))
    return name


def se_resnet(phase: str = "DEPLOY", depth: int = 50, batch: int = 1, num_classes: int = 1000, width_div: int = 1, size: int = 224,
              reduction: int = 16, form: str = "scale", fillers: bool = True) -> str:
    """SE-ResNet-50 / 101 / 152: models.resnet's bottleneck stages with a Squeeze-and-Excitation block behind the last BatchNorm / Scale of
    every residual branch - global AVE pooling, a squeeze to out // reduction channels with an in-place ReLU, an excite back to out, a
    Sigmoid, the gate applied to the branch, the Eltwise with the shortcut and the ReLU.
    form "scale": squeeze and excite are InnerProduct layers, the (N, C) gate is applied by `Scale { axis: 0 }` with two bottoms and an
    Eltwise SUM follows.  form "axpy": they are 1x1 Convolutions and the release's `Axpy` layer (gate, branch, shortcut) applies the gate
    and adds the shortcut - the shape of the published files.  Both need a NetSpec built with scale_gate=True (caffe.Net and the caffe
    tool pass it), and after it has read the Axpy layers both forms have the same layers and blobs by name.
    Names.  The SENet release's, as remembered: conv1/7x7_s2, pool1/3x3_s2, the convolutions conv<stage>_<block>_1x1_reduce / _3x3 /
    _1x1_increase / _1x1_proj, the SE layers conv<stage>_<block>_global_pool / _1x1_down / _1x1_down/relu / _1x1_up / _prob, the block
    output conv<stage>_<block> with conv<stage>_<block>/relu, pool5/7x7_s1, classifier and prob.  The project's own: the BatchNorm, Scale
    and ReLU layers on the convolutions (models.resnet's bn_<conv> / scale_<conv> / <conv>_relu, not the release's <conv>/bn ...), the
    gated Scale conv<stage>_<block>/scale of form "scale" (what an Axpy is read as), and a bias on conv1 as in models.resnet.  Phases,
    width_div and size as in models.resnet; the squeeze width is at least 1."""
    _check_phase(phase)
    if depth not in RESNET_BLOCKS:
        raise ValueError("depth must be one of %s" % sorted(RESNET_BLOCKS))
    if form not in ("scale", "axpy"):
        raise ValueError("form must be 'scale' or 'axpy'")
    if reduction < 1:
        raise ValueError("reduction must be at least 1")
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "SE-ResNet-%d"' % depth)
    _inputs(w, phase, batch, ["data"], size, ("label", (batch,)))
    _rn_conv_bn(w, "", "data", wd(64), 7, 3, 2, phase, True, conv_name="conv1/7x7_s2", bias=True)
    w.layer("pool1/3x3_s2", "Pooling", ["conv1/7x7_s2"], ["pool1/3x3_s2"], "  pooling_param { pool: MAX kernel_size: 3 stride: 2 }")
    feat = "pool1/3x3_s2"
    for stage, count in zip((2, 3, 4, 5), RESNET_BLOCKS[depth]):
        mid, out = wd(64 << (stage - 2)), wd(256 << (stage - 2))
        for bi in range(count):
            tag = "conv%d_%d" % (stage, bi + 1)
            stride = 2 if bi == 0 and stage > 2 else 1
            short = feat if bi else _rn_conv_bn(w, "", feat, out, 1, 0, stride, phase, False, conv_name=tag + "_1x1_proj")
            x = _rn_conv_bn(w, "", feat, mid, 1, 0, stride, phase, True, conv_name=tag + "_1x1_reduce")
            x = _rn_conv_bn(w, "", x, mid, 3, 1, 1, phase, True, conv_name=tag + "_3x3")
            x = _rn_conv_bn(w, "", x, out, 1, 0, 1, phase, False, conv_name=tag + "_1x1_increase")
            w.layer(tag + "_global_pool", "Pooling", [x], [tag + "_global_pool"], "  pooling_param { pool: AVE global_pooling: true }")
            g = _se_fc(w, tag + "_1x1_down", tag + "_global_pool", max(out // reduction, 1), form)
            w.layer(g + "/relu", "ReLU", [g], [g])
            g = _se_fc(w, tag + "_1x1_up", g, out, form)
            w.layer(tag + "_prob", "Sigmoid", [g], [tag + "_prob"])
            if form == "scale":
                w.layer(tag + "/scale", "Scale", [x, tag + "_prob"], [tag + "/scale"], "  scale_param { axis: 0 }")
                w.layer(tag, "Eltwise", [tag + "/scale", short], [tag])
            else:
                w.layer(tag, "Axpy", [tag + "_prob", x, short], [tag])
            w.layer(tag + "/relu", "ReLU", [tag], [tag])
            feat = tag
    w.layer("pool5/7x7_s1", "Pooling", [feat], ["pool5/7x7_s1"], "  pooling_param { pool: AVE global_pooling: true }")
    _cn_fc(w, "classifier", "pool5/7x7_s1", num_classes, 0.01, 0.0)
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", ["classifier"], ["prob"])
    else:
        if phase == "TEST":
            w.layer("accuracy", "Accuracy", ["classifier", "label"], ["accuracy"])
        w.layer("loss", "SoftmaxWithLoss", ["classifier", "label"], ["loss"])
    return w.text() if fillers else _strip_fillers(w.text())


def se_resnet50(phase: str = "DEPLOY", **kw) -> str:
    return se_resnet(phase, depth=50, **kw)


def se_resnet101(phase: str = "DEPLOY", **kw) -> str:
    return se_resnet(phase, depth=101, **kw)


def se_resnet152(phase: str = "DEPLOY", **kw) -> str:
    return se_resnet(phase, depth=152, **kw)


# ----------------------------------------------------------------------
# DeepLab-LargeFOV and the DeepLab-v2 ASPP head on VGG16 (Chen, Papandreou, Kokkinos, Murphy, Yuille: "Semantic Image Segmentation with
# Deep Convolutional Nets and Fully Connected CRFs" / "DeepLab: ... Atrous Convolution, and Fully Connected CRFs"; the published names)
# ----------------------------------------------------------------------

def _dl_conv(w: _Writer, name: str, bottom: str, num_output: int, k: int, pad: int = 0, dilation: int = 1, relu: Optional[str] = None,
             drop: Optional[str] = None, lr: Tuple[float, float] = (1.0, 2.0), std: Optional[float] = None) -> str:
    geo = ["    num_output: %d" % num_output] + (["    pad: %d" % pad] if pad else []) + ["    kernel_size: %d" % k] + \
          (["    dilation: %d" % dilation] if dilation != 1 else [])
    fill = '    weight_filler { type: "xavier" }' if std is None else '    weight_filler { type: "gaussian" std: %g }' % std
    w.layer(name, "Convolution", [bottom], [name], "  param { lr_mult: %g decay_mult: 1 }\n  param { lr_mult: %g decay_mult: 0 }\n"
            "  convolution_param {\n%s\n%s\n    bias_filler { type: \"constant\" value: 0 }\n  }" % (lr[0], lr[1], "\n".join(geo), fill))
    if relu:
        w.layer(relu, "ReLU", [name], [name])
    if drop:
        w.layer(drop, "Dropout", [name], [name], "  dropout_param { dropout_ratio: 0.5 }")
    return name


def _dl_pool(w: _Writer, name: str, bottom: str, stride: int, pool: str = "MAX") -> str:
    w.layer(name, "Pooling", [bottom], [name], "  pooling_param { pool: %s kernel_size: 3 stride: %d pad: 1 }" % (pool, stride))
    return name


def deeplab_score_size(size: int) -> int:
    """Edge of the score map of the DeepLab nets below for an input edge `size`: three 3x3 / s2 / pad 1 poolings in Caffe's ceil mode
    (321 -> 41); every other layer keeps the extent."""
    for _ in range(3):
        size = -(-(size + 2 - 3) // 2) + 1
    return size


def _deeplab_vgg(w: _Writer, phase: str, batch: int, size: int, width_div: int, interp: bool = False) -> str:
    """conv1_1 .. pool5 of the DeepLab VGG16: pool1 - pool3 3x3 / s2 / pad 1, pool4 and pool5 3x3 / s1 / pad 1, conv5_* with dilation 2
    (pad 2): the stride-8 body.  The label input has the score map's size (the published nets shrink the label in their data layer) -
    or, with `interp`, the image's: the published label_shrink layer (_deeplab_tail) shrinks it, which needs size = 1 modulo 8."""
    if interp and size % 8 != 1:
        raise ValueError("DeepLab with interp=True: size %d is not 1 modulo 8 (zoom_factor 8 of the %d x %d score map gives %d, and "
                         "shrink_factor 8 of the label must give the score map)" % (size, deeplab_score_size(size), deeplab_score_size(size),
                                                                                    8 * (deeplab_score_size(size) - 1) + 1))
    sm = size if interp else deeplab_score_size(size)
    _inputs(w, phase, batch, ["data"], size, ("label", (batch, 1, sm, sm)))
    prev = "data"
    for blk, convs, width_ in VGG16:
        for i in range(1, convs + 1):
            d = 2 if blk == 5 else 1
            prev = _dl_conv(w, "conv%d_%d" % (blk, i), prev, max(width_ // width_div, 1), 3, d, d, relu="relu%d_%d" % (blk, i))
        prev = _dl_pool(w, "pool%d" % blk, prev, 2 if blk <= 3 else 1)
    return prev


def _deeplab_tail(w: _Writer, phase: str, score: str, interp: bool = False, argmax: bool = False) -> None:
    """Loss (and, in TEST, Accuracy) on the score map.  interp, under the published names: DEPLOY ends in fc8_interp, the score map at
    the image's size (Interp, zoom_factor 8); TRAIN / TEST read label_shrink, every 8th pixel of the image-sized label (Interp,
    shrink_factor 8: positions that fall on label pixels, so the class ids and the 255s arrive as they are)."""
    if phase == "DEPLOY":
        if interp:
            w.layer("fc8_interp", "Interp", [score], ["fc8_interp"], "  interp_param {\n    zoom_factor: 8\n  }")
        if argmax:      # the label map behind the DEPLOY tail
            _label_map(w, "fc8_interp" if interp else score)
        return
    label = "label"
    if interp:
        label = "label_shrink"
        w.layer(label, "Interp", ["label"], [label], "  interp_param {\n    shrink_factor: 8\n    pad_beg: 0\n    pad_end: 0\n  }")
    if phase == "TEST":
        w.layer("accuracy", "Accuracy", [score, label], ["accuracy"], "  accuracy_param { ignore_label: 255 }")
    w.layer("loss", "SoftmaxWithLoss", [score, label], ["loss"], "  loss_param { ignore_label: 255 }")


def deeplab_largefov(phase: str = "DEPLOY", batch: int = 1, num_classes: int = 21, width_div: int = 1, fc_div: int = 1, size: int = 321,
                     fc6_dilation: int = 12, interp: bool = False, argmax: bool = False) -> str:
    """DeepLab-LargeFOV on VGG16 with the published names: the stride-8 body (_deeplab_vgg), pool5a (AVE 3x3 / s1 / pad 1), fc6 3x3 with
    1024 outputs at dilation 12 (pad 12), fc7 1x1 (ReLU, Dropout 0.5 behind both) and fc8_voc12 (lr_mult 10 / 20).  TRAIN and TEST end
    in SoftmaxWithLoss with ignore_label 255 (TEST adds Accuracy) on a `label` input of the score map's size; DEPLOY ends at
    fc8_voc12.  interp=True adds the published Interp layers (_deeplab_tail): DEPLOY ends in fc8_interp at the image's size, and the
    `label` input of TRAIN / TEST has the image's size and is shrunk by label_shrink; size must then be 1 modulo 8.  The published
    ImageSegData layer is not emitted.  argmax=True ends the DEPLOY net in the label map `argmax` (ArgMax, axis 1) behind its last
    blob.  width_div / fc_div divide the VGG widths and the 1024."""
    _check_phase(phase)
    w = _Writer()
    w.raw('name: "DeepLab-LargeFOV"')
    feat = _deeplab_vgg(w, phase, batch, size, width_div, interp)
    feat = _dl_pool(w, "pool5a", feat, 1, "AVE")
    fc = max(1024 // fc_div, 1)
    _dl_conv(w, "fc6", feat, fc, 3, fc6_dilation, fc6_dilation, relu="relu6", drop="drop6")
    _dl_conv(w, "fc7", "fc6", fc, 1, relu="relu7", drop="drop7")
    _dl_conv(w, "fc8_voc12", "fc7", num_classes, 1, lr=(10.0, 20.0), std=0.01)
    _deeplab_tail(w, phase, "fc8_voc12", interp, argmax)
    return w.text()


def deeplab_aspp(phase: str = "DEPLOY", batch: int = 1, num_classes: int = 21, width_div: int = 1, fc_div: int = 1, size: int = 321,
                 rates: Sequence[int] = (6, 12, 18, 24), interp: bool = False, argmax: bool = False) -> str:
    """The DeepLab-v2 VGG16 head (atrous spatial pyramid pooling): behind pool5 one branch per rate r, fc6_i 3x3 with 1024 outputs at
    dilation r (pad r), fc7_i 1x1 (ReLU, Dropout 0.5 behind both), fc8_voc12_i; the branches' scores are summed by the Eltwise
    fc8_voc12.  Phases, label, interp, argmax and width_div / fc_div as deeplab_largefov."""
    _check_phase(phase)
    w = _Writer()
    w.raw('name: "DeepLab-v2-ASPP"')
    feat = _deeplab_vgg(w, phase, batch, size, width_div, interp)
    fc = max(1024 // fc_div, 1)
    scores = []
    for i, r in enumerate(rates, 1):
        _dl_conv(w, "fc6_%d" % i, feat, fc, 3, int(r), int(r), relu="relu6_%d" % i, drop="drop6_%d" % i)
        _dl_conv(w, "fc7_%d" % i, "fc6_%d" % i, fc, 1, relu="relu7_%d" % i, drop="drop7_%d" % i)
        scores.append(_dl_conv(w, "fc8_voc12_%d" % i, "fc7_%d" % i, num_classes, 1, lr=(10.0, 20.0), std=0.01))
    w.layer("fc8_voc12", "Eltwise", scores, ["fc8_voc12"], "  eltwise_param { operation: SUM }")
    _deeplab_tail(w, phase, "fc8_voc12", interp, argmax)
    return w.text()


# ----------------------------------------------------------------------
# Inception-v3 (Szegedy, Vanhoucke, Ioffe, Shlens, Wojna: "Rethinking the Inception Architecture for Computer Vision"): the structure of
# the paper - factorised 1x7 / 7x1 and 1x3 / 3x1 convolutions - under a naming scheme of this project's own
# ----------------------------------------------------------------------

def _iv3_conv(w: _Writer, name: str, bottom: str, num_output: int, kernel, phase: str, pad=0, stride: int = 1) -> str:
    """Convolution `<name>` (bias_term: false; kernel and pad an int or an (h, w) pair, written as kernel_h / kernel_w / pad_h / pad_w
    where the axes differ) with BatchNorm `<name>/bn`, Scale `<name>/scale` (bias_term: true) and ReLU `<name>/relu` in place on its
    top; returns the top."""
    kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    if (kh, ph) == (kw, pw):
        geo = "    num_output: %d\n    kernel_size: %d\n    pad: %d\n    stride: %d\n" % (num_output, kh, ph, stride)
    else:
        geo = "    num_output: %d\n    kernel_h: %d\n    kernel_w: %d\n    pad_h: %d\n    pad_w: %d\n    stride: %d\n" % (num_output, kh, kw, ph, pw, stride)
    fill = "    weight_filler { type: \"gaussian\" std: %g }\n" % (2.0 / (kh * kw * num_output)) ** 0.5
    w.layer(name, "Convolution", [bottom], [name], "  convolution_param {\n%s    bias_term: false\n%s  }" % (geo, fill))
    stats = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3) if phase != "DEPLOY" else "  batch_norm_param { use_global_stats: true }"
    w.layer(name + "/bn", "BatchNorm", [name], [name], stats)
    w.layer(name + "/scale", "Scale", [name], [name], "  scale_param { bias_term: true }")
    w.layer(name + "/relu", "ReLU", [name], [name])
    return name


def _iv3_pool(w: _Writer, name: str, bottom: str, pool: str, stride: int) -> str:
    w.layer(name, "Pooling", [bottom], [name], "  pooling_param { pool: %s kernel_size: 3 stride: %d%s }" % (pool, stride, " pad: 1" if stride == 1 else ""))
    return name


def inception_v3_grids(size) -> List[Tuple[int, int]]:
    """The (h, w) grids of Inception-v3 on a `size` input (an edge or an (h, w) pair): behind the stem (35 at 299), behind the first
    reduction (17) and behind the second (8).  A reduction concatenates a 3x3 / 2 convolution, whose extent Caffe floors, with a
    3x3 / 2 pooling, whose extent Caffe ceils: a size at which the two disagree is a ValueError."""
    from .netspec import conv_out, pool_out
    hw = (size, size) if isinstance(size, int) else tuple(int(v) for v in size)
    if len(hw) != 2 or min(hw) < 1:
        raise ValueError("size must be an edge or an (h, w) pair, got %r" % (size,))

    def stem(v: int) -> int:
        v = conv_out(conv_out(conv_out(v, 3, 2, 0), 3, 1, 0), 3, 1, 1)          # conv1 3x3 / 2, conv2 3x3, conv3 3x3 pad 1
        v = conv_out(pool_out(v, 3, 2, 0), 3, 1, 0) if v >= 3 else 0             # pool1, conv4 1x1, conv5 3x3
        return pool_out(v, 3, 2, 0) if v >= 3 else 0                            # pool2
    grids = [tuple(stem(v) for v in hw)]
    for which in ("reduction_a", "reduction_b"):
        if min(grids[-1]) < 3:
            raise ValueError("inception_v3: a %s input leaves a %dx%d grid in front of %s (at least 3x3)" % (hw, grids[-1][0], grids[-1][1], which))
        c, p = tuple(conv_out(v, 3, 2, 0) for v in grids[-1]), tuple(pool_out(v, 3, 2, 0) for v in grids[-1])
        if c != p:
            raise ValueError("inception_v3: on a %s input %s's 3x3 / 2 convolution gives a %dx%d grid and its 3x3 / 2 pooling %dx%d: they cannot "
                             "be concatenated (299, or 171 x 139, agree)" % (hw, which, c[0], c[1], p[0], p[1]))
        grids.append(c)
    return grids


def inception_v3(phase: str = "DEPLOY", batch: int = 1, classes: int = 1000, width_div: int = 1, size=299, fillers: bool = True) -> str:
    """Inception-v3: the structure of the paper (no published prototxt was at hand: the names below are this project's, and a
    caffemodel from elsewhere maps only if it uses them).  The stem (conv1 3x3 / 2, conv2 3x3, conv3 3x3 pad 1, pool1 MAX 3x3 / 2,
    conv4 1x1, conv5 3x3, pool2 MAX 3x3 / 2), three 35-grid modules mixed_35a / b / c, the grid reduction reduction_a, four 17-grid
    modules mixed_17a .. d with 1x7 / 7x1 chains, reduction_b with its 1x7, 7x1, 3x3 / 2 branch, two 8-grid modules mixed_8a / b with
    the split 1x3 / 3x1 pairs, pool3 (global AVE), drop (ratio 0.2), the InnerProduct `classifier`, and `prob` (DEPLOY), `loss`
    (SoftmaxWithLoss over an (N,) `label`; TRAIN and TEST) and `accuracy` (TEST).  No auxiliary head.

    Names: a convolution is `<module>/<branch>_<kh>x<kw>` (`<branch>` = 1x1, 5x5, 3x3dbl, 7x7, 7x7dbl, 3x3, 7x7x3, pool; a letter
    a, b, c ... where a branch has several of one shape), its top has the same name, and BatchNorm `<name>/bn`, Scale `<name>/scale`
    and ReLU `<name>/relu` follow in place; a module's pooling is `<module>/pool`, its Concat and output blob `<module>`.  A
    rectangular layer is written with kernel_h / kernel_w / pad_h / pad_w.  width_div divides every convolution width, size is the
    image edge or an (h, w) pair; inception_v3_grids refuses a size at which a reduction's convolution and pooling grids differ."""
    _check_phase(phase)
    inception_v3_grids(size)
    hw = (size, size) if isinstance(size, int) else tuple(int(v) for v in size)
    wd = lambda c: max(c // width_div, 1)
    cv = lambda name, bottom, c, k, pad=0, stride=1: _iv3_conv(w, name, bottom, wd(c), k, phase, pad, stride)
    w = _Writer()
    w.raw('name: "Inception-v3"')
    w.layer("data", "Input", [], ["data"], "  input_param { shape { dim: %d dim: 3 dim: %d dim: %d } }" % (batch, hw[0], hw[1]))
    if phase != "DEPLOY":
        w.layer("label", "Input", [], ["label"], "  input_param { shape { dim: %d } }" % batch)
    x = cv("conv1_3x3", "data", 32, 3, 0, 2)
    x = cv("conv2_3x3", x, 32, 3)
    x = cv("conv3_3x3", x, 64, 3, 1)
    x = _iv3_pool(w, "pool1", x, "MAX", 2)
    x = cv("conv4_1x1", x, 80, 1)
    x = cv("conv5_3x3", x, 192, 3)
    x = _iv3_pool(w, "pool2", x, "MAX", 2)
    for m, pf in (("mixed_35a", 32), ("mixed_35b", 64), ("mixed_35c", 64)):
        b1 = cv(m + "/1x1_1x1", x, 64, 1)
        b2 = cv(m + "/5x5_5x5", cv(m + "/5x5_1x1", x, 48, 1), 64, 5, 2)
        b3 = cv(m + "/3x3dbl_1x1", x, 64, 1)
        b3 = cv(m + "/3x3dbl_b_3x3", cv(m + "/3x3dbl_a_3x3", b3, 96, 3, 1), 96, 3, 1)
        b4 = cv(m + "/pool_1x1", _iv3_pool(w, m + "/pool", x, "AVE", 1), pf, 1)
        w.layer(m, "Concat", [b1, b2, b3, b4], [m])
        x = m
    m = "reduction_a"
    b1 = cv(m + "/3x3_3x3", x, 384, 3, 0, 2)
    b2 = cv(m + "/3x3dbl_a_3x3", cv(m + "/3x3dbl_1x1", x, 64, 1), 96, 3, 1)
    b2 = cv(m + "/3x3dbl_b_3x3", b2, 96, 3, 0, 2)
    w.layer(m, "Concat", [b1, b2, _iv3_pool(w, m + "/pool", x, "MAX", 2)], [m])
    x = m
    for m, c7 in (("mixed_17a", 128), ("mixed_17b", 160), ("mixed_17c", 160), ("mixed_17d", 192)):
        b1 = cv(m + "/1x1_1x1", x, 192, 1)
        b2 = cv(m + "/7x7_1x7", cv(m + "/7x7_1x1", x, c7, 1), c7, (1, 7), (0, 3))
        b2 = cv(m + "/7x7_7x1", b2, 192, (7, 1), (3, 0))
        b3 = cv(m + "/7x7dbl_a_7x1", cv(m + "/7x7dbl_1x1", x, c7, 1), c7, (7, 1), (3, 0))
        b3 = cv(m + "/7x7dbl_b_7x1", cv(m + "/7x7dbl_a_1x7", b3, c7, (1, 7), (0, 3)), c7, (7, 1), (3, 0))
        b3 = cv(m + "/7x7dbl_b_1x7", b3, 192, (1, 7), (0, 3))
        b4 = cv(m + "/pool_1x1", _iv3_pool(w, m + "/pool", x, "AVE", 1), 192, 1)
        w.layer(m, "Concat", [b1, b2, b3, b4], [m])
        x = m
    m = "reduction_b"
    b1 = cv(m + "/3x3_3x3", cv(m + "/3x3_1x1", x, 192, 1), 320, 3, 0, 2)
    b2 = cv(m + "/7x7x3_1x7", cv(m + "/7x7x3_1x1", x, 192, 1), 192, (1, 7), (0, 3))
    b2 = cv(m + "/7x7x3_3x3", cv(m + "/7x7x3_7x1", b2, 192, (7, 1), (3, 0)), 192, 3, 0, 2)
    w.layer(m, "Concat", [b1, b2, _iv3_pool(w, m + "/pool", x, "MAX", 2)], [m])
    x = m
    for m in ("mixed_8a", "mixed_8b"):
        b1 = cv(m + "/1x1_1x1", x, 320, 1)
        b2 = cv(m + "/3x3_1x1", x, 384, 1)
        b2a, b2b = cv(m + "/3x3_1x3", b2, 384, (1, 3), (0, 1)), cv(m + "/3x3_3x1", b2, 384, (3, 1), (1, 0))
        b3 = cv(m + "/3x3dbl_3x3", cv(m + "/3x3dbl_1x1", x, 448, 1), 384, 3, 1)
        b3a, b3b = cv(m + "/3x3dbl_1x3", b3, 384, (1, 3), (0, 1)), cv(m + "/3x3dbl_3x1", b3, 384, (3, 1), (1, 0))
        b4 = cv(m + "/pool_1x1", _iv3_pool(w, m + "/pool", x, "AVE", 1), 192, 1)
        w.layer(m, "Concat", [b1, b2a, b2b, b3a, b3b, b4], [m])
        x = m
    w.layer("pool3", "Pooling", [x], ["pool3"], "  pooling_param { pool: AVE global_pooling: true }")
    w.layer("drop", "Dropout", ["pool3"], ["pool3"], "  dropout_param { dropout_ratio: 0.2 }")
    _cn_fc(w, "classifier", "pool3", classes, 0.01, 0.0)
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", ["classifier"], ["prob"])
    else:
        if phase == "TEST":
            w.layer("accuracy", "Accuracy", ["classifier", "label"], ["accuracy"])
        w.layer("loss", "SoftmaxWithLoss", ["classifier", "label"], ["loss"])
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# MobileNet v1 (Howard et al.: "MobileNets: Efficient Convolutional Neural Networks for Mobile Vision Applications") and v2 (Sandler et
# al.: "MobileNetV2: Inverted Residuals and Linear Bottlenecks"): the structure of the papers.  The depthwise layers are written the way
# the published Caffe ports write them - type "Convolution" with group == num_output and engine: CAFFE - so a NetSpec takes them with
# depthwise=True (caffe.Net and the solvers pass it).
# ----------------------------------------------------------------------

def _mb_conv(w: _Writer, name: str, bottom: str, num_output: int, k: int, stride: int, phase: str, relu: Optional[str], group: int = 1,
             act: str = "ReLU") -> str:
    """Convolution `<name>` (bias_term: false, pad k // 2; group > 1: depthwise) with BatchNorm `<name>/bn` and Scale `<name>/scale`
    (bias_term: true) in place on its top and, with `relu`, a layer of that name and of type `act` (ReLU, ReLU6, Swish); returns the top."""
    geo = "    num_output: %d\n    bias_term: false\n    pad: %d\n    kernel_size: %d\n" % (num_output, k // 2, k)
    if group > 1:
        geo += "    group: %d\n    engine: CAFFE\n" % group
    geo += "    stride: %d\n" % stride
    fan = k * k * (1 if group > 1 else num_output)      # (a depthwise filter sees one channel)
    fill = "    weight_filler { type: \"gaussian\" std: %g }\n" % (2.0 / fan) ** 0.5
    w.layer(name, "Convolution", [bottom], [name], "  param { lr_mult: 1 decay_mult: 1 }\n  convolution_param {\n%s%s  }" % (geo, fill))
    stats = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3) if phase != "DEPLOY" else "  batch_norm_param { use_global_stats: true }"
    w.layer(name + "/bn", "BatchNorm", [name], [name], stats)
    w.layer(name + "/scale", "Scale", [name], [name], "  scale_param { bias_term: true }")
    if relu:
        w.layer(relu, act, [name], [name])
    return name


def _mb_tail(w: _Writer, phase: str, feat: str, classes: int, dropout: float = 0.0) -> None:
    """pool6 (global AVE), with `dropout` an in-place Dropout drop6 of that ratio, the 1x1 convolution classifier fc7 and prob (DEPLOY) /
    loss over an (N, 1, 1, 1) `label`, accuracy in TEST."""
    w.layer("pool6", "Pooling", [feat], ["pool6"], "  pooling_param { pool: AVE global_pooling: true }")
    if dropout:
        w.layer("drop6", "Dropout", ["pool6"], ["pool6"], "  dropout_param { dropout_ratio: %g }" % dropout)
    w.layer("fc7", "Convolution", ["pool6"], ["fc7"], "  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }\n"
            "  convolution_param {\n    num_output: %d\n    kernel_size: 1\n    weight_filler { type: \"gaussian\" std: 0.01 }\n"
            "    bias_filler { type: \"constant\" value: 0 }\n  }" % classes)
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", ["fc7"], ["prob"])
    else:
        if phase == "TEST":
            w.layer("accuracy", "Accuracy", ["fc7", "label"], ["accuracy"])
        w.layer("loss", "SoftmaxWithLoss", ["fc7", "label"], ["loss"])


MOBILENET_V1 = (("2_1", 64, 1), ("2_2", 128, 2), ("3_1", 128, 1), ("3_2", 256, 2), ("4_1", 256, 1), ("4_2", 512, 2), ("5_1", 512, 1), ("5_2", 512, 1),
                ("5_3", 512, 1), ("5_4", 512, 1), ("5_5", 512, 1), ("5_6", 1024, 2), ("6", 1024, 1))      # (tag, width of the 1x1, stride of the 3x3)
MOBILENET_V2 = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))      # (t, c, n, s) of the paper


def mobilenet_v1(phase: str = "DEPLOY", batch: int = 1, classes: int = 1000, width_div: int = 1, size: int = 224, fillers: bool = True) -> str:
    """MobileNet v1: the structure of the paper (no published prototxt was at hand).  The stem conv1 3x3 / 2 (32), thirteen pairs of a
    depthwise 3x3 `conv<tag>/dw` and a 1x1 `conv<tag>/sep` with the strides 1, 2, 1, 2, 1, 2, 1 x 5, 2, 1 and the widths 64 .. 1024, every
    convolution bias-free and followed by BatchNorm, Scale (bias_term: true) and ReLU in place; pool6 (global AVE), the 1x1 convolution
    classifier fc7, and prob (DEPLOY), loss (SoftmaxWithLoss over an (N, 1, 1, 1) `label`; TRAIN and TEST) and accuracy (TEST).

    Names: conv1, conv2_1/dw, conv2_1/sep ... conv5_6/dw, conv6/sep, pool6, fc7 and prob are those of the common Caffe port, as far as
    remembered; `<conv>/bn`, `<conv>/scale` and the ReLUs `relu<tag>` are this project's.  A caffemodel from elsewhere maps only where
    the names agree.  A depthwise layer is type "Convolution" with group == num_output and engine: CAFFE, as the ports write it.
    width_div divides every convolution width, size is the image edge."""
    _check_phase(phase)
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "MobileNet-v1"')
    _inputs(w, phase, batch, ["data"], size, ("label", (batch, 1, 1, 1)))
    x, c = _mb_conv(w, "conv1", "data", wd(32), 3, 2, phase, "relu1"), wd(32)
    for tag, width, stride in MOBILENET_V1:
        x = _mb_conv(w, "conv%s/dw" % tag, x, c, 3, stride, phase, "relu%s/dw" % tag, group=c)
        x, c = _mb_conv(w, "conv%s/sep" % tag, x, wd(width), 1, 1, phase, "relu%s/sep" % tag), wd(width)
    _mb_tail(w, phase, x, classes)
    return w.text() if fillers else _strip_fillers(w.text())


def _mb2_block(w: _Writer, tag: str, x: str, cin: int, cout: int, t: int, stride: int, phase: str, act: str = "ReLU") -> str:
    """One inverted residual of MobileNet v2: 1x1 `<tag>/expand` to t * cin (left out at t == 1) + ReLU, depthwise 3x3 `<tag>/dwise` at
    `stride` + ReLU (`act`: ReLU or ReLU6, both layers), the linear 1x1 `<tag>/linear` to cout; with stride 1 and cin == cout the Eltwise sum `block_<tag>` with the input."""
    y, mid = x, cin * t
    if t != 1:
        y = _mb_conv(w, "conv%s/expand" % tag, y, mid, 1, 1, phase, "relu%s/expand" % tag, act=act)
    y = _mb_conv(w, "conv%s/dwise" % tag, y, mid, 3, stride, phase, "relu%s/dwise" % tag, group=mid, act=act)
    y = _mb_conv(w, "conv%s/linear" % tag, y, cout, 1, 1, phase, None)
    if stride == 1 and cin == cout:
        w.layer("block_%s" % tag, "Eltwise", [x, y], ["block_%s" % tag], "  eltwise_param { operation: SUM }")
        y = "block_%s" % tag
    return y


def mobilenet_v2(phase: str = "DEPLOY", batch: int = 1, classes: int = 1000, width_div: int = 1, size: int = 224, fillers: bool = True,
                 relu6: bool = False) -> str:
    """MobileNet v2: the structure of the paper (no published prototxt was at hand).  conv1 3x3 / 2 (32), the seven stages (t, c, n, s) =
    (1,16,1,1), (6,24,2,2), (6,32,3,2), (6,64,4,2), (6,96,3,1), (6,160,3,2), (6,320,1,1) of inverted residuals - 17 depthwise layers,
    linear bottlenecks, 10 Eltwise sums - the 1x1 convolution conv9 to 1280, pool6 (global AVE), the 1x1 classifier fc7 and the ends of
    mobilenet_v1.  Plain ReLU by default, as the common Caffe port has it; relu6=True writes the paper's ReLU6 - `type: "ReLU6"`, the
    MobileNet forks' layer (csrc/neuron.hip) - in the same places under the same names: behind conv1, every expand and depthwise
    convolution and conv9, 35 layers.

    Names: the spelling `conv<stage>_<block>/expand`, `/dwise`, `/linear`, `block_<stage>_<block>`, pool6 and fc7 is the common Caffe
    port's; the numbering (stage 2 .. 8 of the paper's table, block 1 .. n) and conv9, `<conv>/bn`, `<conv>/scale` and the ReLUs are this
    project's, and the first block has no expand layer (t = 1), as in the paper.  width_div divides every width, size is the image edge."""
    _check_phase(phase)
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "MobileNet-v2"')
    _inputs(w, phase, batch, ["data"], size, ("label", (batch, 1, 1, 1)))
    act = "ReLU6" if relu6 else "ReLU"
    x, c = _mb_conv(w, "conv1", "data", wd(32), 3, 2, phase, "relu1", act=act), wd(32)
    for stage, (t, width, n, s) in enumerate(MOBILENET_V2, 2):
        for b in range(n):
            x, c = _mb2_block(w, "%d_%d" % (stage, b + 1), x, c, wd(width), t, s if b == 0 else 1, phase, act), wd(width)
    x = _mb_conv(w, "conv9", x, wd(1280), 1, 1, phase, "relu9", act=act)
    _mb_tail(w, phase, x, classes)
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# EfficientNet-B0 (Tan, Le: "EfficientNet: Rethinking Model Scaling for Convolutional Neural Networks"): MBConv blocks - MobileNet v2's
# inverted residuals with a Squeeze-and-Excitation gate on the depthwise branch - and Swish (BVLC master's layer, csrc/neuron.hip).
# ----------------------------------------------------------------------

EFFICIENTNET_B0 = ((1, 16, 1, 1, 3), (6, 24, 2, 2, 3), (6, 40, 2, 2, 5), (6, 80, 3, 2, 3), (6, 112, 3, 1, 5), (6, 192, 4, 2, 5),
                   (6, 320, 1, 1, 3))      # (expand, channels, repeats, stride, kernel) of the paper's table


def _mbconv_block(w: _Writer, tag: str, x: str, cin: int, cout: int, t: int, stride: int, k: int, phase: str) -> str:
    """One MBConv block: 1x1 `<tag>/expand` to t * cin (left out at t == 1) + Swish, depthwise k x k `<tag>/dwise` at `stride` + Swish, the
    SE gate as se_resnet(form="scale") writes it - global AVE pooling `<tag>/se_pool`, InnerProduct `<tag>/se_reduce` to max(cin // 4, 1)
    + Swish on the (N, s) blob, InnerProduct `<tag>/se_expand`, Sigmoid `<tag>/se_prob`, the two-bottom `Scale { axis: 0 }` `<tag>/se_scale`
    on the depthwise branch -, the linear 1x1 `<tag>/project` to cout; with stride 1 and cin == cout the Eltwise sum `block_<tag>`."""
    y, mid = x, cin * t
    if t != 1:
        y = _mb_conv(w, "conv%s/expand" % tag, y, mid, 1, 1, phase, "swish%s/expand" % tag, act="Swish")
    y = _mb_conv(w, "conv%s/dwise" % tag, y, mid, k, stride, phase, "swish%s/dwise" % tag, group=mid, act="Swish")
    se = "conv%s/se_" % tag
    w.layer(se + "pool", "Pooling", [y], [se + "pool"], "  pooling_param { pool: AVE global_pooling: true }")
    g = _se_fc(w, se + "reduce", se + "pool", max(cin // 4, 1), "scale")
    w.layer("swish%s/se" % tag, "Swish", [g], [g])
    g = _se_fc(w, se + "expand", g, mid, "scale")
    w.layer(se + "prob", "Sigmoid", [g], [se + "prob"])
    w.layer(se + "scale", "Scale", [y, se + "prob"], [se + "scale"], "  scale_param { axis: 0 }")
    y = _mb_conv(w, "conv%s/project" % tag, se + "scale", cout, 1, 1, phase, None)
    if stride == 1 and cin == cout:
        w.layer("block_%s" % tag, "Eltwise", [x, y], ["block_%s" % tag], "  eltwise_param { operation: SUM }")
        y = "block_%s" % tag
    return y


def efficientnet_b0(phase: str = "DEPLOY", batch: int = 1, classes: int = 1000, width_div: int = 1, size: int = 224, fillers: bool = True) -> str:
    """EfficientNet-B0: the structure of the paper in this project's layers (no published prototxt was at hand, so every name is this
    project's own, in the spelling of models.mobilenet_v2: conv1, conv<stage>_<block>/expand, /dwise, /se_pool, /se_reduce, /se_expand,
    /se_prob, /se_scale, /project, block_<stage>_<block>, conv9, pool6, drop6, fc7; `<conv>/bn`, `<conv>/scale`, the Swish layers
    swish1, swish<stage>_<block>/expand, /dwise, /se and swish9).  The stem conv1 3x3 / 2 (32), the seven MBConv stages (expand,
    channels, repeats, stride, kernel) = (1,16,1,1,3), (6,24,2,2,3), (6,40,2,2,5), (6,80,3,2,3), (6,112,3,1,5), (6,192,4,2,5),
    (6,320,1,1,3) - 16 depthwise layers, 9 Eltwise sums -, the 1x1 convolution conv9 to 1280, pool6 (global AVE), Dropout 0.2, the
    classifier fc7 and the ends of mobilenet_v1.  BatchNorm + Scale behind every convolution but the SE layers; `Swish` in place behind
    conv1, every expand and depthwise convolution, every SE squeeze and conv9: 49 layers.  The squeeze width is the block's input
    channels // 4, at least 1.
    Not reproduced: drop-connect (stochastic depth) on the residual branches, and the release's TensorFlow "SAME" padding - at stride 2
    it pads the far edges only; this is Caffe's symmetric pad = k // 2, so a weight file converted from the release does not give the
    release's numbers.  Needs a NetSpec with depthwise=True and scale_gate=True (caffe.Net, the solvers and the caffe tool pass them).
    width_div divides every convolution width, size is the image edge."""
    _check_phase(phase)
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "EfficientNet-B0"')
    _inputs(w, phase, batch, ["data"], size, ("label", (batch, 1, 1, 1)))
    x, c = _mb_conv(w, "conv1", "data", wd(32), 3, 2, phase, "swish1", act="Swish"), wd(32)
    for stage, (t, width, n, s, k) in enumerate(EFFICIENTNET_B0, 2):
        for b in range(n):
            x, c = _mbconv_block(w, "%d_%d" % (stage, b + 1), x, c, wd(width), t, s if b == 0 else 1, k, phase), wd(width)
    x = _mb_conv(w, "conv9", x, wd(1280), 1, 1, phase, "swish9", act="Swish")
    _mb_tail(w, phase, x, classes, dropout=0.2)
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# ShuffleNet v1 (Zhang et al.: "ShuffleNet: An Extremely Efficient Convolutional Neural Network for Mobile Devices") and v2 (Ma et al.:
# "ShuffleNet V2: Practical Guidelines for Efficient CNN Architecture Design"): grouped 1x1 convolutions, depthwise 3x3 convolutions and
# the ports' ShuffleChannel layer (csrc/shuffle.hip).  A channel window has to start on 16 bytes (4 floats) here, so only the widths of
# the papers' tables whose groups and branches are multiples of 4 channels are written; the others are refused with the channel count.
# ----------------------------------------------------------------------

SHUFFLENET_V1 = {1: 144, 2: 200, 3: 240, 4: 272, 8: 384}      # groups -> width of stage 2 (stages 3 and 4 double it), the paper's table
SHUFFLENET_V2 = {0.5: (48, 1024), 1.0: (116, 1024), 1.5: (176, 1024), 2.0: (244, 2048)}      # width -> (stage 2, conv5)
SHUFFLENET_REPEATS = (4, 8, 4)                                   # units of stages 2, 3 and 4, the first of each at stride 2
DEPTHWISE_TYPES = ("Convolution", "ConvolutionDepthwise")


def _shf_conv(w: _Writer, name: str, bottom: str, cin: int, num_output: int, k: int, stride: int, phase: str, relu: bool, group: int = 1,
              depthwise_type: Optional[str] = None) -> str:
    """Convolution `<name>` (bias_term: false, pad k // 2) with BatchNorm `<name>_bn` and Scale `<name>_scale` (bias_term: true) in place
    on its top and, with `relu`, the ReLU `<name>_relu`; returns the top.  group > 1: a grouped convolution, whose groups must be
    whole 16-byte segments of 4 channels on both sides.  depthwise_type: the layer is depthwise (num_output == cin), written as
    type "Convolution" with group: C engine: CAFFE or as type "ConvolutionDepthwise" without a group."""
    geo = "    num_output: %d\n    bias_term: false\n    pad: %d\n    kernel_size: %d\n" % (num_output, k // 2, k)
    type_ = "Convolution"
    if depthwise_type is not None:
        type_ = depthwise_type
        if depthwise_type == "Convolution":
            geo += "    group: %d\n    engine: CAFFE\n" % num_output
    elif group > 1:
        for what, c in (("input", cin), ("output", num_output)):
            if c % group or (c // group) % 4:
                raise ValueError("ShuffleNet: %s has %d %s channels in %d groups: %s channels per group are no whole 16-byte segments "
                                 "(multiples of 4)" % (name, c, what, group, "%d" % (c // group) if c % group == 0 else "%d / %d" % (c, group)))
        geo += "    group: %d\n" % group
    geo += "    stride: %d\n" % stride
    fan = k * k * (1 if depthwise_type is not None else num_output // group)
    fill = "    weight_filler { type: \"gaussian\" std: %g }\n" % (2.0 / fan) ** 0.5
    w.layer(name, type_, [bottom], [name], "  param { lr_mult: 1 decay_mult: 1 }\n  convolution_param {\n%s%s  }" % (geo, fill))
    stats = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3) if phase != "DEPLOY" else "  batch_norm_param { use_global_stats: true }"
    w.layer(name + "_bn", "BatchNorm", [name], [name], stats)
    w.layer(name + "_scale", "Scale", [name], [name], "  scale_param { bias_term: true }")
    if relu:
        w.layer(name + "_relu", "ReLU", [name], [name])
    return name


def _shf_stem(w: _Writer, name: str, phase: str, batch: int, size: int, c1: int) -> Tuple[str, int]:
    """Inputs, conv1 3x3 / 2 to c1 channels + BatchNorm, Scale, ReLU, pool1 MAX 3x3 / 2; returns the top and its edge."""
    w.raw('name: "%s"' % name)
    _inputs(w, phase, batch, ["data"], size, ("label", (batch, 1, 1, 1)))
    _shf_conv(w, "conv1", "data", 3, c1, 3, 2, phase, True)
    w.layer("pool1", "Pooling", ["conv1"], ["pool1"], "  pooling_param { pool: MAX kernel_size: 3 stride: 2 }")
    h = (size + 2 - 3) // 2 + 1                   # convolution: rounded down
    return "pool1", -(-(h - 3) // 2) + 1          # pooling: rounded up


def _shf_tail(w: _Writer, phase: str, feat: str, classes: int) -> None:
    """pool_ave (global AVE), the 1x1 convolution classifier fc1000 and prob (DEPLOY) / loss over an (N, 1, 1, 1) `label`, accuracy in TEST."""
    w.layer("pool_ave", "Pooling", [feat], ["pool_ave"], "  pooling_param { pool: AVE global_pooling: true }")
    w.layer("fc1000", "Convolution", ["pool_ave"], ["fc1000"], "  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }\n"
            "  convolution_param {\n    num_output: %d\n    kernel_size: 1\n    weight_filler { type: \"gaussian\" std: 0.01 }\n"
            "    bias_filler { type: \"constant\" value: 0 }\n  }" % classes)
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", ["fc1000"], ["prob"])
    else:
        if phase == "TEST":
            w.layer("accuracy", "Accuracy", ["fc1000", "label"], ["accuracy"])
        w.layer("loss", "SoftmaxWithLoss", ["fc1000", "label"], ["loss"])


def _check_depthwise_type(depthwise_type: str) -> None:
    if depthwise_type not in DEPTHWISE_TYPES:
        raise ValueError("depthwise_type must be one of %s" % list(DEPTHWISE_TYPES))


def shufflenet_v1(phase: str = "DEPLOY", groups: int = 3, batch: int = 1, classes: int = 1000, width_div: int = 1, size: int = 224,
                  fillers: bool = True, depthwise_type: str = "Convolution") -> str:
    """ShuffleNet v1 1x: the structure of the paper (no published prototxt was at hand).  conv1 3x3 / 2 (24) + BatchNorm, Scale, ReLU,
    pool1 MAX 3x3 / 2, stages 2 - 4 of 4, 8 and 4 units at the widths 240 / 480 / 960 (groups = 3), pool_ave (global AVE), the 1x1
    classifier fc1000 and prob (DEPLOY), loss (SoftmaxWithLoss over an (N, 1, 1, 1) `label`; TRAIN and TEST) and accuracy (TEST).
    Unit `resx<i>`, i = 1 .. 16: the grouped 1x1 `resx<i>_conv1` to a quarter of the unit's width (not grouped in resx1, whose input has
    24 channels) + BatchNorm, Scale, ReLU; `shuffle<i>`, ShuffleChannel { group: groups }; the depthwise 3x3 `resx<i>_conv2` + BatchNorm,
    Scale; the grouped 1x1 `resx<i>_conv3` + BatchNorm, Scale; then at stride 1 the Eltwise SUM `resx<i>_elewise` with the input, at
    stride 2 - the first unit of a stage - the Concat `resx<i>_concat` of the AVE-pooled input `resx<i>_match_conv` and the branch, which
    then has the unit's width less the input's; ReLU in place on either.
    The two branches of a stride-2 unit must agree under Caffe's shape rules, where a convolution rounds down and a pooling up: beside
    the depthwise `k3 s2 p1` the shortcut is AVE 3x3 / 2 with pad 0 on an even edge and with pad 1 on an odd one (Caffe's AVE pooling
    divides by the window clipped to the padded blob, so with the pad the border means differ from the paper's).
    Names: conv1, pool1, resx<i>_conv1 / _conv2 / _conv3, shuffle<i>, resx<i>_match_conv, resx<i>_concat, resx<i>_elewise, pool_ave and
    fc1000 are those of the common Caffe port as far as remembered; `<conv>_bn`, `<conv>_scale`, the ReLUs `<blob>_relu` and prob are
    this project's.  A caffemodel from elsewhere maps only where the names agree.
    groups: only 3 (and 1, without grouped layers, at 144 / 288 / 576) keeps every group of every grouped convolution on whole 16-byte
    segments; 2, 4 and 8 - groups of 25, 17 and 45 channels - are refused with that count.  width_div divides the stage widths, and above 1 conv1
    becomes the largest multiple of 4 * groups at or below 24 / width_div (at least one such multiple): with groups = 3 only 1 and 5 divide
    every group into multiples of 4, anything else is refused the same way.  In halves the net stops at its first grouped convolution, resx1_conv3 with
    groups of 20 input channels: no whole segments of 8 halves.
    depthwise_type: "Convolution" writes the depthwise layers with group: C engine: CAFFE (a NetSpec takes them with depthwise=True, as
    caffe.Net and the solvers pass it), "ConvolutionDepthwise" as the ports' layer of that type."""
    _check_phase(phase)
    _check_depthwise_type(depthwise_type)
    if groups not in SHUFFLENET_V1:
        raise ValueError("groups must be one of %s" % sorted(SHUFFLENET_V1))
    w = _Writer()
    quantum = 4 * groups
    c = 24 if width_div == 1 else max(24 // width_div // quantum, 1) * quantum
    x, h = _shf_stem(w, "ShuffleNet-v1-g%d" % groups, phase, batch, size, c)
    unit = 0
    for stage, repeats in enumerate(SHUFFLENET_REPEATS):
        width = max((SHUFFLENET_V1[groups] << stage) // width_div, 1)
        for b in range(repeats):
            unit += 1
            tag, stride = "resx%d" % unit, 2 if b == 0 else 1
            if width % 4:
                raise ValueError("ShuffleNet v1: unit %s has %d channels: its bottleneck is no whole number of channels" % (tag, width))
            mid, out = width // 4, width - c if stride == 2 else width
            y = _shf_conv(w, tag + "_conv1", x, c, mid, 1, 1, phase, True, group=1 if unit == 1 else groups)
            w.layer("shuffle%d" % unit, "ShuffleChannel", [y], ["shuffle%d" % unit], "  shuffle_channel_param { group: %d }" % groups)
            y = _shf_conv(w, tag + "_conv2", "shuffle%d" % unit, mid, mid, 3, stride, phase, False, depthwise_type=depthwise_type)
            y = _shf_conv(w, tag + "_conv3", y, mid, out, 1, 1, phase, False, group=groups)
            if stride == 2:
                w.layer(tag + "_match_conv", "Pooling", [x], [tag + "_match_conv"],
                        "  pooling_param { pool: AVE kernel_size: 3 stride: 2%s }" % (" pad: 1" if h % 2 else ""))
                w.layer(tag + "_concat", "Concat", [tag + "_match_conv", y], [tag + "_concat"])
                x, h = tag + "_concat", (h + 2 - 3) // 2 + 1
            else:
                w.layer(tag + "_elewise", "Eltwise", [x, y], [tag + "_elewise"], "  eltwise_param { operation: SUM }")
                x = tag + "_elewise"
            w.layer(x + "_relu", "ReLU", [x], [x])
            c = width
    _shf_tail(w, phase, x, classes)
    return w.text() if fillers else _strip_fillers(w.text())


def shufflenet_v2(phase: str = "DEPLOY", width: float = 0.5, batch: int = 1, classes: int = 1000, width_div: int = 1, size: int = 224,
                  fillers: bool = True, depthwise_type: str = "Convolution") -> str:
    """ShuffleNet v2 at 0.5x or 1.5x: the structure of the paper (no published prototxt was at hand).  conv1 3x3 / 2 (24) + BatchNorm,
    Scale, ReLU, pool1 MAX 3x3 / 2, stages 2 - 4 of 4, 8 and 4 units at the widths 48 / 96 / 192 (0.5x) or 176 / 352 / 704 (1.5x), the 1x1
    convolution conv5 to 1024 + BatchNorm, Scale, ReLU, and the ends of shufflenet_v1 (pool_ave, fc1000, prob / loss / accuracy).
    Unit `stage<s>_<b>` at stride 1: the Slice `<unit>/slice` cuts the input in halves `<unit>/left` and `<unit>/right`; the right half
    goes through the 1x1 `<unit>/conv1` + BatchNorm, Scale, ReLU, the depthwise 3x3 `<unit>/dw` + BatchNorm, Scale and the 1x1
    `<unit>/conv2` + BatchNorm, Scale, ReLU, every one of half the unit's width; the Concat `<unit>/concat` of the left half and that
    branch; `<unit>/shuffle`, ShuffleChannel { group: 2 }, the unit's top.  At stride 2 - the first unit of a stage - there is no Slice:
    the left branch is the depthwise 3x3 / 2 `<unit>/left_dw` + BatchNorm, Scale and the 1x1 `<unit>/left_conv` + BatchNorm, Scale, ReLU
    on the whole input, the right branch starts from the whole input too, and each has half the new width.  Both branches of such a
    unit are `k3 s2 p1` convolutions, so they agree on every edge; no pooling is needed beside them.
    Names: conv1, pool1, conv5, pool_ave and fc1000 are the common Caffe port's as far as remembered; every unit's names, `<conv>_bn`,
    `<conv>_scale` and the ReLUs are this project's own.
    width: a half of the unit's width is a channel window (the Slice tops), which must start on 16 bytes: 24 / 48 / 96 channels (0.5x) and
    88 / 176 / 352 (1.5x) do, the 58 of 1.0x and the 122 of 2.0x do not, and those widths are refused with that count.  width_div divides
    every width and is refused the same way where a half is no multiple of 4 any more (0.5x: 1, 2, 3 and 6).  In halves the net runs
    where every half is a multiple of 8 (0.5x at width_div 1 and 3, 1.5x at 1): the Slice tops are then windows on 16 bytes of halves.
    depthwise_type: as in shufflenet_v1."""
    _check_phase(phase)
    _check_depthwise_type(depthwise_type)
    if width not in SHUFFLENET_V2:
        raise ValueError("width must be one of %s" % sorted(SHUFFLENET_V2))
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    stage2, last = SHUFFLENET_V2[width]
    x, _h = _shf_stem(w, "ShuffleNet-v2-%gx" % width, phase, batch, size, wd(24))
    c = wd(24)
    for stage, repeats in enumerate(SHUFFLENET_REPEATS, 2):
        full = wd(stage2 << (stage - 2))
        half = full // 2
        if full % 2 or half % 4:
            raise ValueError("ShuffleNet v2 %gx: the units of stage %d have %d channels, branches of %s: a branch is a channel window and "
                             "must be whole 16-byte segments (a multiple of 4 channels)" % (width, stage, full, "%d" % half if full % 2 == 0 else "%d / 2" % full))
        for b in range(repeats):
            tag = "stage%d_%d" % (stage, b + 1)
            if b == 0:
                y = _shf_conv(w, tag + "/left_dw", x, c, c, 3, 2, phase, False, depthwise_type=depthwise_type)
                left = _shf_conv(w, tag + "/left_conv", y, c, half, 1, 1, phase, True)
                right, cr = x, c
            else:
                left, right, cr = tag + "/left", tag + "/right", half
                w.layer(tag + "/slice", "Slice", [x], [left, right], "  slice_param { axis: 1 slice_point: %d }" % half)
            y = _shf_conv(w, tag + "/conv1", right, cr, half, 1, 1, phase, True)
            y = _shf_conv(w, tag + "/dw", y, half, half, 3, 2 if b == 0 else 1, phase, False, depthwise_type=depthwise_type)
            y = _shf_conv(w, tag + "/conv2", y, half, half, 1, 1, phase, True)
            w.layer(tag + "/concat", "Concat", [left, y], [tag + "/concat"])
            w.layer(tag + "/shuffle", "ShuffleChannel", [tag + "/concat"], [tag + "/shuffle"], "  shuffle_channel_param { group: 2 }")
            x, c = tag + "/shuffle", full
    x = _shf_conv(w, "conv5", x, c, wd(last), 1, 1, phase, True)
    _shf_tail(w, phase, x, classes)
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# SegNet and SegNet-Basic (Badrinarayanan, Kendall, Cipolla: "SegNet: A Deep Convolutional Encoder-Decoder Architecture for Image
# Segmentation"): encoders whose MAX poolings keep their indices (a second top, the mask) and decoders that unpool by them (the SegNet
# fork's Upsample layer).  The fork's `BN` layer is written as BatchNorm + Scale, its class-weighted loss as a plain SoftmaxWithLoss.
# ----------------------------------------------------------------------

def _hw(size) -> Tuple[int, int]:
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def _sn_conv(w: _Writer, name: str, bottom: str, num_output: int, k: int, phase: str, relu: Optional[str], bn: bool = True) -> str:
    """Convolution `<name>` (pad k // 2, with a bias) and, with `bn`, BatchNorm `<name>_bn` and Scale `<name>_scale` (bias_term: true) in
    place on its top; with `relu`, a ReLU of that name; returns the top."""
    w.layer(name, "Convolution", [bottom], [name], "  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }\n"
            "  convolution_param {\n    num_output: %d\n%s    kernel_size: %d\n    weight_filler { type: \"gaussian\" std: %g }\n"
            "    bias_filler { type: \"constant\" value: 0 }\n  }" % (num_output, "    pad: %d\n" % (k // 2) if k > 1 else "", k,
                                                                   (2.0 / (k * k * num_output)) ** 0.5))
    if bn:
        stats = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3) if phase != "DEPLOY" else "  batch_norm_param { use_global_stats: true }"
        w.layer(name + "_bn", "BatchNorm", [name], [name], stats)
        w.layer(name + "_scale", "Scale", [name], [name], "  scale_param { bias_term: true }")
    if relu:
        w.layer(relu, "ReLU", [name], [name])
    return name


def _sn_pool(w: _Writer, name: str, bottom: str) -> str:
    """2 x 2 / stride 2 MAX pooling with its mask: tops `<name>` and `<name>_mask`."""
    w.layer(name, "Pooling", [bottom], [name, name + "_mask"], "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }")
    return name


def _sn_upsample(w: _Writer, name: str, bottom: str, mask: str, hw: Tuple[int, int]) -> str:
    """Upsample by `mask` to hw, the extents of the pooling's bottom: `scale: 2` where both are even, else upsample_h / upsample_w - the
    way the published nets undo a ceil-mode pooling of an odd extent."""
    body = "scale: 2" if hw[0] % 2 == 0 and hw[1] % 2 == 0 else "upsample_h: %d upsample_w: %d" % hw
    w.layer(name, "Upsample", [bottom, mask], [name], "  upsample_param { %s }" % body)
    return name


def _sn_inputs(w: _Writer, phase: str, batch: int, hw: Tuple[int, int]) -> None:
    w.layer("data", "Input", [], ["data"], "  input_param { shape { dim: %d dim: 3 dim: %d dim: %d } }" % (batch, hw[0], hw[1]))
    if phase != "DEPLOY":
        w.layer("label", "Input", [], ["label"], "  input_param { shape { dim: %d dim: 1 dim: %d dim: %d } }" % (batch, hw[0], hw[1]))


def _sn_tail(w: _Writer, phase: str, score: str, argmax: bool = False) -> None:
    """prob (Softmax; DEPLOY) or loss (SoftmaxWithLoss, ignore_label 255; TRAIN and TEST) with accuracy in TEST.  argmax: DEPLOY ends
    in the label map `argmax` behind prob."""
    if phase == "DEPLOY":
        w.layer("prob", "Softmax", [score], ["prob"])
        if argmax:
            _label_map(w, "prob")
        return
    if phase == "TEST":
        w.layer("accuracy", "Accuracy", [score, "label"], ["accuracy"], "  accuracy_param { ignore_label: 255 }")
    w.layer("loss", "SoftmaxWithLoss", [score, "label"], ["loss"], "  loss_param { ignore_label: 255 }")


def _halved(hw: Tuple[int, int]) -> Tuple[int, int]:
    return (hw[0] + 1) // 2, (hw[1] + 1) // 2      # 2 x 2 / stride 2 in Caffe's ceil mode


def segnet_basic(phase: str = "DEPLOY", classes: int = 11, batch: int = 1, size=(360, 480), width_div: int = 1, argmax: bool = False) -> str:
    """SegNet-Basic: four encoder stages conv<i> 7x7 (64) + BatchNorm + ReLU + pool<i> 2x2 / 2 with the mask pool<i>_mask, four decoder
    stages upsample<i> (by pool<i>_mask) + conv_decode<i> 7x7 (64) + BatchNorm without a ReLU, and the 1x1 conv_classifier.  DEPLOY ends
    in prob (Softmax); TRAIN and TEST in loss (SoftmaxWithLoss over an (N, 1, H, W) `label`, ignore_label 255), TEST with accuracy.

    Names: conv1 .. conv4, relu<i>, pool<i> / pool<i>_mask, upsample<i>, conv_decode<i>, conv_classifier, `<conv>_bn`, loss, accuracy and
    prob are the published net's, as far as remembered.  `<conv>_bn` is a BatchNorm here (the fork's type is BN, which holds the scale and
    shift as well) and `<conv>_scale` is this project's; the published input LRN (norm) is not emitted, and the loss is not weighted
    by class frequencies.  An Upsample carries `scale: 2`, or upsample_h / upsample_w where the pooling's bottom has an odd extent.
    width_div divides the 64; size is the image edge or (height, width).  argmax=True ends the DEPLOY net in `argmax`, the label map
    behind prob (ArgMax, axis 1), as the published web-demo prototxt does."""
    _check_phase(phase)
    hw, c = _hw(size), max(64 // width_div, 1)
    w = _Writer()
    w.raw('name: "SegNet-Basic"')
    _sn_inputs(w, phase, batch, hw)
    x, planes = "data", []
    for i in range(1, 5):
        x = _sn_conv(w, "conv%d" % i, x, c, 7, phase, "relu%d" % i)
        planes.append(hw)
        x, hw = _sn_pool(w, "pool%d" % i, x), _halved(hw)
    for i in range(4, 0, -1):
        x = _sn_upsample(w, "upsample%d" % i, x, "pool%d_mask" % i, planes[i - 1])
        x = _sn_conv(w, "conv_decode%d" % i, x, c, 7, phase, None)
    x = _sn_conv(w, "conv_classifier", x, classes, 1, phase, None, bn=False)
    _sn_tail(w, phase, x, argmax)
    return w.text()


SEGNET_DECODER = ((5, (512, 512, 512)), (4, (512, 512, 256)), (3, (256, 256, 128)), (2, (128, 64)), (1, (64, 0)))      # widths of conv<b>_<n>_D .. conv<b>_1_D (0: the classes)


def segnet(phase: str = "DEPLOY", classes: int = 11, batch: int = 1, size=(360, 480), width_div: int = 1, argmax: bool = False) -> str:
    """SegNet: the 13 convolutions of VGG16 (3x3, pad 1) as the encoder, each with BatchNorm + ReLU, all five poolings 2x2 / 2 with a
    mask; the mirrored decoder upsample<b> (by pool<b>_mask) + conv<b>_<n>_D .. conv<b>_1_D, each with BatchNorm + ReLU but the last,
    conv1_1_D, which gives the class scores.  Ends as segnet_basic.

    Names: conv1_1 .. conv5_3, relu<b>_<i>, pool<b> / pool<b>_mask, upsample5 .. upsample1, conv5_3_D .. conv1_1_D, relu<b>_<i>_D and
    `<conv>_bn` are the published net's, as far as remembered; `<conv>_bn` is a BatchNorm here (the fork's BN also scales and shifts) and
    `<conv>_scale` is this project's.  The loss is not weighted by class frequencies.  width_div divides every width; size is the
    image edge or (height, width)."""
    _check_phase(phase)
    hw = _hw(size)
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "SegNet"')
    _sn_inputs(w, phase, batch, hw)
    x, planes = "data", {}
    for blk, convs, width_ in VGG16:
        for i in range(1, convs + 1):
            x = _sn_conv(w, "conv%d_%d" % (blk, i), x, wd(width_), 3, phase, "relu%d_%d" % (blk, i))
        planes[blk] = hw
        x, hw = _sn_pool(w, "pool%d" % blk, x), _halved(hw)
    for blk, widths in SEGNET_DECODER:
        x = _sn_upsample(w, "upsample%d" % blk, x, "pool%d_mask" % blk, planes[blk])
        for j, width_ in enumerate(widths):
            i = len(widths) - j
            if (blk, i) == (1, 1):
                x = _sn_conv(w, "conv1_1_D", x, classes, 3, phase, None, bn=False)
            else:
                x = _sn_conv(w, "conv%d_%d_D" % (blk, i), x, wd(width_), 3, phase, "relu%d_%d_D" % (blk, i))
    _sn_tail(w, phase, x, argmax)
    return w.text()


# ----------------------------------------------------------------------
# SSD (Liu et al.: "SSD: Single Shot MultiBox Detector") deploy nets: the detection head of Caffe-SSD (the weiliu89 fork) on MobileNet v1
# (the common Caffe port) and on VGG16 (SSD300).  Layer and blob names are the published ones, as remembered.
# ----------------------------------------------------------------------

def _ssd_refuse_training(phase: str) -> None:
    _check_phase(phase)
    if phase != "DEPLOY":
        raise NotImplementedError("SSD %s net: MultiBoxLoss (and AnnotatedData / DetectionEvaluate) are not built - only the DEPLOY net" % phase)


def _ssd_head(w: _Writer, feat: str, priors: int, classes: int, k: int, box: str, norm_from: Optional[str] = None) -> None:
    """One head over the blob `feat`: <feat>_mbox_loc / _mbox_conf (k x k convolutions with 4 / `classes` outputs per prior), each
    through Permute(0, 2, 3, 1) and Flatten, and <feat>_mbox_priorbox over (feat, data) with the prior_box_param `box`."""
    for kind, per in (("loc", 4), ("conf", classes)):
        nm = "%s_mbox_%s" % (feat, kind)
        _dl_conv(w, nm, feat, priors * per, k, pad=k // 2)
        w.layer(nm + "_perm", "Permute", [nm], [nm + "_perm"], "  permute_param { order: 0 order: 2 order: 3 order: 1 }")
        w.layer(nm + "_flat", "Flatten", [nm + "_perm"], [nm + "_flat"], "  flatten_param { axis: 1 }")
    w.layer(feat + "_mbox_priorbox", "PriorBox", [norm_from or feat, "data"], [feat + "_mbox_priorbox"], "  prior_box_param {\n%s\n  }" % box)


def _ssd_tail(w: _Writer, feats: Sequence[str], classes: int, conf_thr: float, top_k: int, keep_top_k: int) -> None:
    """mbox_loc / mbox_conf / mbox_priorbox (the Concats), mbox_conf_reshape -> mbox_conf_softmax -> mbox_conf_flatten, detection_out."""
    for kind, axis in (("loc", 1), ("conf", 1)):
        w.layer("mbox_" + kind, "Concat", ["%s_mbox_%s_flat" % (f, kind) for f in feats], ["mbox_" + kind], "  concat_param { axis: %d }" % axis)
    w.layer("mbox_priorbox", "Concat", [f + "_mbox_priorbox" for f in feats], ["mbox_priorbox"], "  concat_param { axis: 2 }")
    w.layer("mbox_conf_reshape", "Reshape", ["mbox_conf"], ["mbox_conf_reshape"],
            "  reshape_param { shape { dim: 0 dim: -1 dim: %d } }" % classes)
    w.layer("mbox_conf_softmax", "Softmax", ["mbox_conf_reshape"], ["mbox_conf_softmax"], "  softmax_param { axis: 2 }")
    w.layer("mbox_conf_flatten", "Flatten", ["mbox_conf_softmax"], ["mbox_conf_flatten"], "  flatten_param { axis: 1 }")
    w.layer("detection_out", "DetectionOutput", ["mbox_loc", "mbox_conf_flatten", "mbox_priorbox"], ["detection_out"],
            "  include { phase: TEST }\n  detection_output_param {\n    num_classes: %d\n    share_location: true\n    background_label_id: 0\n"
            "    nms_param { nms_threshold: 0.45 top_k: %d }\n    code_type: CENTER_SIZE\n    keep_top_k: %d\n    confidence_threshold: %g\n  }"
            % (classes, top_k, keep_top_k, conf_thr))


def _ssd_box(sizes: Tuple[float, Optional[float]], ratios: Sequence[float], scale: float, step: Optional[int] = None) -> str:
    s = ["    min_size: %g" % (sizes[0] * scale)] + (["    max_size: %g" % (sizes[1] * scale)] if sizes[1] is not None else [])
    s += ["    aspect_ratio: %g" % r for r in ratios]
    s += ["    flip: true", "    clip: false"] + ["    variance: %g" % v for v in (0.1, 0.1, 0.2, 0.2)]
    if step is not None:
        s.append("    step: %d" % step)
    return "\n".join(s + ["    offset: 0.5"])


MOBILENET_SSD_BODY = ((1, 64, 1), (2, 128, 2), (3, 128, 1), (4, 256, 2), (5, 256, 1), (6, 512, 2), (7, 512, 1), (8, 512, 1), (9, 512, 1),
                      (10, 512, 1), (11, 512, 1), (12, 1024, 2), (13, 1024, 1))      # (n of conv<n>/dw + conv<n>, width, stride of the 3x3)
MOBILENET_SSD_EXTRAS = ((14, 256, 512), (15, 128, 256), (16, 128, 256), (17, 64, 128))      # conv<n>_1 1x1, conv<n>_2 3x3 / 2
MOBILENET_SSD_BOXES = (("conv11", (60.0, None), (2.0,)), ("conv13", (105.0, 150.0), (2.0, 3.0)), ("conv14_2", (150.0, 195.0), (2.0, 3.0)),
                       ("conv15_2", (195.0, 240.0), (2.0, 3.0)), ("conv16_2", (240.0, 285.0), (2.0, 3.0)), ("conv17_2", (285.0, 300.0), (2.0, 3.0)))


def mobilenet_ssd(phase: str = "DEPLOY", classes: int = 21, size: int = 300, width_div: int = 1, batch: int = 1, fillers: bool = True) -> str:
    """MobileNet-SSD, the common Caffe port, as remembered: the MobileNet v1 body conv0, conv1/dw, conv1 .. conv13/dw, conv13 (every
    convolution bias-free with BatchNorm, Scale and ReLU, as models.mobilenet_v1 writes them - the published deploy file has them merged
    into biased convolutions), the extras conv14_1 (1x1) / conv14_2 (3x3 / 2) .. conv17_2, and six heads: conv11 with 3 priors per cell
    (min_size 60, aspect ratio 2), conv13 and conv14_2 .. conv17_2 with 6 (min / max 105 / 150 .. 285 / 300, ratios 2 and 3) - 1917 priors
    at 300 x 300.  Heads are 1x1 convolutions; offset 0.5, variances .1 .1 .2 .2, CENTER_SIZE, confidence_threshold 0.25, nms_threshold
    0.45, top_k 100, keep_top_k 100.  width_div divides the body's and the extras' widths, size is the image edge (the box sizes scale
    with it).  TRAIN and TEST are refused: MultiBoxLoss is not built."""
    _ssd_refuse_training(phase)
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "MobileNet-SSD"')
    _inputs(w, phase, batch, ["data"], size, None)
    x, c = _mb_conv(w, "conv0", "data", wd(32), 3, 2, phase, "conv0/relu"), wd(32)
    for n, width, stride in MOBILENET_SSD_BODY:
        x = _mb_conv(w, "conv%d/dw" % n, x, c, 3, stride, phase, "conv%d/dw/relu" % n, group=c)
        x, c = _mb_conv(w, "conv%d" % n, x, wd(width), 1, 1, phase, "conv%d/relu" % n), wd(width)
    for n, mid, out in MOBILENET_SSD_EXTRAS:
        x = _mb_conv(w, "conv%d_1" % n, x, wd(mid), 1, 1, phase, "conv%d_1/relu" % n)
        x = _mb_conv(w, "conv%d_2" % n, x, wd(out), 3, 2, phase, "conv%d_2/relu" % n)
    for feat, sizes, ratios in MOBILENET_SSD_BOXES:
        _ssd_head(w, feat, (1 + 2 * len(ratios)) + (1 if sizes[1] is not None else 0), classes, 1, _ssd_box(sizes, ratios, size / 300.0))
    _ssd_tail(w, [f for f, _s, _r in MOBILENET_SSD_BOXES], classes, 0.25, 100, 100)
    return w.text() if fillers else _strip_fillers(w.text())


SSD300_BOXES = (("conv4_3_norm", (30.0, 60.0), (2.0,), 8), ("fc7", (60.0, 111.0), (2.0, 3.0), 16), ("conv6_2", (111.0, 162.0), (2.0, 3.0), 32),
                ("conv7_2", (162.0, 213.0), (2.0, 3.0), 64), ("conv8_2", (213.0, 264.0), (2.0,), 100), ("conv9_2", (264.0, 315.0), (2.0,), 300))


def ssd300_vgg(phase: str = "DEPLOY", classes: int = 21, size: int = 300, width_div: int = 1, batch: int = 1, heads: int = 6,
               fillers: bool = True) -> str:
    """SSD300 on VGG16, as remembered: conv1_1 .. conv5_3 with 2x2 / 2 poolings (Caffe's ceil mode: 300 -> 150 -> 75 -> 38 -> 19), pool5
    3x3 / 1 / pad 1, fc6 as a 3x3 convolution with dilation 6 (pad 6) and fc7 1x1 (1024 each), the extras conv6_1 (1x1, 256) / conv6_2
    (3x3 / 2, 512), conv7_1 / conv7_2 (128 / 256, / 2), conv8_1 / conv8_2 and conv9_1 / conv9_2 (128 / 256, 3x3 without pad), and six heads
    of 3x3 convolutions: conv4_3_norm - Normalize(across_spatial: false, channel_shared: false, scale_filler 20) of conv4_3 - with 4 priors
    per cell, fc7, conv6_2 and conv7_2 with 6, conv8_2 and conv9_2 with 4: 8732 priors at 300 x 300.  confidence_threshold 0.01,
    nms_threshold 0.45, top_k 400, keep_top_k 200.  width_div divides every width, size is the image edge (box sizes scale with it; the
    published `step` values are written at 300 only), heads keeps the first `heads` heads and drops the layers behind the last one (a small
    test net).  TRAIN and TEST are refused: MultiBoxLoss is not built."""
    _ssd_refuse_training(phase)
    if not 1 <= heads <= len(SSD300_BOXES):
        raise ValueError("ssd300_vgg: heads must be 1 .. %d" % len(SSD300_BOXES))
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "VGG_VOC0712_SSD_300x300_deploy"')
    _inputs(w, phase, batch, ["data"], size, None)
    boxes = SSD300_BOXES[:heads]
    last = boxes[-1][0]
    prev = "data"

    def body() -> None:
        nonlocal prev
        for blk, convs, width_ in VGG16:
            for i in range(1, convs + 1):
                prev = _dl_conv(w, "conv%d_%d" % (blk, i), prev, wd(width_), 3, 1, relu="relu%d_%d" % (blk, i))
                if (blk, i) == (4, 3):
                    w.layer("conv4_3_norm", "Normalize", ["conv4_3"], ["conv4_3_norm"], "  norm_param {\n    across_spatial: false\n"
                            "    scale_filler { type: \"constant\" value: 20 }\n    channel_shared: false\n  }")
                    if last == "conv4_3_norm":
                        return
            if blk < 5:
                w.layer("pool%d" % blk, "Pooling", [prev], ["pool%d" % blk], "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }")
            else:
                w.layer("pool5", "Pooling", [prev], ["pool5"], "  pooling_param { pool: MAX kernel_size: 3 stride: 1 pad: 1 }")
            prev = "pool%d" % blk
        prev = _dl_conv(w, "fc6", prev, wd(1024), 3, 6, 6, relu="relu6")
        prev = _dl_conv(w, "fc7", prev, wd(1024), 1, relu="relu7")
        for n, mid, out, stride, pad in ((6, 256, 512, 2, 1), (7, 128, 256, 2, 1), (8, 128, 256, 1, 0), (9, 128, 256, 1, 0)):
            if last == prev:
                return
            prev = _dl_conv(w, "conv%d_1" % n, prev, wd(mid), 1, relu="conv%d_1_relu" % n)
            nm = "conv%d_2" % n
            w.layer(nm, "Convolution", [prev], [nm], "  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }\n"
                    "  convolution_param {\n    num_output: %d\n    pad: %d\n    kernel_size: 3\n    stride: %d\n    weight_filler { type: \"xavier\" }\n"
                    "    bias_filler { type: \"constant\" value: 0 }\n  }" % (wd(out), pad, stride))
            w.layer(nm + "_relu", "ReLU", [nm], [nm])
            prev = nm

    body()
    for feat, sizes, ratios, step in boxes:
        _ssd_head(w, feat, (1 + 2 * len(ratios)) + 1, classes, 3, _ssd_box(sizes, ratios, size / 300.0, step if size == 300 else None))
    _ssd_tail(w, [f for f, _s, _r, _st in boxes], classes, 0.01, 400, 200)
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# R-FCN (Dai, Li, He, Sun: "R-FCN: Object Detection via Region-based Fully Convolutional Networks") on ResNet-50 / 101: the deploy net of
# the py-R-FCN release (class-agnostic boxes), layer and blob names as remembered
# ----------------------------------------------------------------------

def rfcn_resnet(phase: str = "DEPLOY", depth: int = 50, classes: int = 21, size=(600, 1000), width_div: int = 1, batch: int = 1,
                pre_nms_topn: int = 6000, post_nms_topn: int = 300, scales: Sequence[float] = (8, 16, 32), fillers: bool = True) -> str:
    """The R-FCN deploy net on the ResNet body of models.resnet (published names: conv1 .. res4f / res4b22 at stride 16, res5a .. res5c
    at stride 1 with dilation 2 in their 3x3 convolutions).  RPN over the last res4 block: rpn_conv/3x3 (512) with rpn_relu/3x3,
    rpn_cls_score (2 x 9) and rpn_bbox_pred (4 x 9), the softmax chain rpn_cls_score_reshape -> rpn_cls_prob -> rpn_cls_prob_reshape, and
    `proposal` over (rpn_cls_prob_reshape, rpn_bbox_pred, im_info) with the top rois.  Region stage over res5c: conv_new_1 (1x1, 1024) with
    conv_new_1_relu, rfcn_cls (classes x 49) and rfcn_bbox (8 x 49), psroipooled_cls_rois / psroipooled_loc_rois (PSROIPooling,
    spatial_scale 0.0625, group_size 7), ave_cls_score_rois -> cls_score and ave_bbox_pred_rois -> bbox_pred (AVE 7 x 7), cls_prob.
    Inputs: data (batch, 3, h, w) and im_info (1, 3).  `size` is the image edge or (height, width).

    With the default pre / post_nms_topn and scales the proposal layer is written as the published files write it, a Python layer naming
    rpn.proposal_layer.ProposalLayer with param_str "'feat_stride': 16"; with others as `type: "Proposal"` with a proposal_param.  This
    project's own: the published files end in cls_prob_reshape / bbox_pred_reshape, two Reshape layers from (R, C, 1, 1) to (R, C) that
    are left out here - cls_prob and bbox_pred are (R, classes, 1, 1) and (R, 8, 1, 1); width_div, scales and the two topn arguments
    (small test nets).  DEPLOY only: TRAIN and TEST need AnchorTarget / ProposalTarget and a backward pass through the poolings, which
    are not built."""
    _check_phase(phase)
    if phase != "DEPLOY":
        raise NotImplementedError("R-FCN %s net: AnchorTarget / ProposalTarget and the backward pass of PSROIPooling are not built - only "
                                  "the DEPLOY net" % phase)
    if depth not in (50, 101):
        raise ValueError("rfcn_resnet: depth must be 50 or 101")
    if batch != 1:
        raise NotImplementedError("rfcn_resnet: batch %d (the Proposal layer takes one image a forward)" % batch)
    h, wdt = _hw(size)
    wd = lambda c: max(c // width_div, 1)
    w = _Writer()
    w.raw('name: "ResNet-%d-RFCN"' % depth)
    w.layer("data", "Input", [], ["data"], "  input_param { shape { dim: %d dim: 3 dim: %d dim: %d } }" % (batch, h, wdt))
    w.layer("im_info", "Input", [], ["im_info"], "  input_param { shape { dim: 1 dim: 3 } }")
    _rn_conv_bn(w, "", "data", wd(64), 7, 3, 2, phase, True, conv_name="conv1", bias=True)
    w.layer("pool1", "Pooling", ["conv1"], ["pool1"], "  pooling_param { pool: MAX kernel_size: 3 stride: 2 }")
    feat, res4 = "pool1", ""
    for stage, count in zip((2, 3, 4, 5), RESNET_BLOCKS[depth]):
        mid, out = wd(64 << (stage - 2)), wd(256 << (stage - 2))
        dil = 2 if stage == 5 else 1
        for bi, letter in enumerate(_resnet_block_names(count, depth > 50 and stage in (3, 4))):
            tag = "%d%s" % (stage, letter)
            stride = 2 if bi == 0 and stage in (3, 4) else 1
            short = feat if bi else _rn_conv_bn(w, tag + "_branch1", feat, out, 1, 0, stride, phase, False)
            x = _rn_conv_bn(w, tag + "_branch2a", feat, mid, 1, 0, stride, phase, True)
            x = _rn_conv_bn(w, tag + "_branch2b", x, mid, 3, dil, 1, phase, True, dilation=dil)
            x = _rn_conv_bn(w, tag + "_branch2c", x, out, 1, 0, 1, phase, False)
            feat = "res" + tag
            w.layer(feat, "Eltwise", [short, x], [feat])
            w.layer(feat + "_relu", "ReLU", [feat], [feat])
        if stage == 4:
            res4 = feat
    a = 3 * len(scales)
    _dl_conv(w, "rpn_conv/3x3", res4, wd(512), 3, 1, relu="rpn_relu/3x3", std=0.01)
    _dl_conv(w, "rpn_cls_score", "rpn_conv/3x3", 2 * a, 1, std=0.01)
    _dl_conv(w, "rpn_bbox_pred", "rpn_conv/3x3", 4 * a, 1, std=0.01)
    w.layer("rpn_cls_score_reshape", "Reshape", ["rpn_cls_score"], ["rpn_cls_score_reshape"], "  reshape_param { shape { dim: 0 dim: 2 dim: -1 dim: 0 } }")
    w.layer("rpn_cls_prob", "Softmax", ["rpn_cls_score_reshape"], ["rpn_cls_prob"])
    w.layer("rpn_cls_prob_reshape", "Reshape", ["rpn_cls_prob"], ["rpn_cls_prob_reshape"],
            "  reshape_param { shape { dim: 0 dim: %d dim: -1 dim: 0 } }" % (2 * a))
    bottoms = ["rpn_cls_prob_reshape", "rpn_bbox_pred", "im_info"]
    if (pre_nms_topn, post_nms_topn, tuple(float(v) for v in scales)) == (6000, 300, (8.0, 16.0, 32.0)):
        w.layer("proposal", "Python", bottoms, ["rois"], "  python_param {\n    module: 'rpn.proposal_layer'\n    layer: 'ProposalLayer'\n"
                "    param_str: \"'feat_stride': 16\"\n  }")
    else:
        w.layer("proposal", "Proposal", bottoms, ["rois"], "  proposal_param {\n    feat_stride: 16\n%s\n    pre_nms_topn: %d\n    post_nms_topn: %d\n  }"
                % ("\n".join("    scale: %g" % v for v in scales), pre_nms_topn, post_nms_topn))
    _dl_conv(w, "conv_new_1", feat, wd(1024), 1, relu="conv_new_1_relu", std=0.01)
    for name, dim, pooled, ave, top in (("rfcn_cls", classes, "psroipooled_cls_rois", "ave_cls_score_rois", "cls_score"),
                                        ("rfcn_bbox", 8, "psroipooled_loc_rois", "ave_bbox_pred_rois", "bbox_pred")):
        _dl_conv(w, name, "conv_new_1", dim * 49, 1, std=0.01)
        w.layer(pooled, "PSROIPooling", [name, "rois"], [pooled], "  psroi_pooling_param {\n    spatial_scale: 0.0625\n    output_dim: %d\n"
                "    group_size: 7\n  }" % dim)
        w.layer(ave, "Pooling", [pooled], [top], "  pooling_param { pool: AVE kernel_size: 7 stride: 7 }")
    w.layer("cls_prob", "Softmax", ["cls_score"], ["cls_prob"])
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# Faster R-CNN (Ren, He, Girshick, Sun: "Faster R-CNN: Towards Real-Time Object Detection with Region Proposal Networks") on VGG16: the
# test net of the py-faster-rcnn release, layer and blob names as remembered
# ----------------------------------------------------------------------

def faster_rcnn_vgg16(phase: str = "DEPLOY", classes: int = 21, size=(600, 1000), width_div: int = 1, fc_div: int = 1, batch: int = 1,
                      post_nms_topn: int = 300, pre_nms_topn: int = 6000, fillers: bool = True) -> str:
    """The Faster R-CNN test net on VGG16 (published names): conv1_1 .. conv5_3 with relu<b>_<i> and the 2x2 / 2 poolings pool1 .. pool4
    (no pool5: conv5_3 is the stride-16 feature map).  RPN over conv5_3: rpn_conv/3x3 (512) with rpn_relu/3x3, rpn_cls_score (2 x 9) and
    rpn_bbox_pred (4 x 9), the softmax chain rpn_cls_score_reshape -> rpn_cls_prob -> rpn_cls_prob_reshape, and `proposal` over
    (rpn_cls_prob_reshape, rpn_bbox_pred, im_info) with the top rois.  Region stage: roi_pool5 (ROIPooling 7 x 7, spatial_scale 0.0625)
    over (conv5_3, rois), fc6 and fc7 (4096, relu6 / drop6, relu7 / drop7), cls_score (classes) and bbox_pred (4 x classes) over fc7,
    cls_prob.  Inputs: data (batch, 3, h, w) and im_info (1, 3).  `size` is the image edge or (height, width).

    fc6 runs over all post_nms_topn rows of roi_pool5 - 300 in the published net, far above the 32 rows of the weight-streaming
    InnerProduct kernels: the net needs a NetSpec built with ip_gemm=True (caffe.Net and the caffe tool pass it).

    With the default pre / post_nms_topn the proposal layer is written as the published file writes it, a Python layer naming
    rpn.proposal_layer.ProposalLayer with param_str "'feat_stride': 16"; with others as `type: "Proposal"` with a proposal_param.  This
    project's own: width_div (the body's and the RPN's widths), fc_div (the 4096 of fc6 / fc7), the two topn arguments (small test nets),
    and the lr_mult 1 / 2 param blocks on every learnable layer (the published test file has none).  DEPLOY only: TRAIN and TEST need
    AnchorTarget / ProposalTarget, SmoothL1Loss and a backward pass through ROIPooling, which are not built."""
    _check_phase(phase)
    if phase != "DEPLOY":
        raise NotImplementedError("Faster R-CNN %s net: AnchorTarget / ProposalTarget, SmoothL1Loss and the backward pass of ROIPooling are "
                                  "not built - only the DEPLOY net" % phase)
    if batch != 1:
        raise NotImplementedError("faster_rcnn_vgg16: batch %d (the Proposal layer takes one image a forward)" % batch)
    h, wdt = _hw(size)
    wd = lambda c: max(c // width_div, 1)
    fc = max(4096 // fc_div, 1)
    w = _Writer()
    w.raw('name: "VGG_ILSVRC_16_layers"')
    w.layer("data", "Input", [], ["data"], "  input_param { shape { dim: %d dim: 3 dim: %d dim: %d } }" % (batch, h, wdt))
    w.layer("im_info", "Input", [], ["im_info"], "  input_param { shape { dim: 1 dim: 3 } }")
    prev = "data"
    for blk, convs, width_ in VGG16:
        for i in range(1, convs + 1):
            prev = _dl_conv(w, "conv%d_%d" % (blk, i), prev, wd(width_), 3, 1, relu="relu%d_%d" % (blk, i))
        if blk < 5:
            w.layer("pool%d" % blk, "Pooling", [prev], ["pool%d" % blk], "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }")
            prev = "pool%d" % blk
    _dl_conv(w, "rpn_conv/3x3", "conv5_3", wd(512), 3, 1, relu="rpn_relu/3x3", std=0.01)
    _dl_conv(w, "rpn_cls_score", "rpn_conv/3x3", 18, 1, std=0.01)
    _dl_conv(w, "rpn_bbox_pred", "rpn_conv/3x3", 36, 1, std=0.01)
    w.layer("rpn_cls_score_reshape", "Reshape", ["rpn_cls_score"], ["rpn_cls_score_reshape"], "  reshape_param { shape { dim: 0 dim: 2 dim: -1 dim: 0 } }")
    w.layer("rpn_cls_prob", "Softmax", ["rpn_cls_score_reshape"], ["rpn_cls_prob"])
    w.layer("rpn_cls_prob_reshape", "Reshape", ["rpn_cls_prob"], ["rpn_cls_prob_reshape"], "  reshape_param { shape { dim: 0 dim: 18 dim: -1 dim: 0 } }")
    bottoms = ["rpn_cls_prob_reshape", "rpn_bbox_pred", "im_info"]
    if (pre_nms_topn, post_nms_topn) == (6000, 300):
        w.layer("proposal", "Python", bottoms, ["rois"], "  python_param {\n    module: 'rpn.proposal_layer'\n    layer: 'ProposalLayer'\n"
                "    param_str: \"'feat_stride': 16\"\n  }")
    else:
        w.layer("proposal", "Proposal", bottoms, ["rois"], "  proposal_param {\n    feat_stride: 16\n    pre_nms_topn: %d\n    post_nms_topn: %d\n  }"
                % (pre_nms_topn, post_nms_topn))
    w.layer("roi_pool5", "ROIPooling", ["conv5_3", "rois"], ["roi_pool5"], "  roi_pooling_param {\n    pooled_w: 7\n    pooled_h: 7\n"
            "    spatial_scale: 0.0625\n  }")
    _cn_fc(w, "fc6", "roi_pool5", fc, 0.005, 0.1, "relu6", "drop6")
    _cn_fc(w, "fc7", "fc6", fc, 0.005, 0.1, "relu7", "drop7")
    _cn_fc(w, "cls_score", "fc7", classes, 0.01, 0.0)
    _cn_fc(w, "bbox_pred", "fc7", 4 * classes, 0.001, 0.0)
    w.layer("cls_prob", "Softmax", ["cls_score"], ["cls_prob"])
    return w.text() if fillers else _strip_fillers(w.text())


# ----------------------------------------------------------------------
# MTCNN (Zhang et al. 2016: P-Net / R-Net / O-Net) and ENet (Paszke et al. 2016): the two published families whose activation is PReLU.
# Both need a NetSpec built with activations=True (caffe.Net, the solvers and the caffe tool pass it).
# ----------------------------------------------------------------------

def _prelu(w: _Writer, name: str, blob: str) -> None:
    """PReLU `<name>` in place on `blob`: one slope per channel, Caffe's default filler (constant 0.25), decay_mult 0."""
    w.layer(name, "PReLU", [blob], [blob], "  param { lr_mult: 1 decay_mult: 0 }")


def _mt_conv(w: _Writer, name: str, bottom: str, num_output: int, k: int, prelu: Optional[str] = None) -> str:
    w.layer(name, "Convolution", [bottom], [name], "  param { lr_mult: 1 decay_mult: 1 }\n  param { lr_mult: 2 decay_mult: 0 }\n"
            "  convolution_param {\n    num_output: %d\n    kernel_size: %d\n    weight_filler { type: \"xavier\" }\n"
            "    bias_filler { type: \"constant\" value: 0 }\n  }" % (num_output, k))
    if prelu:
        _prelu(w, prelu, name)
    return name


def _mt_pool(w: _Writer, name: str, bottom: str, k: int) -> str:
    w.layer(name, "Pooling", [bottom], [name], "  pooling_param { pool: MAX kernel_size: %d stride: 2 }" % k)
    return name


def mtcnn_grid(net: str, size) -> Tuple[int, int]:
    """Extents of the blob in front of the heads (P-Net: of the heads' maps) for an input of `size`, pooling in Caffe's ceil mode."""
    convs = {"pnet": ((3, 2), (3, 0), (3, 0)), "rnet": ((3, 3), (3, 3), (2, 0)), "onet": ((3, 3), (3, 3), (3, 2), (2, 0))}[net]
    out = []
    for v in _hw(size):
        for k, pool in convs:
            v = v - k + 1
            if pool:
                v = -(-(v - pool) // 2) + 1
        out.append(v)
    return out[0], out[1]


def mtcnn(net: str = "pnet", phase: str = "DEPLOY", batch: int = 1, size=None) -> str:
    """The three nets of MTCNN.  P-Net (12 x 12, fully convolutional - any `size` in DEPLOY): conv1 3x3x10, PReLU1, pool1 MAX 2x2 / 2,
    conv2 3x3x16, PReLU2, conv3 3x3x32, PReLU3, the 1x1 heads conv4-1 (2, Softmax prob1) and conv4-2 (4 box offsets).  R-Net (24 x 24):
    conv1 3x3x28, pool1 3x3 / 2, conv2 3x3x48, pool2 3x3 / 2, conv3 2x2x64, InnerProduct conv4 (128), heads conv5-1 (2, prob1) and conv5-2
    (4).  O-Net (48 x 48): conv1 3x3x32, pool1 3x3 / 2, conv2 3x3x64, pool2 3x3 / 2, conv3 3x3x64, pool3 2x2 / 2, conv4 2x2x128,
    InnerProduct conv5 (256), Dropout drop5, prelu5, heads conv6-1 (2, prob1), conv6-2 (4) and conv6-3 (10 landmark coordinates).  A
    PReLU, one slope per channel, follows every convolution and the first InnerProduct, in place.

    Names: conv*, pool*, PReLU1 .. PReLU3 (P-Net), prelu1 .. prelu5 (R-Net, O-Net), drop5, conv4-1 .. conv6-3 and prob1 are the published
    deploy files', as far as remembered.  The TRAIN / TEST forms are this project's (the release has deploy files only): Input `label`
    (one class per position of the class head), `roi` (the box targets, the box head's shape) and for O-Net `pts`, SoftmaxWithLoss
    `cls_loss` on the class head and EuclideanLoss `roi_loss` (O-Net: and `pts_loss`) on the others.  `size` is the image edge or
    (height, width); R-Net and O-Net end in InnerProduct layers and take their own size only."""
    _check_phase(phase)
    if net not in ("pnet", "rnet", "onet"):
        raise ValueError("net must be 'pnet', 'rnet' or 'onet'")
    own = {"pnet": 12, "rnet": 24, "onet": 48}[net]
    hw = _hw(own if size is None else size)
    if net != "pnet" and hw != (own, own):
        raise ValueError("%s takes %d x %d images (it ends in InnerProduct layers)" % (net, own, own))
    if phase != "DEPLOY" and net == "pnet" and hw != (own, own):
        raise ValueError("pnet trains on 12 x 12 crops; another size is for the DEPLOY form")
    if min(mtcnn_grid(net, hw)) < 1:
        raise ValueError("%s needs images of at least %d x %d" % (net, own, own))
    w = _Writer()
    w.raw('name: "%s"' % {"pnet": "PNet", "rnet": "RNet", "onet": "ONet"}[net])
    w.layer("data", "Input", [], ["data"], "  input_param { shape { dim: %d dim: 3 dim: %d dim: %d } }" % (batch, hw[0], hw[1]))
    if net == "pnet":
        x = _mt_conv(w, "conv1", "data", 10, 3, "PReLU1")
        x = _mt_pool(w, "pool1", x, 2)
        x = _mt_conv(w, "conv2", x, 16, 3, "PReLU2")
        x = _mt_conv(w, "conv3", x, 32, 3, "PReLU3")
        heads = [_mt_conv(w, "conv4-1", x, 2, 1), _mt_conv(w, "conv4-2", x, 4, 1)]
    else:
        widths = (28, 48, 64) if net == "rnet" else (32, 64, 64, 128)
        x = _mt_pool(w, "pool1", _mt_conv(w, "conv1", "data", widths[0], 3, "prelu1"), 3)
        x = _mt_pool(w, "pool2", _mt_conv(w, "conv2", x, widths[1], 3, "prelu2"), 3)
        if net == "rnet":
            x = _mt_conv(w, "conv3", x, widths[2], 2, "prelu3")
            fc, act, head = "conv4", "prelu4", "conv5"
        else:
            x = _mt_pool(w, "pool3", _mt_conv(w, "conv3", x, widths[2], 3, "prelu3"), 2)
            x = _mt_conv(w, "conv4", x, widths[3], 2, "prelu4")
            fc, act, head = "conv5", "prelu5", "conv6"
        _cn_fc(w, fc, x, 128 if net == "rnet" else 256, 0.0, 0.0, filler="xavier", drop="drop5" if net == "onet" else None, ratio=0.25)
        _prelu(w, act, fc)
        heads = [head + "-%d" % (i + 1) for i in range(2 if net == "rnet" else 3)]
        for nm, n_out in zip(heads, (2, 4, 10)):
            _cn_fc(w, nm, fc, n_out, 0.0, 0.0, filler="xavier")
    if phase == "DEPLOY":
        w.layer("prob1", "Softmax", [heads[0]], ["prob1"])
        return w.text()
    gh, gw = mtcnn_grid(net, hw)
    shape = (lambda c: (batch, c, gh, gw)) if net == "pnet" else (lambda c: (batch, c))
    targets = list(zip(("label", "roi", "pts"), (1, 4, 10)))[:len(heads)]
    for nm, c in targets:
        shp = shape(c) if not (nm == "label" and net != "pnet") else (batch,)
        w.layer(nm, "Input", [], [nm], "  input_param { shape { %s } }" % " ".join("dim: %d" % d for d in shp))
    w.layer("cls_loss", "SoftmaxWithLoss", [heads[0], "label"], ["cls_loss"])
    for hd, (nm, _c_) in list(zip(heads, targets))[1:]:
        w.layer(nm + "_loss", "EuclideanLoss", [hd, nm], [nm + "_loss"], "  loss_weight: 0.5")
    return w.text()


def _en_conv(w: _Writer, name: str, bottom: str, num_output: int, kernel, phase: str, pad=0, stride: int = 1, dilation: int = 1,
             deconv: bool = False, bn: bool = True, prelu: bool = True, bias: bool = False) -> str:
    """Convolution (or, with `deconv`, Deconvolution) `<name>`, without a bias unless `bias`; with `bn` BatchNorm `<name>/bn` and Scale
    `<name>/scale` (bias_term: true), with `prelu` PReLU `<name>/prelu`, all in place on its top; returns the top."""
    kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    geo = "    num_output: %d\n" % num_output
    geo += "    kernel_size: %d\n" % kh if kh == kw else "    kernel_h: %d\n    kernel_w: %d\n" % (kh, kw)
    if ph or pw:
        geo += "    pad: %d\n" % ph if (kh, ph) == (kw, pw) else "    pad_h: %d\n    pad_w: %d\n" % (ph, pw)
    if stride != 1:
        geo += "    stride: %d\n" % stride
    if dilation != 1:
        geo += "    dilation: %d\n" % dilation
    if not bias:
        geo += "    bias_term: false\n"
    fill = "    weight_filler { type: \"gaussian\" std: %g }\n" % (2.0 / (kh * kw * num_output)) ** 0.5
    w.layer(name, "Deconvolution" if deconv else "Convolution", [bottom], [name],
            "  param { lr_mult: 1 decay_mult: 1 }\n%s  convolution_param {\n%s%s  }" % ("  param { lr_mult: 2 decay_mult: 0 }\n" if bias else "", geo, fill))
    if bn:
        stats = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3) if phase != "DEPLOY" else "  batch_norm_param { use_global_stats: true }"
        w.layer(name + "/bn", "BatchNorm", [name], [name], stats)
        w.layer(name + "/scale", "Scale", [name], [name], "  scale_param { bias_term: true }")
    if prelu:
        _prelu(w, name + "/prelu", name)
    return name


def _en_bottleneck(w: _Writer, tag: str, x: str, cin: int, cout: int, kind, phase: str, ratio: float, mask: Optional[str] = None,
                   hw: Optional[Tuple[int, int]] = None) -> str:
    """One ENet bottleneck `<tag>`: 1x1 reduce to cout / 4, at least 2 (`down`: a 2x2 / 2 convolution), the main convolution (`regular` 3x3, an int
    d: 3x3 with dilation d, `asym`: 5x1 then 1x5, `down`: 3x3, `up`: a 2x2 / 2 Deconvolution), 1x1 expand, Dropout, Eltwise SUM with the
    shortcut (`down`: MAX pooling 2x2 / 2 with the mask `<tag>/pool_mask`, then a 1x1 convolution that widens; `up`: a 1x1 convolution,
    then Upsample by `mask` to `hw`) and PReLU.  Returns the top, `<tag>`."""
    mid = max(cout // 4, 2)      # (never one channel: a Deconvolution of one channel into one reads as a depthwise one, which does not learn)
    b = _en_conv(w, tag + "/reduce", x, mid, 2 if kind == "down" else 1, phase, stride=2 if kind == "down" else 1)
    if kind == "asym":
        b = _en_conv(w, tag + "/conv_a", b, mid, (5, 1), phase, pad=(2, 0), bn=False, prelu=False)
        b = _en_conv(w, tag + "/conv", b, mid, (1, 5), phase, pad=(0, 2))
    elif kind == "up":
        b = _en_conv(w, tag + "/conv", b, mid, 2, phase, stride=2, deconv=True)
    else:
        d = kind if isinstance(kind, int) else 1
        b = _en_conv(w, tag + "/conv", b, mid, 3, phase, pad=d, dilation=d)
    b = _en_conv(w, tag + "/expand", b, cout, 1, phase, prelu=False)
    w.layer(tag + "/drop", "Dropout", [b], [b], "  dropout_param { dropout_ratio: %g }" % ratio)
    s = x
    if kind == "down":
        w.layer(tag + "/pool", "Pooling", [x], [tag + "/pool", tag + "/pool_mask"], "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }")
        s = _en_conv(w, tag + "/short", tag + "/pool", cout, 1, phase, prelu=False)
    elif kind == "up":
        s = _en_conv(w, tag + "/short", x, cout, 1, phase, prelu=False)
        s = _sn_upsample(w, tag + "/unpool", s, mask, hw)
    w.layer(tag, "Eltwise", [b, s], [tag])
    _prelu(w, tag + "/prelu", tag)
    return tag


ENET_STAGE = ("regular", 2, "asym", 4, "regular", 8, "asym", 16)      # bottlenecks x.1 .. x.8 of stages 2 and 3 (an int: the dilation)


def enet(phase: str = "DEPLOY", classes: int = 19, batch: int = 1, size=(512, 1024), width_div: int = 1, argmax: bool = False) -> str:
    """ENet in the layers this project has.  `initial`: a 3x3 / 2 convolution to 13 channels beside a 2x2 / 2 MAX pooling of the image,
    Concat to 16, BatchNorm + Scale + PReLU.  Stage 1: a downsampling bottleneck and four regular ones (64 channels); stage 2: a
    downsampling one and regular, dilated 2, asymmetric 5, dilated 4, regular, dilated 8, asymmetric 5, dilated 16 (128); stage 3: those
    eight again; stage 4: an upsampling bottleneck and two regular ones (64); stage 5: an upsampling one and a regular one (16);
    `fullconv`, a 2x2 / 2 Deconvolution to `classes`.  Every convolution of a bottleneck carries BatchNorm + Scale, the first two a PReLU
    as well; a plain Dropout (0.01 in stage 1, 0.1 after it) closes the branch; a PReLU follows the sum.

    Where the paper pads the pooled shortcut of a downsampling bottleneck with zero channels, a 1x1 convolution + BatchNorm + Scale widens it
    here (Caffe has no zero-padding layer); the paper's SpatialDropout is a plain Dropout; the decoder's shortcuts are a 1x1 convolution +
    BatchNorm + Scale, then an Upsample by the mask of the matching downsampling bottleneck.  ALL layer and blob names are this project's:
    `initial`, `b<stage>_<index>` with `/reduce`, `/conv` (`/conv_a` for the 5x1 half), `/expand`, `/drop`, `/short`, `/pool`,
    `/pool_mask`, `/unpool` and `<conv>/bn`, `/scale`, `/prelu`.  Ends as models.segnet: prob (DEPLOY, with argmax=True the label map
    `argmax` behind it), or loss (SoftmaxWithLoss, ignore_label 255) with accuracy in TEST.  width_div divides the widths; size is the
    image edge or (height, width), multiples of 8."""
    _check_phase(phase)
    hw = _hw(size)
    if hw[0] % 8 or hw[1] % 8:
        raise ValueError("enet takes images whose extents are multiples of 8, got %d x %d" % hw)
    c16, c64, c128 = max(16 // width_div, 4), max(64 // width_div, 4), max(128 // width_div, 4)
    w = _Writer()
    w.raw('name: "ENet"')
    _sn_inputs(w, phase, batch, hw)
    _en_conv(w, "initial/conv", "data", c16 - 3, 3, phase, pad=1, stride=2, bn=False, prelu=False, bias=True)
    w.layer("initial/pool", "Pooling", ["data"], ["initial/pool"], "  pooling_param { pool: MAX kernel_size: 2 stride: 2 }")
    w.layer("initial", "Concat", ["initial/conv", "initial/pool"], ["initial"])
    stats = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3) if phase != "DEPLOY" else "  batch_norm_param { use_global_stats: true }"
    w.layer("initial/bn", "BatchNorm", ["initial"], ["initial"], stats)
    w.layer("initial/scale", "Scale", ["initial"], ["initial"], "  scale_param { bias_term: true }")
    _prelu(w, "initial/prelu", "initial")
    h2, h4 = (hw[0] // 2, hw[1] // 2), (hw[0] // 4, hw[1] // 4)
    x = _en_bottleneck(w, "b1_0", "initial", c16, c64, "down", phase, 0.01)
    for i in range(1, 5):
        x = _en_bottleneck(w, "b1_%d" % i, x, c64, c64, "regular", phase, 0.01)
    x = _en_bottleneck(w, "b2_0", x, c64, c128, "down", phase, 0.1)
    for stage in (2, 3):
        for i, kind in enumerate(ENET_STAGE):
            x = _en_bottleneck(w, "b%d_%d" % (stage, i + 1), x, c128, c128, kind, phase, 0.1)
    x = _en_bottleneck(w, "b4_0", x, c128, c64, "up", phase, 0.1, "b2_0/pool_mask", h4)
    for i in (1, 2):
        x = _en_bottleneck(w, "b4_%d" % i, x, c64, c64, "regular", phase, 0.1)
    x = _en_bottleneck(w, "b5_0", x, c64, c16, "up", phase, 0.1, "b1_0/pool_mask", h2)
    x = _en_bottleneck(w, "b5_1", x, c16, c16, "regular", phase, 0.1)
    x = _en_conv(w, "fullconv", x, classes, 2, phase, stride=2, deconv=True, bn=False, prelu=False, bias=True)
    _sn_tail(w, phase, x, argmax)
    return w.text()
