"""Shape inference and refusals of the SSD head's layers: Permute, Flatten, Reshape, Concat(axis 2), PriorBox, Normalize,
DetectionOutput (no GPU).  What the device takes of them is storage.plan_blobs' decision and is tested through it."""
import numpy as np
import pytest

import ref_ssd64 as R
from fcn_object_detector_amd import models, proto, ssd, storage
from fcn_object_detector_amd.netspec import NetSpec, fill_params

HEAD = 'input: "data" input_shape { dim: 2 dim: 3 dim: 32 dim: 48 }\ninput: "feat" input_shape { dim: 2 dim: 12 dim: 4 dim: 6 }\n'


def infer(text, phase="TEST"):
    spec = NetSpec(proto.parse_text(HEAD + text), phase)
    return spec, spec.infer()


def plan(text, f16=False):
    spec, shapes = infer(text)
    return storage.plan_blobs(spec, shapes, spec.data_tops(), [b for b in spec.output_blobs() if b in shapes], f16, True, True)


def layer(name, type_, bottoms, body="", top=None):
    return 'layer { name: "%s" type: "%s" %s top: "%s" %s }\n' % (name, type_, " ".join('bottom: "%s"' % b for b in bottoms), top or name, body)


PERM = layer("perm", "Permute", ["feat"], "permute_param { order: 0 order: 2 order: 3 order: 1 }")


def test_permute_shapes_and_what_the_device_takes():
    assert infer(PERM)[1]["perm"] == (2, 4, 6, 12)
    assert infer(layer("p", "Permute", ["feat"], "permute_param { order: 0 order: 3 }"))[1]["p"] == (2, 6, 12, 4)      # missing axes appended in order
    assert infer(layer("p", "Permute", ["feat"], "permute_param { order: 1 order: 0 order: 3 order: 2 }"))[1]["p"] == (12, 2, 6, 4)
    with pytest.raises(ValueError, match="layer p: Permute order"):
        infer(layer("p", "Permute", ["feat"], "permute_param { order: 0 order: 0 }"))
    with pytest.raises(NotImplementedError, match="layer p: Permute of a 4-d blob to order"):
        plan(layer("p", "Permute", ["feat"], "permute_param { order: 0 order: 3 order: 1 order: 2 }") + layer("f", "Flatten", ["p"]))
    with pytest.raises(NotImplementedError, match="layer perm: the Permute top perm is an output"):
        plan(PERM)
    with pytest.raises(NotImplementedError, match="layer perm: the Permute top perm feeds"):
        plan(PERM + layer("r", "ReLU", ["perm"]))


def test_flatten_forms():
    assert infer(PERM + layer("flat", "Flatten", ["perm"], "flatten_param { axis: 1 }"))[1]["flat"] == (2, 288)
    p = plan(PERM + layer("flat", "Flatten", ["perm"]))
    assert p.gathers == {"flat": ("flat", [("flat", "feat", 0)])} and p.permutes == {"perm": "feat"} and "perm" not in p.views
    assert p.views["flat"].root == "flat" and p.views["flat"].cstride == 288
    # (c) a 4-d blob with H = W = 1 is a view
    text = layer("gp", "Pooling", ["feat"], "pooling_param { pool: AVE global_pooling: true }") + layer("flat", "Flatten", ["gp"])
    assert infer(text)[1]["flat"] == (2, 12) and plan(text).alias["flat"] == ("gp", 0)
    with pytest.raises(NotImplementedError, match="layer flat: Flatten of the .* blob feat"):
        plan(layer("flat", "Flatten", ["feat"]))
    with pytest.raises(NotImplementedError, match="layer flat: Flatten of axes 2..3"):
        infer(layer("flat", "Flatten", ["feat"], "flatten_param { axis: 2 }"))
    with pytest.raises(NotImplementedError, match="layer flat: Flatten of axes 1..2"):
        infer(layer("flat", "Flatten", ["feat"], "flatten_param { end_axis: 2 }"))


RESHAPE = PERM + layer("flat", "Flatten", ["perm"]) + layer("rs", "Reshape", ["flat"], "reshape_param { shape { dim: 0 dim: -1 dim: 3 } }")


def test_reshape_softmax_and_flatten_back_are_views():
    text = RESHAPE + layer("sm", "Softmax", ["rs"], "softmax_param { axis: 2 }") + layer("back", "Flatten", ["sm"])
    shapes = infer(text)[1]
    assert (shapes["rs"], shapes["sm"], shapes["back"]) == ((2, 96, 3), (2, 96, 3), (2, 288))
    p = plan(text)
    assert p.alias["rs"] == ("flat", 0) and p.alias["back"] == ("sm", 0) and {"rs", "sm"} <= p.rows
    assert p.views["rs"].nchw == (2, 288, 1, 1) and p.views["sm"].cstride == p.views["flat"].cstride == 288      # one row stride for all of them
    assert infer(RESHAPE.replace("dim: 0 dim: -1 dim: 3", "dim: 2 dim: 32 dim: 9"))[1]["rs"] == (2, 32, 9)
    for dims, err, what in (("dim: 0 dim: -1 dim: 7", ValueError, "the -1 has no whole value"), ("dim: 0 dim: -1 dim: -1", ValueError, "at most one -1"),
                            ("dim: 2 dim: 5 dim: 5", ValueError, r"Reshape of \(2, 288\)")):
        with pytest.raises(err, match="layer rs: .*" + what):
            infer(RESHAPE.replace("dim: 0 dim: -1 dim: 3", dims))
    with pytest.raises(NotImplementedError, match="layer rs: Reshape with axis 1"):
        infer(RESHAPE.replace("reshape_param {", "reshape_param { axis: 1"))
    with pytest.raises(NotImplementedError, match=r"layer rs: Reshape of \(2, 288\) to \(2, 4, 6, 12\)"):
        plan(RESHAPE.replace("dim: 0 dim: -1 dim: 3", "dim: 0 dim: 4 dim: 6 dim: 12"))
    with pytest.raises(NotImplementedError, match=r"layer rs: Reshape of \(2, 288\) to \(4, 48, 3\)"):
        plan(RESHAPE.replace("dim: 0 dim: -1 dim: 3", "dim: 4 dim: -1 dim: 3"))


BOX = "prior_box_param { min_size: 8 max_size: 16 aspect_ratio: 2 aspect_ratio: 3 variance: 0.1 variance: 0.1 variance: 0.2 variance: 0.2 %s }"


def test_priorbox_and_its_concat():
    a = layer("pa", "PriorBox", ["feat", "data"], BOX % "")
    b = layer("pb", "PriorBox", ["feat", "data"], "prior_box_param { min_size: 4 aspect_ratio: 2 flip: false clip: true step: 8 offset: 0.25 }")
    spec, shapes = infer(a + b + layer("pri", "Concat", ["pa", "pb"], "concat_param { axis: 2 }"))
    assert shapes["pa"] == (1, 2, 4 * 6 * 6 * 4) and shapes["pb"] == (1, 2, 4 * 6 * 2 * 4) and shapes["pri"] == (1, 2, 768)
    assert set(spec.prior_blobs) == {"pa", "pb", "pri"}
    pa = ssd.priorbox_params(spec.layers[0])
    assert pa.per_cell == 6 and pa.ratios[:2] == (1.0, 2.0) and len(pa.ratios) == 5 and pa.variance == (0.1, 0.1, 0.2, 0.2)
    got = ssd.prior_boxes(pa, 4, 6, 32, 48)
    want = R.prior_box(4, 6, 32, 48, [8.0], [16.0], [2.0, 3.0], variance=(0.1, 0.1, 0.2, 0.2))
    assert got.dtype == np.float32 and got.shape == want.shape and np.max(np.abs(got - want)) < 1e-6
    pb = ssd.priorbox_params(spec.layers[1])
    got = ssd.prior_boxes(pb, 4, 6, 32, 48)
    want = R.prior_box(4, 6, 32, 48, [4.0], aspect_ratios=[2.0], flip=False, clip=True, variance=(0.1,), step=8, offset=0.25)
    assert pb.per_cell == 2 and np.max(np.abs(got - want)) < 1e-6 and got.min() >= 0.0
    # img_h / img_w and step_h / step_w
    pc = ssd.priorbox_params(proto_layer(layer("pc", "PriorBox", ["feat", "data"], "prior_box_param { min_size: 4 img_h: 64 img_w: 96 step_h: 16 step_w: 12 }")))
    assert np.max(np.abs(ssd.prior_boxes(pc, 4, 6, 32, 48) - R.prior_box(4, 6, 64, 96, [4.0], step=(16.0, 12.0)))) < 1e-6
    for body, pattern in (("min_size: 8 min_size: 9 max_size: 16", "layer pa: PriorBox with 1 max_size for 2 min_size"),
                          ("min_size: 8 max_size: 8", "layer pa: PriorBox max_size 8 is not above min_size 8"),
                          ("min_size: 8 variance: 0.1 variance: 0.2", "layer pa: PriorBox with 2 variance values")):
        with pytest.raises(ValueError, match=pattern):
            infer(layer("pa", "PriorBox", ["feat", "data"], "prior_box_param { %s }" % body))
    # every other Concat axis keeps its refusal; a Concat(axis 2) of anything but PriorBox tops too
    with pytest.raises(NotImplementedError, match="Concat along axis 2"):
        infer(RESHAPE + layer("cc", "Concat", ["rs", "rs"], "concat_param { axis: 2 }"))
    with pytest.raises(NotImplementedError, match="Concat along axis 3"):
        infer(layer("cc", "Concat", ["feat", "feat"], "concat_param { axis: 3 }"))


def proto_layer(text):
    return NetSpec(proto.parse_text(HEAD + text), "TEST").layers[0]


def test_normalize():
    text = layer("norm", "Normalize", ["feat"], "norm_param { across_spatial: false scale_filler { type: \"constant\" value: 20 } channel_shared: false }")
    spec, shapes = infer(text)
    assert shapes["norm"] == (2, 12, 4, 6) and spec.param_shapes["norm"] == [(12,)]
    assert np.all(fill_params(spec)["norm"][0] == 20.0)
    spec, _ = infer(layer("norm", "Normalize", ["feat"], "norm_param { across_spatial: false channel_shared: true }"))
    assert spec.param_shapes["norm"] == [(1,)] and fill_params(spec)["norm"][0].tolist() == [1.0]      # scale_filler defaults to constant 1
    segs, words = storage.param_layout(spec, plan(layer("norm", "Normalize", ["feat"], "norm_param { across_spatial: false }")).views, False)
    assert [(s.layer, s.kind, s.shape) for s in segs] == [("norm", storage.PLAIN, (1,))] and words == 4
    with pytest.raises(NotImplementedError, match="layer norm: Normalize with across_spatial: true"):
        infer(layer("norm", "Normalize", ["feat"]))


DET = ('input: "loc" input_shape { dim: 2 dim: 40 }\ninput: "conf" input_shape { dim: 2 dim: 30 }\n'
       + layer("pa", "PriorBox", ["feat", "data"], "prior_box_param { min_size: 8 }").replace("feat", "f1")
       + layer("det", "DetectionOutput", ["loc", "conf", "pa"], "detection_output_param { num_classes: 3 %s }"))
DET = 'input: "f1" input_shape { dim: 2 dim: 4 dim: 2 dim: 5 }\n' + DET


def test_detection_output_shapes_and_refusals():
    spec, shapes = infer(DET % "keep_top_k: 7 confidence_threshold: 0.3 nms_param { nms_threshold: 0.45 top_k: 5 }")
    assert shapes["det"] == (1, 1, 14, 7) and list(spec.detection_blobs) == ["det"]
    dp = ssd.detection_params(spec.layers[-1])
    assert (dp.num_classes, dp.background, dp.nms_threshold, dp.top_k, dp.code_type, dp.variance_encoded, dp.keep_top_k, dp.confidence_threshold) == \
        (3, 0, 0.45, 5, ssd.CODE_CORNER, False, 7, 0.3)                                             # CORNER is Caffe's default
    assert infer(DET % "nms_param { top_k: 5 }")[1]["det"] == (1, 1, 2 * 2 * 5, 7)                 # no keep_top_k: (classes - 1) * top_k per image
    assert ssd.detection_params(proto_det("nms_param { top_k: 5 }")).nms_threshold == 0.3
    assert ssd.detection_params(proto_det("keep_top_k: 3 code_type: CENTER_SIZE variance_encoded_in_target: true background_label_id: 2")).code_type == ssd.CODE_CENTER_SIZE
    p = plan(DET % "keep_top_k: 7 nms_param { top_k: 5 }")
    assert p.detections == {"det": 14} and p.views["det"].shape == (14 * 7 + 4,) and p.views["det"].nchw is None and p.root_bytes["det"] == 4 * 102
    for body, what in (("keep_top_k: 7 share_location: false", "share_location: false"), ("keep_top_k: 7 nms_param { eta: 0.9 }", "eta 0.9"),
                       ("keep_top_k: 7 code_type: CORNER_SIZE", "code_type CORNER_SIZE"), ("nms_param { nms_threshold: 0.4 }", "neither keep_top_k nor"),
                       ('keep_top_k: 7 save_output_param { output_directory: "/tmp/x" }', "writes no files")):
        with pytest.raises(NotImplementedError, match="layer det: DetectionOutput with .*" + what):
            infer(DET % body)
    infer(DET % 'keep_top_k: 7 save_output_param { output_directory: "" }')
    with pytest.raises(ValueError, match="layer det: DetectionOutput conf .* is not 10 priors x 4 classes"):
        infer((DET % "keep_top_k: 7").replace("num_classes: 3", "num_classes: 4"))
    with pytest.raises(ValueError, match="layer det: DetectionOutput bottoms disagree"):
        infer((DET % "keep_top_k: 7").replace("dim: 2 dim: 40", "dim: 2 dim: 44"))


def proto_det(body):
    return NetSpec(proto.parse_text(HEAD + DET % body), "TEST").layers[-1]


@pytest.mark.parametrize("t", ["MultiBoxLoss", "AnnotatedData", "DetectionEvaluate", "VideoData"])
def test_training_layers_are_refused_by_name(t):
    with pytest.raises(NotImplementedError, match="layer type '%s' \\(layer x\\): SSD's training and evaluation layers" % t):
        infer(layer("x", t, ["feat"]))


def test_the_half_float_engine_keeps_its_wording():
    with pytest.raises(NotImplementedError, match=r"f16 engine: layer type Permute \(perm\) has no half-float kernel"):
        plan(PERM + layer("flat", "Flatten", ["perm"]), f16=True)


def test_mobilenet_ssd_shapes():
    spec = NetSpec(proto.parse_text(models.mobilenet_ssd()), "TEST", depthwise=True)
    s = spec.infer()
    assert (s["mbox_loc"], s["mbox_conf"], s["mbox_priorbox"]) == ((1, 7668), (1, 40257), (1, 2, 7668))
    assert s["conv11_mbox_loc"] == (1, 12, 19, 19) and s["conv13_mbox_conf"] == (1, 126, 10, 10) and s["conv17_2"][2:] == (1, 1)
    assert s["conv11_mbox_loc_perm"] == (1, 19, 19, 12) and s["conv11_mbox_loc_flat"] == (1, 4332)
    assert s["mbox_conf_reshape"] == s["mbox_conf_softmax"] == (1, 1917, 21) and s["mbox_conf_flatten"] == (1, 40257)
    assert s["detection_out"] == (1, 1, 100, 7) and spec.output_blobs() == ["detection_out"]
    for phase in ("TRAIN", "TEST"):
        with pytest.raises(NotImplementedError, match="MultiBoxLoss"):
            models.mobilenet_ssd(phase)
    small = NetSpec(proto.parse_text(models.mobilenet_ssd(width_div=8, size=96, batch=2, classes=5)), "TEST", depthwise=True).infer()
    assert small["mbox_loc"] == (2, 816) and small["mbox_conf"] == (2, 204 * 5) and small["detection_out"] == (1, 1, 200, 7)


def test_ssd300_vgg_shapes():
    spec = NetSpec(proto.parse_text(models.ssd300_vgg()), "TEST")
    s = spec.infer()
    assert (s["mbox_loc"], s["mbox_conf"], s["mbox_priorbox"]) == ((1, 34928), (1, 183372), (1, 2, 34928))
    assert s["conv4_3_norm"] == (1, 512, 38, 38) and s["fc7"] == (1, 1024, 19, 19) and s["conv9_2"] == (1, 256, 1, 1)
    assert spec.param_shapes["conv4_3_norm"] == [(512,)] and s["detection_out"] == (1, 1, 200, 7)
    with pytest.raises(NotImplementedError, match="MultiBoxLoss"):
        models.ssd300_vgg("TRAIN")
    frag = NetSpec(proto.parse_text(models.ssd300_vgg(width_div=16, size=64, batch=2, heads=2)), "TEST").infer()
    assert frag["mbox_loc"] == (2, (64 * 4 + 16 * 6) * 4) and "conv6_1" not in frag and "conv4_3_norm" in frag
