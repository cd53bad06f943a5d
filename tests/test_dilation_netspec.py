"""convolution_param { dilation } in the shape rules, and the text of the DeepLab writers (no GPU)."""
import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec, conv_out, layer_dilation

NET = """
input: "data" input_shape { dim: 1 dim: 3 dim: 9 dim: 9 }
layer { name: "c" type: "%s" bottom: "data" top: "c" convolution_param { num_output: 4 kernel_size: 3 %s } }
"""


def shapes(extra, type_="Convolution"):
    spec = NetSpec(proto.parse_text(NET % (type_, extra)), "TEST")
    return spec, spec.infer()


def test_output_size_follows_the_dilated_window():
    assert shapes("dilation: 2")[1]["c"] == (1, 4, 5, 5)
    assert shapes("dilation: 2 pad: 2")[1]["c"] == (1, 4, 9, 9)
    assert shapes("dilation: 2 dilation: 2 pad: 2")[1]["c"] == (1, 4, 9, 9)
    assert shapes("dilation: 3 pad: 1 stride: 2")[1]["c"] == (1, 4, 3, 3)       # (9 + 2 - 7) // 2 + 1
    assert shapes("dilation: 4 pad: 4")[1]["c"] == (1, 4, 9, 9)
    spec, _ = shapes("dilation: 2 pad: 2")
    assert spec.param_shapes["c"] == [(4, 3, 3, 3), (4,)] and layer_dilation(spec.layers[0]) == 2


def test_dilation_one_and_no_dilation_give_the_dense_shapes():
    for extra in ("", "pad: 1", "stride: 2", "pad: 2 stride: 3"):
        assert shapes(extra)[1] == shapes(extra + " dilation: 1")[1]
    assert shapes("pad: 1 dilation: 1")[1]["c"] == (1, 4, 9, 9) and shapes("")[1]["c"] == (1, 4, 7, 7)
    assert shapes("stride: 2", "Deconvolution")[1] == shapes("stride: 2 dilation: 1", "Deconvolution")[1]
    for h, k, s, p in ((9, 3, 1, 0), (224, 7, 2, 3), (12, 5, 3, 2)):
        assert conv_out(h, k, s, p) == conv_out(h, k, s, p, 1) == (h + 2 * p - k) // s + 1


def test_refusals_name_the_layer():
    with pytest.raises(NotImplementedError, match=r"layer c\b.*dilation"):
        shapes("dilation: 2 dilation: 3")
    with pytest.raises(NotImplementedError, match=r"layer c\b.*dilation"):
        shapes("dilation: 2 dilation: 2 dilation: 2")
    with pytest.raises(NotImplementedError, match=r"layer c\b.*Deconvolution"):
        shapes("dilation: 2", "Deconvolution")
    with pytest.raises(ValueError, match=r"layer c\b"):
        shapes("dilation: 0")
    with pytest.raises(ValueError, match=r"layer c\b.*exceeds"):
        shapes("dilation: 5")                                                     # an 11 x 11 window on 9 x 9


VGG_BLOBS = ["conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3",
             "conv4_1", "conv4_2", "conv4_3", "pool4", "conv5_1", "conv5_2", "conv5_3", "pool5"]


def _spec(text, phase):
    spec = NetSpec(proto.parse_text(text), "TEST" if phase == "DEPLOY" else phase)
    return spec, spec.infer()


@pytest.mark.parametrize("phase", ["TRAIN", "TEST", "DEPLOY"])
def test_deeplab_largefov_names_and_shapes(phase):
    spec, sh = _spec(models.deeplab_largefov(phase, batch=2, num_classes=5, width_div=8, fc_div=8, size=201), phase)
    assert models.deeplab_score_size(201) == 26 and models.deeplab_score_size(321) == 41
    for nm, c, e in (("conv1_2", 8, 201), ("pool1", 8, 101), ("pool2", 16, 51), ("pool3", 32, 26), ("pool4", 64, 26), ("conv5_3", 64, 26),
                     ("pool5", 64, 26), ("pool5a", 64, 26), ("fc6", 128, 26), ("fc7", 128, 26), ("fc8_voc12", 5, 26)):
        assert sh[nm] == (2, c, e, e), nm
    assert sh["fc6"][2:] == sh["pool5a"][2:]                                      # fc6 keeps its bottom's extent: pad == dilation
    by = {l.name: l for l in spec.layers}
    assert [l.name for l in spec.layers if l.type in ("Convolution", "Pooling")] == VGG_BLOBS + ["pool5a", "fc6", "fc7", "fc8_voc12"]
    assert {n: layer_dilation(by[n]) for n in ("conv4_3", "conv5_1", "conv5_2", "conv5_3", "fc6", "fc7")} == \
        {"conv4_3": 1, "conv5_1": 2, "conv5_2": 2, "conv5_3": 2, "fc6": 12, "fc7": 1}
    for n, (k, s, p) in (("pool1", (3, 2, 1)), ("pool3", (3, 2, 1)), ("pool4", (3, 1, 1)), ("pool5", (3, 1, 1)), ("pool5a", (3, 1, 1))):
        pp = by[n].sub("pooling_param")
        assert (int(pp.get("kernel_size")), int(pp.get("stride")), int(pp.get("pad"))) == (k, s, p), n
    assert str(by["pool5a"].sub("pooling_param").get("pool")) == "AVE" and str(by["pool5"].sub("pooling_param").get("pool")) == "MAX"
    assert int(by["fc6"].sub("convolution_param").get("pad")) == 12 and int(by["conv5_1"].sub("convolution_param").get("pad")) == 2
    assert spec.param_shapes["fc6"] == [(128, 64, 3, 3), (128,)]
    assert [l.type for l in spec.layers if l.name in ("relu6", "drop6", "relu7", "drop7")] == ["ReLU", "Dropout", "ReLU", "Dropout"]
    assert not any(l.type in ("Interp", "ImageSegData") for l in spec.layers)
    if phase == "DEPLOY":
        assert spec.output_blobs() == ["fc8_voc12"] and "label" not in sh
    else:
        assert sh["label"] == (2, 1, 26, 26) and sh["loss"] == ()
        assert int(by["loss"].sub("loss_param").get("ignore_label")) == 255 and by["loss"].bottoms == ["fc8_voc12", "label"]
        assert ("accuracy" in by) == (phase == "TEST")


def test_deeplab_largefov_published_widths():
    spec, sh = _spec(models.deeplab_largefov("DEPLOY"), "DEPLOY")
    assert sh["data"] == (1, 3, 321, 321) and sh["fc6"] == (1, 1024, 41, 41) and sh["fc8_voc12"] == (1, 21, 41, 41)
    assert spec.param_shapes["fc6"] == [(1024, 512, 3, 3), (1024,)] and spec.param_shapes["conv5_1"][0] == (512, 512, 3, 3)
    _, sh6 = _spec(models.deeplab_largefov("DEPLOY", fc6_dilation=6), "DEPLOY")
    assert sh6["fc6"] == sh["fc6"]


@pytest.mark.parametrize("phase", ["TRAIN", "TEST"])
def test_deeplab_aspp_names_and_shapes(phase):
    spec, sh = _spec(models.deeplab_aspp(phase, batch=2, num_classes=5, width_div=8, fc_div=8, size=137, rates=(2, 4, 6, 8)), phase)
    by = {l.name: l for l in spec.layers}
    assert models.deeplab_score_size(137) == 18 and sh["pool5"] == (2, 64, 18, 18) and "pool5a" not in sh
    for i, r in enumerate((2, 4, 6, 8), 1):
        assert layer_dilation(by["fc6_%d" % i]) == r and int(by["fc6_%d" % i].sub("convolution_param").get("pad")) == r
        assert by["fc6_%d" % i].bottoms == ["pool5"]
        assert sh["fc6_%d" % i] == (2, 128, 18, 18) and sh["fc7_%d" % i] == (2, 128, 18, 18) and sh["fc8_voc12_%d" % i] == (2, 5, 18, 18)
    assert by["fc8_voc12"].type == "Eltwise" and by["fc8_voc12"].bottoms == ["fc8_voc12_%d" % i for i in range(1, 5)]
    assert sh["fc8_voc12"] == (2, 5, 18, 18) and sh["label"] == (2, 1, 18, 18)
    _, pub = _spec(models.deeplab_aspp("DEPLOY"), "DEPLOY")
    assert pub["fc6_4"] == (1, 1024, 41, 41) and pub["fc8_voc12"] == (1, 21, 41, 41)
