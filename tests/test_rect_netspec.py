"""Per-axis geometry of Convolution layers as netspec reads it (no GPU): kernel_h / kernel_w, pad_h / pad_w, stride_h / stride_w and
the repeated-field spelling by Caffe's rules, the shapes of tops and blobs, what stays refused by layer name, and the shapes of
models.inception_v3."""
import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import Layer, NetSpec, is_rectangular, kernel_stride_pad, layer_geometry

NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 9 dim: 11 }
layer { name: "c" type: "%s" bottom: "data" top: "c" %s }
"""


def conv(params, type_="Convolution"):
    body = "pooling_param { pool: MAX %s }" % params if type_ == "Pooling" else "convolution_param { num_output: 5 %s }" % params
    return NET % (type_, body)


def infer(text, phase="TEST"):
    spec = NetSpec(proto.parse_text(text), phase)
    return spec, spec.infer()


def layer(params):
    return NetSpec(proto.parse_text(conv(params)), "TEST").layers[0]


def test_a_1x7_layer_keeps_the_grid_and_its_blob_is_rectangular():
    spec, shapes = infer(conv("kernel_h: 1 kernel_w: 7 pad_h: 0 pad_w: 3"))
    assert shapes["c"] == (2, 5, 9, 11)
    assert spec.param_shapes["c"] == [(5, 3, 1, 7), (5,)]
    assert layer_geometry(spec.layers[0]) == (1, 7, 1, 1, 0, 3) and is_rectangular(spec.layers[0])


def test_a_7x1_layer_with_stride_h_is_sized_per_axis():
    spec, shapes = infer(conv("kernel_h: 7 kernel_w: 1 stride_h: 2 stride_w: 1 pad_h: 3 pad_w: 0 bias_term: false"))
    assert shapes["c"] == (2, 5, (9 + 6 - 7) // 2 + 1, 11) == (2, 5, 5, 11)
    assert spec.param_shapes["c"] == [(5, 3, 7, 1)]
    spec, shapes = infer(conv("kernel_h: 3 kernel_w: 5 pad_h: 0 pad_w: 2 stride_h: 2 stride_w: 1 dilation: 2"))
    assert shapes["c"] == (2, 5, (9 - 5) // 2 + 1, 11 + 4 - 9 + 1) == (2, 5, 3, 7)


def test_the_repeated_field_spelling_means_h_then_w():
    a = layer("kernel_size: 1 kernel_size: 7 pad: 0 pad: 3 stride: 2 stride: 1")
    assert layer_geometry(a) == (1, 7, 2, 1, 0, 3)
    spec, shapes = infer(conv("kernel_size: 1 kernel_size: 7 pad: 0 pad: 3"))
    assert shapes["c"] == (2, 5, 9, 11) and spec.param_shapes["c"][0] == (5, 3, 1, 7)
    assert layer_geometry(layer("kernel_size: 3 kernel_size: 3 pad: 1 pad: 1")) == (3, 3, 1, 1, 1, 1)


def test_a_square_kernel_with_pad_h_and_pad_w_gets_that_pad():
    _, a = infer(conv("kernel_size: 3 pad_h: 1 pad_w: 1"))
    _, b = infer(conv("kernel_size: 3 pad: 1"))
    assert a["c"] == b["c"] == (2, 5, 9, 11)
    assert not is_rectangular(layer("kernel_size: 3 pad_h: 1 pad_w: 1"))
    assert is_rectangular(layer("kernel_size: 3 pad_h: 1 pad_w: 2"))
    _, c = infer(conv("kernel_size: 3 pad_h: 1 pad_w: 2"))
    assert c["c"] == (2, 5, 9, 13)


def test_kernel_stride_pad_keeps_its_answers_for_layers_whose_axes_agree():
    assert kernel_stride_pad(layer("kernel_size: 3 stride: 1 pad: 1").sub("convolution_param")) == (3, 1, 1)
    assert kernel_stride_pad(layer("kernel_size: 7 stride: 2 pad: 3").sub("convolution_param")) == (7, 2, 3)
    assert kernel_stride_pad(layer("kernel_size: 1").sub("convolution_param")) == (1, 1, 0)
    assert kernel_stride_pad(layer("kernel_h: 3 kernel_w: 3 stride_h: 2 stride_w: 2 pad_h: 1 pad_w: 1").sub("convolution_param")) == (3, 2, 1)
    assert kernel_stride_pad(proto.parse_text("pool: MAX kernel_size: 3 stride: 2")) == (3, 2, 0)
    with pytest.raises(NotImplementedError, match="axes differ"):
        kernel_stride_pad(layer("kernel_h: 1 kernel_w: 7").sub("convolution_param"))


@pytest.mark.parametrize("params,what", [
    ("kernel_size: 3 kernel_h: 3 kernel_w: 3", "both kernel_size and kernel_h / kernel_w"),
    ("kernel_h: 3", "kernel_h without kernel_w"),
    ("kernel_w: 3", "kernel_w without kernel_h"),
    ("kernel_size: 3 pad: 1 pad_h: 1 pad_w: 1", "both pad and pad_h / pad_w"),
    ("kernel_size: 3 pad_h: 1", "pad_h without pad_w"),
    ("kernel_size: 3 pad_w: 1", "pad_w without pad_h"),
    ("kernel_size: 3 stride: 1 stride_h: 1 stride_w: 1", "both stride and stride_h / stride_w"),
    ("kernel_size: 3 stride_h: 2", "stride_h without stride_w"),
    ("kernel_size: 3 stride_w: 2", "stride_w without stride_h"),
    ("kernel_size: 3 kernel_size: 3 kernel_size: 3", "kernel_size given 3 times"),
    ("kernel_size: 3 pad: 1 pad: 1 pad: 1", "pad given 3 times"),
    ("kernel_size: 3 stride: 1 stride: 1 stride: 1", "stride given 3 times"),
    ("kernel_h: 3 kernel_h: 3 kernel_w: 3", "kernel_h given 2 times"),
    ("pad: 1", "without kernel_size"),
    ("kernel_size: 0", "kernel_size 0x0 is below 1"),
    ("kernel_h: 1 kernel_w: 0", "kernel_size 1x0 is below 1"),
    ("kernel_size: 3 stride: 0", "stride 0x0 is below 1"),
    ("kernel_size: 3 stride_h: 1 stride_w: 0", "stride 1x0 is below 1"),
    ("kernel_size: 3 pad: -1", "pad -1x-1 is below 0"),
    ("kernel_size: 3 pad_h: 0 pad_w: -2", "pad 0x-2 is below 0"),
])
def test_malformed_geometry_is_a_value_error_that_names_the_layer(params, what):
    with pytest.raises(ValueError, match="layer c.*" + what):
        layer_geometry(layer(params))
    with pytest.raises(ValueError, match="layer c.*" + what):
        infer(conv(params))


def test_a_window_larger_than_the_padded_bottom_names_the_layer():
    with pytest.raises(ValueError, match="layer c: the 1x13 window"):
        infer(conv("kernel_h: 1 kernel_w: 13"))


def test_rectangular_pooling_and_deconvolution_stay_refused_by_layer_name():
    with pytest.raises(NotImplementedError, match="layer c: Pooling with kernel 1x3"):
        infer(conv("kernel_h: 1 kernel_w: 3", "Pooling"))
    with pytest.raises(NotImplementedError, match="layer c: Pooling with kernel 3x3 stride 2x1"):
        infer(conv("kernel_size: 3 stride_h: 2 stride_w: 1", "Pooling"))
    with pytest.raises(NotImplementedError, match="layer c: Deconvolution with kernel 1x4"):
        infer(conv("kernel_h: 1 kernel_w: 4", "Deconvolution"))
    with pytest.raises(NotImplementedError, match="layer c: Deconvolution with kernel 4x4 stride 2x2 pad 1x0"):
        infer(conv("kernel_size: 4 stride: 2 pad_h: 1 pad_w: 0", "Deconvolution"))
    _, s = infer(conv("kernel_h: 3 kernel_w: 3 stride_h: 2 stride_w: 2", "Pooling"))      # axes that agree, written per axis
    assert s["c"] == (2, 3, 4, 5)
    _, s = infer(conv("kernel_h: 4 kernel_w: 4 stride_h: 2 stride_w: 2 pad_h: 1 pad_w: 1", "Deconvolution"))
    assert s["c"] == (2, 5, 18, 22)


def test_inception_v3_shapes_at_299():
    spec, s = infer(models.inception_v3("TRAIN", batch=2), "TRAIN")
    assert s["pool2"] == (2, 192, 35, 35)
    assert [s[m] for m in ("mixed_35a", "mixed_35b", "mixed_35c")] == [(2, 256, 35, 35), (2, 288, 35, 35), (2, 288, 35, 35)]
    assert s["reduction_a"] == (2, 768, 17, 17) and all(s["mixed_17" + c] == (2, 768, 17, 17) for c in "abcd")
    assert s["reduction_b"] == (2, 1280, 8, 8) and s["mixed_8a"] == s["mixed_8b"] == (2, 2048, 8, 8)
    assert s["pool3"] == (2, 2048, 1, 1) and s["classifier"] == (2, 1000) and s["loss"] == ()
    assert spec.param_shapes["mixed_17b/7x7_1x7"] == [(160, 160, 1, 7)] and spec.param_shapes["mixed_17b/7x7_7x1"] == [(192, 160, 7, 1)]
    assert spec.param_shapes["mixed_8a/3x3_1x3"] == [(384, 384, 1, 3)] and spec.param_shapes["reduction_b/7x7x3_7x1"] == [(192, 192, 7, 1)]
    rect = [l.name for l in spec.layers if l.type == "Convolution" and is_rectangular(l)]
    assert len(rect) == 4 * 6 + 2 + 2 * 4 and len([l for l in spec.layers if l.type == "Convolution"]) == 94
    for phase, last in (("DEPLOY", "prob"), ("TEST", "loss")):
        sp, sh = infer(models.inception_v3(phase), "TEST")
        assert sp.layers[-1].name == last and sh["mixed_8b"] == (1, 2048, 8, 8)
    assert "label" not in infer(models.inception_v3("DEPLOY"))[1] and "accuracy" in infer(models.inception_v3("TEST"))[1]


def test_inception_v3_reduced_net():
    spec, s = infer(models.inception_v3("TRAIN", batch=2, classes=6, width_div=8, size=(171, 139)), "TRAIN")
    assert models.inception_v3_grids((171, 139)) == [(19, 15), (9, 7), (4, 3)]
    assert s["data"] == (2, 3, 171, 139) and s["mixed_35c"] == (2, 36, 19, 15) and s["mixed_17d"] == (2, 96, 9, 7)
    assert s["mixed_8b"] == (2, 256, 4, 3) and s["classifier"] == (2, 6)
    assert spec.param_shapes["mixed_17a/7x7dbl_a_7x1"] == [(16, 16, 7, 1)]


def test_inception_v3_refuses_a_size_whose_reduction_grids_disagree():
    with pytest.raises(ValueError, match=r"reduction_a's 3x3 / 2 convolution gives a 17x17 grid and its 3x3 / 2 pooling 18x18"):
        models.inception_v3("DEPLOY", size=301)
    with pytest.raises(ValueError, match=r"reduction_a.* 17x17 grid .* 17x18"):      # one axis agrees, the other does not
        models.inception_v3("DEPLOY", size=(299, 301))
    with pytest.raises(ValueError, match="reduction_b"):
        models.inception_v3("DEPLOY", size=315)
    with pytest.raises(ValueError, match="at least 3x3"):
        models.inception_v3("DEPLOY", size=40)
    assert models.inception_v3_grids(299) == [(35, 35), (17, 17), (8, 8)]
