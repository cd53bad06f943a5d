"""ELU, ReLU6, Clip, AbsVal, BNLL and Swish in NetSpec (no GPU): shapes on 4-d and 2-d blobs for a bare NetSpec and NetSpec.public alike -
these layers need no keyword -, the parameters neuron_params reads, each refusal by layer name, and the two model writers that use them."""
import hashlib
import inspect

import pytest

from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import ACT_TYPES, FEATURES, NEURON_TYPES, Layer, NetSpec, neuron_params

DATA4 = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 6 dim: 5 dim: 7 } } }\n'
DATA2 = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 3 dim: 10 } } }\n'
BODY = {"ELU": "elu_param { alpha: 0.5 }", "ReLU6": "", "Clip": "clip_param { min: -1 max: 2.5 }", "AbsVal": "", "BNLL": "", "Swish": "swish_param { beta: 1.5 }"}
BUILD = {"bare": lambda msg, phase: NetSpec(msg, phase), "public": NetSpec.public}


def layer(t, bottom="data", top="y", body=None, name="n"):
    return 'layer { name: "%s" type: "%s" bottom: "%s" top: "%s" %s }\n' % (name, t, bottom, top, BODY[t] if body is None else body)


def test_the_types_and_the_unchanged_surface():
    assert NEURON_TYPES == ("ELU", "ReLU6", "Clip", "AbsVal", "BNLL", "Swish") and ACT_TYPES == ("PReLU", "TanH", "Bias")
    assert FEATURES == ("depthwise", "ip_gemm", "rconv_f16", "tconv_f16", "scale_gate", "activations")      # no new keyword
    assert list(inspect.signature(NetSpec.__init__).parameters)[1:] == ["msg", "phase"] + list(FEATURES)
    assert set(L.NEURON_MODES) == set(NEURON_TYPES)


@pytest.mark.parametrize("how", sorted(BUILD))
@pytest.mark.parametrize("phase", ["TEST", "TRAIN"])
@pytest.mark.parametrize("t", NEURON_TYPES)
def test_tops_take_the_bottoms_shape(t, phase, how):
    for data, shape in ((DATA4, (2, 6, 5, 7)), (DATA2, (3, 10))):
        spec = BUILD[how](proto.parse_text(data + layer(t)), phase)
        spec.infer()
        assert spec.blob_shapes["y"] == shape and "n" not in spec.param_shapes      # no blob: nothing for a caffemodel to carry
        if t != "AbsVal":
            spec = BUILD[how](proto.parse_text(data + layer(t, top="data")), phase)
            spec.infer()
            assert spec.blob_shapes["data"] == shape


def test_the_parameters():
    lay = lambda t, body=None: Layer(proto.parse_text(layer(t, body=body)).getall("layer")[0])
    assert neuron_params(lay("ELU")) == (L.NEURON_ELU, 0.5, 0.0) and neuron_params(lay("ELU", "")) == (L.NEURON_ELU, 1.0, 0.0)
    assert neuron_params(lay("ELU", "elu_param { alpha: 0 }")) == (L.NEURON_ELU, 0.0, 0.0)
    assert neuron_params(lay("ReLU6")) == (L.NEURON_CLIP, 0.0, 6.0) and neuron_params(lay("Clip")) == (L.NEURON_CLIP, -1.0, 2.5)
    assert neuron_params(lay("Clip", "clip_param { min: -3 max: -1 }")) == (L.NEURON_CLIP, -3.0, -1.0)
    assert neuron_params(lay("AbsVal")) == (L.NEURON_ABSVAL, 0.0, 0.0) and neuron_params(lay("BNLL")) == (L.NEURON_BNLL, 0.0, 0.0)
    assert neuron_params(lay("Swish")) == (L.NEURON_SWISH, 1.5, 0.0) and neuron_params(lay("Swish", "")) == (L.NEURON_SWISH, 1.0, 0.0)
    assert neuron_params(lay("Swish", "swish_param { beta: -2 }")) == (L.NEURON_SWISH, -2.0, 0.0)


REFUSALS = [
    ("a negative alpha", layer("ELU", body="elu_param { alpha: -0.1 }"), NotImplementedError, "layer n: ELU with alpha -0.1"),
    ("Clip without bounds", layer("Clip", body=""), ValueError, "layer n: Clip needs clip_param"),
    ("Clip without max", layer("Clip", body="clip_param { min: 0 }"), ValueError, "layer n: Clip needs clip_param"),
    ("Clip without min", layer("Clip", body="clip_param { max: 6 }"), ValueError, "layer n: Clip needs clip_param"),
    ("Clip with min == max", layer("Clip", body="clip_param { min: 2 max: 2 }"), ValueError, "layer n: Clip with min 2 >= max 2"),
    ("Clip with min > max", layer("Clip", body="clip_param { min: 6 max: 0 }"), ValueError, "layer n: Clip with min 6 >= max 0"),
    ("AbsVal in place", layer("AbsVal", top="data"), ValueError, "layer n: AbsVal does not allow in-place computation"),
]
REFUSALS += [("%s with two bottoms" % t, layer(t, bottom='data" bottom: "data'), ValueError, "layer n: %s takes one bottom and has one top, got 2 and 1" % t)
             for t in NEURON_TYPES]
REFUSALS += [("%s with two tops" % t, layer(t, top='y" top: "z'), ValueError, "layer n: %s takes one bottom and has one top, got 1 and 2" % t)
             for t in NEURON_TYPES]


@pytest.mark.parametrize("how", sorted(BUILD))
@pytest.mark.parametrize("what,text,exc,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_by_layer_name(what, text, exc, msg, how):
    with pytest.raises(exc, match=msg):
        BUILD[how](proto.parse_text(DATA4 + text), "TEST").infer()


@pytest.mark.parametrize("how", sorted(BUILD))
@pytest.mark.parametrize("t", NEURON_TYPES)
def test_a_blob_of_another_rank_is_refused(t, how):
    for dims in ("dim: 4", "dim: 2 dim: 3 dim: 4", "dim: 2 dim: 3 dim: 4 dim: 5 dim: 6"):
        data = 'layer { name: "data" type: "Input" top: "data" input_param { shape { %s } } }\n' % dims
        with pytest.raises(ValueError, match="layer n: %s takes one 4-d or 2-d bottom" % t):
            BUILD[how](proto.parse_text(data + layer(t)), "TEST").infer()


@pytest.mark.parametrize("t", ["Exp", "Log", "Threshold"])
def test_the_neighbours_keep_the_generic_refusal(t):
    with pytest.raises(NotImplementedError, match="layer type '%s' .layer n.$" % t):
        NetSpec.public(proto.parse_text(DATA4 + 'layer { name: "n" type: "%s" bottom: "data" top: "y" }\n' % t), "TEST").infer()


def test_mobilenet_v2_is_unchanged_and_takes_relu6():
    # the text of the parent commit, by its SHA-256: the default and a small TRAIN net
    assert hashlib.sha256(models.mobilenet_v2().encode()).hexdigest() == "f4bf2a82c2c78f56d1bf0a49e6022b23611ebf771387f1c2111a1364cfc6a87c"
    small = dict(batch=2, width_div=4, size=64, classes=10)
    assert hashlib.sha256(models.mobilenet_v2("TRAIN", **small).encode()).hexdigest() == "a5150e9501fea2c7d7ba25e6185fd16531822b36b4931e01913a6599da64216b"
    assert models.mobilenet_v2(relu6=False) == models.mobilenet_v2() and 'type: "ReLU6"' not in models.mobilenet_v2()
    for phase in ("DEPLOY", "TRAIN", "TEST"):
        plain, six = models.mobilenet_v2(phase, **small), models.mobilenet_v2(phase, relu6=True, **small)
        assert six == plain.replace('type: "ReLU"', 'type: "ReLU6"')      # the same places, the same names
        assert six.count('type: "ReLU6"') == 35 == 1 + 16 + 17 + 1 and 'type: "ReLU"' not in six      # conv1, expands, depthwise, conv9
        spec = NetSpec.public(proto.parse_text(six), "TEST" if phase == "DEPLOY" else phase)
        spec.infer()
        assert sum(l.type == "ReLU6" for l in spec.layers) == 35 and sum(spec.is_depthwise(l) for l in spec.layers) == 17


@pytest.mark.parametrize("width_div,size", [(1, 224), (4, 64)])
def test_efficientnet_b0_infers(width_div, size):
    for phase in ("DEPLOY", "TRAIN", "TEST"):
        txt = models.efficientnet_b0(phase, batch=2, classes=10, width_div=width_div, size=size)
        spec = NetSpec.public(proto.parse_text(txt), "TEST" if phase == "DEPLOY" else phase)
        spec.infer()
        count = lambda f: sum(bool(f(l)) for l in spec.layers)
        assert count(spec.is_depthwise) == 16 and count(lambda l: l.type == "Swish") == 49 and count(lambda l: l.type == "Eltwise") == 9
        assert all(l.tops == l.bottoms for l in spec.layers if l.type == "Swish")      # in place, every one
        assert count(lambda l: l.type == "Scale" and len(l.bottoms) == 2) == 16 and count(lambda l: l.type == "Sigmoid") == 16
        assert count(lambda l: l.type == "Dropout") == 1 and count(lambda l: l.type == "BatchNorm") == 1 + 15 + 16 + 16 + 1
        wd = lambda c: max(c // width_div, 1)
        assert spec.blob_shapes["conv1"] == (2, wd(32), size // 2, size // 2) and spec.blob_shapes["conv9"] == (2, wd(1280), size // 32, size // 32)
        assert spec.blob_shapes["conv2_1/se_reduce"] == (2, max(wd(32) // 4, 1)) and spec.blob_shapes["conv2_1/se_prob"] == (2, wd(32))
        assert spec.blob_shapes["conv4_1/se_reduce"] == (2, max(wd(24) // 4, 1)) and spec.blob_shapes["conv4_1/dwise"][1] == 6 * wd(24)
        k5 = [l.name for l in spec.layers if spec.is_depthwise(l) and int(l.sub("convolution_param").get("kernel_size")) == 5]
        assert len(k5) == 2 + 3 + 4 and all(int(next(q for q in spec.layers if q.name == n).sub("convolution_param").get("pad")) == 2 for n in k5)
        assert spec.blob_shapes["fc7"] == (2, 10, 1, 1)
        assert ("prob" in spec.blob_shapes) == (phase == "DEPLOY") and ("accuracy" in spec.blob_shapes) == (phase == "TEST")
    assert models.efficientnet_b0(fillers=False).count("filler") == 0
