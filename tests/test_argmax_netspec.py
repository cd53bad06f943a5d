"""ArgMax in NetSpec: the shapes of every form, each refusal by layer name, and the model writers' `argmax` option (no GPU)."""
import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec, argmax_form

NET = """
input: "data" input_shape { %s }
layer { name: "am" type: "ArgMax" bottom: "data" %s top: "%s" argmax_param { %s } }
"""


def infer(dims, param, top="am", extra=""):
    spec = NetSpec(proto.parse_text(NET % (" ".join("dim: %d" % d for d in dims), extra, top, param)), "TEST")
    return spec.infer()["am"] if top == "am" else spec.infer()


@pytest.mark.parametrize("dims,param,want", [
    ((2, 21, 9, 13), "axis: 1", (2, 1, 9, 13)),
    ((2, 21, 9, 13), "axis: -3 top_k: 5", (2, 5, 9, 13)),
    ((2, 21, 9, 13), "axis: 1 out_max_val: true top_k: 2", (2, 2, 9, 13)),      # the values, not indices and values
    ((3, 1000), "axis: 1 top_k: 5", (3, 5)),
    ((3, 1000), "axis: -1", (3, 1)),
    ((3, 1000), "top_k: 5", (3, 1, 5)),                                          # Caffe's legacy shape
    ((3, 1000), "top_k: 5 out_max_val: true", (3, 2, 5)),
    ((3, 1000, 1, 1), "", (3, 1, 1)),
    ((3, 1000, 1, 1), "out_max_val: true top_k: 32", (3, 2, 32)),
    ((3, 40, 1, 1), "axis: 1 top_k: 32", (3, 32, 1, 1)),
])
def test_shapes_of_every_form(dims, param, want):
    assert infer(dims, param) == want


def test_the_form_as_the_engine_reads_it():
    spec = NetSpec(proto.parse_text(NET % ("dim: 3 dim: 10", "", "am", "top_k: 4 out_max_val: true")), "TEST")
    spec.infer()
    assert argmax_form(spec.layers[-1], (3, 10)) == (4, True, True)
    spec = NetSpec(proto.parse_text(NET % ("dim: 3 dim: 10 dim: 2 dim: 2", "", "am", "axis: 1")), "TEST")
    assert argmax_form(spec.layers[-1], (3, 10, 2, 2)) == (1, False, False)


@pytest.mark.parametrize("dims,param,top,extra,err,words", [
    ((2, 21, 9, 13), "", "am", "", NotImplementedError, "without an axis"),              # the legacy form over a real plane
    ((2, 21, 9, 13), "axis: 2", "am", "", NotImplementedError, "axis 2"),
    ((2, 21, 9, 13), "axis: 0", "am", "", NotImplementedError, "axis 0"),
    ((3, 10), "axis: -3", "am", "", NotImplementedError, "axis -3"),
    ((2, 21, 9, 13), "axis: 1 top_k: 22", "am", "", ValueError, "top_k 22"),
    ((2, 21, 9, 13), "axis: 1 top_k: 0", "am", "", ValueError, "top_k 0"),
    ((3, 1000), "top_k: 33", "am", "", NotImplementedError, "top_k 33"),
    ((2, 21, 9, 13), "axis: 1", "am", 'bottom: "data"', ValueError, "one bottom"),
    ((2, 21, 9, 13), "axis: 1", "data", "", ValueError, "in place"),
    ((2, 21, 9), "axis: 1", "am", "", ValueError, "4-d or 2-d"),
])
def test_each_refusal_names_the_layer(dims, param, top, extra, err, words):
    with pytest.raises(err) as e:
        infer(dims, param, top, extra)
    assert "layer am" in str(e.value) and words in str(e.value)


def outputs(text):
    spec = NetSpec(proto.parse_text(text), "TEST")
    shapes = spec.infer()
    return spec, {b: shapes[b] for b in spec.output_blobs()}


def test_the_writers_end_in_the_label_map_on_request():
    tiny = dict(width_div=16)
    assert outputs(models.segnet_basic(argmax=True, size=(24, 40), **tiny))[1] == {"argmax": (1, 1, 24, 40)}
    assert outputs(models.segnet(argmax=True, size=32, **tiny))[1] == {"argmax": (1, 1, 32, 32)}
    assert outputs(models.deeplab_largefov(argmax=True, interp=True, size=41, fc_div=64, **tiny))[1] == {"argmax": (1, 1, 41, 41)}
    assert outputs(models.deeplab_largefov(argmax=True, size=41, fc_div=64, **tiny))[1] == {"argmax": (1, 1, 6, 6)}
    assert outputs(models.deeplab_aspp(argmax=True, interp=True, size=41, fc_div=64, **tiny))[1] == {"argmax": (1, 1, 41, 41)}
    for fn in (models.voc_fcn32s, models.voc_fcn16s, models.voc_fcn8s):
        spec, outs = outputs(fn(argmax=True, shape=(1, 3, 40, 48), fc_div=256, **tiny))
        assert outs == {"argmax": (1, 1, 40, 48)} and spec.layers[-1].bottoms == ["score"]
    # the layer sits behind the DEPLOY tail only, and the defaults emit the text they always did
    for phase in ("TRAIN", "TEST"):
        assert "ArgMax" not in models.segnet_basic(phase, argmax=True) and "ArgMax" not in models.deeplab_aspp(phase, argmax=True)
    assert "ArgMax" not in models.voc_fcn8s("TRAIN", argmax=True)
    for fn in (models.segnet, models.segnet_basic, models.deeplab_largefov, models.deeplab_aspp, models.voc_fcn32s, models.voc_fcn16s, models.voc_fcn8s):
        assert fn() == fn(argmax=False) and "ArgMax" not in fn()
        assert fn(argmax=True).startswith(fn()) and fn(argmax=True).count('type: "ArgMax"') == 1
