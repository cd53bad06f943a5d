"""InnerProduct in the net description (no GPU): shapes, parameter shapes, fillers from inner_product_param, refusals by layer name."""
import math

import numpy as np
import pytest

from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec, fill_params

NET = """
name: "ip"
input: "data"
input_shape { dim: 3 dim: 6 dim: 5 dim: 4 }
layer { name: "fc1" type: "InnerProduct" bottom: "data" top: "fc1"
  param { lr_mult: 1 decay_mult: 1 } param { lr_mult: 2 decay_mult: 0 }
  inner_product_param { num_output: 16 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.25 } } }
layer { name: "relu1" type: "ReLU" bottom: "fc1" top: "fc1" }
layer { name: "drop1" type: "Dropout" bottom: "fc1" top: "fc1" dropout_param { dropout_ratio: 0.5 } }
layer { name: "fc2" type: "InnerProduct" bottom: "fc1" top: "fc2" inner_product_param { num_output: 7 bias_term: false
  weight_filler { type: "gaussian" std: 0.01 } } }
layer { name: "prob" type: "Softmax" bottom: "fc2" top: "prob" }
"""


def test_shapes_and_parameter_shapes():
    spec = NetSpec(proto.parse_text(NET), "TEST")
    shapes = spec.infer()
    assert shapes["fc1"] == (3, 16) and shapes["fc2"] == (3, 7) and shapes["prob"] == (3, 7)
    assert spec.param_shapes["fc1"] == [(16, 120), (16,)] and spec.param_shapes["fc2"] == [(7, 16)]
    assert spec.layers[0].lr_mult == [1.0, 2.0] and spec.layers[0].decay_mult == [1.0, 0.0]
    assert spec.output_blobs() == ["prob"]


def test_fillers_come_from_inner_product_param():
    spec = NetSpec(proto.parse_text(NET), "TEST")
    spec.infer()
    p = fill_params(spec, seed=3)
    w, b = p["fc1"]
    bound = math.sqrt(3.0 / 120)                  # xavier, FAN_IN = K of a 2-d blob
    assert w.shape == (16, 120) and np.abs(w).max() <= bound and np.abs(w).max() > 0.8 * bound and abs(float(w.mean())) < 0.2 * bound
    assert np.array_equal(b, np.full(16, 0.25, np.float32))
    assert len(p["fc2"]) == 1 and 0.005 < float(p["fc2"][0].std()) < 0.02


@pytest.mark.parametrize("extra,what", [("axis: 2", "axis"), ("transpose: true", "transpose")])
def test_refusals_name_the_layer(extra, what):
    txt = NET.replace("num_output: 16", "num_output: 16 " + extra)
    with pytest.raises(NotImplementedError, match="fc1.*%s" % what):
        NetSpec(proto.parse_text(txt), "TEST").infer()


TWO = """
input: "data"
input_shape { dim: 3 dim: 6 dim: 2 dim: 2 }
layer { name: "a" type: "InnerProduct" bottom: "data" top: "a" inner_product_param { num_output: 8 } }
layer { name: "b" type: "InnerProduct" bottom: "data" top: "b" inner_product_param { num_output: 12 } }
"""


def test_concat_and_slice_over_2d_blobs():
    cat = TWO + 'layer { name: "cat" type: "Concat" bottom: "a" bottom: "b" top: "cat" }\n'
    shapes = NetSpec(proto.parse_text(cat + 'layer { name: "o" type: "InnerProduct" bottom: "cat" top: "o" inner_product_param { num_output: 5 } }'),
                     "TEST").infer()
    assert shapes["cat"] == (3, 20) and shapes["o"] == (3, 5)
    sl = TWO + 'layer { name: "sl" type: "Slice" bottom: "b" top: "b0" top: "b1" slice_param { slice_point: 4 } }'
    shapes = NetSpec(proto.parse_text(sl), "TEST").infer()
    assert shapes["b0"] == (3, 4) and shapes["b1"] == (3, 8)
    with pytest.raises(ValueError, match="layer mix: Concat"):      # a 4-d and a 2-d bottom: refused by layer name
        NetSpec(proto.parse_text(TWO + 'layer { name: "mix" type: "Concat" bottom: "data" bottom: "a" top: "m" }'), "TEST").infer()
    with pytest.raises(ValueError, match="cat3"):
        NetSpec(proto.parse_text(TWO + """
input: "v"
input_shape { dim: 3 }
layer { name: "cat3" type: "Concat" bottom: "a" bottom: "v" top: "m" }"""), "TEST").infer()


def test_accuracy_and_loss_over_2d_scores():
    txt = NET.replace('layer { name: "prob" type: "Softmax" bottom: "fc2" top: "prob" }', """
input: "label"
input_shape { dim: 3 }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc2" bottom: "label" top: "loss" }
layer { name: "acc" type: "Accuracy" bottom: "fc2" bottom: "label" top: "acc" }""")
    shapes = NetSpec(proto.parse_text(txt), "TEST").infer()
    assert shapes["loss"] == () and shapes["acc"] == ()
