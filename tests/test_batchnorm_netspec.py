"""BatchNorm and Scale in the net description (no GPU): shapes, parameter shapes, forced zero multipliers, fillers, the device layout of
the blobs, the caffemodel round trip with the (1,) factor blob, models.resnet, and the refusals by layer name."""
import os
from collections import Counter

import numpy as np
import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd import storage as S
from fcn_object_detector_amd.netspec import NetSpec, bn_global_stats, fill_params

# a convolution with the reference's commented-out pair behind it, un-commented: separate tops, the ReLU in place on the Scale's top
SEPARATE = """
name: "pair"
input: "data"
input_shape { dim: 2 dim: 3 dim: 8 dim: 8 }
layer { name: "conv1_1" type: "Convolution" bottom: "data" top: "conv1_1" convolution_param { num_output: 6 pad: 1 kernel_size: 3 } }
layer { name: "conv1_1/bn" type: "BatchNorm" bottom: "conv1_1" top: "conv1_1/bn" }
layer { name: "conv1_1/bn_sc" type: "Scale" bottom: "conv1_1/bn" top: "conv1_1/bn_sc" scale_param { bias_term: true } }
layer { name: "relu1_1" type: "ReLU" bottom: "conv1_1/bn_sc" top: "conv1_1/bn_sc" }
layer { name: "conv1_2" type: "Convolution" bottom: "conv1_1/bn_sc" top: "conv1_2" convolution_param { num_output: 4 kernel_size: 1 } }
"""

INPLACE = """
name: "inplace"
input: "data"
input_shape { dim: 2 dim: 3 dim: 8 dim: 8 }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" convolution_param { num_output: 6 pad: 1 kernel_size: 3 bias_term: false } }
layer { name: "bn1" type: "BatchNorm" bottom: "conv1" top: "conv1" param { lr_mult: 0 } param { lr_mult: 0 } param { lr_mult: 0 }
  batch_norm_param { moving_average_fraction: 0.9 eps: 0.001 } }
layer { name: "scale1" type: "Scale" bottom: "conv1" top: "conv1" scale_param { bias_term: true
  filler { type: "constant" value: 0.5 } bias_filler { type: "constant" value: 0.25 } } }
layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
layer { name: "fc" type: "InnerProduct" bottom: "conv1" top: "fc" inner_product_param { num_output: 5 } }
layer { name: "bn_fc" type: "BatchNorm" bottom: "fc" top: "fc_bn" }
layer { name: "scale_fc" type: "Scale" bottom: "fc_bn" top: "fc_sc" }
"""


def _spec(txt, phase="TEST"):
    spec = NetSpec(proto.parse_text(txt), phase)
    spec.infer()
    return spec


def _views(spec):
    plan = S.plan_blobs(spec, spec.blob_shapes, spec.data_tops(), spec.output_blobs(), False, True, True)
    return plan


def test_shapes_and_parameter_shapes_on_4d_and_2d_blobs():
    spec = _spec(INPLACE)
    sh = spec.blob_shapes
    assert sh["conv1"] == (2, 6, 8, 8) and sh["fc"] == (2, 5) and sh["fc_bn"] == (2, 5) and sh["fc_sc"] == (2, 5)
    assert spec.param_shapes["bn1"] == [(6,), (6,), (1,)] and spec.param_shapes["scale1"] == [(6,), (6,)]
    assert spec.param_shapes["bn_fc"] == [(5,), (5,), (1,)] and spec.param_shapes["scale_fc"] == [(5,)]      # bias_term defaults to false
    sep = _spec(SEPARATE)
    assert sep.blob_shapes["conv1_1/bn"] == sep.blob_shapes["conv1_1/bn_sc"] == (2, 6, 8, 8)
    assert sep.output_blobs() == ["conv1_2"]


def test_use_global_stats_defaults_to_the_phase():
    bn = next(l for l in _spec(INPLACE).layers if l.name == "bn1")
    assert bn_global_stats(bn, "TEST") and not bn_global_stats(bn, "TRAIN")
    frozen = _spec(INPLACE.replace("eps: 0.001", "eps: 0.001 use_global_stats: true"), "TRAIN")
    assert bn_global_stats(next(l for l in frozen.layers if l.name == "bn1"), "TRAIN")
    off = _spec(INPLACE.replace("eps: 0.001", "eps: 0.001 use_global_stats: false"))
    assert not bn_global_stats(next(l for l in off.layers if l.name == "bn1"), "TEST")


def test_fillers_batchnorm_zero_scale_one_and_zero_by_default():
    p = fill_params(_spec(INPLACE), seed=5)
    assert all(np.array_equal(b, np.zeros(b.shape, np.float32)) for b in p["bn1"]) and p["bn1"][2].shape == (1,)
    assert np.array_equal(p["scale1"][0], np.full(6, 0.5, np.float32)) and np.array_equal(p["scale1"][1], np.full(6, 0.25, np.float32))
    assert np.array_equal(p["scale_fc"][0], np.ones(5, np.float32))
    q = fill_params(_spec(SEPARATE), seed=5)
    assert np.array_equal(q["conv1_1/bn_sc"][0], np.ones(6, np.float32)) and np.array_equal(q["conv1_1/bn_sc"][1], np.zeros(6, np.float32))


def test_multipliers_are_forced_to_zero_and_segments_are_plain():
    for txt in (INPLACE, SEPARATE):
        spec = _spec(txt, "TRAIN")
        plan = _views(spec)
        segs, words = S.param_layout(spec, plan.views, False)
        by = {(s.layer, s.index): s for s in segs}
        for l in spec.layers:
            if l.type == "BatchNorm":
                for i, shp in enumerate(spec.param_shapes[l.name]):
                    s = by[(l.name, i)]
                    assert s.kind == S.PLAIN and s.host_shape == shp == s.shape and s.lr_mult == 0.0 and s.decay_mult == 0.0 and s.esize == 4
            if l.type == "Scale":
                for i, shp in enumerate(spec.param_shapes[l.name]):
                    s = by[(l.name, i)]
                    assert s.kind == S.PLAIN and s.host_shape == shp and s.lr_mult == 1.0
        assert all(s.offset % 4 == 0 for s in segs) and words >= sum(s.count for s in segs)
        fac = next(s for s in segs if s.host_shape == (1,))
        blob = np.array([3.5], np.float32)
        assert np.array_equal(S.unpack(fac, S.pack(fac, blob)), blob)


def test_a_nonzero_batchnorm_lr_mult_is_refused_by_name():
    with pytest.raises(ValueError, match="bn1.*lr_mult"):
        _spec(INPLACE.replace("param { lr_mult: 0 } param { lr_mult: 0 } param { lr_mult: 0 }", "param { lr_mult: 0 } param { lr_mult: 1 }"))


def test_both_forms_plan_their_blobs():
    sep = _spec(SEPARATE, "TRAIN")
    plan = _views(sep)
    # every top of the separate-top form keeps a buffer of its own (the fused launch leaves the middle ones to read_blob), none is a view
    assert {"conv1_1", "conv1_1/bn", "conv1_1/bn_sc", "conv1_2"} <= set(plan.root_bytes) and not plan.alias
    assert plan.views["conv1_1/bn"].cstride == 8 and plan.views["conv1_1/bn_sc"].cstride == 8
    inp = _spec(INPLACE, "TRAIN")
    plan = _views(inp)
    assert plan.views["conv1"].root == "conv1" and [q.name for q in plan.producers["conv1"]] == ["conv1", "bn1", "scale1", "relu1"]
    assert plan.views["fc_bn"].nchw == (2, 5, 1, 1) and plan.views["fc_bn"].cstride == 8


def test_caffemodel_round_trip_with_the_factor_blob(tmp_path):
    spec = _spec(INPLACE)
    rng = np.random.default_rng(0)
    src = {name: [rng.standard_normal(s).astype(np.float32) for s in shapes] for name, shapes in spec.param_shapes.items()}
    src["bn1"][2][...] = 7.25
    path = os.path.join(str(tmp_path), "bn.caffemodel")
    proto.write_caffemodel(path, [(l.name, l.type, src[l.name]) for l in spec.param_layers()], spec.name)
    assert [b.shape for b in proto.read_caffemodel(path)["bn1"]] == [(6,), (6,), (1,)]
    dst = fill_params(spec, seed=1)
    got = {}
    copied = proto.copy_trained_layers(path, dst, lambda name, blobs: got.__setitem__(name, blobs), log=lambda m: None)
    assert sorted(copied) == sorted(src)
    for name in src:
        assert all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(got[name], src[name])), name
    assert got["bn1"][2].shape == (1,) and float(got["bn1"][2][0]) == 7.25


@pytest.mark.parametrize("depth,n_bn", [(50, 53), (101, 104), (152, 155)])
def test_resnet_parses_with_the_published_structure(depth, n_bn):
    for phase in ("DEPLOY", "TRAIN", "TEST"):
        txt = models.resnet(phase, depth, batch=2)
        spec = _spec(txt, "TEST" if phase == "DEPLOY" else phase)
        cnt = Counter(l.type for l in spec.layers)
        assert cnt["BatchNorm"] == n_bn and cnt["Scale"] == n_bn and cnt["Convolution"] == n_bn and cnt["InnerProduct"] == 1
        assert cnt["Eltwise"] == (n_bn - 5) // 3 and cnt["Pooling"] == 2
        last = [l for l in spec.layers if l.type == "Eltwise"][-1].tops[0]
        assert last == "res5c" and spec.blob_shapes[last] == (2, 2048, 7, 7) and spec.blob_shapes["pool5"] == (2, 2048, 1, 1)
        assert spec.blob_shapes["conv1"] == (2, 64, 112, 112) and spec.blob_shapes["pool1"] == (2, 64, 56, 56)
        assert spec.blob_shapes["fc1000"] == (2, 1000)
        names = [l.name for l in spec.layers]
        for nm in ("conv1", "bn_conv1", "scale_conv1", "conv1_relu", "pool1", "res2a_branch1", "bn2a_branch1", "scale2a_branch1", "res2a_branch2a",
                   "res2a_branch2a_relu", "bn2a_branch2b", "scale2a_branch2c", "res2a", "res2a_relu", "res5c_branch2c", "pool5", "fc1000"):
            assert nm in names, nm
        assert ("res3b1_branch2a" in names) == (depth > 50) and ("res3b" in names) == (depth == 50)
        assert spec.param_shapes["conv1"] == [(64, 3, 7, 7), (64,)] and spec.param_shapes["res2a_branch1"] == [(256, 64, 1, 1)]
        conv = {l.name: l.sub("convolution_param") for l in spec.layers if l.type == "Convolution"}
        assert int(conv["res3a_branch1"].get("stride")) == 2 and int(conv["res3a_branch2a"].get("stride")) == 2
        assert int(conv["res2a_branch2a"].get("stride")) == 1 and int(conv["res3a_branch2b"].get("stride")) == 1
        bn = next(l for l in spec.layers if l.name == "bn_conv1")
        assert (bn.sub("batch_norm_param").get("use_global_stats") is not None) == (phase == "DEPLOY")
        assert spec.output_blobs() == (["prob"] if phase == "DEPLOY" else ["loss"] if phase == "TRAIN" else ["accuracy", "loss"])


def test_resnet_reduced_width_and_size():
    spec = _spec(models.resnet("TRAIN", 50, batch=2, width_div=8, size=64), "TRAIN")
    assert spec.blob_shapes["res5c"] == (2, 256, 2, 2) and spec.blob_shapes["pool5"] == (2, 256, 1, 1)
    with pytest.raises(ValueError, match="depth"):
        models.resnet("DEPLOY", 34)


REFUSED = [
    ('layer { name: "bias1" type: "Bias" bottom: "conv1" top: "conv1" }', "bias1"),
    ('layer { name: "prelu1" type: "PReLU" bottom: "conv1" top: "conv1" }', "prelu1"),
    ('layer { name: "sc2" type: "Scale" bottom: "conv1" bottom: "data" top: "sc2" }', "sc2.*two bottoms"),
    ('layer { name: "sc0" type: "Scale" bottom: "conv1" top: "sc0" scale_param { axis: 0 } }', "sc0.*axis"),
    ('layer { name: "sc3" type: "Scale" bottom: "conv1" top: "sc3" scale_param { num_axes: 2 } }', "sc3.*num_axes"),
]


@pytest.mark.parametrize("layer,match", REFUSED)
def test_out_of_scope_forms_are_refused_by_layer_name(layer, match):
    head = INPLACE.split('layer { name: "bn1"')[0]
    with pytest.raises(NotImplementedError, match=match):
        _spec(head + layer)


def test_depthwise_convolution_stays_refused_by_name():
    txt = INPLACE.split('layer { name: "bn1"')[0] + \
        'layer { name: "dw" type: "Convolution" bottom: "conv1" top: "dw" convolution_param { num_output: 6 kernel_size: 3 group: 6 } }\n' \
        'layer { name: "bn_dw" type: "BatchNorm" bottom: "dw" top: "dw" }'
    spec = _spec(txt)
    with pytest.raises(NotImplementedError, match="dw.*depthwise"):
        S.param_layout(spec, _views(spec).views, False)
