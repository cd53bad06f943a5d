"""PReLU, Bias and TanH in the net description (no GPU): both states of the opt-in keyword, shapes and parameter shapes on 4-d and 2-d
blobs, fillers, multipliers, the device layout of the blobs, the caffemodel round trip of both slope shapes, every refusal by layer
name, and the two model writers."""
import numpy as np
import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd import storage as S
from fcn_object_detector_amd.netspec import ACT_TYPES, NetSpec, fill_params

HEAD = """
name: "acts"
input: "data"
input_shape { dim: 2 dim: 3 dim: 8 dim: 8 }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" convolution_param { num_output: 6 pad: 1 kernel_size: 3 } }
"""
NET = HEAD + """
layer { name: "prelu1" type: "PReLU" bottom: "conv1" top: "conv1" param { lr_mult: 3 decay_mult: 0 } }
layer { name: "bias1" type: "Bias" bottom: "conv1" top: "b1" }
layer { name: "tanh1" type: "TanH" bottom: "b1" top: "t1" }
layer { name: "prelu2" type: "PReLU" bottom: "t1" top: "p2" prelu_param { channel_shared: true filler { type: "constant" value: -0.5 } } }
layer { name: "fc" type: "InnerProduct" bottom: "p2" top: "fc" inner_product_param { num_output: 5 } }
layer { name: "prelu3" type: "PReLU" bottom: "fc" top: "fc" }
layer { name: "bias3" type: "Bias" bottom: "fc" top: "fc" bias_param { axis: 1 num_axes: 1 filler { type: "gaussian" std: 2 } } }
layer { name: "tanh3" type: "TanH" bottom: "fc" top: "fc" }
"""


def spec_of(txt, phase="TEST", **kw):
    spec = NetSpec(proto.parse_text(txt), phase, **kw)
    spec.infer()
    return spec


def test_a_bare_netspec_is_as_before_and_names_the_opt_in():
    for layer, name in (('layer { name: "bias1" type: "Bias" bottom: "conv1" top: "conv1" }', "bias1"),
                        ('layer { name: "prelu1" type: "PReLU" bottom: "conv1" top: "conv1" }', "prelu1")):
        for kw in ({}, {"activations": False}):
            with pytest.raises(NotImplementedError, match="%s.*activations=True" % name):
                spec_of(HEAD + layer, **kw)
    bare = spec_of(HEAD + 'layer { name: "tanh1" type: "TanH" bottom: "conv1" top: "t" }')      # (refused by the engines: tests/test_act_plan.py)
    assert bare.blob_shapes["t"] == (2, 6, 8, 8) and not bare.activations and "tanh1" not in bare.param_shapes
    assert ACT_TYPES == ("PReLU", "TanH", "Bias")


def test_the_keyword_is_keyword_only(tmp_path):
    msg = proto.parse_text(NET)
    with pytest.raises(TypeError):
        NetSpec(msg, "TEST", True, True, True, True, True, True)
    path = tmp_path / "net.prototxt"
    path.write_text(NET)
    with pytest.raises(TypeError):
        NetSpec.from_file(str(path), "TEST", True, True)
    spec = NetSpec.from_file(str(path), "TEST", activations=True)
    assert spec.activations and spec.infer()["p2"] == (2, 6, 8, 8)
    with pytest.raises(NotImplementedError, match="prelu1"):
        NetSpec.from_file(str(path), "TEST").infer()


def test_shapes_parameter_shapes_and_multipliers():
    spec = spec_of(NET, activations=True)
    sh = spec.blob_shapes
    assert sh["conv1"] == sh["b1"] == sh["t1"] == sh["p2"] == (2, 6, 8, 8) and sh["fc"] == (2, 5)
    assert spec.param_shapes["prelu1"] == [(6,)] and spec.param_shapes["bias1"] == [(6,)] and spec.param_shapes["prelu2"] == [()]
    assert spec.param_shapes["prelu3"] == [(5,)] and spec.param_shapes["bias3"] == [(5,)]      # channels are shape[1] of a 2-d blob
    assert "tanh1" not in spec.param_shapes and "tanh3" not in spec.param_shapes
    assert [l.name for l in spec.param_layers()] == ["conv1", "prelu1", "bias1", "prelu2", "fc", "prelu3", "bias3"]
    prelu1 = next(l for l in spec.layers if l.name == "prelu1")
    assert prelu1.lr_mult == [3.0] and prelu1.decay_mult == [0.0]


def test_fillers():
    p = fill_params(spec_of(NET, activations=True), seed=3)
    assert np.array_equal(p["prelu1"][0], np.full(6, 0.25, np.float32)) and p["prelu1"][0].dtype == np.float32      # PReLULayer's default
    assert np.array_equal(p["bias1"][0], np.zeros(6, np.float32))                                                     # BiasLayer's default
    assert p["prelu2"][0].shape == () and float(p["prelu2"][0]) == -0.5
    assert np.array_equal(p["prelu3"][0], np.full(5, 0.25, np.float32))
    assert p["bias3"][0].shape == (5,) and 0.3 < np.abs(p["bias3"][0]).max() < 10.0 and len(set(p["bias3"][0].tolist())) == 5


def test_the_blobs_lie_plain_in_the_flat_buffer():
    spec = spec_of(NET, "TRAIN", activations=True)
    plan = S.plan_blobs(spec, spec.blob_shapes, spec.data_tops(), spec.output_blobs(), False, True, True)
    segs, total = S.param_layout(spec, plan.views, False)
    by = {(s.layer, s.index): s for s in segs}
    for name, shape, lr, decay in (("prelu1", (6,), 3.0, 0.0), ("bias1", (6,), 1.0, 1.0), ("prelu2", (), 1.0, 1.0), ("prelu3", (5,), 1.0, 1.0)):
        s = by[(name, 0)]
        assert (s.kind, s.shape, s.host_shape, s.esize, s.lr_mult, s.decay_mult) == (S.PLAIN, shape, shape, 4, lr, decay), name
        assert s.count == int(np.prod(shape)) and s.offset % 4 == 0      # (a segment starts on 16 bytes; a shared slope is one word)
    assert by[("prelu2", 0)].count == 1 and total >= by[("bias3", 0)].offset + 5
    a = np.arange(6, dtype=np.float32)
    assert np.array_equal(S.unpack(by[("prelu1", 0)], S.pack(by[("prelu1", 0)], a)), a)
    one = S.pack(by[("prelu2", 0)], np.array([0.75], np.float32))        # a (1,) blob of an older file into the () slope
    assert one.size == 1 and S.unpack(by[("prelu2", 0)], one).shape == () and float(S.unpack(by[("prelu2", 0)], one)) == 0.75


def test_caffemodel_round_trip_of_both_slope_shapes(tmp_path):
    spec = spec_of(NET, activations=True)
    params = fill_params(spec, seed=4)
    params["prelu1"][0] = np.linspace(-0.5, 0.5, 6).astype(np.float32)
    path = str(tmp_path / "acts.caffemodel")
    proto.write_caffemodel(path, [(l.name, l.type, params[l.name]) for l in spec.param_layers()], spec.name)
    back = proto.read_caffemodel(path)
    assert np.array_equal(back["prelu1"][0], params["prelu1"][0]) and back["prelu1"][0].shape == (6,)
    # Caffe's empty shape is written for the shared slope (BlobShape without a dim); the value comes back as one element
    raw = open(path, "rb").read()
    assert b"prelu2" in raw and back["prelu2"][0].size == 1 and float(back["prelu2"][0].reshape(-1)[0]) == -0.5
    assert proto._ld(7, proto._ld(1, b"")) + proto._ld(5, np.float32(-0.5).tobytes()) in raw
    got = {}
    want = {k: [np.zeros_like(b) for b in v] for k, v in params.items()}
    copied = proto.copy_trained_layers(path, want, lambda name, blobs: got.__setitem__(name, blobs), log=lambda m: None)
    assert set(copied) == set(params) and got["prelu2"][0].shape == () and float(got["prelu2"][0]) == -0.5
    # ... and a file that holds the shared slope as (1,) is read alike
    proto.write_caffemodel(path, [("prelu2", "PReLU", [np.array([0.125], np.float32)])])
    got.clear()
    proto.copy_trained_layers(path, want, lambda name, blobs: got.__setitem__(name, blobs), log=lambda m: None)
    assert got["prelu2"][0].shape == () and float(got["prelu2"][0]) == 0.125


REFUSED = [
    ('layer { name: "b2" type: "Bias" bottom: "conv1" bottom: "data" top: "b2" }', NotImplementedError, "b2.*two bottoms"),
    ('layer { name: "b0" type: "Bias" bottom: "conv1" top: "b0" bias_param { axis: 0 } }', NotImplementedError, "b0.*axis 0"),
    ('layer { name: "bn" type: "Bias" bottom: "conv1" top: "bn" bias_param { num_axes: 2 } }', NotImplementedError, "bn.*num_axes 2"),
    ('layer { name: "bm" type: "Bias" bottom: "conv1" top: "bm" bias_param { axis: 1 num_axes: -1 } }', NotImplementedError, "bm.*num_axes -1"),
    ('layer { name: "p2" type: "PReLU" bottom: "conv1" bottom: "data" top: "p2" }', ValueError, "p2.*one 4-d or 2-d bottom"),
    ('layer { name: "pt" type: "PReLU" bottom: "conv1" top: "pt" top: "pu" }', ValueError, "pt.*one top"),
]


@pytest.mark.parametrize("layer,exc,match", REFUSED)
def test_refusals_by_layer_name(layer, exc, match):
    with pytest.raises(exc, match=match):
        spec_of(HEAD + layer, activations=True)


def test_a_blob_of_another_rank_is_refused_by_name():
    txt = 'input: "data"\ninput_shape { dim: 2 dim: 3 dim: 8 }\nlayer { name: "p3" type: "PReLU" bottom: "data" top: "p3" }'
    with pytest.raises(ValueError, match="p3.*4-d or 2-d"):
        spec_of(txt, activations=True)


@pytest.mark.parametrize("net,size,grid,widths", [("pnet", 12, (1, 1), (10, 16, 32)), ("rnet", 24, (3, 3), (28, 48, 64)), ("onet", 48, (3, 3), (32, 64, 64, 128))])
def test_mtcnn_writers(net, size, grid, widths):
    for phase in ("DEPLOY", "TRAIN", "TEST"):
        txt = models.mtcnn(net, phase, 2)
        with pytest.raises(NotImplementedError, match="activations=True"):
            spec_of(txt, "TRAIN" if phase == "TRAIN" else "TEST")
        spec = spec_of(txt, "TRAIN" if phase == "TRAIN" else "TEST", activations=True)
        sh = spec.blob_shapes
        assert sh["data"] == (2, 3, size, size) and models.mtcnn_grid(net, size) == grid
        assert [sh["conv%d" % (i + 1)][1] for i in range(len(widths))] == list(widths)
        prelus = [l for l in spec.layers if l.type == "PReLU"]
        assert len(prelus) == {"pnet": 3, "rnet": 4, "onet": 5}[net] and all(l.tops == l.bottoms for l in prelus)      # in place everywhere
        assert all(spec.param_shapes[l.name] == [(sh[l.tops[0]][1],)] for l in prelus)
        if phase == "DEPLOY":
            assert spec.output_blobs() == {"pnet": ["conv4-2", "prob1"], "rnet": ["conv5-2", "prob1"], "onet": ["conv6-2", "conv6-3", "prob1"]}[net]
        else:
            assert spec.output_blobs() == ["cls_loss", "roi_loss"] + (["pts_loss"] if net == "onet" else [])
    if net == "pnet":
        assert [l.name for l in spec.layers if l.type == "PReLU"] == ["PReLU1", "PReLU2", "PReLU3"]
        assert sh["conv4-1"] == (2, 2, 1, 1) and sh["conv4-2"] == (2, 4, 1, 1) and sh["pool1"] == (2, 10, 5, 5)
        big = spec_of(models.mtcnn("pnet", "DEPLOY", 2, size=(33, 47)), activations=True).blob_shapes      # fully convolutional
        assert big["prob1"] == (2, 2) + models.mtcnn_grid("pnet", (33, 47)) == (2, 2, 12, 19) and big["conv4-2"] == (2, 4, 12, 19)
        with pytest.raises(ValueError):
            models.mtcnn("pnet", "TRAIN", 2, size=24)
    elif net == "rnet":
        assert sh["pool1"] == (2, 28, 11, 11) and sh["pool2"] == (2, 48, 4, 4) and sh["conv3"] == (2, 64, 3, 3) and sh["conv4"] == (2, 128)
        with pytest.raises(ValueError):
            models.mtcnn("rnet", "DEPLOY", 2, size=48)
    else:
        assert sh["pool3"] == (2, 64, 4, 4) and sh["conv4"] == (2, 128, 3, 3) and sh["conv5"] == (2, 256) and sh["conv6-3"] == (2, 10)
        assert [l.type for l in spec.layers if l.bottoms == ["conv5"] and l.tops == ["conv5"]] == ["Dropout", "PReLU"]


def test_enet_writer():
    spec = spec_of(models.enet("DEPLOY"), activations=True)
    sh = spec.blob_shapes
    assert sh["data"] == (1, 3, 512, 1024) and sh["initial/conv"][1] == 13 and sh["initial/pool"][1] == 3 and sh["initial"] == (1, 16, 256, 512)
    assert sh["b1_4"] == (1, 64, 128, 256) and sh["b2_8"] == sh["b3_8"] == (1, 128, 64, 128) and sh["b4_2"] == (1, 64, 128, 256)
    assert sh["b5_1"] == (1, 16, 256, 512) and sh["fullconv"] == (1, 19, 512, 1024) and spec.output_blobs() == ["prob"]
    by = {l.name: l for l in spec.layers}
    geo = lambda n: by[n].sub("convolution_param")
    assert [int(geo("b2_%d/conv" % i).get("dilation", 1)) for i in range(1, 9)] == [1, 2, 1, 4, 1, 8, 1, 16]
    assert (int(geo("b2_3/conv_a").get("kernel_h")), int(geo("b2_3/conv_a").get("kernel_w"))) == (5, 1)
    assert (int(geo("b2_3/conv").get("kernel_h")), int(geo("b2_3/conv").get("kernel_w"))) == (1, 5)
    assert int(geo("b1_0/reduce").get("kernel_size")) == 2 and int(geo("b1_0/reduce").get("stride")) == 2 and sh["b1_0/reduce"][1] == 16
    assert by["b4_0/conv"].type == by["b5_0/conv"].type == by["fullconv"].type == "Deconvolution"
    # every Upsample pairs with the mask of its stage: the decoder undoes the downsampling bottlenecks in reverse order
    ups = [l for l in spec.layers if l.type == "Upsample"]
    assert [(l.name, l.bottoms[1]) for l in ups] == [("b4_0/unpool", "b2_0/pool_mask"), ("b5_0/unpool", "b1_0/pool_mask")]
    for l in ups:
        pool = spec.mask_blobs[l.bottoms[1]]
        assert sh[l.tops[0]][2:] == sh[pool.bottoms[0]][2:] and sh[l.bottoms[0]] == sh[l.bottoms[1]]
    n_prelu = sum(l.type == "PReLU" for l in spec.layers)
    assert n_prelu == 1 + 3 * (5 + 17 + 3 + 2) and sum(l.type == "Dropout" for l in spec.layers) == 27
    small = spec_of(models.enet("TRAIN", classes=5, batch=2, size=(32, 64), width_div=4), "TRAIN", activations=True)
    assert small.blob_shapes["fullconv"] == (2, 5, 32, 64) and small.blob_shapes["b2_0"] == (2, 32, 4, 8) and small.output_blobs() == ["loss"]
    assert spec_of(models.enet("DEPLOY", argmax=True), activations=True).output_blobs() == ["argmax"]
    with pytest.raises(ValueError):
        models.enet("DEPLOY", size=(100, 200))
