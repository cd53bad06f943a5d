"""Nets with Interp layers through the public surface, -m gpu, against torch in float64 on the CPU (tests/torch_interp_ref.py), in the
style of tests/test_gpu_dilated_nets.py.

DeepLab-LargeFOV with interp=True at width_div 8, fc_div 8, 5 classes, an input edge of 73 (score map 10 x 10) and fc6 at dilation 2:
DEPLOY ends in fc8_interp at 73 x 73; TRAIN takes a 73 x 73 label with 255s and shrinks it.  A pyramid-pooling head written out below:
the 1-bin branch is Interp's n1 == 1 case, the feature map's gradient has five consumers, and its in-place ReLU rides in the
convolution while its Concat copies (the mask is applied after the last of the five has written).  A half-float net that ends in an Interp.

Thresholds are the project's: rel_err < 1e-4 for blobs and the loss, < 5e-4 for parameter gradients, or 4 x torch float32's own error
against torch float64 where that is larger.  Measured on the CPU for the cases below, with the ReLU masks and MAX-pooling
argmaxes of a float32 pass standing in for the device's: LargeFOV DEPLOY blobs at most 8.9e-7 (fc8_voc12), TRAIN blobs at most 7.0e-7
(conv5_3) and parameter gradients at most 7.9e-7 (fc6); the pyramid head's blobs at most 3.6e-7 (up1) and gradients at most 3.4e-7
(red1's bank) - far below a quarter of either threshold, so the exception is written into the checks but does not bind here.  The backward comparison adopts the device's ReLU masks and
MAX-pooling argmaxes in the reference, as tests/test_gpu_dilated_nets.py explains; forward blobs and the loss are compared without any
adoption.  The half-float net is held to the half-float net threshold of tests/test_gpu_f16_vgg.py (5e-3) against the float32 engine."""
import sys

import numpy as np
import pytest
import torch

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_interp_ref import as_torch, max_pool_argmax, random_params, torch_net

pytestmark = pytest.mark.gpu
F32 = np.float32
LARGEFOV = dict(num_classes=5, width_div=8, fc_div=8, size=73, fc6_dilation=2, interp=True)
LF_BLOBS = ["conv1_2", "pool3", "conv5_3", "pool5a", "fc6", "fc7", "fc8_voc12"]


def make(text, phase):
    msg = proto.parse_text(text)
    spec = NetSpec(msg, phase)
    spec.infer()
    return msg, spec


def inputs_for(spec, seed, classes=5):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in spec.input_shapes.items():
        if name == "label":
            lab = rng.integers(0, classes, shp).astype(F32)
            lab[rng.random(shp) < 0.1] = 255
            out[name] = lab
        else:
            out[name] = rng.standard_normal(shp).astype(F32)
    return out


def own_error(spec, params, x, names, **kw):
    """rel_err of torch float32 against torch float64 for the named blobs: the reference's own rounding error."""
    with torch.no_grad():
        a = torch_net(spec, as_torch(params), x, **kw)
        b = torch_net(spec, as_torch(params, dtype=torch.float32), x, dtype=torch.float32, **kw)
    return {n: rel_err(b[n].numpy(), a[n].numpy()) for n in names}


def test_largefov_deploy_ends_at_image_resolution(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    txt = models.deeplab_largefov("DEPLOY", batch=1, **LARGEFOV)
    msg, spec = make(txt, "TEST")
    path, weights = str(tmp_path / "deploy.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(txt)
    params = random_params(spec, 11)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST)
    assert [op.name for op in net._engine.ops if op.kind == "interp"] == ["fc8_interp"]
    x = inputs_for(spec, 1)
    net.blobs["data"].data[...] = x["data"]
    out = net.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    names = LF_BLOBS + ["fc8_interp"]
    own = own_error(spec, params, x, names)
    assert list(net.outputs) == ["fc8_interp"] and out["fc8_interp"].shape == (1, 5, 73, 73) and net.blobs["fc8_voc12"].data.shape == (1, 5, 10, 10)
    for name in names:
        err = rel_err(net.blobs[name].data, ref[name].numpy())
        print("NET %s %.3g (torch float32: %.3g)" % (name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    # the corners are aligned: every 8th pixel of the upsampled map is the score map's, bit for bit
    assert np.array_equal(out["fc8_interp"][:, :, ::8, ::8], net.blobs["fc8_voc12"].data)


def _train_engine(monkeypatch, graph, text, seed=3, params=None):
    monkeypatch.setenv("FCN_NO_GRAPH", "0" if graph else "1")
    msg, spec = make(text, "TRAIN")
    params = random_params(spec, seed) if params is None else params
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    return spec, params, eng


def check_step(eng, spec, params, x, out, interior, seed, label=""):
    """Loss, interior blobs and every parameter gradient of one step against torch float64 under the rule of the module text."""
    with torch.no_grad():
        fwd = torch_net(spec, as_torch(params), x, dropout_seed=seed)
    own = own_error(spec, params, x, interior, dropout_seed=seed)
    want = float(fwd["total_loss"])
    print("STEP %s loss %.6g want %.6g" % (label, out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want), (out["total_loss"], want)
    for name in interior:
        err = rel_err(eng.read_blob(name), fwd[name].numpy())
        print("BLOB %s %s %.3g (torch float32: %.3g)" % (label, name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    masks = {l.name: eng.read_blob(l.tops[0]) > 0 for l in spec.layers if l.type == "ReLU"}
    argmax = max_pool_argmax(spec, eng.read_blob)
    P = as_torch(params, grad=True)
    torch_net(spec, P, x, dropout_seed=seed, relu_masks=masks, pool_argmax=argmax)["total_loss"].backward()
    P32 = as_torch(params, grad=True, dtype=torch.float32)
    torch_net(spec, P32, x, dropout_seed=seed, relu_masks=masks, pool_argmax=argmax, dtype=torch.float32)["total_loss"].backward()
    got = eng.download_grads()
    for l in spec.param_layers():
        assert eng._learns(l), l.name
        for i, (g, r, r32) in enumerate(zip(got[l.name], P[l.name], P32[l.name])):
            assert g.shape == tuple(r.grad.shape), l.name
            own_g = rel_err(r32.grad.numpy(), r.grad.numpy())
            err = rel_err(g, r.grad.numpy())
            print("GRAD %s %s[%d] %.3g (torch float32: %.3g)" % (label, l.name, i, err, own_g))
            assert err < max(5e-4, 4 * own_g), "parameter gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, err, own_g)


@pytest.mark.parametrize("graph", [True, False])
def test_largefov_trains_on_an_image_sized_label(gpu, monkeypatch, graph):
    spec, params, eng = _train_engine(monkeypatch, graph, models.deeplab_largefov("TRAIN", batch=2, **LARGEFOV))
    assert [op.name for op in eng.ops if op.kind == "interp"] == ["label_shrink"]
    assert "interp_bwd" not in [op.kind for op in eng.bwd_ops], "nothing learns below the label"
    assert eng.blobs["label"].shape == (2, 1, 73, 73) and eng.blobs["label_shrink"].shape == (2, 1, 10, 10)
    x = inputs_for(spec, 5)
    assert (x["label"][:, :, ::8, ::8] == 255).any()
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=7)
    assert eng.read_blob("label_shrink").tobytes() == np.ascontiguousarray(x["label"][:, :, ::8, ::8]).tobytes()
    check_step(eng, spec, params, x, out, LF_BLOBS, 7, "largefov+interp graph=%d" % graph)
    g1 = eng.download_grads()
    eng.step(seed=7)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k])), "the same step again: the same bits"
    eng.close()


FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
BRANCH = """
layer { name: "pool%(b)d" type: "Pooling" bottom: "feat" top: "pool%(b)d" pooling_param { pool: AVE kernel_size: %(k)d stride: %(k)d } }
layer { name: "red%(b)d" type: "Convolution" bottom: "pool%(b)d" top: "red%(b)d" convolution_param { num_output: 2 kernel_size: 1 FILL } }
layer { name: "up%(b)d" type: "Interp" bottom: "red%(b)d" top: "up%(b)d" interp_param { height: 12 width: 12 } }
"""
PYRAMID = ("""
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 12 }
input: "label" input_shape { dim: 2 dim: 1 dim: 45 dim: 45 }
layer { name: "feat" type: "Convolution" bottom: "data" top: "feat" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "relu_feat" type: "ReLU" bottom: "feat" top: "feat" }
""" + "".join(BRANCH % dict(b=b, k=12 // b) for b in (1, 2, 3, 6)) + """
layer { name: "cat" type: "Concat" bottom: "feat" bottom: "up1" bottom: "up2" bottom: "up3" bottom: "up6" top: "cat" }
layer { name: "score" type: "Convolution" bottom: "cat" top: "score" convolution_param { num_output: 4 kernel_size: 3 pad: 1 FILL } }
layer { name: "score_up" type: "Interp" bottom: "score" top: "score_up" interp_param { zoom_factor: 4 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "score_up" bottom: "label" top: "loss" loss_param { ignore_label: 255 } }
""").replace("FILL", FILL)
PYRAMID_BLOBS = ["feat", "pool1", "pool6", "red1", "red3", "up1", "up2", "up3", "up6", "cat", "score", "score_up"]


def test_pyramid_pooling_head_trains(gpu, monkeypatch):
    msg, spec0 = make(PYRAMID, "TRAIN")
    assert spec0.blob_shapes["pool1"] == (2, 8, 1, 1) and spec0.blob_shapes["pool6"] == (2, 8, 6, 6) and spec0.blob_shapes["cat"] == (2, 16, 12, 12)
    assert spec0.blob_shapes["score_up"] == (2, 4, 45, 45)
    spec, params, eng = _train_engine(monkeypatch, True, PYRAMID, params=fill_params(spec0, seed=5))
    assert sorted(op.name for op in eng.ops if op.kind == "interp") == ["score_up", "up1", "up2", "up3", "up6"]
    assert sorted(op.name for op in eng.bwd_ops if op.kind == "interp_bwd") == ["score_up", "up1", "up2", "up3", "up6"]
    x = inputs_for(spec, 8, classes=4)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=1)
    check_step(eng, spec, params, x, out, PYRAMID_BLOBS, 1, "pyramid")
    g1 = eng.download_grads()
    eng.step(seed=1)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k])), "the same step again: the same bits"
    eng.close()


HALF = """
input: "data" input_shape { dim: 2 dim: 3 dim: 19 dim: 23 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 16 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "c1" type: "Convolution" bottom: "c0" top: "c1" convolution_param { num_output: 5 kernel_size: 3 pad: 1 FILL } }
layer { name: "up" type: "Interp" bottom: "c1" top: "up" interp_param { zoom_factor: 4 } }
""".replace("FILL", FILL)


def test_half_float_engine_ends_in_an_interp(gpu):
    msg, spec = make(HALF, "TEST")
    params = fill_params(spec, seed=2)
    x = np.random.default_rng(4).standard_normal((2, 3, 19, 23)).astype(F32)
    outs = {}
    for dtype in ("f32", "f16"):
        eng = Engine(NetSpec(msg, "TEST"), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0, autotune=False, dtype=dtype)
        assert (eng.blobs["c1"].esize, eng.blobs["up"].esize) == ((2, 4) if dtype == "f16" else (4, 4))
        assert [op.kind for op in eng.ops][-1] == "interp"
        eng.host_array("data")[...] = x
        outs[dtype] = eng.forward()["up"].copy()
        eng.close()
    assert outs["f16"].dtype == np.float32 and outs["f16"].shape == (2, 5, 73, 89)
    err = rel_err(outs["f16"], outs["f32"])
    print("F16NET up rel %.3g" % err)
    assert err < 5e-3
