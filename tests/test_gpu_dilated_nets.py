"""DeepLab-LargeFOV and the DeepLab-v2 ASPP head (models.deeplab_largefov / deeplab_aspp) through the public surface, -m gpu, against
torch in float64 on the CPU (tests/torch_dilated_ref.py), in the style of tests/test_gpu_resnet.py.

The nets: VGG16 at width_div 8 (widths 8 .. 64), fc6 / fc7 at 128, 5 classes.  LargeFOV on an input edge of 201: the score map is
26 x 26, wider than 2 * 12 + 1, so the pixels in its middle see all nine taps of fc6 (dilation 12) inside the image.  ASPP with the
rates (2, 4, 6, 8) on an edge of 137 (18 x 18).

Thresholds are the project's: rel_err < 1e-4 for blobs and the loss, < 5e-4 for parameter gradients.  Where the reference's OWN float32
error is too close to them the rule of DESIGN.md 4.13 applies: the same case runs in torch float32 on the CPU against the float64 net
and the threshold of that quantity is the larger of the project's and 4 x that error.  Measured on the CPU for the steps below:
LargeFOV blobs at most 9.0e-7 (conv5_3), parameter gradients at most 2.7e-6 (conv2_1); ASPP blobs at most 7.8e-7, parameter gradients
at most 1.1e-6 (conv2_1) - with the ReLU masks and MAX-pooling argmaxes of a float32 pass standing in for the device's; far below a quarter of either threshold, so the
exception is written into the checks but does not bind here.
The backward comparison adopts the device's ReLU masks in the reference, as tests/test_gpu_resnet.py does, and the device's MAX-pooling
argmaxes with them (torch_dilated_ref.torch_net: pool4 / pool5 are 3x3 windows at stride 1 over ReLU outputs, and with the masks alone
torch float32 against torch float64 is off by 2e-3 at conv5_3's bank through one window that is zero but for a unit of +-1e-9);
forward blobs and the loss are compared without any adoption."""
import sys

import numpy as np
import pytest
import torch

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_dilated_ref import as_torch, max_pool_argmax, random_params, torch_net

pytestmark = pytest.mark.gpu
F32 = np.float32
SMALL = dict(num_classes=5, width_div=8, fc_div=8)
LARGEFOV = dict(SMALL, size=201)
ASPP = dict(SMALL, size=137, rates=(2, 4, 6, 8))
LF_BLOBS = ["conv1_2", "pool1", "pool3", "conv4_3", "pool4", "conv5_1", "conv5_3", "pool5", "pool5a", "fc6", "fc7", "fc8_voc12"]
ASPP_BLOBS = ["pool3", "conv5_3", "pool5", "fc6_1", "fc6_4", "fc7_2", "fc8_voc12_1", "fc8_voc12_3", "fc8_voc12"]


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


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


def test_largefov_test_phase_forward_through_caffe_net(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    txt = models.deeplab_largefov("TEST", batch=1, **LARGEFOV)
    msg, spec = make(txt, "TEST")
    path, weights = str(tmp_path / "test.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(txt)
    params = random_params(spec, 11)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST)
    eng = net._engine
    dconvs = [op.name for op in eng.ops if op.kind == "dconv"]
    assert [n.split(" ")[0] for n in dconvs] == ["conv5_1", "conv5_2", "conv5_3", "fc6"] and "[d12 " in dconvs[3] and "[d2 " in dconvs[0]
    assert "relu" not in [op.kind for op in eng.ops], "every in-place ReLU rides in a convolution's epilogue, the dilated ones included"
    x = inputs_for(spec, 1)
    for k, v in x.items():
        net.blobs[k].data[...] = v
    out = net.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    own = own_error(spec, params, x, LF_BLOBS)
    assert net.blobs["fc6"].data.shape == (1, 128, 26, 26) and net.blobs["fc8_voc12"].data.shape == (1, 5, 26, 26)
    for name in LF_BLOBS:
        err = rel_err(net.blobs[name].data, ref[name].numpy())
        print("NET %s %.3g (torch float32: %.3g)" % (name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    assert sorted(net.outputs) == ["accuracy", "loss"]
    assert abs(float(out["loss"]) - float(ref["loss"])) <= 1e-4 * abs(float(ref["loss"])), (float(out["loss"]), float(ref["loss"]))
    assert abs(float(out["accuracy"]) - float(ref["accuracy"])) <= 1.5 / (26 * 26), (float(out["accuracy"]), float(ref["accuracy"]))
    for l in spec.param_layers():                      # the caffemodel round trip: every blob as it was written
        for i, want in enumerate(params[l.name]):
            assert np.array_equal(eng.read_param(l.name, i), want), l.name


def _train_engine(monkeypatch, graph, text, seed=3):
    monkeypatch.setenv("FCN_NO_GRAPH", "0" if graph else "1")
    msg, spec = make(text, "TRAIN")
    params = random_params(spec, seed)
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
    worst = (0.0, None)
    for l in spec.param_layers():
        assert eng._learns(l), l.name
        for i, (g, r, r32) in enumerate(zip(got[l.name], P[l.name], P32[l.name])):
            assert g.shape == tuple(r.grad.shape), l.name
            own_g = rel_err(r32.grad.numpy(), r.grad.numpy())
            err = rel_err(g, r.grad.numpy())
            worst = max(worst, (err, "%s[%d] own %.3g" % (l.name, i, own_g)))
            print("GRAD %s %s[%d] %.3g (torch float32: %.3g)" % (label, l.name, i, err, own_g))
            assert err < max(5e-4, 4 * own_g), "parameter gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, err, own_g)
    print("GRAD %s worst %.3g at %s" % (label, worst[0], worst[1]))


@pytest.mark.parametrize("graph", [True, False])
def test_largefov_one_training_step(gpu, monkeypatch, graph):
    spec, params, eng = _train_engine(monkeypatch, graph, models.deeplab_largefov("TRAIN", batch=2, **LARGEFOV))
    bk = [(op.kind, op.name.split(" ")[0]) for op in eng.bwd_ops]
    dil = ["conv5_1", "conv5_2", "conv5_3", "fc6"]
    assert [n for k, n in bk if k == "dconv_dgrad"] == dil[::-1]
    wg = {op.name: op for op in eng.bwd_ops if op.kind == "wgrad"}
    assert all(wg[n].layers == [n] and wg[n].sel is None for n in dil)
    assert eng.blobs["fc8_voc12"].shape == (2, 5, 26, 26) and eng.blobs["label"].shape == (2, 1, 26, 26)
    x = inputs_for(spec, 5)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=7)
    check_step(eng, spec, params, x, out, LF_BLOBS, 7, "largefov graph=%d" % graph)
    g1 = eng.download_grads()
    eng.step(seed=7)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k])), "the same step again: the same bits"
    now = eng.download_params()
    assert all(np.array_equal(a, b) for k in params for a, b in zip(now[k], params[k]))      # (base_lr 0)
    eng.close()


def test_aspp_forward(gpu):
    txt = models.deeplab_aspp("DEPLOY", batch=2, **ASPP)
    msg, spec = make(txt, "TEST")
    params = random_params(spec, 13)
    eng = Engine(NetSpec(msg, "TEST"), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0, autotune=False)
    heads = [op for op in eng.ops if op.kind == "dconv" and op.name.startswith("fc6_")]
    assert len(heads) == 1 and heads[0].name.startswith("fc6_1+fc6_2+fc6_3+fc6_4 [d2,4,6,8 "), "the four branches read pool5 in ONE launch"
    assert heads[0].flops == 4 * 2.0 * 2 * 18 * 18 * 64 * 128 * 9
    x = inputs_for(spec, 2)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    own = own_error(spec, params, x, ASPP_BLOBS)
    for name in ASPP_BLOBS:
        err = rel_err(eng.read_blob(name), ref[name].numpy())
        print("ASPP %s %.3g (torch float32: %.3g)" % (name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    assert out["fc8_voc12"].shape == (2, 5, 18, 18)
    eng.close()


def test_aspp_one_training_step(gpu, monkeypatch):
    spec, params, eng = _train_engine(monkeypatch, True, models.deeplab_aspp("TRAIN", batch=2, **ASPP), seed=4)
    bk = [(op.kind, op.name.split(" ")[0]) for op in eng.bwd_ops]
    assert sorted(n for k, n in bk if k == "dconv_dgrad") == ["conv5_1", "conv5_2", "conv5_3", "fc6_1", "fc6_2", "fc6_3", "fc6_4"]
    x = inputs_for(spec, 6)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=9)
    check_step(eng, spec, params, x, out, ASPP_BLOBS, 9, "aspp")
    eng.close()


FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
HAND = """
input: "data" input_shape { dim: 2 dim: 3 dim: 23 dim: 19 }
%s
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "atrous" type: "Convolution" bottom: "c0" top: "atrous" convolution_param { num_output: 8 kernel_size: 3 %s FILL } }
layer { name: "ra" type: "ReLU" bottom: "atrous" top: "atrous" }
%s
""".replace("FILL", FILL)


def hand(extra, train=None):
    if train is None:
        return HAND % ("", extra, "")
    return HAND % ('input: "target" input_shape { dim: 2 dim: 8 dim: %d dim: %d }' % train, extra,
                   'layer { name: "loss" type: "EuclideanLoss" bottom: "atrous" bottom: "target" top: "loss" }')


def test_dilated_stride_two_forward(gpu):
    msg, spec = make(hand("dilation: 3 pad: 2 stride: 2"), "TEST")
    assert spec.blob_shapes["atrous"] == (2, 8, 11, 9)                   # (23 + 4 - 7) // 2 + 1, (19 + 4 - 7) // 2 + 1
    params = fill_params(spec, seed=2)
    eng = Engine(NetSpec(msg, "TEST"), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0, autotune=False)
    assert [op.kind for op in eng.ops if op.name.startswith("atrous")] == ["dconv"]
    x = inputs_for(spec, 3)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    eng.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    for name in ("c0", "atrous"):
        assert rel_err(eng.read_blob(name), ref[name].numpy()) < 1e-4, name
    eng.close()


def _train(text):
    msg, spec = make(text, "TRAIN")
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    return TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params=fill_params(spec, seed=1), device=0, solver=sp, autotune=False)


def test_refusals_by_layer_name(gpu):
    msg, _ = make(hand("dilation: 2 pad: 2"), "TEST")
    with pytest.raises(NotImplementedError, match="f16 engine: Convolution atrous with dilation 2"):
        Engine(NetSpec(msg, "TEST"), device=0, autotune=False, dtype="f16")
    msg, _ = make(hand("dilation: 2 pad: 2 group: 2"), "TEST")
    with pytest.raises(NotImplementedError, match="Convolution atrous: group 2 together with dilation 2"):
        Engine(NetSpec(msg, "TEST"), device=0, autotune=False)
    with pytest.raises(NotImplementedError, match="dilated Convolution atrous: .*stride 2"):
        _train(hand("dilation: 2 pad: 2 stride: 2", train=(12, 10)))
    with pytest.raises(NotImplementedError, match="dilated Convolution atrous: .*pad 5 above"):
        _train(hand("dilation: 2 pad: 5", train=(29, 25)))
    with pytest.raises(NotImplementedError, match="layer atrous: dilation"):
        make(hand("dilation: 2 dilation: 3 pad: 2"), "TEST")
    _train(hand("dilation: 2 pad: 4", train=(27, 23))).close()          # pad == dil (k-1): the data gradient runs with pad' = 0
