"""Nets that end in ArgMax through caffe.Net and Engine, float32 and half-float, -m gpu, against the float64 reference
(tests/ref_argmax64.py).

Tiny nets: a 1 x 1 Convolution with weights near the identity over a map of regions with one dominant class each (the maps of
tests/argmax_cases.py), so that the float64 scores - computed here with numpy - are known on the CPU and a seed can be chosen there:
the first whose scores (blended, where the net has an Interp) keep NET_MARGIN = 2^-6 of the pixel's largest magnitude between rank 0
and rank 1 at EVERY pixel.  The half-float engine rounds the weights, the input and the convolution's result to halves, 2^-11
relative each on terms that sum to at most twice the largest score: 3 * 2^-10 of it per score, 3 * 2^-9 between two - under half the
margin; the unfused half path rounds the blend once more (2^-10 between two).  Labels must therefore be exact in both engines, fused and
unfused.  Probabilities are held to the project's net thresholds (1e-4 float32, 5e-3 half-float, relative).

The model nets (SegNet-Basic in both engines, DeepLab-LargeFOV with Interp in float32 - the half-float engine has no dilated
convolution -, width_div 8, edge 40 / 41) are deep: their scores are not known on the
CPU to better than the engines' own thresholds.  What is checked there is the new launch against its own input: the blob in front of
the fused chain is read from the engine, the float64 reference runs on exactly those values, and the labels must agree wherever -
which is everywhere, asserted - the reference's gap exceeds 2^-16 of the largest score (64 times the float32 blend's bound of
8 * 2^-24; the fused launch blends in float32 whatever it reads)."""
import sys

import numpy as np
import pytest

import argmax_cases as A
import ref_argmax64 as R
from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec
from fcn_object_detector_amd.train import SolverParams, TrainEngine

pytestmark = pytest.mark.gpu
F32 = np.float32
NET_MARGIN = 2.0 ** -6
C, H, W = 5, 3, 4
VALUE_TOL = {"f32": 1e-4, "f16": 5e-3}

HEAD = """
input: "data" input_shape { dim: 2 dim: %d dim: %d dim: %d }
layer { name: "score" type: "Convolution" bottom: "data" top: "score" convolution_param { num_output: %d kernel_size: 1 } }
""" % (C, H, W, C)
INTERP = 'layer { name: "up" type: "Interp" bottom: "score" top: "up" interp_param { zoom_factor: 3 } }\n'
SOFTMAX = 'layer { name: "prob" type: "Softmax" bottom: "%s" top: "prob" }\n'
ARGMAX = 'layer { name: "am" type: "ArgMax" bottom: "%s" top: "am" argmax_param { axis: 1 %s } }\n'


def conv_params(seed):
    rng = np.random.default_rng(seed)
    w = np.eye(C) + 0.1 * rng.standard_normal((C, C))
    return {"score": [w.reshape(C, C, 1, 1).astype(F32), (0.1 * rng.standard_normal(C)).astype(F32)]}


def scores64(params, x):
    w, b = (a.astype(np.float64) for a in params["score"])
    return np.einsum("oc,nchw->nohw", w[:, :, 0, 0], x.astype(np.float64)) + b.reshape(1, -1, 1, 1)


def margin_seed(interp, softmax):
    """(params, x, float64 blob in front of the ArgMax): the first seed that keeps NET_MARGIN at every pixel."""
    import ref_interp64 as RI
    for seed in range(4000):
        params = conv_params(seed)
        x = A._regions(np.random.default_rng(seed), 2, C, H, W).astype(F32)
        y = scores64(params, x)
        if interp:
            y = RI.interp(y, 3 * H - 2, 3 * W - 2)
        if R.margin(y, 1) >= NET_MARGIN and (not softmax or R.margin(R.softmax(y), 1) >= NET_MARGIN):
            return params, x, y
    raise AssertionError("no seed keeps the margin")


def engine(text, params, dtype, fuse=True, x=None):
    eng = Engine(NetSpec(proto.parse_text(text), "TEST"), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                 autotune=False, dtype=dtype, fuse=fuse)
    if x is not None:
        eng.host_array(eng.inputs[0])[...] = x
    return eng


def kinds(eng):
    return [(op.kind, op.name) for op in eng.ops if op.kind in ("interp", "softmax", "argmax")]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_conv_interp_argmax(gpu, dtype):
    params, x, y64 = margin_seed(True, False)
    text = HEAD + INTERP + ARGMAX % ("up", "")
    fused, plain = engine(text, params, dtype, True, x), engine(text, params, dtype, False, x)
    assert kinds(fused) == [("argmax", "up+am")] and kinds(plain) == [("interp", "up"), ("argmax", "am")]
    assert fused.blobs["am"].esize == 4 and fused.blobs["up"].esize == (2 if dtype == "f16" else 4)
    out = fused.forward()
    assert list(out) == ["am"] and out["am"].shape == (2, 1, 3 * H - 2, 3 * W - 2) and out["am"].dtype == F32
    labels = out["am"].copy()
    assert np.array_equal(labels, R.argmax(y64)), "labels against the float64 reference"
    assert np.array_equal(plain.forward()["am"], labels), "fused and unfused engines name the same classes"
    assert fused.forward()["am"].tobytes() == labels.tobytes(), "two forward() calls give the same bits"
    # the blob the fused launch skipped is filled on demand, with the layer's own launch
    assert fused.read_blob("up").tobytes() == plain.read_blob("up").tobytes()
    assert rel_err(fused.read_blob("up"), y64) < VALUE_TOL[dtype]
    rows = [r for r in fused.time_ops(3) if r[0] == "argmax"]
    assert len(rows) == 1 and rows[0][1] == "up+am" and rows[0][3] == 0.0 and rows[0][4] > 0, "the `caffe time` row"
    fused.close()
    plain.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_conv_softmax_argmax_values(gpu, dtype):
    params, x, y64 = margin_seed(False, True)
    text = HEAD + SOFTMAX % "score" + ARGMAX % ("prob", "out_max_val: true top_k: 2")
    fused, plain = engine(text, params, dtype, True, x), engine(text, params, dtype, False, x)
    assert kinds(fused) == [("argmax", "prob+am")] and kinds(plain) == [("softmax", "prob"), ("argmax", "am")]
    want = R.argmax(y64, 2, "values", probs=True)
    for eng in (fused, plain):
        got = eng.forward()["am"]
        assert got.shape == (2, 2, H, W) and rel_err(got, want) < VALUE_TOL[dtype]
    assert fused.read_blob("prob").tobytes() == plain.read_blob("prob").tobytes()
    fused.close()
    plain.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_softmax_that_is_also_an_output_keeps_its_launch(gpu, dtype, monkeypatch):
    params, x, y64 = margin_seed(False, True)
    text = HEAD + SOFTMAX % "score" + ARGMAX % ("prob", "")
    fused = engine(text, params, dtype, True, x)
    keep = NetSpec.output_blobs
    monkeypatch.setattr(NetSpec, "output_blobs", lambda self: ["prob"] + keep(self))      # a caller that wants the probabilities too
    both = engine(text, params, dtype, True, x)
    monkeypatch.setattr(NetSpec, "output_blobs", keep)
    assert kinds(fused) == [("argmax", "prob+am")] and kinds(both) == [("softmax", "prob"), ("argmax", "am")]
    out = both.forward()
    assert sorted(out) == ["am", "prob"] and rel_err(out["prob"], R.softmax(y64)) < VALUE_TOL[dtype]
    assert np.array_equal(out["am"], R.argmax(y64)) and np.array_equal(fused.forward()["am"], out["am"])
    fused.close()
    both.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_classifier_top_5_in_the_legacy_shape(gpu, dtype):
    """(N, C, 1, 1) scores -> prob -> ArgMax { top_k: 5 }: 300 classes, the wave-per-pixel side.  The convolution is the identity, so the
    scores are the margin case itself (rounded to halves by the half-float engine: the case is made of halves)."""
    n, c = 3, 300
    x = A.plain_margin(c, n, 5, True).astype(F32).reshape(c, n).T.reshape(n, c, 1, 1)
    params = {"score": [np.eye(c, dtype=F32).reshape(c, c, 1, 1), np.zeros(c, F32)]}
    text = ('input: "data" input_shape { dim: %d dim: %d dim: 1 dim: 1 }\n'
            'layer { name: "score" type: "Convolution" bottom: "data" top: "score" convolution_param { num_output: %d kernel_size: 1 } }\n'
            % (n, c, c) + SOFTMAX % "score")
    for param, shape in (("top_k: 5", (n, 1, 5)), ("top_k: 5 out_max_val: true", (n, 2, 5))):
        tail = 'layer { name: "am" type: "ArgMax" bottom: "prob" top: "am" argmax_param { %s } }\n' % param
        fused, plain = engine(text + tail, params, dtype, True, x), engine(text + tail, params, dtype, False, x)
        assert kinds(fused) == [("argmax", "prob+am")]
        want = R.argmax(x.astype(np.float64), 5, "pairs" if shape[1] == 2 else "legacy", probs=True)
        for eng in (fused, plain):
            got = eng.forward()["am"]
            assert got.shape == shape and np.array_equal(got[:, 0], want[:, 0]), "indices"
            assert eng.read_blob("am").shape == shape
            if shape[1] == 2:
                assert rel_err(got[:, 1], want[:, 1]) < VALUE_TOL[dtype]
        fused.close()
        plain.close()


def model_net(tmp_path, text, dtype, seed, random_params):
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    spec = NetSpec(proto.parse_text(text), "TEST")
    spec.infer()
    path, weights = str(tmp_path / "deploy.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(text)
    params = random_params(spec, seed)      # (BatchNorm statistics with a variance, as tests/test_gpu_segnet.py draws them)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST, dtype=dtype)
    net.blobs["data"].data[...] = np.random.default_rng(seed).standard_normal(spec.input_shapes["data"]).astype(F32)
    return net


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_segnet_basic_returns_the_label_map(gpu, tmp_path, monkeypatch, dtype):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    from torch_segnet_ref import random_params
    net = model_net(tmp_path, models.segnet_basic("DEPLOY", classes=4, size=40, width_div=8, argmax=True), dtype, 3, random_params)
    assert [op.name for op in net._engine.ops if op.kind == "argmax"] == ["prob+argmax"] and "softmax" not in [op.kind for op in net._engine.ops]
    out = net.forward()
    assert list(out) == ["argmax"] and out["argmax"].shape == (1, 1, 40, 40)
    x64 = net.blobs["conv_classifier"].data.astype(np.float64)
    assert R.margin(x64, 1) >= 2.0 ** -16
    assert np.array_equal(out["argmax"], R.argmax(x64)) and len(np.unique(out["argmax"])) > 1
    assert rel_err(net.blobs["prob"].data, R.softmax(x64)) < VALUE_TOL[dtype]      # (filled on demand)
    assert net.forward()["argmax"].tobytes() == out["argmax"].tobytes()
    net._engine.close()


def test_deeplab_largefov_returns_the_label_map(gpu, tmp_path, monkeypatch, dtype="f32"):
    """float32 only: the half-float engine refuses DeepLab's dilated convolutions by layer name (tests/test_gpu_dilated_nets.py); the
    half-float form of the fused launch runs in test_conv_interp_argmax above."""
    from torch_interp_ref import random_params
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.deeplab_largefov("DEPLOY", num_classes=5, width_div=8, fc_div=8, size=41, fc6_dilation=2, interp=True, argmax=True)
    net = model_net(tmp_path, txt, dtype, 5, random_params)
    assert [op.name for op in net._engine.ops if op.kind == "argmax"] == ["fc8_interp+argmax"] and "interp" not in [op.kind for op in net._engine.ops]
    out = net.forward()
    assert list(out) == ["argmax"] and out["argmax"].shape == (1, 1, 41, 41)
    x64 = net.blobs["fc8_voc12"].data.astype(np.float64)
    import ref_interp64 as RI
    y64 = RI.interp(x64, 41, 41)
    assert R.margin(y64, 1) >= 2.0 ** -16
    assert np.array_equal(out["argmax"], R.argmax(y64))
    assert rel_err(net.blobs["fc8_interp"].data, y64) < VALUE_TOL[dtype]
    assert net.forward()["argmax"].tobytes() == out["argmax"].tobytes()
    net._engine.close()


def test_a_train_net_with_an_argmax_beside_the_loss_takes_a_step(gpu):
    text = ('input: "label" input_shape { dim: 2 dim: 1 dim: %d dim: %d }\n' % (H, W) + HEAD +
            ARGMAX % ("score", "") + 'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "score" bottom: "label" top: "loss" }\n')
    params, x, y64 = margin_seed(False, False)
    msg = proto.parse_text(text)
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=SolverParams(base_lr=0.01, momentum=0.9), autotune=False)
    assert "argmax" in [op.kind for op in eng.ops]
    eng.host_array("data")[...] = x
    eng.host_array("label")[...] = np.random.default_rng(0).integers(0, C, (2, 1, H, W)).astype(F32)
    first = eng.step(seed=1)
    assert np.array_equal(eng.read_blob("am"), R.argmax(y64)), "the label map beside the loss"
    second = eng.step(seed=2)
    assert np.isfinite(first["total_loss"]) and second["total_loss"] < first["total_loss"], "the step moved the weights"
    eng.close()
