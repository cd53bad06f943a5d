"""The published FCN-32s / 16s / 8s structure (models.voc_fcn*) through the public surface, -m gpu: `caffe.Net` forward, TrainEngine
loss and parameter gradients, `caffe.SGDSolver`, the half-float engine with a Crop between half blobs - against torch on the CPU in
float64 (conv2d, max_pool2d(ceil_mode=True), conv_transpose2d, slicing, cross_entropy) - and the untouched plans of the reference's nets.
The builders' fillers are on (fillers=True): the published files initialise their score layers with zeros, which would make parity
vacuous."""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine, dropout_layer_salt
from fcn_object_detector_amd.netspec import NetSpec, bilinear_kernel, crop_window, fill_params, kernel_stride_pad
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from oracle import caffe_ref as R
from test_gpu_tconv_net import _reference_train_net

pytestmark = pytest.mark.gpu
BUILDERS = {32: models.voc_fcn32s, 16: models.voc_fcn16s, 8: models.voc_fcn8s}
SMALL = dict(num_classes=5, width_div=16, fc_div=128, fillers=True)      # VGG widths 4 .. 32, fc6 / fc7 32


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def torch_net(spec, params, inputs, dropout_seed=None):
    """float64 forward of a NetSpec on the CPU.  params: {layer: [torch tensors]} (leaves when gradients are wanted).  TRAIN-phase Dropout
    takes the device's counter-based mask (oracle.caffe_ref.dropout_mask).  Returns every blob."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in inputs.items()}
    for l in spec.layers:
        t = l.type
        if t in ("Input", "Python", "Data"):
            continue
        x = B[l.bottoms[0]]
        if t in ("Convolution", "Deconvolution"):
            p = l.sub("convolution_param")
            k, s, pad = kernel_stride_pad(p)
            w, b = params[l.name][0], (params[l.name][1] if len(params[l.name]) > 1 else None)
            if t == "Convolution":
                y = F.conv2d(x, w, b, stride=s, padding=pad)
            else:
                y = F.conv_transpose2d(x, w, b, stride=s, padding=pad, groups=int(p.get("group", 1)))
        elif t == "ReLU":
            y = torch.relu(x)
        elif t == "Pooling":
            k, s, pad = kernel_stride_pad(l.sub("pooling_param"))
            y = F.max_pool2d(x, k, s, pad, ceil_mode=True)
        elif t == "Dropout":
            if spec.phase == "TEST":
                y = x
            else:
                ratio = float(l.sub("dropout_param").get("dropout_ratio", 0.5))
                seed = (dropout_seed + dropout_layer_salt(spec, l)) & 0xFFFFFFFF      # every Dropout layer draws its own mask
                y = x * torch.as_tensor(R.dropout_mask(tuple(x.shape), ratio, seed).astype(np.float64)) / (1.0 - ratio)
        elif t == "Crop":
            _, (_, oc, oy, ox) = crop_window(l, tuple(x.shape), tuple(B[l.bottoms[1]].shape))
            _, c, h, w = spec.blob_shapes[l.tops[0]]
            y = x[:, oc:oc + c, oy:oy + h, ox:ox + w]
        elif t == "Eltwise":
            y = x + B[l.bottoms[1]]
        elif t == "Sigmoid":
            y = torch.sigmoid(x)
        elif t == "EuclideanLoss":
            y = ((x - B[l.bottoms[1]]) ** 2).sum() / (2 * x.shape[0])
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
        elif t == "SoftmaxWithLoss":
            lab = B[l.bottoms[1]][:, 0].long()
            y = F.cross_entropy(x, lab, ignore_index=255, reduction="sum") / x.shape[0]
        else:
            raise NotImplementedError(t)
        B[l.tops[0]] = y
    return B


def as_torch(params, grad=False):
    return {k: [torch.tensor(np.asarray(a, np.float64), requires_grad=grad) for a in v] for k, v in params.items()}


def shaken(params, seed):
    """The bilinear filler writes the same filter for every channel pair: scale each entry so that a transposed or permuted bank shows."""
    rng = np.random.default_rng(seed)
    return {k: [(a * rng.uniform(0.5, 1.5, a.shape)).astype(np.float32) for a in v] for k, v in params.items()}


@pytest.mark.parametrize("variant", [32, 16, 8])
def test_deploy_forward_through_caffe_net(gpu, tmp_path, variant):
    caffe = _caffe()
    path = str(tmp_path / "deploy.prototxt")
    open(path, "w").write(BUILDERS[variant]("TEST", shape=(2, 3, 64, 48), **SMALL))
    msg = proto.parse_file(path)
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = shaken(fill_params(spec, seed=variant), variant)
    weights = str(tmp_path / "w.caffemodel")
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST)      # (the autotuner walks the tile configurations of conv1_1's pad 100 here)
    assert net.outputs == ["score"] and "data" not in net.outputs
    kinds = [op.kind for op in net._engine.ops]
    assert kinds.count("crop") == {32: 1, 16: 2, 8: 3}[variant]
    x = np.random.default_rng(1).standard_normal((2, 3, 64, 48)).astype(np.float32)
    net.blobs["data"].data[...] = x
    out = net.forward()
    ref = torch_net(spec, as_torch(params), {"data": x})
    assert out["score"].shape == (2, 5, 64, 48)
    names = ["conv1_1", "pool1", "pool3", "pool5", "fc6", "score_fr", "score"] + {32: ["upscore"], 16: ["upscore2", "score_pool4c", "fuse_pool4", "upscore16"],
                                                                                8: ["score_pool4c", "score_pool3c", "fuse_pool3", "upscore8"]}[variant]
    for name in names:
        assert tuple(net.blobs[name].data.shape) == tuple(ref[name].shape), name
        assert rel_err(net.blobs[name].data, ref[name].numpy()) < 1e-4, name
    assert np.array_equal(out["score"], net.blobs["score"].data)
    # a Crop is a copy: bit-equal to the window of its input as the device holds it
    up = {32: "upscore", 16: "upscore16", 8: "upscore8"}[variant]
    off = {32: 19, 16: 27, 8: 31}[variant]
    assert np.array_equal(net.blobs["score"].data, net.blobs[up].data[:, :, off:off + 64, off:off + 48])


def _train_engine(monkeypatch, variant, graph):
    monkeypatch.setenv("FCN_NO_GRAPH", "0" if graph else "1")
    msg = proto.parse_text(BUILDERS[variant]("TRAIN", shape=(2, 3, 64, 48), **SMALL))
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    params = shaken(fill_params(spec, seed=3), 4)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    return spec, params, eng


# what each variant crops: (cropped blob, Crop top, offset)
CROPS = {32: [("upscore", "score", 19)], 16: [("score_pool4", "score_pool4c", 5), ("upscore16", "score", 27)],
         8: [("score_pool3", "score_pool3c", 9), ("score_pool4", "score_pool4c", 5), ("upscore8", "score", 31)]}


@pytest.mark.parametrize("variant,graph", [(8, True), (8, False), (16, True), (32, True)], ids=["8s-graph", "8s-no_graph", "16s", "32s"])
def test_loss_and_parameter_gradients(gpu, monkeypatch, variant, graph):
    """One training step of the width-reduced net.  The data gradient of a group-1 Deconvolution is a forward convolution of dY with the
    layer's kernel and stride: k64 / s32 (4096 taps) in FCN-32s, k32 / s16 in FCN-16s, k16 / s8 in FCN-8s."""
    spec, params, eng = _train_engine(monkeypatch, variant, graph)
    bk = [(op.kind, op.name) for op in eng.bwd_ops]
    assert sorted(n for k, n in bk if k == "crop_bwd") == sorted(top for _, top, _ in CROPS[variant])
    ups = [l.name for l in spec.layers if l.type == "Deconvolution"]
    assert all(any(k == "dgrad" and n.startswith(u) for k, n in bk) for u in ups), bk      # every upsampling layer passes its gradient down
    assert [dropout_layer_salt(spec, l) for l in spec.layers if l.type == "Dropout"] == [0, 1 << 28]
    assert "data" not in eng.grad_blobs and "label" not in eng.grad_blobs      # the shape donor of `score` gets no gradient blob
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3, 64, 48)).astype(np.float32)
    lab = rng.integers(0, 5, (2, 1, 64, 48)).astype(np.float32)
    lab[rng.random(lab.shape) < 0.1] = 255
    eng.host_array("data")[...] = x
    eng.host_array("label")[...] = lab
    out = eng.step(seed=7)
    P = as_torch(params, grad=True)
    ref = torch_net(spec, P, {"data": x, "label": lab}, dropout_seed=7)
    loss = ref["loss"]
    loss.backward()
    want = float(loss.detach())
    assert abs(out["loss"] - want) < 1e-4 * abs(want), (out["loss"], want)
    for name in ["fc6", "fc7", "score_fr", "score"] + [n for pair in CROPS[variant] for n in pair[:2]]:
        assert rel_err(eng.read_blob(name), ref[name].detach().numpy()) < 1e-4, name
    # drop6 and drop7 drop different units although fc6 and fc7 have one shape
    z6, z7 = eng.read_blob("fc6") == 0, eng.read_blob("fc7") == 0
    assert 0.3 < z6.mean() < 0.95 and not np.array_equal(z6, z7)
    # the gradient of a cropped blob: dY inside the window, exact zeros outside
    for name, top, off in CROPS[variant]:
        gx, gy = eng.read_grad(name), eng.read_grad(top)
        h, w = gy.shape[2:]
        assert np.array_equal(gx[:, :, off:off + h, off:off + w], gy), name
        mask = np.ones(gx.shape, bool)
        mask[:, :, off:off + h, off:off + w] = False
        assert np.all(gx[mask] == 0), name
    got = eng.download_grads()
    learn = [l for l in spec.param_layers() if eng._learns(l)]
    assert {"conv1_1", "fc6", "fc7", "score_fr"} <= {l.name for l in learn} and not set(ups) & {l.name for l in learn}
    for l in learn:
        for g, r in zip(got[l.name], P[l.name]):
            assert g.shape == tuple(r.grad.shape), l.name
            assert rel_err(g, r.grad.numpy()) < 5e-4, "parameter gradient of " + l.name
    g1 = eng.download_grads()
    eng.step(seed=7)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k]))      # the same step again: the same bits
    eng.close()


FANIN = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 14 }
input: "small" input_shape { dim: 2 dim: 1 dim: 6 dim: 7 }
input: "label" input_shape { dim: 2 dim: 1 dim: 6 dim: 7 }
layer { name: "c" type: "Convolution" bottom: "data" top: "c"
  convolution_param { num_output: 6 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "a" type: "Crop" bottom: "c" bottom: "small" top: "a" crop_param { offset: 1 offset: 2 } }
layer { name: "b" type: "Crop" bottom: "c" bottom: "small" top: "b" crop_param { offset: 5 offset: 6 } }
layer { name: "sum" type: "Eltwise" bottom: "a" bottom: "b" top: "sum" eltwise_param { operation: SUM } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "sum" bottom: "label" top: "loss" loss_param { normalize: false } }
"""


def test_two_crops_of_one_blob_accumulate(gpu):
    """Gradient fan-in: the second crop_bwd into dC adds inside its window and leaves the first one's result alone elsewhere."""
    msg = proto.parse_text(FANIN)
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    params = fill_params(spec, seed=1)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    assert [op.kind for op in eng.bwd_ops].count("crop_bwd") == 2 and "small" not in eng.grad_blobs
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 3, 12, 14)).astype(np.float32)
    lab = rng.integers(0, 6, (2, 1, 6, 7)).astype(np.float32)
    eng.host_array("data")[...] = x
    eng.host_array("label")[...] = lab
    out = eng.step(seed=1)
    P = as_torch(params, grad=True)
    ref = torch_net(spec, P, {"data": x, "label": lab, "small": np.zeros((2, 1, 6, 7))})
    ref["c"].retain_grad()
    ref["loss"].backward()
    assert abs(out["loss"] - float(ref["loss"].detach())) < 1e-4 * abs(float(ref["loss"].detach()))
    assert rel_err(eng.read_grad("c"), ref["c"].grad.numpy()) < 1e-5
    gs = eng.read_grad("sum")
    want = np.zeros((2, 6, 12, 14), np.float32)
    want[:, :, 5:11, 6:13] = gs                  # reverse layer order: b first (plain), then a (accumulating)
    want[:, :, 1:7, 2:9] += gs
    assert np.array_equal(eng.read_grad("c"), want)
    got = eng.download_grads()
    for g, r in zip(got["c"], P["c"]):
        assert rel_err(g, r.grad.numpy()) < 2e-4
    eng.close()


def test_full_width_fcn32s_forward(gpu):
    msg = proto.parse_text(models.voc_fcn32s("TEST", shape=(1, 3, 64, 48), fillers=True))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    assert spec.param_shapes["fc6"][0] == (4096, 512, 7, 7)
    params = fill_params(spec, seed=2)
    eng = Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False)
    x = np.random.default_rng(3).standard_normal((1, 3, 64, 48)).astype(np.float32)
    eng.host_array("data")[...] = x
    out = eng.forward()
    got = {n: eng.read_blob(n).copy() for n in ("conv1_1", "pool5", "fc6", "fc7", "score_fr", "upscore")}
    eng.close()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), {"data": x})
    assert out["score"].shape == (1, 21, 64, 48) and ref["upscore"].shape[2:] == (128, 96)
    for name, g in got.items():
        assert rel_err(g, ref[name].numpy()) < 2e-4, name
    assert rel_err(out["score"], ref["score"].numpy()) < 2e-4


def _write_job(tmp_path):
    net = tmp_path / "train.prototxt"
    net.write_text(models.voc_fcn8s("TRAIN", shape=(2, 3, 64, 48), **SMALL))
    solver = tmp_path / "solver.prototxt"
    solver.write_text('net: "%s"\nbase_lr: 2e-6\nmomentum: 0.9\nweight_decay: 1e-5\nlr_policy: "fixed"\ndisplay: 0\nmax_iter: 100\n'
                      'snapshot: 0\nsnapshot_prefix: "%s"\n' % (net, tmp_path / "snap"))
    return str(solver)


def test_sgd_solver_learns_snapshots_and_restores(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 3, 64, 48)).astype(np.float32)
    lab = np.zeros((2, 1, 64, 48), np.float32)
    lab[:, :, 20:50, 10:30] = 3
    lab[:, :, :4] = 255

    # the published initialisation of the upsampling layers (net surgery): bilinear interpolation per class, nothing across classes -
    # the bilinear FILLER writes the same filter for every pair of classes, which makes all scores equal
    msg = proto.parse_text(models.voc_fcn8s("TRAIN", shape=(2, 3, 64, 48), **SMALL))
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    params = fill_params(spec, seed=0)
    for l in spec.param_layers():
        if l.type == "Deconvolution":
            w = params[l.name][0]
            w[...] = 0
            for i in range(w.shape[0]):
                w[i, i] = bilinear_kernel(w.shape[2])
    weights = str(tmp_path / "init.caffemodel")
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])

    def make():
        s = caffe.SGDSolver(_write_job(tmp_path), log=None, autotune=False)
        s.net.copy_from(weights)
        s.engine.host_array("data")[...] = x
        s.engine.host_array("label")[...] = lab
        return s
    a = make()
    losses = [a.step(1)["loss"] for _ in range(12)]
    assert all(np.isfinite(losses)) and losses[-1] < 0.8 * losses[0], losses
    assert tuple(a.net.blobs["score"].data.shape) == (2, 5, 64, 48) and tuple(a.net.blobs["data"].data.shape[2:]) == (64, 48)
    a.snapshot()
    b = make()
    b.restore(str(tmp_path / "snap_iter_12.solverstate"))
    assert b.iter == 12
    la, lb = [a.step(1)["loss"] for _ in range(2)], [b.step(1)["loss"] for _ in range(2)]
    assert la == lb
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    a.close()
    b.close()


HALF = """
input: "data" input_shape { dim: 2 dim: 3 dim: 32 dim: 40 }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1"
  convolution_param { num_output: 16 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
layer { name: "pool1" type: "Pooling" bottom: "conv1" top: "pool1" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
layer { name: "score_fr" type: "Convolution" bottom: "pool1" top: "score_fr"
  convolution_param { num_output: 5 kernel_size: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "up" type: "Deconvolution" bottom: "score_fr" top: "up" param { lr_mult: 0 }
  convolution_param { num_output: 5 group: 5 bias_term: false kernel_size: 4 stride: 2 weight_filler { type: "bilinear" } } }
layer { name: "score" type: "Crop" bottom: "up" bottom: "data" top: "score" crop_param { axis: 2 offset: 1 } }
layer { name: "prob" type: "Softmax" bottom: "score" top: "prob" }
"""


def test_half_float_engine_crops_half_blobs(gpu):
    msg = proto.parse_text(HALF)
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=6)
    x = np.random.default_rng(8).random((2, 3, 32, 40), dtype=np.float32)
    outs = {}
    for dt in ("f32", "f16"):
        eng = Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False, dtype=dt)
        assert [op.kind for op in eng.ops].count("crop") == 1 and eng.outputs == ["prob"]
        if dt == "f16":
            assert eng.blobs["up"].esize == 2 and eng.blobs["score"].esize == 2 and eng.blobs["prob"].esize == 4
        eng.host_array("data")[...] = x
        outs[dt] = (eng.forward()["prob"].copy(), eng.read_blob("score").copy(), eng.read_blob("up").copy())
        eng.close()
    assert outs["f16"][0].shape == (2, 5, 32, 40)
    assert rel_err(outs["f16"][0], outs["f32"][0]) < 5e-3 and rel_err(outs["f16"][1], outs["f32"][1]) < 5e-3
    assert np.array_equal(outs["f16"][1], outs["f16"][2][:, :, 1:33, 1:41])      # the half Crop is a copy too


MIXED = """
input: "data" input_shape { dim: 1 dim: 5 dim: 8 dim: 9 }
input: "small" input_shape { dim: 1 dim: 5 dim: 6 dim: 7 }
layer { name: "cut" type: "Crop" bottom: "data" bottom: "small" top: "window" crop_param { offset: 1 } }
layer { name: "prob" type: "Softmax" bottom: "window" top: "prob" }
"""


def test_half_float_engine_refuses_a_mixed_crop_by_layer_name(gpu):
    """`data` is a float32 input, `window` a half blob (Softmax reads it): the Crop layer itself refuses, naming the layer `cut`."""
    with pytest.raises(NotImplementedError, match="Crop cut copies between half and float32"):
        Engine(NetSpec(proto.parse_text(MIXED), "TEST"), params={}, device=0, autotune=False, dtype="f16")
    eng = Engine(NetSpec(proto.parse_text(MIXED), "TEST"), params={}, device=0, autotune=False)      # the float32 engine takes it
    x = np.random.default_rng(0).standard_normal((1, 5, 8, 9)).astype(np.float32)
    eng.host_array("data")[...] = x
    eng.forward()
    assert np.array_equal(eng.read_blob("window"), x[:, :, 1:7, 1:8])
    eng.close()


@pytest.mark.parametrize("which", ["googlenet_detectnet_train", "fcn_bbox", "bounding_box"])
def test_plans_of_the_reference_nets_hold_no_crop(gpu, which):
    txt, shapes = _reference_train_net(which)
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TRAIN")
    spec.infer(shapes)
    assert not any(l.type == "Crop" for l in spec.layers)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), shapes, params=fill_params(spec, seed=0), device=0, solver=sp, autotune=False)
    kinds, bkinds = [op.kind for op in eng.ops], [op.kind for op in eng.bwd_ops]
    assert "crop" not in kinds and "crop_bwd" not in bkinds
    # otherwise as before
    n_deconv = sum(1 for l in spec.layers if l.type == "Deconvolution")
    assert kinds.count("deconv") == n_deconv and kinds.count("loss") == sum(1 for l in spec.layers if l.type.endswith("Loss"))
    assert bkinds.count("flip") == 1 and bkinds.count("maxpool_bwd") == sum(
        1 for l in spec.layers if l.type == "Pooling" and l.tops[0] in eng.grad_blobs and l.bottoms[0] in eng.grad_blobs)
    eng.close()
