"""Transposed convolution through the public surface (-m gpu): `caffe.Net` forward of group-1 Deconvolution layers, TrainEngine
gradients of a net with strided convolutions and a learnable Deconvolution against float64 references, `caffe.SGDSolver` on that
net, and the untouched plans of the reference's own nets."""
import sys

import numpy as np
import pytest

import ref64
import ref_tconv64 as T
from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from oracle.net_ref import RefNet

pytestmark = pytest.mark.gpu

NEW_KINDS = {"tconv", "tconv_pack", "tconv_dgrad", "channel_sum"}

DEPLOY = """
name: "upsample"
input: "data"
input_shape { dim: 2 dim: 5 dim: 7 dim: 9 }
layer { name: "score" type: "Convolution" bottom: "data" top: "score"
  convolution_param { num_output: 6 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "up2" type: "Deconvolution" bottom: "score" top: "up2"
  convolution_param { num_output: 7 kernel_size: 4 stride: 2 pad: 1 weight_filler { type: "gaussian" std: 0.2 } bias_filler { type: "constant" value: -0.05 } } }
layer { name: "up2/relu" type: "ReLU" bottom: "up2" top: "up2" }
layer { name: "up8" type: "Deconvolution" bottom: "up2" top: "up8"
  convolution_param { num_output: 3 bias_term: false kernel_size: 16 stride: 8 pad: 4 weight_filler { type: "bilinear" } } }
"""

TRAIN = """
name: "strided"
input: "data"
input_shape { dim: 2 dim: 3 dim: 15 dim: 18 }
input: "target"
input_shape { dim: 2 dim: 4 dim: 8 dim: 8 }
layer { name: "c1" type: "Convolution" bottom: "data" top: "c1"
  convolution_param { num_output: 8 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "c1/relu" type: "ReLU" bottom: "c1" top: "c1" }
layer { name: "c2" type: "Convolution" bottom: "c1" top: "c2"
  convolution_param { num_output: 10 kernel_size: 3 stride: 2 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "c2/relu" type: "ReLU" bottom: "c2" top: "c2" }
layer { name: "c3" type: "Convolution" bottom: "c2" top: "c3"
  convolution_param { num_output: 6 kernel_size: 1 stride: 2 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.05 } } }
layer { name: "up" type: "Deconvolution" bottom: "c3" top: "up"
  convolution_param { num_output: 4 kernel_size: 4 stride: 2 pad: 1 weight_filler { type: "gaussian" std: 0.3 } bias_filler { type: "constant" value: 0.02 } } }
layer { name: "loss" type: "EuclideanLoss" bottom: "up" bottom: "target" top: "loss" }
"""
# data 15 x 18 -> c1 15 x 18 -> c2 (k3 s2 p0) 7 x 8: (18 - 3) % 2 = 1, the last column of c1 is under no window
#              -> c3 (k1 s2) 4 x 4: (8 - 1) % 2 = 1 and only every other pixel of c2 is read -> up (k4 s2 p1) 8 x 8


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def test_group1_deconvolution_forward_through_caffe_net(gpu, tmp_path):
    caffe = _caffe()
    path = str(tmp_path / "deploy.prototxt")
    open(path, "w").write(DEPLOY)
    msg = proto.parse_file(path)
    spec = NetSpec(msg, "TEST")
    spec.infer()
    assert spec.param_shapes["up2"] == [(6, 7, 4, 4), (7,)] and spec.param_shapes["up8"] == [(7, 3, 16, 16)]
    params = fill_params(spec, seed=3)
    rng = np.random.default_rng(1)
    params["up8"][0] = (params["up8"][0] * rng.uniform(0.5, 1.5, params["up8"][0].shape)).astype(np.float32)      # (not the same filter 21 times)
    weights = str(tmp_path / "w.caffemodel")
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST)
    x = rng.standard_normal((2, 5, 7, 9)).astype(np.float32)
    net.blobs["data"].data[...] = x
    out = net.forward()
    ref = RefNet(msg, "TEST", params)
    ref.blobs["data"] = x
    rb = ref.forward()
    assert out["up8"].shape == (2, 3, 112, 144)
    for name in ("up2", "up8"):
        assert rel_err(net.blobs[name].data, rb[name]) < 1e-4, name
    # the blobs round-trip at Caffe's shape (Cin, Cout, kh, kw), through net.params and through a written .caffemodel
    for name in ("up2", "up8"):
        assert net.params[name][0].data.shape == params[name][0].shape and np.array_equal(net.params[name][0].data, params[name][0])
    assert np.array_equal(net.params["up2"][1].data, params["up2"][1])
    saved = str(tmp_path / "saved.caffemodel")
    net.save(saved)
    back = proto.read_caffemodel(saved)
    assert back["up8"][0].shape == (7, 3, 16, 16) and np.array_equal(back["up2"][0], params["up2"][0])


def test_other_groupings_stay_refused_by_name(gpu):
    txt = DEPLOY.replace("num_output: 7 kernel_size: 4", "num_output: 6 group: 2 kernel_size: 4")
    msg = proto.parse_text(txt)
    from fcn_object_detector_amd.engine import Engine
    spec = NetSpec(msg, "TEST")
    spec.infer()
    with pytest.raises(NotImplementedError, match="up2"):
        Engine(NetSpec(msg, "TEST"), params=fill_params(spec, seed=0), device=0, autotune=False)


def _train_setup(lr=0.0):
    msg = proto.parse_text(TRAIN)
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    shapes = dict(spec.input_shapes)
    params = fill_params(spec, seed=5)
    rng = np.random.default_rng(2)
    data = {"data": rng.standard_normal(shapes["data"]).astype(np.float32), "target": rng.standard_normal(shapes["target"]).astype(np.float32)}
    sp = SolverParams(base_lr=lr, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), shapes, params={k: [a.copy() for a in v] for k, v in params.items()}, device=0, solver=sp,
                      autotune=False)
    return msg, spec, params, data, eng


def _forward64(params, data, relu_from=None):
    """float64 forward of TRAIN; returns every blob (post-ReLU where the prototxt has one) and the loss."""
    P = {k: [np.asarray(a, np.float64) for a in v] for k, v in params.items()}
    c1 = np.maximum(ref64.conv2d(data["data"], P["c1"][0], P["c1"][1], 1, 1), 0)
    c2 = np.maximum(ref64.conv2d(c1, P["c2"][0], P["c2"][1], 0, 2), 0)
    c3 = ref64.conv2d(c2, P["c3"][0], P["c3"][1], 0, 2)
    up = T.tconv2d(c3, P["up"][0], P["up"][1], 1, 2)
    diff = up - np.asarray(data["target"], np.float64)
    return dict(c1=c1, c2=c2, c3=c3, up=up), float((diff ** 2).sum() / (2 * diff.shape[0]))


def test_train_engine_gradients_of_strided_convs_and_learnable_deconv(gpu):
    msg, spec, params, data, eng = _train_setup()
    kinds = [op.kind for op in eng.bwd_ops]
    assert kinds.count("tconv_dgrad") == 2 and kinds.count("tconv_pack") == 2 and "channel_sum" in kinds, kinds
    assert "tconv" in [op.kind for op in eng.ops]
    for k, v in data.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=1)
    blobs, loss = _forward64(params, data)
    assert abs(out["loss"] - loss) < 1e-4 * abs(loss)
    for name in ("c2", "c3", "up"):
        assert rel_err(eng.read_blob(name), blobs[name]) < 1e-4, name
    # float64 backward on the DEVICE's ReLU masks (tests/test_gpu_train.py explains why)
    c1d, c2d = eng.read_blob("c1"), eng.read_blob("c2")
    P = {k: [np.asarray(a, np.float64) for a in v] for k, v in params.items()}
    n = data["data"].shape[0]
    d_up = (blobs["up"] - data["target"]) / n
    want = {}
    # Deconvolution: dX = conv(dY, blob), dW[ci, co] = wgrad with the roles swapped, db = sum dY
    d_c3 = ref64.conv2d(d_up, P["up"][0], None, 1, 2)
    dw_up, _ = ref64.conv2d_wgrad(d_up, blobs["c3"], 4, 1, 2)
    want["up"] = [dw_up, d_up.sum(axis=(0, 2, 3))]
    want["c3"] = list(ref64.conv2d_wgrad(blobs["c2"], d_c3, 1, 0, 2))
    d_c2 = T.tconv2d(d_c3, P["c3"][0], None, 0, 2, blobs["c2"].shape[2:]) * (c2d > 0)
    assert np.all(d_c2[:, :, 1::2, :] == 0) and np.all(d_c2[:, :, :, 1::2] == 0)
    want["c2"] = list(ref64.conv2d_wgrad(blobs["c1"], d_c2, 3, 0, 2))
    d_c1 = T.tconv2d(d_c2, P["c2"][0], None, 0, 2, blobs["c1"].shape[2:]) * (c1d > 0)
    assert np.all(d_c1[:, :, :, -1] == 0)                      # the column under no window
    want["c1"] = list(ref64.conv2d_wgrad(data["data"], d_c1, 3, 1, 1))
    for name, d in (("up", d_up), ("c3", d_c3), ("c2", d_c2), ("c1", d_c1)):
        assert rel_err(eng.read_grad(name), d) < 1e-4, "gradient of blob " + name
    got = eng.download_grads()
    for name, gs in want.items():
        for g, r in zip(got[name], gs):
            assert g.shape == r.shape, name
            assert rel_err(g, r) < 2e-4, "parameter gradient of " + name
    # one central-difference probe per parameter blob (float64 forward; the largest-gradient entry, away from ReLU kinks by its size)
    for name in ("c1", "c2", "c3", "up"):
        for bi in range(2):
            g = want[name][bi]
            at = np.unravel_index(int(np.argmax(np.abs(g))), g.shape)
            h = 1e-4
            lo, hi = ({k: [a.astype(np.float64).copy() for a in v] for k, v in params.items()} for _ in range(2))
            lo[name][bi][at] -= h
            hi[name][bi][at] += h
            num = (_forward64(hi, data)[1] - _forward64(lo, data)[1]) / (2 * h)
            assert abs(num - got[name][bi][at]) < 2e-3 * max(abs(num), 1e-3), (name, bi, num, got[name][bi][at])
    # the same step again: the same bits
    g1 = eng.download_grads()
    eng.step(seed=1)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k]))
    eng.close()


def test_frozen_group1_deconvolution_needs_only_the_data_gradient(gpu):
    txt = TRAIN.replace('bottom: "c3" top: "up"', 'bottom: "c3" top: "up" param { lr_mult: 0 } param { lr_mult: 0 }')
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params=fill_params(spec, seed=5), device=0, solver=sp, autotune=False)
    kinds = [op.kind for op in eng.bwd_ops]
    assert "channel_sum" not in kinds and not any(op.kind == "wgrad" and op.name.startswith("up") for op in eng.bwd_ops)
    assert any(op.kind == "dgrad" and op.name.startswith("up") for op in eng.bwd_ops)
    eng.close()


def _write_job(tmp_path):
    net = tmp_path / "train_val.prototxt"
    net.write_text(TRAIN)
    solver = tmp_path / "solver.prototxt"
    solver.write_text('net: "%s"\nbase_lr: 0.002\nmomentum: 0.9\nweight_decay: 1e-5\nlr_policy: "fixed"\ndisplay: 0\nmax_iter: 100\n'
                      'snapshot: 0\nsnapshot_prefix: "%s"\n' % (net, tmp_path / "snap"))
    return str(solver)


def test_sgd_solver_learns_snapshots_and_restores(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 3, 15, 18)).astype(np.float32)
    y = rng.standard_normal((2, 4, 8, 8)).astype(np.float32) * 0.5

    def make():
        s = caffe.SGDSolver(_write_job(tmp_path), log=None, autotune=False)
        s.engine.host_array("data")[...] = x
        s.engine.host_array("target")[...] = y
        return s
    a = make()
    w0 = a.engine.download_params()["up"][0].copy()
    losses = [a.step(1)["loss"] for _ in range(20)]
    assert losses[-1] < 0.8 * losses[0] and all(np.isfinite(losses)), losses
    assert not np.array_equal(a.engine.download_params()["up"][0], w0)             # the deconvolution learns
    a.snapshot()
    back = proto.read_caffemodel(str(tmp_path / "snap_iter_20.caffemodel"))
    assert back["up"][0].shape == (6, 4, 4, 4) and back["up"][1].shape == (4,)
    assert np.array_equal(back["up"][0], a.engine.download_params()["up"][0])
    b = make()
    b.restore(str(tmp_path / "snap_iter_20.solverstate"))
    assert b.iter == 20
    la, lb = [a.step(1)["loss"] for _ in range(2)], [b.step(1)["loss"] for _ in range(2)]
    assert la == lb
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    a.close()
    b.close()


def _reference_train_net(which):
    """(prototxt, input shapes) of the reference's training nets at reduced size, as tests/test_gpu_train.py / test_gpu_vgg.py build them."""
    if which == "googlenet_detectnet_train":
        g = (2, 6, 8)
        return models.googlenet_detectnet_train("m", "L", "unused", num_classes=1), {
            "data": (2, 3, 96, 128), "coverage-label": (g[0], 1) + g[1:], "bbox-label": (g[0], 4) + g[1:], "size-block": (g[0], 4) + g[1:],
            "obj-block": (g[0], 4) + g[1:], "coverage-block": (g[0], 4) + g[1:]}
    classes, n, size = 2, 2, 64
    blk = (n, 4 * classes, size // 8, size // 8)
    shapes = {"data": (n, 3, size, size), "bbox-label": blk, "size-block": blk, "obj-block": blk, "coverage-block": blk}
    if which == "fcn_bbox":
        shapes["label"] = (n, 1, size, size)
        return models.vgg16_fcn_bbox_train("m", "L", "unused", num_classes=classes), shapes
    shapes["coverage-label"] = (n, classes, size // 8, size // 8)
    return models.vgg16_bounding_box_train("m", "L", "unused", num_classes=classes), shapes


@pytest.mark.parametrize("which", ["googlenet_detectnet_train", "fcn_bbox", "bounding_box"])
def test_plans_of_the_reference_nets_are_untouched(gpu, which):
    from fcn_object_detector_amd.netspec import kernel_stride_pad
    txt, shapes = _reference_train_net(which)
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TRAIN")
    spec.infer(shapes)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), shapes, params=fill_params(spec, seed=0), device=0, solver=sp, autotune=False)
    assert not NEW_KINDS & {op.kind for op in eng.ops} and not NEW_KINDS & {op.kind for op in eng.bwd_ops}
    n_deconv = sum(1 for l in spec.layers if l.type == "Deconvolution")
    assert sum(op.kind == "deconv" for op in eng.ops) == n_deconv
    assert sum(op.kind == "deconv_bwd" for op in eng.bwd_ops) == sum(
        1 for l in spec.layers if l.type == "Deconvolution" and l.tops[0] in eng.grad_blobs and l.bottoms[0] in eng.grad_blobs)
    need = [l for l in spec.layers if l.type == "Convolution" and l.bottoms[0] in eng.grad_blobs and l.tops[0] in eng.grad_blobs]
    assert need and all(kernel_stride_pad(l.sub("convolution_param"))[1] == 1 for l in need)      # no strided layer below a learning one
    flips = [op for op in eng.bwd_ops if op.kind == "flip"]
    assert len(flips) == 1 and flips[0].name == "%d filter banks" % len(need)
    eng.close()
