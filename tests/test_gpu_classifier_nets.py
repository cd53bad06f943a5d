"""CaffeNet, the GOTURN tracker and BVLC GoogLeNet (models.caffenet / goturn_tracker / bvlc_googlenet) through the public surface, -m gpu:
`caffe.Net` forward in the float32 and the half-float engine, one TrainEngine step (InnerProduct backward, grouped Convolution,
AVE-pooling backward), `caffe.SGDSolver`, the `caffe` tool - against torch on the CPU in float64 (tests/torch_classifier_ref.py) at the
thresholds of tests/test_gpu_fcn_published.py: rel_err < 1e-4 for blobs and the loss, < 5e-4 for parameter gradients; the half-float
engine at tests/test_gpu_f16_vgg.py's 5e-3 against the reference rounded where the engine rounds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PYCAFFE, ROOT, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_classifier_ref import as_torch, random_params, torch_net

pytestmark = pytest.mark.gpu
CAFFE = os.path.join(ROOT, "fcn_object_detector_amd", "caffe_tool.py")

# width_div 2 keeps every group of CaffeNet's conv2 / conv4 / conv5 at whole 16-byte segments of floats AND halves (24 / 96 / 96 input and
# 64 / 96 / 64 output channels per group); GoogLeNet at width_div 4 keeps every inception member a multiple of 4 channels (Concat members
# are written in place), the half-float case takes width_div 2: its pooling kernels want multiples of 8
NETS = {
    "caffenet": (models.caffenet, dict(batch=2, num_classes=10, width_div=2, fc_div=32, size=99)),
    "goturn": (models.goturn_tracker, dict(batch=2, width_div=2, fc_div=32, size=99)),
    "googlenet": (models.bvlc_googlenet, dict(batch=2, num_classes=10, width_div=4, fc_div=16, size=224)),
}
INTERIOR = {
    "caffenet": ["conv1", "norm1", "conv2", "norm2", "conv3", "conv4", "conv5", "pool5", "fc6", "fc7", "fc8"],
    "goturn": ["conv2", "conv5", "pool5", "conv2_p", "conv4_p", "pool5_p", "pool5_concat", "fc6-new", "fc7-newb", "fc8-shapes"],
    "googlenet": ["conv2/3x3", "inception_3b/output", "inception_4a/output", "inception_4e/output", "pool4/3x3_s2", "inception_5b/output",
                  "pool5/7x7_s1", "loss3/classifier"],
}


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def make(which, phase, **over):
    fn, kw = NETS[which]
    txt = fn(phase, **dict(kw, **over))
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TEST" if phase == "DEPLOY" else phase)
    spec.infer()
    return txt, msg, spec


def inputs_for(spec, seed, classes=10):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in spec.input_shapes.items():
        if name == "label":
            out[name] = rng.integers(0, classes, shp).astype(np.float32)
        elif name == "bbox":
            out[name] = rng.uniform(0, 10, shp).astype(np.float32)
        else:
            out[name] = rng.standard_normal(shp).astype(np.float32)
    return out


@pytest.mark.parametrize("which", ["caffenet", "goturn", "googlenet"])
def test_test_phase_forward_through_caffe_net(gpu, tmp_path, monkeypatch, which):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    txt, msg, spec = make(which, "TEST")
    path, weights = str(tmp_path / "test.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(txt)
    params = random_params(spec, 11)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST)
    x = inputs_for(spec, 1)
    for k, v in x.items():
        net.blobs[k].data[...] = v
    out = net.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    for name in INTERIOR[which]:
        assert tuple(net.blobs[name].data.shape) == tuple(ref[name].shape), name
        err = rel_err(net.blobs[name].data, ref[name].numpy())
        print("NET %s %s %.3g" % (which, name, err))
        assert err < 1e-4, name
    assert sorted(out) == sorted(net.outputs) and len(out) >= 1
    for name in net.outputs:
        want = float(ref[name])
        assert abs(float(out[name]) - want) <= 1e-4 * max(abs(want), 1e-30), (name, float(out[name]), want)
    # the grouped layers' banks and the fc banks come back from the device in Caffe's layout
    for l in spec.param_layers():
        for i, want in enumerate(params[l.name]):
            assert np.array_equal(net._engine.read_param(l.name, i), want), l.name


@pytest.mark.parametrize("which", ["caffenet", "goturn", "googlenet"])
def test_half_float_engine_forward_through_caffe_net(gpu, tmp_path, monkeypatch, which):
    """Deploy form in TEST phase (a half-float engine has no loss / Accuracy kernel).  The reference rounds where the engine rounds:
    banks that read a half blob are halves, every half blob is rounded when it is stored."""
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    txt, msg, spec = make(which, "DEPLOY", **(dict(width_div=2) if which == "googlenet" else {}))
    path, weights = str(tmp_path / "deploy.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(txt)
    params = random_params(spec, 12)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST, dtype="f16")
    eng = net._engine
    assert eng.f16
    x = inputs_for(spec, 2)
    for k, v in x.items():
        net.blobs[k].data[...] = v
    out = net.forward()
    r16 = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
    half_bank = {l.name for l in spec.param_layers() if eng.blobs[l.bottoms[0]].esize == 2}
    assert {l.name for l in spec.param_layers() if l.type == "InnerProduct"} <= half_bank
    p16 = {k: [r16(v[0]) if k in half_bank else v[0]] + list(v[1:]) for k, v in params.items()}
    rnd = lambda name, y: y.to(torch.float16).to(torch.float64) if eng.blobs[name].esize == 2 else y
    with torch.no_grad():
        ref = torch_net(spec, as_torch(p16), x, round_blob=rnd)
    for name in INTERIOR[which] + list(eng.outputs):
        err = rel_err(eng.read_blob(name), ref[name].numpy())
        print("F16NET %s %s %.3g" % (which, name, err))
        assert err < 5e-3, name
    for name in eng.outputs:
        assert out[name].dtype == np.float32 and eng.blobs[name].esize == 4


def _train_engine(monkeypatch, which, graph, seed=3):
    monkeypatch.setenv("FCN_NO_GRAPH", "0" if graph else "1")
    txt, msg, spec = make(which, "TRAIN")
    params = random_params(spec, seed)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    return spec, params, eng


def ip_pads_are_zero(eng, spec):
    """Pad columns of every InnerProduct weight gradient and pad channels of every InnerProduct dX are exact zeros ON THE DEVICE (the
    solver, weight decay, L1 regularisation and clipping run over the packed buffer).  Returns how many pad channels were looked at."""
    from fcn_object_detector_amd import lib as L
    flat = _device_grad_flat(eng)
    padded = 0
    for l in spec.layers:
        if l.type != "InnerProduct":
            continue
        seg = eng.param_segs[(l.name, 0)]
        c, h, w, cs = seg.bottom
        bank = flat[seg.offset:seg.offset + seg.count].reshape(seg.shape[0], h * w, cs)
        assert bank[:, :, :c].any() and not bank[:, :, c:].any(), l.name
        padded += cs - c
        gb = eng.grad_blobs.get(l.bottoms[0])
        if gb is not None and gb.cstride > gb.channels:
            raw = np.empty((gb.pixels, gb.cstride), np.float32)
            L.call("fcn_memcpy_d2h_async", raw.ctypes.data, gb.buf.ptr, raw.nbytes, eng.stream)
            L.call("fcn_stream_sync", eng.stream)
            assert raw[:, :gb.channels].any() and not raw[:, gb.channels:].any(), l.name
    return padded


def _device_grad_flat(eng):
    flat = np.empty(max(eng.param_count, 4), np.float32)
    from fcn_object_detector_amd import lib as L
    L.call("fcn_memcpy_d2h_async", flat.ctypes.data, eng.grad_flat.ptr, flat.nbytes, eng.stream)
    L.call("fcn_stream_sync", eng.stream)
    return flat


@pytest.mark.parametrize("which,graph", [("caffenet", True), ("caffenet", False), ("goturn", True), ("goturn", False), ("googlenet", True),
                                         ("googlenet", False)])
def test_one_training_step(gpu, monkeypatch, which, graph):
    spec, params, eng = _train_engine(monkeypatch, which, graph)
    bk = [(op.kind, op.name) for op in eng.bwd_ops]
    ips = [l.name for l in spec.layers if l.type == "InnerProduct"]
    assert sorted(n for k, n in bk if k == "wgrad" and n in ips) == sorted(ips), bk
    if which == "goturn":
        # the frozen towers: no gradient blob, no weight gradient, no data-gradient launch below fc6-new
        frozen = [l.name for l in spec.param_layers() if l.type == "Convolution"]
        assert len(frozen) == 10 and not any(eng._learns(l) for l in spec.param_layers() if l.name in frozen)
        assert not any(b in eng.grad_blobs for b in ("pool5", "pool5_p", "pool5_concat", "conv5", "image", "target"))
        assert not any(k in ("dgrad", "tconv_dgrad", "maxpool_bwd", "lrn_bwd", "flip") for k, _ in bk), bk
        assert [n for k, n in bk if k == "inner_product_bwd"] == ["fc8-shapes", "fc7-newb", "fc7-new"]
    if which == "googlenet":
        assert sorted(n for k, n in bk if k == "avepool_bwd") == ["loss1/ave_pool", "loss2/ave_pool", "pool5/7x7_s1"]
    x = inputs_for(spec, 5)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=7)
    P = as_torch(params, grad=True)
    ref = torch_net(spec, P, x, dropout_seed=7)
    ref["total_loss"].backward()
    want = float(ref["total_loss"].detach())
    print("STEP %s loss %.6g want %.6g" % (which, out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want), (out["total_loss"], want)
    for name in eng.loss_blobs:
        assert abs(out[name] - float(ref[name].detach())) < 1e-4 * abs(float(ref[name].detach())), name
    for name in INTERIOR[which][-3:]:
        assert rel_err(eng.read_blob(name), ref[name].detach().numpy()) < 1e-4, name
    got = eng.download_grads()
    learn = [l for l in spec.param_layers() if eng._learns(l)]
    assert set(ips) <= {l.name for l in learn}
    for l in learn:
        for g, r in zip(got[l.name], P[l.name]):
            assert g.shape == tuple(r.grad.shape), l.name
            err = rel_err(g, r.grad.numpy())
            print("GRAD %s %s %.3g" % (which, l.name, err))
            assert err < 5e-4, "parameter gradient of " + l.name
    for l in spec.param_layers():
        if not eng._learns(l):
            assert all(not g.any() for g in got[l.name]), l.name
    ip_pads_are_zero(eng, spec)
    g1 = eng.download_grads()
    eng.step(seed=7)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k]))      # the same step again: the same bits
    eng.close()


FANIN = """
input: "data" input_shape { dim: 3 dim: 3 dim: 9 dim: 9 }
input: "label" input_shape { dim: 3 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0"
  convolution_param { num_output: 6 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "%s" type: "%s" bottom: "c0" top: "%s" %s }
layer { name: "%s" type: "%s" bottom: "c0" top: "%s" %s }
layer { name: "pool" type: "Pooling" bottom: "conv" top: "pool" pooling_param { pool: AVE global_pooling: true } }
layer { name: "fc2" type: "InnerProduct" bottom: "pool" top: "fc2" inner_product_param { num_output: 5 weight_filler { type: "xavier" } } }
layer { name: "sum" type: "Eltwise" bottom: "fc" bottom: "fc2" top: "sum" eltwise_param { operation: SUM } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "sum" bottom: "label" top: "loss" }
"""
_FC = ("fc", "InnerProduct", "fc", 'inner_product_param { num_output: 5 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } }')
_CONV = ("conv", "Convolution", "conv", 'convolution_param { num_output: 7 kernel_size: 3 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } }')


def _small_step(text, seed=1):
    msg = proto.parse_text(text)
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    params = random_params(spec, seed)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    x = inputs_for(spec, 0, classes=5)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=1)
    P = as_torch(params, grad=True)
    ref = torch_net(spec, P, x, dropout_seed=1)
    return spec, eng, out, P, ref


@pytest.mark.parametrize("order", ["fc_first", "conv_first"])
def test_inner_product_and_convolution_accumulate_into_one_gradient(gpu, order):
    """c0 (6 channels in pixels of 8) feeds an InnerProduct and a convolution: whichever comes later in the backward pass adds into dc0.
    The global AVE pooling behind the convolution is the 7x7-on-7x7 case of the new kernel; the InnerProduct over c0 has two pad
    channels per pixel, the one over the pooled 7 channels one."""
    a, b = (_FC, _CONV) if order == "fc_first" else (_CONV, _FC)
    spec, eng, out, P, ref = _small_step(FANIN % (a + b))
    kinds = [(op.kind, op.name.split(" ")[0]) for op in eng.bwd_ops if op.kind in ("dgrad", "inner_product_bwd")]
    kinds = [kn for kn in kinds if kn[1] in ("fc", "conv")]      # (the two that write dc0)
    assert kinds == ([("dgrad", "conv"), ("inner_product_bwd", "fc")] if order == "fc_first" else [("inner_product_bwd", "fc"), ("dgrad", "conv")])
    ref["c0"].retain_grad()
    ref["total_loss"].backward()
    assert abs(out["loss"] - float(ref["total_loss"].detach())) < 1e-4 * abs(float(ref["total_loss"].detach()))
    assert eng.read_grad("fc").shape == (3, 5) and eng.read_grad("c0").shape == (3, 6, 9, 9)
    assert rel_err(eng.read_grad("c0"), ref["c0"].grad.numpy()) < 1e-4
    got = eng.download_grads()
    for name in ("c0", "fc", "conv", "fc2"):
        for g, r in zip(got[name], P[name]):
            assert rel_err(g, r.grad.numpy()) < 5e-4, name
    assert ip_pads_are_zero(eng, spec) == 3      # fc over c0: 6 channels in pixels of 8; fc2 over pool: 7 channels in pixels of 8
    eng.close()


TWO_CONSUMERS = """
input: "data" input_shape { dim: 2 dim: 3 dim: 11 dim: 10 }
input: "label" input_shape { dim: 2 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0"
  convolution_param { num_output: 8 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "ave" type: "Pooling" bottom: "c0" top: "ave" pooling_param { pool: AVE kernel_size: 3 stride: 2 pad: 1 } }
layer { name: "max" type: "Pooling" bottom: "c0" top: "max" pooling_param { pool: MAX kernel_size: 3 stride: 2 pad: 1 } }
layer { name: "fa" type: "InnerProduct" bottom: "ave" top: "fa" inner_product_param { num_output: 4 weight_filler { type: "xavier" } } }
layer { name: "fm" type: "InnerProduct" bottom: "max" top: "fm" inner_product_param { num_output: 4 weight_filler { type: "xavier" } } }
layer { name: "sum" type: "Eltwise" bottom: "fa" bottom: "fm" top: "sum" eltwise_param { operation: SUM } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "sum" bottom: "label" top: "loss" }
"""


@pytest.mark.parametrize("swap", [False, True])
def test_ave_pooling_backward_accumulates(gpu, swap):
    """c0 feeds an AVE and a MAX pooling.  In reverse layer order the later layer's backward writes dc0 first: with the AVE pooling
    ahead of the MAX pooling in the net, fcn_avepool_bwd_f32 runs second and takes its `accumulate` path."""
    text = TWO_CONSUMERS
    if swap:
        lines = text.split("\n")
        i, j = [k for k, ln in enumerate(lines) if ln.startswith('layer { name: "ave"') or ln.startswith('layer { name: "max"')]
        lines[i], lines[j] = lines[j], lines[i]
        text = "\n".join(lines)
    spec, eng, out, P, ref = _small_step(text, seed=2)
    order = [op.kind for op in eng.bwd_ops if op.kind in ("avepool_bwd", "maxpool_bwd")]
    assert order == (["avepool_bwd", "maxpool_bwd"] if swap else ["maxpool_bwd", "avepool_bwd"])
    ref["c0"].retain_grad()
    ref["total_loss"].backward()
    assert rel_err(eng.read_grad("c0"), ref["c0"].grad.numpy()) < 1e-4
    got = eng.download_grads()
    for g, r in zip(got["c0"], P["c0"]):
        assert rel_err(g, r.grad.numpy()) < 5e-4
    eng.close()


GROUPED_STRIDED = """
input: "data" input_shape { dim: 2 dim: 3 dim: 13 dim: 12 }
input: "label" input_shape { dim: 2 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0"
  convolution_param { num_output: 8 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "g2" type: "Convolution" bottom: "c0" top: "g2"
  convolution_param { num_output: 16 group: 2 kernel_size: 3 stride: 2 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "r2" type: "ReLU" bottom: "g2" top: "g2" }
layer { name: "g4" type: "Convolution" bottom: "g2" top: "g4"
  convolution_param { num_output: 16 group: 4 kernel_size: 3 pad: 1 bias_term: false weight_filler { type: "xavier" } } }
layer { name: "fc" type: "InnerProduct" bottom: "g4" top: "fc" inner_product_param { num_output: 5 weight_filler { type: "xavier" } } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }
"""


def test_grouped_convolution_strided_and_without_bias(gpu):
    """A strided grouped layer (one tap-major bank and one transposed-convolution launch per group) under a stride-1 layer in four groups
    without a bias; both data gradients land under an in-place ReLU."""
    spec, eng, out, P, ref = _small_step(GROUPED_STRIDED, seed=4)
    bk = [(op.kind, op.name.split(" ")[0]) for op in eng.bwd_ops]
    assert [n for k, n in bk if k == "tconv_dgrad"] == ["g2", "g2#1"] and ("dgrad", "g4") in bk
    for name in ("c0", "g2"):
        ref[name].retain_grad()
    ref["total_loss"].backward()
    assert abs(out["loss"] - float(ref["total_loss"].detach())) < 1e-4 * abs(float(ref["total_loss"].detach()))
    for name in ("g2", "g4", "fc"):
        assert rel_err(eng.read_blob(name), ref[name].detach().numpy()) < 1e-4, name
    got = eng.download_grads()
    for name in ("c0", "g2", "g4", "fc"):
        for g, r in zip(got[name], P[name]):
            assert g.shape == tuple(r.grad.shape) and rel_err(g, r.grad.numpy()) < 5e-4, name
    eng.close()


def _write_job(tmp_path, max_iter=100, snapshot=0):
    net = tmp_path / "train.prototxt"
    net.write_text(NETS["caffenet"][0]("TRAIN", **NETS["caffenet"][1]))
    solver = tmp_path / "solver.prototxt"
    solver.write_text('net: "%s"\nbase_lr: 0.01\nmomentum: 0.9\nweight_decay: 1e-4\nlr_policy: "fixed"\ndisplay: 1\nmax_iter: %d\n'
                      'snapshot: %d\nsnapshot_prefix: "%s"\n' % (net, max_iter, snapshot, tmp_path / "snap"))
    return str(solver), str(net)


def test_sgd_solver_learns_snapshots_and_restores(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    txt, msg, spec = make("caffenet", "TRAIN")
    params = fill_params(spec, seed=0)      # the writer's own fillers (gaussian 0.01 / 0.005): scores near zero, a loss near ln 10
    weights = str(tmp_path / "init.caffemodel")
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    x = inputs_for(spec, 4)
    job, _ = _write_job(tmp_path)

    def start():
        s = caffe.SGDSolver(job, log=None, autotune=False)
        s.net.copy_from(weights)
        for k, v in x.items():
            s.engine.host_array(k)[...] = v
        return s
    a = start()
    # copy_from round-trips the grouped banks and the fc banks exactly
    got = a.engine.download_params()
    assert all(np.array_equal(u, v) for k in params for u, v in zip(got[k], params[k]))
    assert got["conv2"][0].shape == (128, 24, 5, 5) and got["fc6"][0].shape == (128, 128 * 2 * 2)
    losses = [a.step(1)["loss"] for _ in range(8)]      # (two images: the biases of fc8 alone take the loss from ln 10 towards ln 2)
    print("LOSSES", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    a.snapshot()
    b = start()
    b.restore(str(tmp_path / "snap_iter_8.solverstate"))
    assert b.iter == 8
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    la, lb = [a.step(1)["loss"] for _ in range(2)], [b.step(1)["loss"] for _ in range(2)]
    assert la == lb
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    a.close()
    b.close()


def test_caffe_tool_trains_and_tests(gpu, tmp_path):
    job, _ = _write_job(tmp_path, max_iter=3, snapshot=3)
    test_net = tmp_path / "test.prototxt"
    test_net.write_text(NETS["caffenet"][0]("TEST", **NETS["caffenet"][1]))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PYCAFFE, os.environ.get("PYTHONPATH", "")]), FCN_AUTOTUNE="0")
    r = subprocess.run([sys.executable, CAFFE, "train", "--solver=%s" % job, "--gpu=0"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    weights = tmp_path / "snap_iter_3.caffemodel"
    assert weights.exists()
    r = subprocess.run([sys.executable, CAFFE, "test", "--model=%s" % test_net, "--weights=%s" % weights, "--iterations=2", "--gpu=0"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "accuracy = " in r.stderr and "loss = " in r.stderr, r.stderr[-2000:]


def test_full_size_caffenet_at_its_deploy_batch(gpu):
    txt = models.caffenet("DEPLOY", batch=10)
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TEST")
    spec.infer()
    assert spec.blob_shapes["pool5"] == (10, 256, 6, 6) and spec.param_shapes["fc6"][0] == (4096, 9216)
    params = random_params(spec, 2)
    eng = Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False)
    x = np.random.default_rng(3).standard_normal((10, 3, 227, 227)).astype(np.float32)
    eng.host_array("data")[...] = x
    out = eng.forward()
    got = {n: eng.read_blob(n).copy() for n in ("conv2", "conv5", "fc6", "fc8")}
    eng.close()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), {"data": x})
    for name, g in got.items():
        assert rel_err(g, ref[name].numpy()) < 1e-4, name
    assert rel_err(out["prob"], ref["prob"].numpy()) < 1e-4
    # 33 rows are past the streaming kernels: refused by layer name
    msg33 = proto.parse_text(models.caffenet("DEPLOY", batch=33, width_div=2, fc_div=32, size=99, num_classes=10))
    with pytest.raises(NotImplementedError, match="InnerProduct fc6: a batch of 33 rows"):
        Engine(NetSpec(msg33, "TEST"), device=0, autotune=False)


def test_full_size_bvlc_googlenet(gpu):
    msg = proto.parse_text(models.bvlc_googlenet("DEPLOY", batch=2))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    assert spec.blob_shapes["pool5/7x7_s1"] == (2, 1024, 1, 1)
    params = random_params(spec, 5)
    eng = Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False)
    x = np.random.default_rng(6).standard_normal((2, 3, 224, 224)).astype(np.float32)
    eng.host_array("data")[...] = x
    out = eng.forward()
    got = {n: eng.read_blob(n).copy() for n in ("inception_4e/output", "pool5/7x7_s1", "loss3/classifier")}
    eng.close()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), {"data": x})
    for name, g in got.items():
        assert rel_err(g, ref[name].numpy()) < 1e-4, name
    assert rel_err(out["prob"], ref["prob"].numpy()) < 1e-4


def test_refusals_by_layer_name(gpu):
    bad = GROUPED_STRIDED.replace("num_output: 8 kernel_size: 3 pad: 1", "num_output: 6 kernel_size: 3 pad: 1")      # group 2 over 6 channels
    with pytest.raises(NotImplementedError, match="grouped Convolution g2: group 2 leaves 3 input"):
        Engine(NetSpec(proto.parse_text(bad), "TRAIN"), device=0, autotune=False)
