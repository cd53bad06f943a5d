"""InnerProduct above 32 rows through the engines and the public surface, -m gpu: CaffeNet (models.caffenet, width_div 2, fc_div 32,
99 x 99 images, 10 classes) at a deploy batch of 33 in the float32 and the half-float engine and through caffe.Net, one training step at
a batch of 40 with every parameter gradient, a fan-in net whose InnerProduct adds into a gradient a convolution wrote (and the other
way round), and the small Faster R-CNN net of tests/faster_rcnn_case.py, whose fc6 runs over all 48 rows of roi_pool5.

References and thresholds are the project's: torch on the CPU in float64 (tests/torch_classifier_ref.py), rel_err < 1e-4 for blobs and
the loss, < 5e-4 for parameter gradients; the half-float engine against the float64 product of the operands rounded where the engine
rounds, at the thresholds of tests/test_gpu_forward_plan_paths_f16.py (rel_err < TOL = 3.16e-3, conftest.elem_err at 2^-10 within
4 x MEASURED_ELEM behind a computed half blob); the region net against tests/region_net_ref.py, whose decision margin
tests/test_ip_gemm_faster_rcnn_ref.py asserts without a GPU."""
import sys

import numpy as np
import pytest
import torch

import faster_rcnn_case as FR
import region_cases as RC
from conftest import PYCAFFE, elem_err, rel_err
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from test_gpu_forward_plan_paths_f16 import ELEM_TOL, MEASURED_ELEM, TOL
from torch_classifier_ref import as_torch, random_params, torch_net

pytestmark = pytest.mark.gpu
KW = dict(width_div=2, fc_div=32, size=99, num_classes=10)
FC = ["fc6", "fc7", "fc8"]


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def make(phase, batch):
    txt = models.caffenet(phase, batch=batch, **KW)
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TEST" if phase == "DEPLOY" else phase, ip_gemm=True)
    spec.infer()
    return txt, msg, spec


@pytest.fixture(scope="module")
def deploy():
    """The deploy net at 33 images, its parameters, input and float64 reference: computed once, left unchanged."""
    txt, msg, spec = make("DEPLOY", 33)
    params = random_params(spec, 21)
    x = np.random.default_rng(22).standard_normal(spec.input_shapes["data"]).astype(np.float32)
    with torch.no_grad():
        ref = {k: v.numpy() for k, v in torch_net(spec, as_torch(params), {"data": x}).items()}
    return dict(txt=txt, msg=msg, spec=spec, params=params, x=x, ref=ref)


def ip_kinds(eng):
    return [(op.kind, op.name) for op in eng.ops if op.name in FC]


def test_deploy_float32(gpu, deploy):
    with pytest.raises(NotImplementedError, match="InnerProduct fc6: a batch of 33 rows.*ip_gemm=True"):      # a bare NetSpec still refuses
        Engine(NetSpec(deploy["msg"], "TEST"), device=0, autotune=False)
    eng = Engine(NetSpec(deploy["msg"], "TEST", ip_gemm=True), params=deploy["params"], device=0, autotune=False)
    assert ip_kinds(eng) == [("ip_gemm", n) for n in FC]
    eng.host_array("data")[...] = deploy["x"]
    out = eng.forward()
    for name in ("pool5", "fc6", "fc7", "fc8"):
        err = rel_err(eng.read_blob(name), deploy["ref"][name])
        print("IPGEMM f32 %s %.3g" % (name, err))
        assert err < 1e-4, name
    assert out["prob"].shape == (33, 10) and rel_err(out["prob"], deploy["ref"]["prob"]) < 1e-4
    eng.close()


def test_deploy_half_float(gpu, deploy):
    spec, params = deploy["spec"], deploy["params"]
    eng = Engine(NetSpec(deploy["msg"], "TEST", ip_gemm=True), params=params, device=0, autotune=False, dtype="f16")
    assert eng.f16 and ip_kinds(eng) == [("ip_gemm", n) for n in FC]
    assert eng.blobs["pool5"].esize == 2 and eng.blobs["fc6"].esize == 2 and eng.blobs["prob"].esize == 4
    eng.host_array("data")[...] = deploy["x"]
    out = eng.forward()
    r16 = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
    half_bank = {l.name for l in spec.param_layers() if eng.blobs[l.bottoms[0]].esize == 2}
    assert set(FC) <= half_bank
    p16 = {k: [r16(v[0]) if k in half_bank else v[0]] + list(v[1:]) for k, v in params.items()}
    rnd = lambda name, y: y.to(torch.float16).to(torch.float64) if eng.blobs[name].esize == 2 else y
    with torch.no_grad():
        ref = torch_net(spec, as_torch(p16), {"data": deploy["x"]}, round_blob=rnd)
    for name in ("fc6", "fc7", "fc8", "prob"):
        got, want = eng.read_blob(name), ref[name].numpy()
        err, el = rel_err(got, want), elem_err(got, want, ELEM_TOL)[0]
        print("IPGEMM f16 %s rel_err %.3g elem_err ratio %.3g" % (name, err, el))
        assert err < TOL, name
        assert el <= 4 * MEASURED_ELEM, name
    assert out["prob"].dtype == np.float32
    eng.close()


def test_public_surface(gpu, deploy, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    path, weights = str(tmp_path / "deploy.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(deploy["txt"])
    proto.write_caffemodel(weights, [(l.name, l.type, deploy["params"][l.name]) for l in deploy["spec"].param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST)
    assert net._engine.spec.ip_gemm
    net.blobs["data"].data[...] = deploy["x"]
    out = net.forward()
    fc7 = deploy["spec"].blob_shapes["fc7"][1]
    assert net.blobs["fc7"].data.shape == (33, fc7) == (33, 128)
    for name in FC:
        assert rel_err(net.blobs[name].data, deploy["ref"][name]) < 1e-4, name
    assert rel_err(out["prob"], deploy["ref"]["prob"]) < 1e-4
    # one replay of the captured graph gives the bits of the eager run
    assert net._engine.graph_io is not None
    first = out["prob"].tobytes() + net.blobs["fc6"].data.tobytes()
    monkeypatch.setenv("FCN_NO_GRAPH", "1")
    net.blobs["data"].data[...] = deploy["x"]
    eager = net.forward()
    assert eager["prob"].tobytes() + net.blobs["fc6"].data.tobytes() == first
    monkeypatch.setenv("FCN_NO_GRAPH", "0")
    net.blobs["data"].data[...] = deploy["x"]
    again = net.forward()
    assert again["prob"].tobytes() + net.blobs["fc6"].data.tobytes() == first
    net._engine.close()


def inputs_for(spec, seed, classes):
    rng = np.random.default_rng(seed)
    return {name: (rng.integers(0, classes, shp).astype(np.float32) if name == "label" else rng.standard_normal(shp).astype(np.float32))
            for name, shp in spec.input_shapes.items()}


def _step(msg, spec, seed, classes):
    params = random_params(spec, seed)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN", ip_gemm=True), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()},
                      device=0, solver=sp, autotune=False)
    x = inputs_for(spec, seed + 1, classes)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=7)
    P = as_torch(params, grad=True)
    ref = torch_net(spec, P, x, dropout_seed=7)
    return eng, out, P, ref


def test_one_training_step_at_40_images(gpu):
    txt, msg, spec = make("TRAIN", 40)
    with pytest.raises(NotImplementedError, match="InnerProduct fc\\d: a batch of 40 rows"):
        TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params=random_params(spec, 3), device=0,
                    solver=SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD"), autotune=False)
    eng, out, P, ref = _step(msg, spec, 31, 10)
    bk = [(op.kind, op.name) for op in eng.bwd_ops if op.name in FC and op.kind in ("wgrad", "ip_gemm_bwd", "inner_product_bwd")]
    assert sorted(bk) == sorted([("wgrad", n) for n in FC] + [("ip_gemm_bwd", n) for n in FC]), bk
    ref["total_loss"].backward()
    want = float(ref["total_loss"].detach())
    print("IPGEMM step loss %.6g want %.6g" % (out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want)
    for name in FC:
        assert rel_err(eng.read_blob(name), ref[name].detach().numpy()) < 1e-4, name
    got = eng.download_grads()
    for l in spec.param_layers():
        assert eng._learns(l)
        for g, r in zip(got[l.name], P[l.name]):
            assert g.shape == tuple(r.grad.shape), l.name
            err = rel_err(g, r.grad.numpy())
            print("IPGEMM grad %s %.3g" % (l.name, err))
            assert err < 5e-4, "parameter gradient of " + l.name
    g1 = eng.download_grads()
    eng.step(seed=7)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k]))      # the same step again: the same bits
    eng.close()


FANIN = """
input: "data" input_shape { dim: 40 dim: 3 dim: 9 dim: 9 }
input: "label" input_shape { dim: 40 }
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


@pytest.mark.parametrize("order", ["fc_first", "conv_first"])
def test_the_bottoms_gradient_accumulates(gpu, order):
    """c0 feeds an InnerProduct and a convolution at 40 images: whichever comes first in the net runs second in the backward pass and adds
    into dc0 - fc_first is the GEMM's FCN_CONV_ACCUM.  c0 has 6 channels in pixels of 8: the pad channels of dX stay zeros."""
    a, b = (_FC, _CONV) if order == "fc_first" else (_CONV, _FC)
    msg = proto.parse_text(FANIN % (a + b))
    spec = NetSpec(msg, "TRAIN", ip_gemm=True)
    spec.infer()
    eng, out, P, ref = _step(msg, spec, 41, 5)
    kinds = [(op.kind, op.name.split(" ")[0]) for op in eng.bwd_ops if op.kind in ("dgrad", "ip_gemm_bwd", "inner_product_bwd")]
    kinds = [kn for kn in kinds if kn[1] in ("fc", "conv")]
    assert kinds == ([("dgrad", "conv"), ("ip_gemm_bwd", "fc")] if order == "fc_first" else [("ip_gemm_bwd", "fc"), ("dgrad", "conv")])
    ref["c0"].retain_grad()
    ref["total_loss"].backward()
    assert abs(out["loss"] - float(ref["total_loss"].detach())) < 1e-4 * abs(float(ref["total_loss"].detach()))
    assert eng.read_grad("c0").shape == (40, 6, 9, 9)
    assert rel_err(eng.read_grad("c0"), ref["c0"].grad.numpy()) < 1e-4
    got = eng.download_grads()
    for name in ("c0", "fc", "conv", "fc2"):
        for g, r in zip(got[name], P[name]):
            assert rel_err(g, r.grad.numpy()) < 5e-4, name
    gb = eng.grad_blobs["c0"]
    raw = np.empty((gb.pixels, gb.cstride), np.float32)
    L.call("fcn_memcpy_d2h_async", raw.ctypes.data, gb.buf.ptr, raw.nbytes, eng.stream)
    L.call("fcn_stream_sync", eng.stream)
    assert gb.cstride == 8 and raw[:, :6].any() and not raw[:, 6:].any()
    eng.close()


@pytest.fixture(scope="module")
def rcnn(tmp_path_factory):
    """The small Faster R-CNN net through caffe.Net, one forward, and its float64 reference: shared and left unchanged."""
    L.load()
    caffe = _caffe()
    c = FR.case()
    d = tmp_path_factory.mktemp("faster_rcnn")
    deploy, weights = d / "deploy.prototxt", d / "w.caffemodel"
    deploy.write_text(c["text"])
    proto.write_caffemodel(str(weights), [(l.name, l.type, c["params"][l.name]) for l in c["spec"].param_layers()])
    net = caffe.Net(str(deploy), str(weights), caffe.TEST)
    for k, v in c["inputs"].items():
        net.blobs[k].data[...] = v
    out = net.forward()
    yield dict(c, net=net, out={k: v.copy() for k, v in out.items()})
    net._engine.close()


def test_faster_rcnn_head_over_all_rois(gpu, rcnn):
    net, B, count = rcnn["net"], rcnn["ref"], rcnn["count"]
    assert rcnn["margin"] >= RC.MARGIN and 0 < count < 48
    eng = net._engine
    assert [(op.kind, op.name) for op in eng.ops if op.kind in ("ip_gemm", "inner_product")] == [("ip_gemm", n) for n in ("fc6", "fc7", "cls_score", "bbox_pred")]
    assert net.blobs["rois"].shape == (count, 5)
    for nm in FR.BLOBS:
        got = net.blobs[nm].data
        assert got.shape == B[nm].shape, nm
        err = rel_err(got, B[nm])
        print("IPGEMM rcnn %s %.3g" % (nm, err))
        assert err < 1e-4, nm
    for nm in FR.OUTPUTS:      # rows up to the count
        assert rcnn["out"][nm].shape == B[nm].shape == (count, B[nm].shape[1]) and rel_err(rcnn["out"][nm], B[nm]) < 1e-4, nm
    assert np.allclose(net.blobs["cls_prob"].data.sum(axis=1), 1.0, atol=1e-5)
    # the GEMM ran over all 48 rows: the rois behind the count are zeros on the device, every such row of roi_pool5 is the pooling of that one
    # roi (the 1 x 1 window at the origin) and every such row of fc6 the same finite vector, bit for bit
    rois, full = eng.blobs["rois"], eng.blobs["fc6"]
    r, raw = np.empty((48, rois.cstride), np.float32), np.empty((48, full.cstride), np.float32)
    L.call("fcn_memcpy_d2h_async", r.ctypes.data, rois.buf.ptr, r.nbytes, None)
    L.call("fcn_memcpy_d2h_async", raw.ctypes.data, full.buf.ptr, raw.nbytes, None)
    L.call("fcn_device_sync")
    n6 = rcnn["spec"].blob_shapes["fc6"][1]
    assert np.all(r[count:] == 0) and np.all(np.isfinite(raw[:, :n6]))
    assert np.array_equal(raw[count:, :n6], np.broadcast_to(raw[count, :n6], (48 - count, n6))) and raw[count, :n6].any()
    want = np.maximum(rcnn["ref"]["conv5_3"][0, :, 0, 0].repeat(49) @ rcnn["params"]["fc6"][0].astype(np.float64).T + rcnn["params"]["fc6"][1], 0)
    assert rel_err(raw[count, :n6], want) < 1e-4


def test_faster_rcnn_replay_and_eager_give_the_same_bytes(gpu, rcnn, monkeypatch):
    net, outs = rcnn["net"], []
    for no_graph in ("0", "1"):
        monkeypatch.setenv("FCN_NO_GRAPH", no_graph)
        for k, v in rcnn["inputs"].items():
            net.blobs[k].data[...] = v
        o = net.forward()
        outs.append(b"".join(o[k].tobytes() for k in FR.OUTPUTS) + net.blobs["rois"].data.tobytes())
    assert net._engine.graph_io is not None
    first = b"".join(rcnn["out"][k].tobytes() for k in FR.OUTPUTS)
    assert all(o.startswith(first) and o == outs[0] for o in outs)
