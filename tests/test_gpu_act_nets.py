"""MTCNN (models.mtcnn) and ENet (models.enet) through the public surface, -m gpu, against torch in float64 on the CPU
(tests/torch_act_ref.py), in the style of tests/test_gpu_se_nets.py.

P-Net through caffe.Net from a prototxt and a caffemodel, at its own 12 x 12 and fully convolutional at 33 x 47, batch 2: every blob at
the project's rel_err < 1e-4 for float32 results; the slopes have both signs (tests/torch_act_ref.act_params), so a PReLU that took
the wrong channel's slope, or a ReLU in its place, is far off.
O-Net in halves (32 / 64 / 64 / 128 channels: every MAX pooling sees whole groups of 8) against the float32 engine on the same weights,
at the project's bound for half-float nets, 5e-3.
One caffe.SGDSolver step on P-Net TRAIN (SoftmaxWithLoss on the class head, EuclideanLoss on the box head): the loss within 1e-4
relative, the slopes moved, and every blob after the update at rel_err < 1e-4 against w - lr * lr_mult * dw from autograd in float64 -
the bound of tests/test_gpu_se_nets.py for its step.  iter_size: 2 on two different batches: the gradient buffer holds the SUM of the
two passes' gradients (the parameter-gradient launch overwrites; the solver's accumulation adds) and the update is their mean.  A
snapshot of a solver with momentum, of a net that holds both slope shapes, restored into a second solver: the same bits, and the next
step gives the same bits.
ENet, models.enet(width_div=4, size=(32, 64), classes=5, batch=2): the TEST forward blob by blob, and one SGD step in TRAIN - batch
statistics, the device's Dropout masks and the two pooling masks (adopted in the reference: an argmax is discontinuous) - at the same
bounds."""
import sys

import numpy as np
import pytest
import torch

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from torch_act_ref import act_params, as_torch, torch_net

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL = 1e-4           # the project's rel_err bound for float32 results
TOL_F16 = 5e-3       # ... and for half-float nets against the float32 engine
ENET = dict(width_div=4, size=(32, 64), classes=5, batch=2)


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def spec_of(txt, phase):
    spec = NetSpec(proto.parse_text(txt), phase, depthwise=True, ip_gemm=True, activations=True)
    spec.infer()
    return spec


def inputs(spec, seed, classes=2):
    rng = np.random.default_rng(seed)
    x = {}
    for name, shp in spec.input_shapes.items():
        if name == "label":
            x[name] = rng.integers(0, classes, shp).astype(F32)
        else:
            x[name] = rng.standard_normal(shp).astype(F32)
    return x


def load(tmp_path, txt, spec, params, tag, **kw):
    caffe = _caffe()
    path, weights = str(tmp_path / (tag + ".prototxt")), str(tmp_path / (tag + ".caffemodel"))
    open(path, "w").write(txt)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    return caffe.Net(path, weights, caffe.TEST, **kw)


def solver(tmp_path, txt, extra="", lr=0.01, momentum=0.0):
    caffe = _caffe()
    train, job = tmp_path / "train.prototxt", tmp_path / "solver.prototxt"
    train.write_text(txt)
    job.write_text('train_net: "%s"\nbase_lr: %g\nmomentum: %g\nweight_decay: 0\nlr_policy: "fixed"\nmax_iter: 10\nsnapshot_prefix: "%s"\n%s'
                   % (train, lr, momentum, tmp_path / "snap", extra))
    return caffe.SGDSolver(str(job), log=None, autotune=False)


def check_update(spec, params, now, grads, lr, what, updates=None):
    """Every blob after one SGD step without momentum or decay: w - lr * lr_mult * dw (BatchNorm: Caffe's moving-average step)."""
    worst = (0.0, None)
    for l in spec.param_layers():
        for i, w0 in enumerate(params[l.name]):
            if l.type == "BatchNorm":
                expect = updates[l.name][i]
            else:
                mult = l.lr_mult[i] if i < len(l.lr_mult) else 1.0
                expect = np.asarray(w0, np.float64) - lr * mult * np.asarray(grads[l.name][i]).reshape(np.shape(w0))
            err = rel_err(np.asarray(now[l.name][i]).reshape(np.shape(expect)), expect)
            worst = max(worst, (err, "%s[%d]" % (l.name, i)))
            assert err < TOL, "%s: blob %d of %s after the step: %.3g" % (what, i, l.name, err)
    print("ACTSTEP %s worst updated blob %.3g at %s" % (what, worst[0], worst[1]))


@pytest.mark.parametrize("size", [12, (33, 47)], ids=["12x12", "33x47"])
def test_pnet_forward(gpu, tmp_path, monkeypatch, size):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.mtcnn("pnet", "DEPLOY", 2, size=size)
    spec = spec_of(txt, "TEST")
    params, x = act_params(spec, 61), inputs(spec, 62)
    assert all((params[n][0] < 0).any() and (params[n][0] > 0).any() for n in ("PReLU1", "PReLU2", "PReLU3"))
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    net = load(tmp_path, txt, spec, params, "pnet")
    eng = net._engine
    assert [op.name for op in eng.ops if op.kind == "act"] == ["PReLU1", "PReLU2", "PReLU3"]
    net.blobs["data"].data[...] = x["data"]
    out = net.forward()
    for n in ("conv1", "pool1", "conv2", "conv3", "conv4-1", "conv4-2", "prob1"):
        err = rel_err(np.array(net.blobs[n].data).reshape(ref[n].shape), ref[n].numpy())
        print("PNET %s %s %.3g" % (size, n, err))
        assert err < TOL, (n, err)
    assert rel_err(out["prob1"], ref["prob1"].numpy()) < TOL and out["prob1"].shape == tuple(ref["prob1"].shape)
    a = {n: eng.read_blob(n).copy() for n in ("conv3", "prob1")}
    eng.forward(use_graph=False)      # a forward without the captured graph: the same bytes
    assert all(a[n].tobytes() == eng.read_blob(n).tobytes() for n in a)


def test_onet_in_halves_against_the_float32_engine(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.mtcnn("onet", "DEPLOY", 2)
    spec = spec_of(txt, "TEST")
    params, x = act_params(spec, 63), inputs(spec, 64)
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    got = {}
    for tag, kw in (("f32", {}), ("f16", {"dtype": "f16"})):
        net = load(tmp_path, txt, spec, params, "onet" + tag, **kw)
        eng = net._engine
        assert len([op for op in eng.ops if op.kind == "act"]) == 5 and eng.f16 == (tag == "f16")
        if tag == "f16":
            assert all(eng.blobs[l.tops[0]].esize == 2 for l in spec.layers if l.type == "PReLU")
        net.blobs["data"].data[...] = x["data"]
        net.forward()
        got[tag] = {n: eng.read_blob(n).astype(np.float64).reshape(ref[n].shape) for n in ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6-1",
                                                                                           "conv6-2", "conv6-3", "prob1")}
    for n in got["f32"]:
        e32, e16 = rel_err(got["f32"][n], ref[n].numpy()), rel_err(got["f16"][n], got["f32"][n])
        print("ONET %s f32 vs float64 %.3g, halves vs f32 %.3g" % (n, e32, e16))
        assert e32 < TOL, (n, e32)
        assert e16 < TOL_F16, (n, e16)


def test_pnet_solver_step(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.mtcnn("pnet", "TRAIN", 8)
    spec = spec_of(txt, "TRAIN")
    params, x = act_params(spec, 65), inputs(spec, 66)
    lr = 0.01
    s = solver(tmp_path, txt, lr=lr)
    eng = s.engine
    assert eng.spec.activations and sorted(n for n in eng.aux_dev if n.startswith("PReLU")) == ["PReLU1", "PReLU2", "PReLU3"]
    assert [op.kind for op in eng.bwd_ops].count("act_bwd_param") == 3 and [op.kind for op in eng.bwd_ops].count("act_bwd") == 3
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = s.step(1)
    P = as_torch(params, grad=True)
    B = torch_net(spec, P, x)
    B["total_loss"].backward()
    want = float(B["total_loss"].detach())
    print("PNETSTEP loss %.6g want %.6g (cls %.6g roi %.6g)" % (out["total_loss"], want, out["cls_loss"], out["roi_loss"]))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want)
    for name in ("cls_loss", "roi_loss"):
        ref_loss = float(B[name].detach())
        assert abs(out[name] - ref_loss) < 1e-4 * abs(ref_loss), (name, out[name], ref_loss)
    now, got = eng.download_params(), eng.download_grads()
    for n in ("PReLU1", "PReLU2", "PReLU3"):
        g64 = P[n][0].grad.numpy()
        err = rel_err(got[n][0], g64)
        print("PNETSTEP d%s %.3g" % (n, err))
        assert err < 5e-4, (n, err)
        assert np.abs(now[n][0] - params[n][0]).max() > 1e-6, "%s: the slopes did not move" % n
        # the movement itself, not only the moved blob: the gradient's bound plus the rounding of the stored slope (2^-24 |a|, twice)
        moved = now[n][0] - params[n][0].astype(np.float64)
        assert rel_err(moved, -lr * g64) < 5e-4 + 2.0 ** -23 * np.abs(params[n][0]).max() / np.abs(lr * g64).max(), n
    check_update(spec, params, now, {k: [p.grad.numpy() for p in v] for k, v in P.items()}, lr, "pnet")
    s.close()


def test_iter_size_2_sums_the_slope_gradient(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.mtcnn("pnet", "TRAIN", 4)
    spec = spec_of(txt, "TRAIN")
    params = act_params(spec, 67)
    batches = [inputs(spec, 68), inputs(spec, 69)]
    lr = 0.02
    s = solver(tmp_path, txt, extra="iter_size: 2\n", lr=lr)
    eng = s.engine
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])

    def feed(j):
        for k, v in batches[j].items():
            eng.host_array(k)[...] = v
    eng.step(feed=feed)
    grads = []
    for x in batches:
        P = as_torch(params, grad=True)
        torch_net(spec, P, x)["total_loss"].backward()
        grads.append({k: [p.grad.numpy() for p in v] for k, v in P.items()})
    total = {k: [a + b for a, b in zip(grads[0][k], grads[1][k])] for k in grads[0]}
    got, now = eng.download_grads(), eng.download_params()
    for n in ("PReLU1", "PReLU2", "PReLU3", "conv2"):
        err, one = rel_err(got[n][0], total[n][0]), rel_err(got[n][0], grads[1][n][0])
        print("ITER2 %s sum %.3g (against the second pass alone: %.3g)" % (n, err, one))
        assert err < 5e-4 and one > 0.05, (n, err, one)      # the sum of both passes - not what the last pass's launch wrote
    check_update(spec, params, now, {k: [0.5 * g for g in v] for k, v in total.items()}, lr, "pnet iter_size 2")
    s.close()


def test_a_snapshot_is_restored_exactly(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.mtcnn("pnet", "TRAIN", 4).replace('top: "conv3"\n  param { lr_mult: 1 decay_mult: 0 }',
                                                  'top: "conv3"\n  param { lr_mult: 1 decay_mult: 0 }\n  prelu_param { channel_shared: true }')
    spec = spec_of(txt, "TRAIN")
    assert spec.param_shapes["PReLU3"] == [()] and spec.param_shapes["PReLU2"] == [(16,)]      # both slope shapes
    params, x = act_params(spec, 70), inputs(spec, 71)
    a = solver(tmp_path, txt, lr=0.05, momentum=0.9)
    for l in spec.param_layers():
        a.engine.set_params(l.name, params[l.name])
    for k, v in x.items():
        a.engine.host_array(k)[...] = v
    a.step(2)
    a.snapshot()
    back = proto.read_caffemodel(str(tmp_path / "snap_iter_2.caffemodel"))
    assert back["PReLU3"][0].size == 1 and back["PReLU2"][0].shape == (16,)
    b = solver(tmp_path, txt, lr=0.05, momentum=0.9)
    b.restore(str(tmp_path / "snap_iter_2.solverstate"))
    assert b.iter == 2
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    assert pa["PReLU3"][0].shape == () and float(pa["PReLU3"][0]) != float(params["PReLU3"][0])      # it learned, and it is still one value
    ha, hb = a.engine.download_history(), b.engine.download_history()
    assert len(ha) == len(hb) and all(np.array_equal(u, v) for u, v in zip(ha, hb)) and any(np.abs(h).max() > 0 for h in ha)
    for k, v in x.items():
        b.engine.host_array(k)[...] = v
    oa, ob = a.step(1), b.step(1)
    assert oa["total_loss"] == ob["total_loss"]
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    a.close()
    b.close()


ENET_BLOBS = ["initial", "b1_0", "b1_4", "b2_0", "b2_2", "b2_3", "b2_8", "b3_8", "b4_0/unpool", "b4_0", "b4_2", "b5_0", "b5_1", "fullconv"]


def enet_labels(spec, x, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, ENET["classes"], spec.input_shapes["label"]).astype(F32)
    lab[rng.random(lab.shape) < 0.1] = 255.0      # ignored pixels
    x["label"] = lab
    return x


def test_enet_forward(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.enet("DEPLOY", **ENET)
    spec = spec_of(txt, "TEST")
    params, x = act_params(spec, 72), inputs(spec, 73)
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    net = load(tmp_path, txt, spec, params, "enet")
    eng = net._engine
    assert len([op for op in eng.ops if op.kind == "act"]) == 82
    net.blobs["data"].data[...] = x["data"]
    out = net.forward()
    for n in ENET_BLOBS + ["prob"]:
        err = rel_err(np.array(net.blobs[n].data).reshape(ref[n].shape), ref[n].numpy())
        print("ENET %s %.3g" % (n, err))
        assert err < TOL, (n, err)
    assert out["prob"].shape == (2, 5, 32, 64)


def test_enet_solver_step(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = models.enet("TRAIN", **ENET)
    spec = spec_of(txt, "TRAIN")
    params = act_params(spec, 74)
    x = enet_labels(spec, inputs(spec, 75), 76)
    lr = 0.01
    s = solver(tmp_path, txt, lr=lr)
    eng = s.engine
    kinds = [op.kind for op in eng.bwd_ops]
    assert kinds.count("act_bwd_param") == 82 and kinds.count("act_bwd") == 82
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = s.step(1)
    masks = {n: eng.read_blob(n + "_mask").astype(np.int64) for n in ("b1_0/pool", "b2_0/pool")}
    updates = {}
    P = as_torch(params, grad=True)
    B = torch_net(spec, P, x, dropout_seed=eng.dropout_seed, updates=updates, pool_argmax=masks)
    B["total_loss"].backward()
    want = float(B["total_loss"].detach())
    print("ENETSTEP loss %.6g want %.6g" % (out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want)
    got = eng.download_grads()
    worst = (0.0, None)
    for l in spec.layers:
        if l.type == "PReLU":
            worst = max(worst, (rel_err(got[l.name][0], P[l.name][0].grad.numpy()), l.name))
    print("ENETSTEP worst slope gradient %.3g at %s" % worst)
    assert worst[0] < 5e-4, worst
    check_update(spec, params, eng.download_params(), {k: [p.grad.numpy() if p.grad is not None else None for p in v] for k, v in P.items()}, lr,
                 "enet", updates)
    s.close()
