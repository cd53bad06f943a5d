"""MobileNet-v2 with ReLU6 (models.mobilenet_v2(relu6=True)) and EfficientNet-B0 (models.efficientnet_b0) through the public surface,
-m gpu, against torch in float64 on the CPU (tests/torch_neuron_ref.py), in the style of tests/test_gpu_act_nets.py.

Both nets at width_div 4, 64 x 64, batch 2, 10 classes: 2 x 2 pixels at the last BatchNorm (with one pixel and a batch of 2 the batch
statistics are degenerate).  The parameters are tests/torch_resnet_ref.random_params, the biases of the excite layers spread so that the
SE gates lie all over (0.1, 0.9).
  - caffe.Net from a prototxt and a caffemodel, TEST: named blobs and prob;
  - one caffe.SGDSolver step, TRAIN: the loss, every parameter gradient, and every blob after the update against w - lr * lr_mult * dw
    from autograd (BatchNorm: Caffe's moving-average step).  The reference takes the device's Dropout mask (EfficientNet) and the
    device's ReLU6 pass-through masks (MobileNet; tests/torch_neuron_ref.py says why) - forward blobs and the loss adopt nothing;
  - EfficientNet: iter_size: 2 on two different batches - the gradient buffer holds the SUM of both passes, not what the
    last pass's launches wrote - and a snapshot of a solver with momentum restored into a second solver: the same bits, and the next step the same bits;
  - MobileNet-v2 with ReLU6 in halves against the float32 engine on the same weights.
Thresholds are the project's for nets: rel_err < 1e-4 for blobs and the loss, < 5e-4 for parameter gradients, 5e-3 for the half-float
engine against the float32 one.  Where torch's own float32 run of the same graph is not below a quarter of a threshold, the quantity is
held to 4 x that error instead and the print says so (tests/test_gpu_mobilenet.py, tests/test_gpu_interp_nets.py).  A parameter gradient that
is zero in exact arithmetic (a shift in front of a BatchNorm) is measured against its layer's largest gradient
(tests/torch_neuron_ref.grad_errors)."""
import sys

import numpy as np
import pytest
import torch

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from torch_neuron_ref import as_torch, device_masks, grad_errors, neuron_params, torch_net

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL, TOL_GRAD, TOL_F16 = 1e-4, 5e-4, 5e-3
KW = dict(width_div=4, size=64, batch=2, classes=10)
MB2_BLOBS = ["conv1", "conv2_1/dwise", "conv2_1/linear", "conv3_1/expand", "block_3_2", "conv4_1/dwise", "block_4_3", "block_5_4", "conv6_1/linear",
             "block_7_3", "conv8_1/linear", "conv9", "pool6", "fc7"]
EFF_BLOBS = ["conv1", "conv2_1/dwise", "conv2_1/se_reduce", "conv2_1/se_prob", "conv2_1/se_scale", "conv2_1/project", "conv3_1/expand", "block_3_2",
             "conv4_1/dwise", "block_4_2", "conv5_1/se_prob", "block_5_3", "block_6_3", "conv7_1/dwise", "block_7_4", "conv8_1/project", "conv9",
             "pool6", "fc7"]


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def net_text(net, phase):
    return models.mobilenet_v2(phase, relu6=True, **KW) if net == "mobilenet_v2" else models.efficientnet_b0(phase, **KW)


def spec_of(txt, phase):
    spec = NetSpec.public(proto.parse_text(txt), phase)
    spec.infer()
    return spec


def inputs(spec, seed):
    rng = np.random.default_rng(seed)
    x = {name: (rng.integers(0, KW["classes"], shp).astype(F32) if name == "label" else rng.standard_normal(shp).astype(F32))
         for name, shp in spec.input_shapes.items()}
    x["data"][1] = 2.0 * x["data"][1] + 0.5      # two images of different statistics: their SE gates differ
    return x


def allowed(project, own):
    """The project's threshold where the reference's own float32 error is below a quarter of it, else 4 x that error."""
    return project if own < project / 4 else 4 * own


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


def check_update(spec, params, now, grads, lr, what, updates):
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
    print("NEURONSTEP %s worst updated blob %.3g at %s" % (what, worst[0], worst[1]))


@pytest.mark.parametrize("net", ["mobilenet_v2", "efficientnet_b0"])
def test_forward(gpu, tmp_path, monkeypatch, net):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text(net, "DEPLOY")
    spec = spec_of(txt, "TEST")
    params, x = neuron_params(spec, 81), inputs(spec, 82)
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
        ref32 = torch_net(spec, as_torch(params, dtype=torch.float32), x, dtype=torch.float32)
    n = load(tmp_path, txt, spec, params, net)
    eng = n._engine
    acts = [l.name for l in spec.layers if l.type in ("ReLU6", "Swish")]
    assert [op.name for op in eng.ops if op.kind == "neuron"] == acts and len(acts) == (35 if net == "mobilenet_v2" else 49) and not eng.aux_dev
    n.blobs["data"].data[...] = x["data"]
    out = n.forward()
    if net == "mobilenet_v2":      # the clip is at work: values sit on both bounds
        y = eng.read_blob("conv1")
        assert (y == 0.0).any() and (y == 6.0).any() and y.min() == 0.0 and y.max() == 6.0
    else:                           # the gates are spread
        g = eng.read_blob("conv4_1/se_prob")
        assert g.min() < 0.3 and g.max() > 0.7
    for name in (MB2_BLOBS if net == "mobilenet_v2" else EFF_BLOBS) + ["prob"]:
        own = rel_err(ref32[name].numpy(), ref[name].numpy())
        err = rel_err(np.array(n.blobs[name].data).reshape(ref[name].shape), ref[name].numpy())
        print("NEURONNET %s %s %.3g (torch float32: %.3g -> held to %.3g)" % (net, name, err, own, allowed(TOL, own)))
        assert err < allowed(TOL, own), (name, err)
    assert out["prob"].shape == (2, 10, 1, 1) and np.allclose(out["prob"].reshape(2, 10).sum(axis=1), 1.0, atol=1e-5)
    a = eng.read_blob("prob").copy()
    eng.forward(use_graph=False)      # a forward without the captured graph: the same bytes
    assert a.tobytes() == eng.read_blob("prob").tobytes()


def reference_step(spec, params, x, eng):
    """(forward blobs, leaves with float64 gradients, leaves with float32 gradients, BatchNorm updates) of one step, with the device's
    Dropout mask and ReLU6 masks."""
    masks = device_masks(spec, eng.read_blob)
    updates = {}
    with torch.no_grad():
        fwd = torch_net(spec, as_torch(params), x, dropout_seed=eng.dropout_seed, updates=updates)
        fwd32 = torch_net(spec, as_torch(params, dtype=torch.float32), x, dtype=torch.float32, dropout_seed=eng.dropout_seed)
    P = as_torch(params, grad=True)
    torch_net(spec, P, x, dropout_seed=eng.dropout_seed, masks=masks)["total_loss"].backward()
    P32 = as_torch(params, grad=True, dtype=torch.float32)
    torch_net(spec, P32, x, dtype=torch.float32, dropout_seed=eng.dropout_seed, masks=masks)["total_loss"].backward()
    return fwd, fwd32, P, P32, updates


@pytest.mark.parametrize("net", ["mobilenet_v2", "efficientnet_b0"])
def test_one_solver_step(gpu, tmp_path, monkeypatch, net):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text(net, "TRAIN")
    spec = spec_of(txt, "TRAIN")
    params, x = neuron_params(spec, 83), inputs(spec, 84)
    lr = 0.01
    s = solver(tmp_path, txt, lr=lr)
    eng = s.engine
    acts = [l.name for l in spec.layers if l.type in ("ReLU6", "Swish")]
    assert [op.name for op in eng.bwd_ops if op.kind == "neuron_bwd"] == acts[::-1]
    assert sorted(n for n in eng.aux_dev if n in acts) == (sorted(acts) if net == "efficientnet_b0" else [])      # the kept copies: Swish alone
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = s.step(1)
    fwd, fwd32, P, P32, updates = reference_step(spec, params, x, eng)
    want = float(fwd["total_loss"])
    own_loss = abs(float(fwd32["total_loss"]) - want) / abs(want)
    print("NEURONSTEP %s loss %.6g want %.6g (torch float32: %.3g)" % (net, out["total_loss"], want, own_loss))
    assert abs(out["total_loss"] - want) < allowed(TOL, own_loss) * abs(want)
    for name in (MB2_BLOBS if net == "mobilenet_v2" else EFF_BLOBS):
        own = rel_err(fwd32[name].numpy(), fwd[name].numpy())
        err = rel_err(eng.read_blob(name).reshape(fwd[name].shape), fwd[name].numpy())
        print("NEURONSTEP %s blob %s %.3g (torch float32: %.3g -> held to %.3g)" % (net, name, err, own, allowed(TOL, own)))
        assert err < allowed(TOL, own), (name, err)
    got = eng.download_grads()
    worst = (0.0, None)
    for l in spec.param_layers():
        if l.type == "BatchNorm":
            continue
        errs = grad_errors(got[l.name], [r.grad.numpy() for r in P[l.name]], [r.grad.numpy() for r in P32[l.name]])
        for i, (err, own) in enumerate(errs):
            worst = max(worst, (err, "%s[%d] own %.3g" % (l.name, i, own)))
            print("NEURONGRAD %s %s[%d] %.3g (torch float32: %.3g -> held to %.3g)" % (net, l.name, i, err, own, allowed(TOL_GRAD, own)))
            assert err < allowed(TOL_GRAD, own), "gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, err, own)
    print("NEURONGRAD %s worst %.3g at %s" % (net, worst[0], worst[1]))
    check_update(spec, params, eng.download_params(), {k: [p.grad.numpy() if p.grad is not None else None for p in v] for k, v in P.items()}, lr,
                 net, updates)
    s.close()


def test_iter_size_2_sums_the_gradients(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text("efficientnet_b0", "TRAIN")
    spec = spec_of(txt, "TRAIN")
    params = neuron_params(spec, 85)
    batches = [inputs(spec, 86), inputs(spec, 87)]
    lr = 0.02
    s = solver(tmp_path, txt, extra="iter_size: 2\n", lr=lr)
    eng = s.engine
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])

    def feed(j):
        for k, v in batches[j].items():
            eng.host_array(k)[...] = v
    eng.step(seed=5, feed=feed)      # (one Dropout seed for both passes)
    grads = []
    for x in batches:
        P = as_torch(params, grad=True)
        torch_net(spec, P, x, dropout_seed=5)["total_loss"].backward()
        grads.append({k: [p.grad.numpy() if p.grad is not None else None for p in v] for k, v in P.items()})
    got = eng.download_grads()
    for n in ("conv1", "conv2_1/se_reduce", "conv4_1/expand", "conv5_2/dwise", "conv8_1/project/scale"):
        total = grads[0][n][0] + grads[1][n][0]
        err, one = rel_err(np.asarray(got[n][0]).reshape(total.shape), total), rel_err(np.asarray(got[n][0]).reshape(total.shape), grads[1][n][0])
        print("NEURONITER2 %s sum %.3g (against the second pass alone: %.3g)" % (n, err, one))
        assert err < TOL_GRAD and one > 0.05, (n, err, one)      # the sum of both passes - not what the last pass's launches wrote
    s.close()


def test_a_snapshot_is_restored_exactly(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text("efficientnet_b0", "TRAIN")
    spec = spec_of(txt, "TRAIN")
    params, x = neuron_params(spec, 88), inputs(spec, 89)
    a = solver(tmp_path, txt, lr=0.02, momentum=0.9)
    for l in spec.param_layers():
        a.engine.set_params(l.name, params[l.name])
    for k, v in x.items():
        a.engine.host_array(k)[...] = v
    a.step(2)
    a.snapshot()
    back = proto.read_caffemodel(str(tmp_path / "snap_iter_2.caffemodel"))
    assert not any(l.name in back for l in spec.layers if l.type == "Swish")      # no blob: a Swish is not in the file
    assert back["conv2_1/se_reduce"][0].shape == tuple(spec.param_shapes["conv2_1/se_reduce"][0])
    b = solver(tmp_path, txt, lr=0.02, momentum=0.9)
    b.restore(str(tmp_path / "snap_iter_2.solverstate"))
    assert b.iter == 2
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    assert np.abs(pa["conv1"][0] - params["conv1"][0]).max() > 0
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


@pytest.mark.parametrize("net", ["mobilenet_v2"])
def test_in_halves_against_the_float32_engine(gpu, tmp_path, monkeypatch, net):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text(net, "DEPLOY")
    spec = spec_of(txt, "TEST")
    params, x = neuron_params(spec, 90), inputs(spec, 91)
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    acts = [l.name for l in spec.layers if l.type in ("ReLU6", "Swish")]
    names = (MB2_BLOBS if net == "mobilenet_v2" else EFF_BLOBS) + ["prob"]
    got = {}
    for tag, kw in (("f32", {}), ("f16", {"dtype": "f16"})):
        n = load(tmp_path, txt, spec, params, net + tag, **kw)
        eng = n._engine
        assert [op.name for op in eng.ops if op.kind == "neuron"] == acts and eng.f16 == (tag == "f16")
        if tag == "f16":
            assert all(eng.blobs[l.tops[0]].esize == 2 for l in spec.layers if l.type in ("ReLU6", "Swish"))
        n.blobs["data"].data[...] = x["data"]
        n.forward()
        got[tag] = {b: eng.read_blob(b).astype(np.float64).reshape(ref[b].shape) for b in names}
    if net == "mobilenet_v2":
        assert got["f16"]["conv1"].max() == 6.0 and got["f16"]["conv1"].min() == 0.0
    for b in names:
        e32, e16 = rel_err(got["f32"][b], ref[b].numpy()), rel_err(got["f16"][b], got["f32"][b])
        print("NEURONF16 %s %s f32 vs float64 %.3g, halves vs f32 %.3g" % (net, b, e32, e16))
        assert e16 < TOL_F16, (b, e16)
