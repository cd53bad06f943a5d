"""ShuffleNet v1 (models.shufflenet_v1, groups = 3) and v2 (models.shufflenet_v2, 0.5x) through the public surface, -m gpu, against torch
in float64 on the CPU (tests/torch_shuffle_ref.py), in the style of tests/test_gpu_neuron_nets.py.

v1 at width_div 5 (stages of 48 / 96 / 192 channels, every group of every grouped convolution a multiple of 4) and v2 at width_div 3
(stages of 16 / 32 / 64, every branch 8 / 16 / 32: windows on 16 bytes of floats and of halves), 64 x 64, batch 2, 10 classes: 2 x 2
pixels at the last BatchNorm.  The parameters are tests/torch_resnet_ref.random_params.  v1 writes its depthwise layers as
ConvolutionDepthwise, v2 as Convolution with group: C - both spellings run.
  - caffe.Net from a prototxt and a caffemodel, TEST: named blobs and prob;
  - one caffe.SGDSolver step, TRAIN: the loss, every parameter gradient, and every blob after the update against w - lr * lr_mult * dw
    from autograd (BatchNorm: Caffe's moving-average step).  The reference takes the device's ReLU pass-through masks
    (tests/torch_shuffle_ref.py says why) - forward blobs and the loss adopt nothing;
  - v2: iter_size: 2 on two different batches - the gradient buffer holds the SUM of both passes - and a snapshot of a solver with
    momentum restored into a second solver: the same bits, and the next step the same bits;
  - v2 in halves against the float32 engine on the same weights.
Thresholds are the project's for nets, as tests/test_gpu_neuron_nets.py states them: rel_err < 1e-4 for blobs and the loss, < 5e-4 for
parameter gradients, 5e-3 for the half-float engine against the float32 one.  Where torch's own float32 run of the same graph is not
below a quarter of a threshold, the quantity is held to 4 x that error instead and the print says so.  A parameter gradient that is zero
in exact arithmetic (a shift in front of a BatchNorm) is measured against its layer's largest gradient
(tests/torch_neuron_ref.grad_errors)."""
import sys

import numpy as np
import pytest
import torch

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from torch_shuffle_ref import as_torch, device_masks, grad_errors, random_params, torch_net

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL, TOL_GRAD, TOL_F16 = 1e-4, 5e-4, 5e-3
KW = {"v1": dict(groups=3, width_div=5, size=64, batch=2, classes=10, depthwise_type="ConvolutionDepthwise"),
      "v2": dict(width=0.5, width_div=3, size=64, batch=2, classes=10, depthwise_type="Convolution")}
BLOBS = {"v1": ["conv1", "pool1", "resx1_conv1", "shuffle1", "resx1_conv2", "resx1_match_conv", "resx1_concat", "shuffle2", "resx2_elewise",
                "resx4_elewise", "shuffle5", "resx5_concat", "resx9_conv3", "resx12_elewise", "resx13_concat", "shuffle16", "resx16_elewise",
                "pool_ave", "fc1000"],
         "v2": ["conv1", "pool1", "stage2_1/left_conv", "stage2_1/conv2", "stage2_1/concat", "stage2_1/shuffle", "stage2_2/left", "stage2_2/right",
                "stage2_2/dw", "stage2_2/shuffle", "stage2_4/shuffle", "stage3_1/shuffle", "stage3_5/concat", "stage3_8/shuffle", "stage4_1/shuffle",
                "stage4_4/shuffle", "conv5", "pool_ave", "fc1000"]}


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def net_text(net, phase):
    return (models.shufflenet_v1 if net == "v1" else models.shufflenet_v2)(phase, **KW[net])


def spec_of(txt, phase):
    spec = NetSpec.public(proto.parse_text(txt), phase)
    spec.infer()
    return spec


def inputs(spec, seed):
    rng = np.random.default_rng(seed)
    x = {name: (rng.integers(0, 10, shp).astype(F32) if name == "label" else rng.standard_normal(shp).astype(F32))
         for name, shp in spec.input_shapes.items()}
    x["data"][1] = 2.0 * x["data"][1] + 0.5      # two images of different statistics
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


def shuffles(spec):
    return [l.name for l in spec.layers if l.type == "ShuffleChannel"]


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
    print("SHUFFLESTEP %s worst updated blob %.3g at %s" % (what, worst[0], worst[1]))


@pytest.mark.parametrize("net", ["v1", "v2"])
def test_forward(gpu, tmp_path, monkeypatch, net):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text(net, "DEPLOY")
    spec = spec_of(txt, "TEST")
    params, x = random_params(spec, 101), inputs(spec, 102)
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
        ref32 = torch_net(spec, as_torch(params, dtype=torch.float32), x, dtype=torch.float32)
    n = load(tmp_path, txt, spec, params, net)
    eng = n._engine
    assert [op.name for op in eng.ops if op.kind == "shuffle"] == shuffles(spec) and len(shuffles(spec)) == 16 and not eng.aux_dev
    n.blobs["data"].data[...] = x["data"]
    out = n.forward()
    for l in spec.layers:      # every shuffle moved its bottom's values, bit for bit
        if l.type == "ShuffleChannel":
            g, a, b = int(l.sub("shuffle_channel_param").get("group")), eng.read_blob(l.bottoms[0]), eng.read_blob(l.tops[0])
            nn, c, h, w = a.shape
            assert b.tobytes() == np.ascontiguousarray(a.reshape(nn, g, c // g, h, w).transpose(0, 2, 1, 3, 4)).tobytes(), l.name
            assert b.tobytes() != a.tobytes()
    for name in BLOBS[net] + ["prob"]:
        own = rel_err(ref32[name].numpy(), ref[name].numpy())
        err = rel_err(np.array(n.blobs[name].data).reshape(ref[name].shape), ref[name].numpy())
        print("SHUFFLENET %s %s %.3g (torch float32: %.3g -> held to %.3g)" % (net, name, err, own, allowed(TOL, own)))
        assert err < allowed(TOL, own), (name, err)
    assert out["prob"].shape == (2, 10, 1, 1) and np.allclose(out["prob"].reshape(2, 10).sum(axis=1), 1.0, atol=1e-5)
    a = eng.read_blob("prob").copy()
    eng.forward(use_graph=False)      # a forward without the captured graph: the same bytes
    assert a.tobytes() == eng.read_blob("prob").tobytes()


def reference_step(spec, params, x, eng):
    """(forward blobs, leaves with float64 gradients, leaves with float32 gradients, BatchNorm updates) of one step, with the device's
    ReLU masks."""
    masks = device_masks(spec, eng.read_blob)
    updates = {}
    with torch.no_grad():
        fwd = torch_net(spec, as_torch(params), x, updates=updates)
        fwd32 = torch_net(spec, as_torch(params, dtype=torch.float32), x, dtype=torch.float32)
    P = as_torch(params, grad=True)
    torch_net(spec, P, x, masks=masks)["total_loss"].backward()
    P32 = as_torch(params, grad=True, dtype=torch.float32)
    torch_net(spec, P32, x, dtype=torch.float32, masks=masks)["total_loss"].backward()
    return fwd, fwd32, P, P32, updates


@pytest.mark.parametrize("net", ["v1", "v2"])
def test_one_solver_step(gpu, tmp_path, monkeypatch, net):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text(net, "TRAIN")
    spec = spec_of(txt, "TRAIN")
    params, x = random_params(spec, 103), inputs(spec, 104)
    lr = 0.01
    s = solver(tmp_path, txt, lr=lr)
    eng = s.engine
    assert [op.name for op in eng.bwd_ops if op.kind == "shuffle_bwd"] == shuffles(spec)[::-1]
    assert not any(n in eng.aux_dev for n in shuffles(spec))
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = s.step(1)
    fwd, fwd32, P, P32, updates = reference_step(spec, params, x, eng)
    want = float(fwd["total_loss"])
    own_loss = abs(float(fwd32["total_loss"]) - want) / abs(want)
    print("SHUFFLESTEP %s loss %.6g want %.6g (torch float32: %.3g)" % (net, out["total_loss"], want, own_loss))
    assert abs(out["total_loss"] - want) < allowed(TOL, own_loss) * abs(want)
    for name in BLOBS[net]:
        own = rel_err(fwd32[name].numpy(), fwd[name].numpy())
        err = rel_err(eng.read_blob(name).reshape(fwd[name].shape), fwd[name].numpy())
        print("SHUFFLESTEP %s blob %s %.3g (torch float32: %.3g -> held to %.3g)" % (net, name, err, own, allowed(TOL, own)))
        assert err < allowed(TOL, own), (name, err)
    got = eng.download_grads()
    worst = (0.0, None)
    for l in spec.param_layers():
        if l.type == "BatchNorm":
            continue
        errs = grad_errors(got[l.name], [r.grad.numpy() for r in P[l.name]], [r.grad.numpy() for r in P32[l.name]])
        for i, (err, own) in enumerate(errs):
            worst = max(worst, (err, "%s[%d] own %.3g" % (l.name, i, own)))
            print("SHUFFLEGRAD %s %s[%d] %.3g (torch float32: %.3g -> held to %.3g)" % (net, l.name, i, err, own, allowed(TOL_GRAD, own)))
            assert err < allowed(TOL_GRAD, own), "gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, err, own)
    print("SHUFFLEGRAD %s worst %.3g at %s" % (net, worst[0], worst[1]))
    check_update(spec, params, eng.download_params(), {k: [p.grad.numpy() if p.grad is not None else None for p in v] for k, v in P.items()}, lr,
                 net, updates)
    s.close()


def test_iter_size_2_sums_the_gradients(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text("v2", "TRAIN")
    spec = spec_of(txt, "TRAIN")
    params = random_params(spec, 105)
    batches = [inputs(spec, 106), inputs(spec, 107)]
    s = solver(tmp_path, txt, extra="iter_size: 2\n", lr=0.02)
    eng = s.engine
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])

    def feed(j):
        for k, v in batches[j].items():
            eng.host_array(k)[...] = v
    eng.step(seed=5, feed=feed)
    grads = []
    for x in batches:
        P = as_torch(params, grad=True)
        torch_net(spec, P, x)["total_loss"].backward()
        grads.append({k: [p.grad.numpy() if p.grad is not None else None for p in v] for k, v in P.items()})
    got = eng.download_grads()
    for n in ("conv1", "stage2_1/left_dw", "stage2_2/conv1", "stage3_4/dw", "stage4_2/conv2_scale", "conv5"):
        total = grads[0][n][0] + grads[1][n][0]
        err, one = rel_err(np.asarray(got[n][0]).reshape(total.shape), total), rel_err(np.asarray(got[n][0]).reshape(total.shape), grads[1][n][0])
        print("SHUFFLEITER2 %s sum %.3g (against the second pass alone: %.3g)" % (n, err, one))
        assert err < TOL_GRAD and one > 0.05, (n, err, one)      # the sum of both passes - not what the last pass's launches wrote
    s.close()


def test_a_snapshot_is_restored_exactly(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text("v2", "TRAIN")
    spec = spec_of(txt, "TRAIN")
    params, x = random_params(spec, 108), inputs(spec, 109)
    a = solver(tmp_path, txt, lr=0.02, momentum=0.9)
    for l in spec.param_layers():
        a.engine.set_params(l.name, params[l.name])
    for k, v in x.items():
        a.engine.host_array(k)[...] = v
    a.step(2)
    a.snapshot()
    back = proto.read_caffemodel(str(tmp_path / "snap_iter_2.caffemodel"))
    assert not any(n in back for n in shuffles(spec))      # no blob: a ShuffleChannel is not in the file
    assert back["stage2_2/dw"][0].shape == tuple(spec.param_shapes["stage2_2/dw"][0])
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


def test_v2_in_halves_against_the_float32_engine(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt = net_text("v2", "DEPLOY")
    spec = spec_of(txt, "TEST")
    params, x = random_params(spec, 110), inputs(spec, 111)
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    names = BLOBS["v2"] + ["prob"]
    got = {}
    for tag, kw in (("f32", {}), ("f16", {"dtype": "f16"})):
        n = load(tmp_path, txt, spec, params, "v2" + tag, **kw)
        eng = n._engine
        assert [op.name for op in eng.ops if op.kind == "shuffle"] == shuffles(spec) and eng.f16 == (tag == "f16")
        if tag == "f16":
            assert all(eng.blobs[l.tops[0]].esize == 2 for l in spec.layers if l.type == "ShuffleChannel")
        n.blobs["data"].data[...] = x["data"]
        n.forward()
        got[tag] = {b: eng.read_blob(b).astype(np.float64).reshape(ref[b].shape) for b in names}
        if tag == "f16":      # the half kernel moves halves, bit for bit
            a, b = eng.read_blob("stage3_2/concat"), eng.read_blob("stage3_2/shuffle")
            nn, c, h, w = a.shape
            assert np.array_equal(b, a.reshape(nn, 2, c // 2, h, w).transpose(0, 2, 1, 3, 4).reshape(a.shape)) and not np.array_equal(a, b)
    for b in names:
        e32, e16 = rel_err(got["f32"][b], ref[b].numpy()), rel_err(got["f16"][b], got["f32"][b])
        print("SHUFFLEF16 %s f32 vs float64 %.3g, halves vs f32 %.3g" % (b, e32, e16))
        assert e16 < TOL_F16, (b, e16)
