"""ResNet-50 (models.resnet) and the BatchNorm / Scale forms through the public surface, -m gpu, against torch in float64 on the CPU
(tests/torch_resnet_ref.py), in the style of tests/test_gpu_classifier_nets.py.

The net: depth 50 at width_div 8 (widths 8 .. 256: every blob whole 16-byte groups of floats and of halves), batch 2, size 128 - the
smallest size at which every BatchNorm sees at least 32 values per channel (res5*: 2 x 4 x 4; bn_conv1: 2 x 64 x 64 = 8192).

Thresholds are the project's: rel_err < 1e-4 for blobs and the loss, < 5e-4 for parameter gradients, 5e-3 for the half-float engine.
Where the reference's OWN float32 error is too close to them the rule of the other published-net files applies: the same case runs in
torch float32 on the CPU against the float64 net - an error of the reference alone - and the threshold of that quantity is the larger of
the project's and 4 x that error (the 4 allows for a different, equally valid summation order).  Measured on the CPU for the training
step below (seed 3 / inputs 5): interior blobs 4.6e-7 (conv1) .. 9.2e-5 (res5c) -> res5c is held to 3.7e-4, every other blob listed to
1e-4; parameter gradients at most 1.9e-4 (scale5c_branch2a) -> 7.4e-4 there, 5e-4 for most.  A batch of 2 leaves BatchNorm badly
conditioned: m = 32 values per channel in stage 5 amplify every rounding of the forward pass.
The backward comparison adopts the device's ReLU masks in the reference (torch_net(relu_masks=...)): two independently rounded
forward passes flip a few near-zero activations, and through 16 residual blocks one flipped unit moves gradients by 1e-2 (torch float32
against torch float64 WITHOUT the adoption: 2e-2 at scale5b_branch2a) - a property of ReLU, not of a kernel.  Forward blobs and the
loss are compared without any adoption.  conv1's bias gradient is mathematically zero (a constant per channel in front of a
batch-statistics BatchNorm): instead of a relative error it is held to the allowance of a float32 sum of the m values of dY per channel
(ref64.dot_bound_rms on sum |dY|), or to 4 x what torch float32 leaves of it where that is larger."""
import os
import sys

import numpy as np
import pytest
import torch

import ref64
from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_resnet_ref import as_torch, random_params, torch_net

pytestmark = pytest.mark.gpu
KW = dict(depth=50, batch=2, num_classes=10, width_div=8, size=128)
INTERIOR = ["conv1", "pool1", "res2a_branch1", "res2a", "res2c", "res3a", "res3d", "res4f", "res5a", "res5c", "pool5", "fc1000"]
F32 = np.float32


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def make(phase, text=None, **over):
    txt = text if text is not None else models.resnet(phase, **dict(KW, **over))
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TEST" if phase == "DEPLOY" else phase)
    spec.infer()
    return txt, msg, spec


def inputs_for(spec, seed, classes=10):
    rng = np.random.default_rng(seed)
    return {name: (rng.integers(0, classes, shp).astype(F32) if name == "label" else rng.standard_normal(shp).astype(F32))
            for name, shp in spec.input_shapes.items()}


def own_error(spec, params, x, names, **kw):
    """rel_err of torch float32 against torch float64 for the named blobs: the reference's own rounding error."""
    with torch.no_grad():
        a = torch_net(spec, as_torch(params), x, **kw)
        b = torch_net(spec, as_torch(params, dtype=torch.float32), x, dtype=torch.float32, **kw)
    return {n: rel_err(b[n].numpy(), a[n].numpy()) for n in names}


def test_test_phase_forward_through_caffe_net(gpu, tmp_path, monkeypatch):
    """Global statistics from moving sums that are not the fillers' zeros and a factor of 2.5, computed in the apply launch's prologue."""
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    txt, msg, spec = make("TEST")
    path, weights = str(tmp_path / "test.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(txt)
    params = random_params(spec, 11)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST)
    eng = net._engine
    kinds = [op.kind for op in eng.ops]
    assert kinds.count("bn_apply") == 53 and "bn_stats" not in kinds and "relu" in kinds      # (relu: the ones on the Eltwise tops)
    assert not eng.aux_dev, "an inference engine keeps nothing for a backward pass"
    x = inputs_for(spec, 1)
    for k, v in x.items():
        net.blobs[k].data[...] = v
    out = net.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    own = own_error(spec, params, x, INTERIOR)
    for name in INTERIOR:
        err = rel_err(net.blobs[name].data, ref[name].numpy())
        print("NET %s %.3g (torch float32: %.3g)" % (name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    for name in net.outputs:
        want = float(ref[name])
        assert abs(float(out[name]) - want) <= 1e-4 * max(abs(want), 1e-30), (name, float(out[name]), want)
    for l in spec.param_layers():
        for i, want in enumerate(params[l.name]):
            assert np.array_equal(eng.read_param(l.name, i), want), l.name


def test_half_float_engine_forward_through_caffe_net(gpu, tmp_path, monkeypatch):
    """The reference rounds where the engine rounds: every half blob as it is stored (once per fused chain - the BatchNorm, Scale and ReLU
    of a chain are one launch in float32), banks that read a half blob as halves.  BatchNorm and Scale blobs stay float32."""
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    txt, msg, spec = make("DEPLOY")
    path, weights = str(tmp_path / "deploy.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(txt)
    params = random_params(spec, 12)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST, dtype="f16")
    eng = net._engine
    assert eng.f16 and eng.blobs["res3a"].esize == 2
    x = inputs_for(spec, 2)
    for k, v in x.items():
        net.blobs[k].data[...] = v
    out = net.forward()
    r16 = lambda a: np.asarray(a, F32).astype(np.float16).astype(F32)
    half_bank = {l.name for l in spec.param_layers() if l.type in ("Convolution", "InnerProduct") and eng.blobs[l.bottoms[0]].esize == 2}
    p16 = {k: [r16(v[0]) if k in half_bank else v[0]] + list(v[1:]) for k, v in params.items()}
    absorbed = {q.name for ch in eng._bn_chains.values() for q in (ch.bn, ch.scale, ch.relu) if q is not None} - \
               {[q for q in (ch.relu, ch.scale, ch.bn) if q is not None][0].name for ch in eng._bn_chains.values()}
    # a chain stores its blob once, behind its last layer; the convolution in front of an in-place chain stores halves too
    layers = iter([l for l in spec.layers if l.type != "Input"])

    def rnd(name, y):
        l = next(layers)
        if l.name in absorbed or eng.blobs[name].esize != 2:
            return y
        return y.to(torch.float16).to(torch.float64)
    with torch.no_grad():
        ref = torch_net(spec, as_torch(p16), x, round_blob=rnd)
    for name in INTERIOR + list(eng.outputs):
        err = rel_err(eng.read_blob(name), ref[name].numpy())
        print("F16NET %s %.3g" % (name, err))
        assert err < 5e-3, name
    assert out["prob"].dtype == F32 and abs(float(out["prob"].sum()) - 2.0) < 1e-3


def _train_engine(monkeypatch, graph, text=None, seed=3, phase_kw=None):
    monkeypatch.setenv("FCN_NO_GRAPH", "0" if graph else "1")
    txt, msg, spec = make("TRAIN", text)
    params = random_params(spec, seed)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    return spec, params, eng


def relu_masks_of(eng, spec):
    return {l.name: eng.read_blob(l.tops[0]) > 0 for l in spec.layers if l.type == "ReLU"}


def check_step(eng, spec, params, x, out, interior, label=""):
    """Loss, interior blobs, parameter gradients of one step against torch float64 under the rule of the module text.  Returns the
    float64 BatchNorm updates of that forward pass."""
    updates = {}
    with torch.no_grad():
        fwd = torch_net(spec, as_torch(params), x, updates=updates)
    own = own_error(spec, params, x, interior)
    want = float(fwd["total_loss"])
    print("STEP %s loss %.6g want %.6g" % (label, out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want), (out["total_loss"], want)
    for name in interior:
        err = rel_err(eng.read_blob(name), fwd[name].numpy())
        print("BLOB %s %s %.3g (torch float32: %.3g)" % (label, name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    masks = relu_masks_of(eng, spec)
    P = as_torch(params, grad=True)
    torch_net(spec, P, x, relu_masks=masks)["total_loss"].backward()
    P32 = as_torch(params, grad=True, dtype=torch.float32)
    torch_net(spec, P32, x, relu_masks=masks, dtype=torch.float32)["total_loss"].backward()
    got = eng.download_grads()
    # a bias directly in front of a batch-statistics BatchNorm adds a constant per channel that the layer subtracts again
    dead_bias = {q.name for ch in eng._bn_chains.values() if ch.bn is not None and not ch.global_stats
                 for q in spec.layers if q.type in ("Convolution", "InnerProduct") and q.tops == [ch.x] and len(spec.param_shapes[q.name]) > 1}
    worst = (0.0, None)
    for l in spec.param_layers():
        if l.type == "BatchNorm":
            assert all(not g.any() for g in got[l.name]), "gradient segments of %s must stay exactly zero" % l.name
            continue
        assert eng._learns(l), l.name
        for i, (g, r, r32) in enumerate(zip(got[l.name], P[l.name], P32[l.name])):
            assert g.shape == tuple(r.grad.shape), l.name
            if l.name in dead_bias and i == 1:
                # mathematically zero: what is left is the rounding of a float32 sum of the m values of dY per channel (magnitude term
                # sum |dY|, the device's own dY), or 4 x what torch float32 leaves of it, whichever is larger
                dy = np.abs(eng.read_grad(l.tops[0]).astype(np.float64))
                dy = dy.reshape(dy.shape[0], dy.shape[1], -1)
                allow = np.maximum(ref64.dot_bound_rms(dy.shape[0] * dy.shape[2], dy.sum(axis=(0, 2))), 4 * np.abs(r32.grad.numpy()).max())
                print("DEAD BIAS %s %s %.3g of its allowance" % (label, l.name, float((np.abs(g) / allow).max())))
                assert np.all(np.abs(g) <= allow), "bias gradient in front of a batch-statistics BatchNorm"
                continue
            own_g = rel_err(r32.grad.numpy(), r.grad.numpy())
            err = rel_err(g, r.grad.numpy())
            worst = max(worst, (err, "%s[%d] own %.3g" % (l.name, i, own_g)))
            assert err < max(5e-4, 4 * own_g), "parameter gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, err, own_g)
    print("GRAD %s worst %.3g at %s" % (label, worst[0], worst[1]))
    return updates


@pytest.mark.parametrize("graph", [True, False])
def test_one_training_step(gpu, monkeypatch, graph):
    spec, params, eng = _train_engine(monkeypatch, graph)
    fk, bk = [op.kind for op in eng.ops], [(op.kind, op.name) for op in eng.bwd_ops]
    assert fk.count("bn_stats") == 53 and fk.count("bn_apply") == 53 and len(eng._bn_chains) == 53
    assert sum(k == "bn_bwd_reduce" for k, _ in bk) == 53 and sum(k == "bn_bwd_apply" for k, _ in bk) == 53
    assert sum(ch.relu is not None for ch in eng._bn_chains.values()) == 33 and all(ch.scale is not None for ch in eng._bn_chains.values())
    assert set(eng.aux_dev) >= set(eng._bn_chains), "x-hat of every chain is kept for the backward pass"
    assert sorted(op.layers[0] for op in eng.bwd_ops if op.kind == "bn_bwd_apply") == sorted(l.name for l in spec.layers if l.type == "Scale")
    x = inputs_for(spec, 5)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step()
    updates = check_step(eng, spec, params, x, out, INTERIOR, "graph=%d" % graph)
    # the three blobs after one step and after three (base_lr 0: the same batch statistics enter three times)
    g1 = eng.download_grads()
    now = eng.download_params()
    for l in spec.layers:
        if l.type == "BatchNorm":
            for i in range(3):
                assert rel_err(now[l.name][i], updates[l.name][i]) < 1e-4, (l.name, i)
    eng.step()
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k])), "the same step again: the same bits"
    eng.step()
    now3 = eng.download_params()
    f = 0.999
    for l in spec.layers:
        if l.type == "BatchNorm":
            b0, b1, b2 = (np.asarray(v, np.float64) for v in params[l.name])
            m0, m1 = updates[l.name][0] - b0 * f, updates[l.name][1] - b1 * f      # the batch's mean and corrected variance
            for i, (start, add) in enumerate(((b0, m0), (b1, m1), (b2, 1.0))):
                want = start
                for _ in range(3):
                    want = want * f + add
                assert rel_err(now3[l.name][i], want) < 1e-4, (l.name, i)
        elif l.name in now:
            assert all(np.array_equal(a, b) for a, b in zip(now3[l.name], params[l.name])), l.name
    eng.close()


def test_frozen_batchnorm_in_a_training_net(gpu, monkeypatch):
    """use_global_stats: true in TRAIN: the blobs normalise and never move, dx = gamma invstd dy', gamma and beta still learn."""
    txt = models.resnet("TRAIN", **KW)
    three = "\n".join(["  param { lr_mult: 0 decay_mult: 0 }"] * 3)
    assert txt.count(three) == 53
    spec, params, eng = _train_engine(monkeypatch, True, text=txt.replace(three, three + "\n  batch_norm_param { use_global_stats: true }"))
    fk, bk = [op.kind for op in eng.ops], [op.kind for op in eng.bwd_ops]
    assert "bn_stats" not in fk and fk.count("bn_apply") == 53 and bk.count("bn_bwd_reduce") == 53 and bk.count("bn_bwd_apply") == 53
    x = inputs_for(spec, 6)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step()
    check_step(eng, spec, params, x, out, INTERIOR[-4:], "frozen")
    now = eng.download_params()
    assert all(np.array_equal(a, b) for k in params for a, b in zip(now[k], params[k]))
    eng.close()


def test_sgd_solver_with_a_test_net_snapshot_and_restore(gpu, tmp_path, monkeypatch):
    """The test net reads the training net's blobs in place: after k steps its score is that of the torch eval-mode net built from
    read_param - the CURRENT moving averages - and a snapshot restores every blob, the (1,) factor included, exactly."""
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    train, test = tmp_path / "train.prototxt", tmp_path / "test.prototxt"
    train.write_text(models.resnet("TRAIN", **KW))
    test.write_text(models.resnet("TEST", **KW))
    job = tmp_path / "solver.prototxt"
    job.write_text('train_net: "%s"\ntest_net: "%s"\ntest_iter: 1\ntest_interval: 1000\ntest_initialization: false\nbase_lr: 0.002\n'
                   'momentum: 0.9\nweight_decay: 1e-4\nlr_policy: "fixed"\nmax_iter: 100\nsnapshot_prefix: "%s"\n' % (train, test, tmp_path / "snap"))
    _, _, spec = make("TRAIN")
    _, _, tspec = make("TEST")
    x = inputs_for(spec, 8)

    def start():
        s = caffe.SGDSolver(str(job), log=None, autotune=False)
        for k, v in x.items():
            s.engine.host_array(k)[...] = v
        return s
    a = start()
    losses = [a.step(1)["loss"] for _ in range(4)]      # (one batch of two images, again and again)
    print("LOSSES", losses)
    assert all(np.isfinite(losses)) and min(losses[1:]) < losses[0], losses
    fac = a.engine.read_param("bn_conv1", 2)
    assert fac.shape == (1,) and abs(float(fac[0]) - (1 + 0.999 + 0.999 ** 2 + 0.999 ** 3)) < 1e-5
    tn = a.test_nets[0]
    assert tn.engine.shared_layers >= {"bn_conv1", "scale_conv1", "conv1", "fc1000"}
    for k, v in x.items():
        tn.engine.host_array(k)[...] = v
    score = a.test(0)
    now = {l.name: [tn.engine.read_param(l.name, i) for i in range(len(tspec.param_shapes[l.name]))] for l in tspec.param_layers()}
    assert np.array_equal(now["bn5c_branch2c"][0], a.engine.read_param("bn5c_branch2c", 0)) and now["bn_conv1"][0].any()
    with torch.no_grad():
        ref = torch_net(tspec, as_torch(now), x)
    own = own_error(tspec, now, x, ["fc1000"])["fc1000"]
    print("SCORE loss %.6g want %.6g accuracy %.3g want %.3g (fc1000, torch float32: %.3g)" % (
        float(score["loss"]), float(ref["loss"]), float(score["accuracy"]), float(ref["accuracy"]), own))
    assert abs(float(score["loss"]) - float(ref["loss"])) < max(1e-4, 4 * own) * abs(float(ref["loss"]))
    assert float(score["accuracy"]) == float(ref["accuracy"])
    a.snapshot()
    b = start()
    b.restore(str(tmp_path / "snap_iter_4.solverstate"))
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    assert pb["bn_conv1"][2].shape == (1,) and float(pb["bn_conv1"][2][0]) == float(pa["bn_conv1"][2][0]) > 3.9
    la, lb = [a.step(1)["loss"] for _ in range(2)], [b.step(1)["loss"] for _ in range(2)]
    assert la == lb
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(u, v) for k in pa for u, v in zip(pa[k], pb[k]))
    a.close()
    b.close()


# the reference's train/bounding_box/deploy.prototxt pairs, un-commented, on a small stand-in: BatchNorm and Scale with tops of their own, the
# ReLU in place on the Scale's top (fused: one launch, the two tops in the middle filled on demand); then a pair whose Scale top goes
# to a Concat-free consumer that is no ReLU (the pair behind conv4_3/conv5_3/concat feeds dropout5 / the heads)
PAIRS = """
name: "pairs"
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 12 }
input: "label" input_shape { dim: 2 }
layer { name: "conv1_1" type: "Convolution" bottom: "data" top: "conv1_1" convolution_param { num_output: 6 pad: 1 kernel_size: 3 } }
layer { name: "conv1_1/bn" type: "BatchNorm" bottom: "conv1_1" top: "conv1_1/bn" }
layer { name: "conv1_1/bn_sc" type: "Scale" bottom: "conv1_1/bn" top: "conv1_1/bn_sc" scale_param { bias_term: true } }
layer { name: "relu1_1" type: "ReLU" bottom: "conv1_1/bn_sc" top: "conv1_1/bn_sc" }
layer { name: "conv1_2" type: "Convolution" bottom: "conv1_1/bn_sc" top: "conv1_2" convolution_param { num_output: 8 pad: 1 kernel_size: 3 } }
layer { name: "concat/bn" type: "BatchNorm" bottom: "conv1_2" top: "concat/bn" }
layer { name: "concat/bn_sc" type: "Scale" bottom: "concat/bn" top: "concat/bn_sc" scale_param { bias_term: true } }
layer { name: "cvg" type: "Convolution" bottom: "concat/bn_sc" top: "cvg" convolution_param { num_output: 4 kernel_size: 1 } }
layer { name: "pool" type: "Pooling" bottom: "cvg" top: "pool" pooling_param { pool: AVE global_pooling: true } }
layer { name: "fc" type: "InnerProduct" bottom: "pool" top: "fc" inner_product_param { num_output: 5 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }
"""

# every unfused form: BatchNorm + ReLU in place without a Scale; Scale alone in place (its input is kept); BatchNorm alone with a top of
# its own; Scale alone without a bias and a ReLU, each with a top of its own; BatchNorm over an (N, C) blob
FORMS = """
name: "forms"
input: "data" input_shape { dim: 4 dim: 3 dim: 9 dim: 8 }
input: "label" input_shape { dim: 4 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 6 pad: 1 kernel_size: 3 } }
layer { name: "bn0" type: "BatchNorm" bottom: "c0" top: "c0" }
layer { name: "relu0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "p" type: "Pooling" bottom: "c0" top: "p" pooling_param { pool: AVE kernel_size: 2 stride: 2 } }
layer { name: "sc1" type: "Scale" bottom: "p" top: "p" scale_param { bias_term: true } }
layer { name: "c1" type: "Convolution" bottom: "p" top: "c1" convolution_param { num_output: 5 kernel_size: 3 pad: 1 bias_term: false } }
layer { name: "bn1" type: "BatchNorm" bottom: "c1" top: "c1bn" batch_norm_param { eps: 0.01 moving_average_fraction: 0.9 } }
layer { name: "c2" type: "Convolution" bottom: "c1bn" top: "c2" convolution_param { num_output: 8 kernel_size: 1 } }
layer { name: "sc2" type: "Scale" bottom: "c2" top: "c2s" }
layer { name: "relu2" type: "ReLU" bottom: "c2s" top: "c2r" }
layer { name: "fc" type: "InnerProduct" bottom: "c2r" top: "fc" inner_product_param { num_output: 7 } }
layer { name: "bnfc" type: "BatchNorm" bottom: "fc" top: "fc" }
layer { name: "scfc" type: "Scale" bottom: "fc" top: "fc" scale_param { bias_term: true } }
layer { name: "fc2" type: "InnerProduct" bottom: "fc" top: "fc2" inner_product_param { num_output: 5 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc2" bottom: "label" top: "loss" }
"""


@pytest.mark.parametrize("which", ["pairs", "forms"])
def test_separate_tops_and_unfused_forms_forward_and_backward(gpu, monkeypatch, which):
    text = PAIRS if which == "pairs" else FORMS
    spec, params, eng = _train_engine(monkeypatch, True, text=text, seed=9)
    chains = {k: [q.name if q is not None else None for q in (ch.bn, ch.scale, ch.relu)] for k, ch in eng._bn_chains.items()}
    if which == "pairs":
        assert chains == {"conv1_1/bn": ["conv1_1/bn", "conv1_1/bn_sc", "relu1_1"], "concat/bn": ["concat/bn", "concat/bn_sc", None]}
        assert eng._bn_chains["conv1_1/bn"].mids == ["conv1_1/bn"] and eng._bn_chains["concat/bn"].mids == ["concat/bn"]
        interior = ["conv1_1", "conv1_1/bn", "conv1_1/bn_sc", "conv1_2", "concat/bn", "concat/bn_sc", "cvg", "fc"]
    else:
        assert chains == {"bn0": ["bn0", None, "relu0"], "sc1": [None, "sc1", None], "bn1": ["bn1", None, None], "sc2": [None, "sc2", "relu2"],
                          "bnfc": ["bnfc", "scfc", None]}
        assert set(eng.aux_dev) >= {"bn0", "sc1", "bn1", "bnfc"} and "sc2" not in eng.aux_dev      # (sc2's input is still in its bottom blob)
        interior = ["c0", "p", "c1", "c1bn", "c2", "c2s", "c2r", "fc", "fc2"]
    x = inputs_for(spec, 2, classes=5)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step()
    updates = check_step(eng, spec, params, x, out, interior, which)
    now = eng.download_params()
    for name, want in updates.items():
        for i in range(3):
            assert rel_err(now[name][i], want[i]) < 1e-4, (name, i)
    g1 = eng.download_grads()
    eng.step()
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k]))
    eng.close()


def test_refusals_by_layer_name(gpu):
    txt = models.resnet("DEPLOY", **KW).replace("use_global_stats: true", "use_global_stats: false")
    with pytest.raises(NotImplementedError, match="BatchNorm bn_conv1 with batch statistics"):
        Engine(NetSpec(proto.parse_text(txt), "TEST"), device=0, autotune=False, dtype="f16")
    tanh = PAIRS.replace('type: "ReLU"', 'type: "TanH"')
    with pytest.raises(NotImplementedError, match="TanH.*relu1_1"):
        Engine(NetSpec(proto.parse_text(tanh), "TEST"), device=0, autotune=False)
