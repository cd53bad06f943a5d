"""Inception-v3 (models.inception_v3) and a factorised residual block through the public surface, -m gpu, against torch in float64 on
the CPU (tests/torch_rect_ref.py), in the style of tests/test_gpu_dilated_nets.py and tests/test_gpu_resnet.py.

The nets: Inception-v3 at width_div 8 (widths 4 .. 48 per branch, 256 channels in front of the pool), batch 2, 171 x 139 - grids 19 x 15,
9 x 7 and 4 x 3, so no grid is square and every 1x7 / 7x1 filter is wider than half of its grid - and 6 classes.  The block: 3x1, 1x3,
then 3x1 and 1x3 at dilation 2 (the non-bottleneck-1D block of ERFNet), BatchNorm + Scale behind each pair, an Eltwise sum with the
block's input, on 23 x 19.

Thresholds are the project's: rel_err < 1e-4 for blobs and the loss, < 5e-4 for parameter gradients.  Where the reference's OWN float32
error is too close to them the rule of DESIGN.md 4.13 applies: the same case runs in torch float32 on the CPU against the float64 net
and the threshold of that quantity is the larger of the project's and 4 x that error.  Measured on the CPU for the steps below (the
masks and argmaxes of the float32 pass standing in for the device's): the block's blobs at most 3.9e-7 and gradients
9.7e-7 - the exception does not bind; Inception-v3's listed blobs 2.0e-7 (conv1_3x3) .. 3.5e-5 (mixed_17d) .. 9.1e-5 (mixed_8b), and 178
of its 284 parameter gradients above 1.25e-4, the worst 3.8e-4 (mixed_35b/pool_1x1/scale gamma) - so the rule binds for the blobs from
mixed_17d on (up to 3.7e-4) and most gradients (up to 1.5e-3): the batch of 2 leaves the BatchNorms of the 4 x 3 grid 24 values per
channel, and 94 of them follow one another.
The backward comparison adopts the device's ReLU masks and MAX-pooling argmaxes in the reference, as tests/test_gpu_dilated_nets.py
does; forward blobs and the loss are compared without any adoption.  A bias-free convolution in front of a batch-statistics BatchNorm
has no dead bias gradient (tests/test_gpu_resnet.py) - every convolution here is bias-free but the block's, which are checked as its."""
import numpy as np
import pytest
import torch

import ref64
from conftest import rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params, is_rectangular
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_rect_ref import as_torch, max_pool_argmax, random_params, torch_net

pytestmark = pytest.mark.gpu
F32 = np.float32
IV3 = dict(batch=2, classes=6, width_div=8, size=(171, 139))
IV3_BLOBS = ["conv1_3x3", "conv3_3x3", "pool2", "mixed_35a", "mixed_35c", "reduction_a", "mixed_17a/7x7_1x7", "mixed_17a/7x7_7x1",
             "mixed_17b/7x7dbl_b_1x7", "mixed_17d", "reduction_b/7x7x3_7x1", "reduction_b", "mixed_8a/3x3_1x3", "mixed_8a/3x3dbl_3x1", "mixed_8b",
             "pool3", "classifier"]


def make(text, phase):
    msg = proto.parse_text(text)
    spec = NetSpec(msg, phase)
    spec.infer()
    return msg, spec


def inputs_for(spec, seed, classes=6):
    rng = np.random.default_rng(seed)
    return {name: (rng.integers(0, classes, shp).astype(F32) if name == "label" else rng.standard_normal(shp).astype(F32))
            for name, shp in spec.input_shapes.items()}


def own_error(spec, params, x, names, **kw):
    """rel_err of torch float32 against torch float64 for the named blobs: the reference's own rounding error."""
    with torch.no_grad():
        a = torch_net(spec, as_torch(params), x, **kw)
        b = torch_net(spec, as_torch(params, dtype=torch.float32), x, dtype=torch.float32, **kw)
    return {n: rel_err(b[n].numpy(), a[n].numpy()) for n in names}


def _train_engine(monkeypatch, text, seed=3, lr=0.0):
    monkeypatch.setenv("FCN_NO_GRAPH", "0")
    msg, spec = make(text, "TRAIN")
    params = random_params(spec, seed)
    sp = SolverParams(base_lr=lr, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    return spec, params, eng


def reference_step(spec, params, x, seed, masks, argmax):
    """(float64 forward without adoption, float64 leaves after backward with adoption, float32 leaves likewise)."""
    with torch.no_grad():
        fwd = torch_net(spec, as_torch(params), x, dropout_seed=seed)
    P = as_torch(params, grad=True)
    torch_net(spec, P, x, dropout_seed=seed, relu_masks=masks, pool_argmax=argmax)["total_loss"].backward()
    P32 = as_torch(params, grad=True, dtype=torch.float32)
    torch_net(spec, P32, x, dropout_seed=seed, relu_masks=masks, pool_argmax=argmax, dtype=torch.float32)["total_loss"].backward()
    return fwd, P, P32


def check_step(eng, spec, params, x, out, interior, seed, label=""):
    """Loss, interior blobs and every parameter gradient of one step against torch float64 under the rule of the module text."""
    masks = {l.name: eng.read_blob(l.tops[0]) > 0 for l in spec.layers if l.type == "ReLU"}
    argmax = max_pool_argmax(spec, eng.read_blob)
    fwd, P, P32 = reference_step(spec, params, x, seed, masks, argmax)
    own = own_error(spec, params, x, interior, dropout_seed=seed)
    want = float(fwd["total_loss"])
    print("STEP %s loss %.6g want %.6g" % (label, out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want), (out["total_loss"], want)
    for name in interior:
        err = rel_err(eng.read_blob(name), fwd[name].numpy())
        print("BLOB %s %s %.3g (torch float32: %.3g)" % (label, name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    got = eng.download_grads()
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
            if l.name in dead_bias and i == 1:      # mathematically zero: held as tests/test_gpu_resnet.py holds conv1's
                dy = np.abs(eng.read_grad(l.tops[0]).astype(np.float64))
                dy = dy.reshape(dy.shape[0], dy.shape[1], -1)
                allow = np.maximum(ref64.dot_bound_rms(dy.shape[0] * dy.shape[2], dy.sum(axis=(0, 2))), 4 * np.abs(r32.grad.numpy()).max())
                assert np.all(np.abs(g) <= allow), "bias gradient of %s in front of a batch-statistics BatchNorm" % l.name
                continue
            own_g = rel_err(r32.grad.numpy(), r.grad.numpy())
            err = rel_err(g, r.grad.numpy())
            worst = max(worst, (err, "%s[%d] own %.3g" % (l.name, i, own_g)))
            print("GRAD %s %s[%d] %.3g (torch float32: %.3g)" % (label, l.name, i, err, own_g))
            assert err < max(5e-4, 4 * own_g), "parameter gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, err, own_g)
    print("GRAD %s worst %.3g at %s" % (label, worst[0], worst[1]))


def test_inception_v3_one_training_step(gpu, monkeypatch):
    spec, params, eng = _train_engine(monkeypatch, models.inception_v3("TRAIN", **IV3))
    rect = [l.name for l in spec.layers if l.type == "Convolution" and is_rectangular(l)]
    assert len(rect) == 34
    fwd_rect = [n for op in eng.ops if op.kind == "rconv" for n in op.name.split(" ")[0].split("+")]
    assert sorted(fwd_rect) == sorted(rect), "every rectangular layer runs through the rectangular kernels, and nothing else does"
    shared = [op.name.split(" ")[0] for op in eng.ops if op.kind == "rconv" and "+" in op.name]
    assert sorted(shared) == sorted("%s/%s_1x3+%s/%s_3x1" % (m, b, m, b) for m in ("mixed_8a", "mixed_8b") for b in ("3x3", "3x3dbl")), shared
    assert sorted(op.name.split(" ")[0] for op in eng.bwd_ops if op.kind == "rconv_dgrad") == sorted(rect)
    wg = {op.name: op for op in eng.bwd_ops if op.kind == "wgrad"}
    assert all(wg[n].layers == [n] and wg[n].sel is None for n in rect)
    assert eng.blobs["mixed_17d"].shape == (2, 96, 9, 7) and eng.blobs["mixed_8b"].shape == (2, 256, 4, 3)
    x = inputs_for(spec, 5)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=7)
    check_step(eng, spec, params, x, out, IV3_BLOBS, 7, "inception_v3")
    g1 = eng.download_grads()
    eng.step(seed=7)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k])), "the same step again: the same bits"
    eng.close()


def test_inception_v3_deploy_runs_with_frozen_statistics(gpu):
    msg, spec = make(models.inception_v3("DEPLOY", **IV3), "TEST")
    params = random_params(spec, 3)
    eng = Engine(NetSpec(msg, "TEST"), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0, autotune=False)
    assert sum(len(op.name.split(" ")[0].split("+")) for op in eng.ops if op.kind == "rconv") == 34
    assert "relu" not in [op.kind for op in eng.ops], "every in-place ReLU rides in a launch in front of it"
    x = inputs_for(spec, 2)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    own = own_error(spec, params, x, IV3_BLOBS + ["prob"])
    for name in IV3_BLOBS + ["prob"]:
        err = rel_err(eng.read_blob(name), ref[name].numpy())
        print("DEPLOY %s %.3g (torch float32: %.3g)" % (name, err, own[name]))
        assert err < max(1e-4, 4 * own[name]), name
    assert out["prob"].shape == (2, 6) and np.allclose(out["prob"].sum(axis=1), 1.0, atol=1e-5)
    now = {l.name: [eng.read_param(l.name, i) for i in range(3)] for l in spec.layers if l.type == "BatchNorm"}
    assert all(np.array_equal(a, b) for k in now for a, b in zip(now[k], params[k])), "frozen statistics do not move"
    eng.close()


def test_inception_v3_one_solver_step_changes_every_learnable_blob(gpu, monkeypatch):
    spec, params, eng = _train_engine(monkeypatch, models.inception_v3("TRAIN", **IV3), lr=0.01)
    x = inputs_for(spec, 5)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    eng.step(seed=7)
    now = eng.download_params()
    for l in spec.param_layers():
        if l.type == "BatchNorm":
            continue
        for i, (a, b) in enumerate(zip(now[l.name], params[l.name])):
            assert a.shape == b.shape and np.all(np.isfinite(a)) and not np.array_equal(a, b), "blob %d of %s did not move" % (i, l.name)
    eng.close()


FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
BN = """layer { name: "NAME/bn" type: "BatchNorm" bottom: "NAME" top: "NAME" param { lr_mult: 0 } param { lr_mult: 0 } param { lr_mult: 0 } }
layer { name: "NAME/scale" type: "Scale" bottom: "NAME" top: "NAME" scale_param { bias_term: true } }"""
BLOCK = """
input: "data" input_shape { dim: 2 dim: 3 dim: 23 dim: 19 }
input: "target" input_shape { dim: 2 dim: 5 dim: 23 dim: 19 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 12 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "b/3x1a" type: "Convolution" bottom: "c0" top: "b/3x1a" convolution_param { num_output: 12 kernel_h: 3 kernel_w: 1 pad_h: 1 pad_w: 0 FILL } }
layer { name: "b/3x1a/relu" type: "ReLU" bottom: "b/3x1a" top: "b/3x1a" }
layer { name: "b/1x3a" type: "Convolution" bottom: "b/3x1a" top: "b/1x3a" convolution_param { num_output: 12 kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1 FILL } }
%s
layer { name: "b/1x3a/relu" type: "ReLU" bottom: "b/1x3a" top: "b/1x3a" }
layer { name: "b/3x1b" type: "Convolution" bottom: "b/1x3a" top: "b/3x1b" convolution_param { num_output: 12 kernel_h: 3 kernel_w: 1 pad_h: 2 pad_w: 0 dilation: 2 FILL } }
layer { name: "b/3x1b/relu" type: "ReLU" bottom: "b/3x1b" top: "b/3x1b" }
layer { name: "b/1x3b" type: "Convolution" bottom: "b/3x1b" top: "b/1x3b" convolution_param { num_output: 12 kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 2 dilation: 2 FILL } }
%s
layer { name: "b" type: "Eltwise" bottom: "c0" bottom: "b/1x3b" top: "b" }
layer { name: "b/relu" type: "ReLU" bottom: "b" top: "b" }
layer { name: "score" type: "Convolution" bottom: "b" top: "score" convolution_param { num_output: 5 kernel_size: 1 FILL } }
layer { name: "loss" type: "EuclideanLoss" bottom: "score" bottom: "target" top: "loss" }
""".replace("FILL", FILL) % (BN.replace("NAME", "b/1x3a"), BN.replace("NAME", "b/1x3b"))
BLOCK_BLOBS = ["c0", "b/3x1a", "b/1x3a", "b/3x1b", "b/1x3b", "b", "score"]


def test_factorised_residual_block_trains(gpu, monkeypatch):
    spec, params, eng = _train_engine(monkeypatch, BLOCK, seed=4)
    assert [op.name.split(" ")[0] for op in eng.ops if op.kind == "rconv"] == ["b/3x1a", "b/1x3a", "b/3x1b", "b/1x3b"]
    assert [op.name.split(" ")[0] for op in eng.bwd_ops if op.kind == "rconv_dgrad"] == ["b/1x3b", "b/3x1b", "b/1x3a", "b/3x1a"]
    x = inputs_for(spec, 6)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=1)
    check_step(eng, spec, params, x, out, BLOCK_BLOBS, 1, "block")
    g1 = eng.download_grads()
    eng.step(seed=1)
    g2 = eng.download_grads()
    assert all(np.array_equal(a, b) for k in g1 for a, b in zip(g1[k], g2[k])), "the same step again: the same bits"
    eng.close()


HAND = """
input: "data" input_shape { dim: 2 dim: 3 dim: 23 dim: 19 }
%s
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "rect" type: "Convolution" bottom: "c0" top: "rect" convolution_param { num_output: 8 %s FILL } }
layer { name: "ra" type: "ReLU" bottom: "rect" top: "rect" }
%s
""".replace("FILL", FILL)


def hand(extra, train=None):
    if train is None:
        return HAND % ("", extra, "")
    return HAND % ('input: "target" input_shape { dim: 2 dim: 8 dim: %d dim: %d }' % train, extra,
                   'layer { name: "loss" type: "EuclideanLoss" bottom: "rect" bottom: "target" top: "loss" }')


def test_strided_rectangular_forward(gpu):
    msg, spec = make(hand("kernel_h: 3 kernel_w: 5 pad_h: 0 pad_w: 2 stride_h: 2 stride_w: 1"), "TEST")
    assert spec.blob_shapes["rect"] == (2, 8, 11, 19)
    params = fill_params(spec, seed=2)
    eng = Engine(NetSpec(msg, "TEST"), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0, autotune=False)
    assert [op.kind for op in eng.ops if op.name.startswith("rect")] == ["rconv"]
    x = inputs_for(spec, 3)
    for k, v in x.items():
        eng.host_array(k)[...] = v
    eng.forward()
    with torch.no_grad():
        ref = torch_net(spec, as_torch(params), x)
    for name in ("c0", "rect"):
        assert rel_err(eng.read_blob(name), ref[name].numpy()) < 1e-4, name
    eng.close()


def _train(text):
    msg, spec = make(text, "TRAIN")
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    return TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params=fill_params(spec, seed=1), device=0, solver=sp, autotune=False)


def test_refusals_by_layer_name(gpu):
    msg, _ = make(hand("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1"), "TEST")
    with pytest.raises(NotImplementedError, match=r"f16 engine: rectangular Convolution rect \(1x3"):
        Engine(NetSpec(msg, "TEST"), device=0, autotune=False, dtype="f16")
    msg, _ = make(hand("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1 group: 2"), "TEST")
    with pytest.raises(NotImplementedError, match=r"rectangular Convolution rect \(1x3 stride 1x1 pad 0x1\): group 2"):
        Engine(NetSpec(msg, "TEST"), device=0, autotune=False)
    with pytest.raises(NotImplementedError, match="rectangular Convolution rect: .*stride 1x2"):
        _train(hand("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1 stride_h: 1 stride_w: 2", train=(23, 10)))
    with pytest.raises(NotImplementedError, match="rectangular Convolution rect: .*pad_h 1 above"):
        _train(hand("kernel_h: 1 kernel_w: 3 pad_h: 1 pad_w: 1", train=(25, 19)))
    _train(hand("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 2", train=(23, 21))).close()      # pad == d (k-1): the data gradient runs with pad' = 0
