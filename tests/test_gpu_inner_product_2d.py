"""(N, C) blobs through the engine, -m gpu: what stands behind an InnerProduct, with the kernels those layers already had, against
torch float64 - a Concat of two InnerProduct tops feeding a third (members written in place, and copied where their widths are not
whole 16-byte groups), Slice, Eltwise, Sigmoid, Power, the Euclidean / L1 losses, SoftmaxWithLoss and Accuracy with labels of shape
(N,), (N, 1) and (N, 1, 1, 1); banks whose bottoms carry pad channels (6 channels in pixels of 8, a 10-wide fc in pixels of 12 / 16)
in both engines with read_param round-tripping; and the rows `caffe time` prints."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fcn_object_detector_amd import proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params

pytestmark = pytest.mark.gpu
FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'


def build(txt, dtype="f32", seed=5):
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=seed)
    return Engine(NetSpec(msg, "TEST"), params=params, device=0, dtype=dtype), params


def t64(a):
    return torch.tensor(np.asarray(a, np.float64))


def lin(x, p, relu=False):
    y = F.linear(x.reshape(len(x), -1), t64(p[0]), t64(p[1]) if len(p) > 1 else None)
    return F.relu(y) if relu else y


def close(got, want, tol=1e-5):
    want = np.asarray(want, np.float64)
    return got.shape == want.shape and np.abs(got - want).max() <= tol * max(np.abs(want).max(), 1e-30)


@pytest.mark.parametrize("wa,wb,in_place", [(8, 12, True), (10, 6, False)])
def test_concat_of_two_inner_products_feeds_a_third(gpu, wa, wb, in_place):
    txt = """
input: "data"
input_shape { dim: 5 dim: 6 dim: 3 dim: 3 }
layer { name: "a" type: "InnerProduct" bottom: "data" top: "a" inner_product_param { num_output: %d %s } }
layer { name: "relu_a" type: "ReLU" bottom: "a" top: "a" }
layer { name: "b" type: "InnerProduct" bottom: "data" top: "b" inner_product_param { num_output: %d %s } }
layer { name: "cat" type: "Concat" bottom: "a" bottom: "b" top: "cat" }
layer { name: "o" type: "InnerProduct" bottom: "cat" top: "o" inner_product_param { num_output: 7 %s } }
layer { name: "sl" type: "Slice" bottom: "o" top: "o0" top: "o1" slice_param { slice_point: 3 } }
""" % (wa, FILL, wb, FILL, FILL)
    eng, params = build(txt)
    try:
        x = np.random.default_rng(wa).standard_normal((5, 6, 3, 3)).astype(np.float32)
        eng.host_array("data")[...] = x
        out = eng.forward()
        a, b = lin(t64(x), params["a"], relu=True), lin(t64(x), params["b"])
        cat = torch.cat([a, b], dim=1)
        o = lin(cat, params["o"])
        assert eng.shapes["cat"] == (5, wa + wb) and eng.blobs["data"].cstride == 8      # the first banks skip two pad channels per pixel
        for name, want in (("a", a), ("b", b), ("cat", cat), ("o", o)):
            assert close(eng.read_blob(name), want.numpy()), name
        assert close(out["o0"], o.numpy()[:, :3]) and close(out["o1"], o.numpy()[:, 3:])
        shared = eng.blobs["a"].buf is eng.blobs["cat"].buf
        assert shared == in_place and (eng.blobs["b"].coffset == wa) == in_place      # written at y_coffset, no copy launch
        assert any(op.kind == "copy" and op.name.startswith("cat") for op in eng.ops) != in_place
        for name in ("a", "b", "o"):
            for i, p in enumerate(params[name]):
                assert np.array_equal(eng.read_param(name, i), p), (name, i)
    finally:
        eng.close()


@pytest.mark.parametrize("label_shape", [(6,), (6, 1), (6, 1, 1, 1)], ids=["N", "Nx1", "Nx1x1x1"])
def test_losses_accuracy_and_pointwise_layers_over_2d_blobs(gpu, label_shape):
    txt = """
input: "data"
input_shape { dim: 6 dim: 3 dim: 4 dim: 4 }
input: "label"
input_shape { %s }
input: "target"
input_shape { dim: 6 dim: 10 }
layer { name: "a" type: "InnerProduct" bottom: "data" top: "a" inner_product_param { num_output: 10 %s } }
layer { name: "b" type: "InnerProduct" bottom: "data" top: "b" inner_product_param { num_output: 10 bias_term: false weight_filler { type: "xavier" } } }
layer { name: "sum" type: "Eltwise" bottom: "a" bottom: "b" top: "s" eltwise_param { operation: SUM } }
layer { name: "sig" type: "Sigmoid" bottom: "s" top: "sg" }
layer { name: "pw" type: "Power" bottom: "s" top: "pw" power_param { power: 1 scale: 2 shift: 1 } }
layer { name: "prob" type: "Softmax" bottom: "s" top: "prob" }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "s" bottom: "label" top: "loss" }
layer { name: "acc" type: "Accuracy" bottom: "s" bottom: "label" top: "acc" }
layer { name: "l2" type: "EuclideanLoss" bottom: "s" bottom: "target" top: "l2" }
layer { name: "l1" type: "L1Loss" bottom: "sg" bottom: "target" top: "l1" }
""" % (" ".join("dim: %d" % d for d in label_shape), FILL)
    eng, params = build(txt)
    try:
        rng = np.random.default_rng(len(label_shape))
        x = rng.standard_normal((6, 3, 4, 4)).astype(np.float32)
        target = rng.standard_normal((6, 10)).astype(np.float32)
        s = lin(t64(x), params["a"]) + lin(t64(x), params["b"])
        label = rng.integers(0, 10, 6)
        label[:3] = s.numpy().argmax(axis=1)[:3]                 # some right, some (almost surely) wrong
        eng.host_array("data")[...] = x
        eng.host_array("label")[...] = label.reshape(label_shape).astype(np.float32)
        eng.host_array("target")[...] = target
        out = eng.forward()
        assert eng.shapes["s"] == (6, 10) and eng.blobs["s"].cstride == 12 and eng.host_array("label").shape == label_shape
        assert close(eng.read_blob("s"), s.numpy())
        assert close(out["pw"], (2 * s + 1).numpy()) and close(out["prob"], F.softmax(s, dim=1).numpy())
        assert close(eng.read_blob("sg"), torch.sigmoid(s).numpy())
        assert abs(float(out["loss"]) - float(F.cross_entropy(s, torch.tensor(label)))) <= 1e-5
        assert abs(float(out["acc"]) - float((s.numpy().argmax(axis=1) == label).mean())) <= 1e-6
        assert abs(float(out["l2"]) - float(((s - t64(target)) ** 2).sum() / 12.0)) <= 1e-4
        assert abs(float(out["l1"]) - float((torch.sigmoid(s) - t64(target)).abs().sum() / 6.0)) <= 1e-4
    finally:
        eng.close()


NARROW = """
input: "data"
input_shape { dim: %d dim: 3 dim: 5 dim: 5 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv" convolution_param { num_output: 6 kernel_size: 3 %s } }
layer { name: "relu" type: "ReLU" bottom: "conv" top: "conv" }
layer { name: "fc1" type: "InnerProduct" bottom: "conv" top: "fc1" inner_product_param { num_output: 10 %s } }
layer { name: "relu1" type: "ReLU" bottom: "fc1" top: "fc1" }
layer { name: "fc2" type: "InnerProduct" bottom: "fc1" top: "fc2" inner_product_param { num_output: 7 %s } }
"""


@pytest.mark.parametrize("dtype,batch", [("f32", 1), ("f32", 9), ("f16", 1), ("f16", 9)])
def test_banks_over_bottoms_with_pad_channels(gpu, dtype, batch):
    """6 channels in pixels of 8, then a 10-wide fc in pixels of 12 (float32) / 16 (halves): the packed banks skip the pad columns."""
    eng, params = build(NARROW % (batch, FILL, FILL, FILL), dtype=dtype)
    try:
        half = dtype == "f16"
        r = (lambda a: np.asarray(a, np.float16)) if half else (lambda a: a)
        x = np.random.default_rng(batch).random((batch, 3, 5, 5)).astype(np.float32)
        eng.host_array("data")[...] = x
        out = eng.forward()
        assert eng.blobs["conv"].cstride == 8 and eng.blobs["fc1"].cstride == (16 if half else 12)
        y = F.relu(F.conv2d(t64(r(x)), t64(r(params["conv"][0])), t64(params["conv"][1])))
        f1 = F.relu(F.linear(y.reshape(batch, -1), t64(r(params["fc1"][0])), t64(params["fc1"][1])))
        f2 = F.linear(f1, t64(r(params["fc2"][0])), t64(params["fc2"][1]))
        tol = 1e-2 if half else 1e-5
        assert close(eng.read_blob("fc1"), f1.numpy(), tol) and close(out["fc2"], f2.numpy(), tol)
        for name in ("fc1", "fc2"):
            assert np.array_equal(eng.read_param(name, 0), r(params[name][0]).astype(np.float32)), name
            assert np.array_equal(eng.read_param(name, 1), params[name][1]), name
    finally:
        eng.close()


def test_time_rows(gpu):
    """What `caffe time` prints per layer: an InnerProduct row carries the layer's FLOPs (over the true K) and its bytes."""
    eng, _ = build(NARROW % (4, FILL, FILL, FILL))
    try:
        rows = {name: (kind, ms, flops, nbytes) for kind, name, ms, flops, nbytes in eng.time_ops(reps=3)}
        assert rows["fc1"][0] == rows["fc2"][0] == "inner_product"
        assert rows["fc1"][2] == 2.0 * 4 * (6 * 3 * 3) * 10 and rows["fc2"][2] == 2.0 * 4 * 10 * 7
        assert rows["fc1"][1] > 0 and rows["fc1"][3] >= 4.0 * 10 * 8 * 9 and "relu1" not in rows
    finally:
        eng.close()
