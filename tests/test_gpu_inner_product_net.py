"""InnerProduct through the engine and through `import caffe`, -m gpu: a classifier tail of CaffeNet's size (pool5 256x6x6 -> 4096 ->
4096 -> 1000 -> Softmax, in-place ReLU / Dropout) behind a small convolution stack, every blob against the same net in torch
float64 from the same seeded parameters; float32 and half-float engines, batch 1 and 10; parameters read back and saved bit-exactly; the
forward replayed under a graph equals the eager one; batches and nets the streaming kernels do not take are refused by name."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fcn_object_detector_amd import proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params

pytestmark = pytest.mark.gpu


def net_text(batch, c5=256, fc=4096, classes=1000, bias2=True):
    return """
name: "tail"
input: "data"
input_shape { dim: %d dim: 3 dim: 27 dim: 27 }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" convolution_param { num_output: 24 kernel_size: 5 stride: 2
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
layer { name: "conv5" type: "Convolution" bottom: "conv1" top: "conv5" convolution_param { num_output: %d kernel_size: 3 pad: 1
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu5" type: "ReLU" bottom: "conv5" top: "conv5" }
layer { name: "pool5" type: "Pooling" bottom: "conv5" top: "pool5" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
layer { name: "fc6" type: "InnerProduct" bottom: "pool5" top: "fc6" inner_product_param { num_output: %d
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu6" type: "ReLU" bottom: "fc6" top: "fc6" }
layer { name: "drop6" type: "Dropout" bottom: "fc6" top: "fc6" dropout_param { dropout_ratio: 0.5 } }
layer { name: "fc7" type: "InnerProduct" bottom: "fc6" top: "fc7" inner_product_param { num_output: %d bias_term: %s
  weight_filler { type: "xavier" } } }
layer { name: "relu7" type: "ReLU" bottom: "fc7" top: "fc7" }
layer { name: "fc8" type: "InnerProduct" bottom: "fc7" top: "fc8" inner_product_param { num_output: %d
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.0 } } }
layer { name: "prob" type: "Softmax" bottom: "fc8" top: "prob" }
""" % (batch, c5, fc, fc, "true" if bias2 else "false", classes)


def torch_forward(params, x, half=False):
    """The same net in float64; half: from parameters and input as the half-float engine rounds them."""
    r = (lambda a: a.astype(np.float16)) if half else (lambda a: a)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    blobs = {}
    y = F.relu(F.conv2d(t(x), t(r(params["conv1"][0])), t(params["conv1"][1]), stride=2))
    blobs["conv1"] = y
    y = F.relu(F.conv2d(y, t(r(params["conv5"][0])), t(params["conv5"][1]), padding=1))
    y = F.max_pool2d(y, 2, 2)
    blobs["pool5"] = y
    y = y.reshape(len(x), -1)
    for name in ("fc6", "fc7", "fc8"):
        p = params[name]
        y = F.linear(y, t(r(p[0])), t(p[1]) if len(p) > 1 else None)
        if name != "fc8":
            y = F.relu(y)
        blobs[name] = y
    blobs["prob"] = F.softmax(y, dim=1)
    return {k: v.numpy() for k, v in blobs.items()}


def build(batch, dtype="f32", **kw):
    msg = proto.parse_text(net_text(batch, **kw))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=11)
    return Engine(NetSpec(msg, "TEST"), params=params, device=0, dtype=dtype), params


@pytest.mark.parametrize("batch", [1, 10])
def test_float32_net_matches_torch_float64(gpu, batch):
    eng, params = build(batch)
    try:
        x = np.random.default_rng(batch).standard_normal((batch, 3, 27, 27)).astype(np.float32)
        eng.host_array("data")[...] = x
        out = eng.forward()
        want = torch_forward(params, x)
        assert eng.shapes["pool5"] == (batch, 256, 6, 6) and eng.shapes["fc7"] == (batch, 4096)
        assert eng.read_blob("fc7")[0].shape == (4096,) and out["prob"].shape == (batch, 1000)
        assert np.allclose(out["prob"].sum(axis=1), 1.0, atol=1e-5)
        for name in ("pool5", "fc6", "fc7", "fc8", "prob"):
            got = eng.read_blob(name)
            assert got.shape == want[name].shape, name
            assert np.abs(got - want[name]).max() <= 1e-4 * np.abs(want[name]).max(), name
        eager = {k: v.copy() for k, v in eng.forward(use_graph=False).items()}
        replay = eng.forward()
        assert all(np.array_equal(eager[k], replay[k]) for k in eager)
        for name in ("fc6", "fc7", "fc8"):           # Caffe's (num_output, K) (c, h, w) layout comes back bit-exactly
            for i, a in enumerate(params[name]):
                assert np.array_equal(eng.read_param(name, i), a), (name, i)
        assert [op.name for op in eng.ops if op.kind == "inner_product"] == ["fc6", "fc7", "fc8"]
        assert not any(op.name in ("relu6", "relu7", "drop6") for op in eng.ops)      # fused / identity at TEST
    finally:
        eng.close()


@pytest.mark.parametrize("batch", [1, 10])
def test_half_float_net(gpu, batch):
    eng, params = build(batch, dtype="f16", bias2=False)
    try:
        x = np.random.default_rng(20 + batch).random((batch, 3, 27, 27)).astype(np.float32)
        eng.host_array("data")[...] = x
        out = eng.forward()
        want = torch_forward(params, x.astype(np.float16), half=True)
        assert eng.blobs["fc6"].esize == 2 and eng.blobs["prob"].esize == 4
        for name in ("fc6", "fc7", "fc8"):
            got = eng.read_blob(name)
            assert np.abs(got - want[name]).max() <= 1e-2 * np.abs(want[name]).max(), name      # activations re-rounded to half per layer
        assert np.allclose(out["prob"].sum(axis=1), 1.0, atol=1e-3)
        assert np.abs(out["prob"] - want["prob"]).max() <= 2e-2 * want["prob"].max()
    finally:
        eng.close()


def test_pycaffe_face(gpu, tmp_path, monkeypatch):
    import sys
    monkeypatch.setenv("FCN_TUNE_CACHE", str(tmp_path / "tune.json"))      # the second net replays the first one's convolution tiles
    from conftest import PYCAFFE
    sys.path.insert(0, PYCAFFE)
    try:
        import caffe
        path = tmp_path / "deploy.prototxt"
        path.write_text(net_text(1, c5=32, fc=64, classes=10))
        net = caffe.Net(str(path), caffe.TEST)
        net.blobs["data"].reshape(2, 3, 27, 27)
        x = np.random.default_rng(0).standard_normal((2, 3, 27, 27)).astype(np.float32)
        net.blobs["data"].data[...] = x
        out = net.forward()
        want = torch_forward({k: [b.data for b in v] for k, v in net.params.items()}, x)
        for name in ("fc6", "fc7", "fc8", "prob"):
            assert np.abs(net.blobs[name].data - want[name]).max() <= 1e-4 * np.abs(want[name]).max(), name
        assert out["prob"].shape == (2, 10) and net.blobs["fc7"].data[0].shape == (64,)
        assert net.params["fc6"][0].data.shape == (64, 32 * 6 * 6) and net.params["fc6"][1].data.shape == (64,)
        net.save(str(tmp_path / "w.caffemodel"))
        again = caffe.Net(str(path), str(tmp_path / "w.caffemodel"), caffe.TEST)
        again.blobs["data"].reshape(2, 3, 27, 27)
        again.blobs["data"].data[...] = net.blobs["data"].data
        for name in ("conv1", "conv5", "fc6", "fc7", "fc8"):      # the round trip through the file is bit-exact
            for a, b in zip(net.params[name], again.params[name]):
                assert np.array_equal(a.data, b.data), name
        assert np.array_equal(again.forward()["prob"], out["prob"])      # same weights, same plan: the same bits
    finally:
        sys.path.remove(PYCAFFE)


def test_what_the_streaming_kernels_do_not_take_is_refused_by_name(gpu):
    with pytest.raises(NotImplementedError, match="fc6.*40 rows"):
        build(40, c5=32, fc=64, classes=10)
