"""Backward planning around in-place layers and channel crops, -m gpu.

An in-place one-bottom layer (bottom == top) rewrites dY as dX: the planner must not ask its kernel to accumulate into the very
gradient it reads.  That holds for every such layer type, not only the Dropout layers of the published FCN nets: here an in-place
Sigmoid that no convolution epilogue can take (it follows a pooling).  And the one Crop form whose backward is refused - a crop
along the channel axis - is refused when the plan is built, by layer name."""
import numpy as np
import pytest

from conftest import rel_err
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from test_gpu_fcn_published import as_torch, torch_net

pytestmark = pytest.mark.gpu

INPLACE = """
input: "data" input_shape { dim: 2 dim: 3 dim: 9 dim: 11 }
input: "target" input_shape { dim: 2 dim: 4 dim: 5 dim: 6 }
layer { name: "c1" type: "Convolution" bottom: "data" top: "c1"
  convolution_param { num_output: 8 kernel_size: 3 pad: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "p1" type: "Pooling" bottom: "c1" top: "p1" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
layer { name: "squash" type: "Sigmoid" bottom: "p1" top: "p1" }
layer { name: "c2" type: "Convolution" bottom: "p1" top: "c2"
  convolution_param { num_output: 4 kernel_size: 1 weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.05 } } }
layer { name: "loss" type: "EuclideanLoss" bottom: "c2" bottom: "target" top: "loss" }
"""


def _engine(text):
    msg = proto.parse_text(text)
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    params = fill_params(spec, seed=2)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0,
                      solver=sp, autotune=False)
    return spec, params, eng


def test_in_place_sigmoid_overwrites_its_gradient(gpu):
    spec, params, eng = _engine(INPLACE)
    assert [op.kind for op in eng.bwd_ops].count("sigmoid_bwd") == 1
    rng = np.random.default_rng(1)
    data = {"data": rng.standard_normal((2, 3, 9, 11)).astype(np.float32), "target": rng.standard_normal((2, 4, 5, 6)).astype(np.float32)}
    for k, v in data.items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=0)
    P = as_torch(params, grad=True)
    ref = torch_net(spec, P, data)
    ref["loss"].backward()
    want = float(ref["loss"].detach())
    assert abs(out["loss"] - want) < 1e-4 * abs(want)
    got = eng.download_grads()
    for name in ("c1", "c2"):
        for g, r in zip(got[name], P[name]):
            assert rel_err(g, r.grad.numpy()) < 2e-4, "parameter gradient of " + name      # (dY + f(dY) in p1 would be off by a factor of ~5)
    eng.close()


CHANNEL_CROP = """
input: "data" input_shape { dim: 1 dim: 3 dim: 6 dim: 7 }
input: "like" input_shape { dim: 1 dim: 4 dim: 6 dim: 7 }
input: "target" input_shape { dim: 1 dim: 4 dim: 6 dim: 7 }
layer { name: "c1" type: "Convolution" bottom: "data" top: "c1"
  convolution_param { num_output: 8 kernel_size: 1 weight_filler { type: "xavier" } } }
layer { name: "middle" type: "Crop" bottom: "c1" bottom: "like" top: "four" crop_param { axis: 1 offset: 2 offset: 0 offset: 0 } }
layer { name: "loss" type: "EuclideanLoss" bottom: "four" bottom: "target" top: "loss" }
"""


def test_backward_of_a_channel_crop_is_refused_by_layer_name(gpu):
    with pytest.raises(NotImplementedError, match="Crop middle along the channel axis"):
        _engine(CHANNEL_CROP)
