"""The accumulate paths of the gated Scale's two gradient launches, -m gpu, against torch autograd in float64 (tests/torch_se_ref.py), as
tests/test_gpu_backward_fanout.py checks the other emitters: one tiny TRAIN net per case in which a bottom of the Scale already holds a
gradient when the Scale's backward is reached.

  x_written_first     x has a second reader behind the Scale (an Eltwise SUM): that layer's backward writes G[x] first, so the data gradient
                      accumulates, the gate gradient does not, and the global pooling's backward accumulates into G[x] a third time
  gate_written_first  one gate multiplies two blobs: the later Scale writes G[gate], the earlier one accumulates into it and writes G[x]
In an SE-ResNet both flags are 0; here they differ, in both directions.  Checked: the flags the plan gives the launches, the loss at 1e-4
relative, and every parameter gradient by the rule of tests/test_gpu_resnet.py - rel_err < max(5e-4, 4 x torch float32's own error), the
device's ReLU masks adopted in the reference.  A second step gives the same bits."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_se_ref import as_torch, random_params, torch_se_net

pytestmark = pytest.mark.gpu
F32 = np.float32

HEAD = """
layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 8 dim: 6 dim: 5 } } }
layer { name: "label" type: "Input" top: "label" input_param { shape { dim: 2 } } }
layer { name: "short" type: "Convolution" bottom: "data" top: "short" convolution_param { num_output: 8 kernel_size: 1 } }
layer { name: "x" type: "Convolution" bottom: "data" top: "x" convolution_param { num_output: 8 kernel_size: 3 pad: 1 } }
layer { name: "pool" type: "Pooling" bottom: "x" top: "pool" pooling_param { pool: AVE global_pooling: true } }
layer { name: "down" type: "InnerProduct" bottom: "pool" top: "down" inner_product_param { num_output: 4 } }
layer { name: "down/relu" type: "ReLU" bottom: "down" top: "down" }
layer { name: "up" type: "InnerProduct" bottom: "down" top: "up" inner_product_param { num_output: 8 } }
layer { name: "gate" type: "Sigmoid" bottom: "up" top: "gate" }
layer { name: "sc" type: "Scale" bottom: "x" bottom: "gate" top: "sc" scale_param { axis: 0 } }
"""
TAIL = """
layer { name: "feat" type: "Pooling" bottom: "%s" top: "feat" pooling_param { pool: AVE global_pooling: true } }
layer { name: "fc" type: "InnerProduct" bottom: "feat" top: "fc" inner_product_param { num_output: 5 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }
"""
NETS = {
    "x_written_first": HEAD + """
layer { name: "out" type: "Eltwise" bottom: "sc" bottom: "short" top: "out" }
layer { name: "out/relu" type: "ReLU" bottom: "out" top: "out" }
layer { name: "out2" type: "Eltwise" bottom: "out" bottom: "x" top: "out2" }
""" + TAIL % "out2",
    "gate_written_first": HEAD + """
layer { name: "sc2" type: "Scale" bottom: "short" bottom: "gate" top: "sc2" scale_param { axis: 0 } }
layer { name: "out" type: "Eltwise" bottom: "sc" bottom: "sc2" top: "out" }
layer { name: "out/relu" type: "ReLU" bottom: "out" top: "out" }
""" + TAIL % "out",
}
# scale_gate_bwd launch -> the accumulate flag the plan must give it
FLAGS = {"x_written_first": {"sc:x": 1, "sc:gate": 0}, "gate_written_first": {"sc2:short": 0, "sc2:gate": 0, "sc:x": 0, "sc:gate": 1}}


@pytest.mark.parametrize("case", sorted(NETS))
def test_gradients_against_autograd(gpu, case):
    msg = proto.parse_text(NETS[case])
    spec = NetSpec(msg, "TRAIN", scale_gate=True)
    spec.infer()
    params = random_params(spec, 41)
    rng = np.random.default_rng(42)
    x = {"data": rng.standard_normal(spec.input_shapes["data"]).astype(F32), "label": rng.integers(0, 5, (2,)).astype(F32)}
    x["data"][1] = 2.0 * x["data"][1] + 0.5      # (the two images' gates differ)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN", scale_gate=True), dict(spec.input_shapes), params={k: [a.copy() for a in v] for k, v in params.items()},
                      device=0, solver=sp, autotune=False)
    # (the byte estimate of a data gradient counts dx twice where the plan found its view full; what the launch itself passes is held by
    # tests/test_gate_plan.py and, below, by the gradients)
    n, c, h, w = spec.blob_shapes["x"]
    for op in eng.bwd_ops:
        if op.kind == "scale_gate_bwd" and not op.name.endswith(":gate"):
            assert op.bytes == 4.0 * (2 + FLAGS[case][op.name]) * n * c * h * w, op.name
    assert [op.name for op in eng.bwd_ops if op.kind == "scale_gate_bwd"] == list(FLAGS[case])
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step()
    with torch.no_grad():
        fwd = torch_se_net(spec, as_torch(params), x)
    g = fwd["gate"].numpy()
    assert np.abs(g[0] - g[1]).max() > 0.02
    want = float(fwd["total_loss"])
    print("FANOUT %s loss %.6g want %.6g" % (case, out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want)
    masks = {l.name: eng.read_blob(l.tops[0]) > 0 for l in spec.layers if l.type == "ReLU"}
    P = as_torch(params, grad=True)
    torch_se_net(spec, P, x, relu_masks=masks)["total_loss"].backward()
    P32 = as_torch(params, grad=True, dtype=torch.float32)
    torch_se_net(spec, P32, x, relu_masks=masks, dtype=torch.float32)["total_loss"].backward()
    got = eng.download_grads()
    for l in spec.param_layers():
        for i, (gr, r, r32) in enumerate(zip(got[l.name], P[l.name], P32[l.name])):
            own = rel_err(r32.grad.numpy(), r.grad.numpy())
            err = rel_err(gr, r.grad.numpy())
            print("FANOUT %s %s[%d] %.3g (torch float32: %.3g)" % (case, l.name, i, err, own))
            assert err < max(5e-4, 4 * own), "gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, err, own)
    eng.step()
    again = eng.download_grads()
    assert all(np.array_equal(a, b) for k in got for a, b in zip(got[k], again[k])), "the same step again: the same bits"
    eng.close()
