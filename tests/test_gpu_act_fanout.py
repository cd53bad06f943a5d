"""The backward launches of PReLU, TanH and Bias (csrc/act.hip) in tiny TRAIN nets, -m gpu, against torch autograd in float64
(tests/torch_act_ref.py), as tests/test_gpu_backward_fanout.py and tests/test_gpu_gate_fanout.py check the other emitters.

The nets are tests/torch_act_ref.FANOUT.  Each of the three types out of place, its bottom x shared with a second reader, in both orders
of the file - backward walks the layers in reverse, so in `<type>_accumulates` the other reader has written G[x] when the activation's
data launch runs (accumulate 1) and in `<type>_writes_first` it has not (accumulate 0).  PReLU in place behind a convolution, behind a
BatchNorm / Scale chain and behind an InnerProduct (a 2-d blob): the forward launch keeps the input, both gradient launches read the
copy.  PReLU with lr_mult 0 (the data launch alone) and with channel_shared (one slope, one gradient value); Bias and TanH in place.
Checked: the accumulate flag the plan gives the data launch, the loss at 1e-4 relative, and every parameter gradient by the rule of
tests/test_gpu_gate_fanout.py - rel_err < max(5e-4, 4 x torch float32's own error).  No net here has a ReLU or a MAX pooling, and a PReLU is
continuous at zero, so nothing of the device's forward pass has to be adopted.  A second step gives the same bits.
Without a GPU, on the reference alone: in the two-reader nets both writers of G[x] count - without either, the gradient of the
convolution in front misses by far more than the bound."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_act_ref import FANOUT, as_torch, fanout_case, torch_net

F32 = np.float32
BOUND = 5e-4


def reference(spec, params, x, dtype=torch.float64, cut=()):
    P = as_torch(params, grad=True, dtype=dtype)
    B = torch_net(spec, P, x, dtype=dtype, cut=cut)
    B["total_loss"].backward()
    return B, P


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(FANOUT))
def test_gradients_against_autograd(gpu, case):
    txt, layer, typ, acc = FANOUT[case]
    spec, params, x = fanout_case(case)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(proto.parse_text(txt), "TRAIN", activations=True), dict(spec.input_shapes),
                      params={k: [np.array(a) for a in v] for k, v in params.items()}, device=0, solver=sp, autotune=False)
    l = next(q for q in spec.layers if q.name == layer)
    n_el = int(np.prod(spec.blob_shapes[l.bottoms[0]]))
    learns = typ != "TanH" and l.lr_mult != [0.0]
    ops = [op for op in eng.bwd_ops if op.kind.startswith("act_bwd")]
    assert [(op.kind, op.name) for op in ops] == ([("act_bwd_param", layer)] if learns else []) + [("act_bwd", layer)]
    assert ops[-1].bytes == 4.0 * ((2 if typ == "Bias" else 3) + acc) * n_el, "the accumulate flag of the data launch"
    assert (layer in eng.aux_dev) == (typ == "PReLU" and l.tops == l.bottoms)      # the kept copy: an in-place PReLU alone
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step()
    B, P = reference(spec, params, x)
    want = float(B["total_loss"].detach())
    print("FANOUT %s loss %.6g want %.6g" % (case, out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want)
    _B32, P32 = reference(spec, params, x, torch.float32)
    got = eng.download_grads()
    for pl in spec.param_layers():
        for i, (gr, r, r32) in enumerate(zip(got[pl.name], P[pl.name], P32[pl.name])):
            if r.grad is None or (pl.lr_mult[i:i + 1] == [0.0]):      # (BatchNorm statistics, the frozen slopes: no gradient is computed)
                continue
            own = rel_err(r32.grad.numpy(), r.grad.numpy())
            err = rel_err(np.asarray(gr).reshape(r.grad.shape), r.grad.numpy())
            print("FANOUT %s %s[%d] %.3g (torch float32: %.3g)" % (case, pl.name, i, err, own))
            assert err < max(BOUND, 4 * own), "gradient %d of %s: %.3g (torch float32: %.3g)" % (i, pl.name, err, own)
    if learns:
        assert np.abs(got[layer][0]).max() > 0 and np.asarray(got[layer][0]).shape == tuple(spec.param_shapes[layer][0])
    eng.step()
    again = eng.download_grads()
    assert all(np.array_equal(a, b) for k in got for a, b in zip(got[k], again[k])), "the same step again: the same bits"
    eng.close()


@pytest.mark.parametrize("case", sorted(c for c in FANOUT if c.endswith(("_accumulates", "_writes_first"))))
def test_both_writers_of_the_shared_gradient_count(case):
    """No GPU: a plan that dropped either writer of G[x] - the activation's data launch or the other reader's - is far outside the bound."""
    _txt, layer, _typ, _acc = FANOUT[case]
    spec, params, x = fanout_case(case)
    _B, P = reference(spec, params, x)
    full = P["x"][0].grad.numpy()
    for lost in (layer, "other"):
        _B, Q = reference(spec, params, x, cut=(lost,))
        assert rel_err(Q["x"][0].grad.numpy(), full) > 100 * BOUND, (case, lost)
