"""The backward launch of ShuffleChannel (csrc/shuffle.hip with group C / g) in tiny TRAIN nets, -m gpu, against torch autograd in float64
(tests/torch_shuffle_ref.py), as tests/test_gpu_neuron_fanout.py checks the parameter-free activations.

The nets are tests/torch_shuffle_ref.FANOUT: the layer behind a grouped convolution and behind a Concat of two branches (a view Concat:
its bottom is a buffer two convolutions write into), its bottom x shared with a second reader, in both orders of the file - backward
walks the layers in reverse, so in `*_accumulates` the other reader has written G[x] when the layer's launch runs (accumulate 1) and in
`*_writes_first` it has not (accumulate 0); in front of a Slice whose tops are windows of the layer's top, with and without a second
reader of its bottom; on a 2-d blob.  The groups are 2 of 16 channels and 3 of 12: never self-inverse, so a gradient launched with g
instead of C / g is a different permutation.
Checked: the launches and the accumulate flag the plan gives the gradient launch, the loss at 1e-4 relative, and every parameter gradient
by the rule of tests/test_gpu_neuron_fanout.py - rel_err < max(5e-4, 4 x torch float32's own error).  A second step gives the same bits.
Without a GPU, on the reference alone: in the two-reader nets both writers of G[x] count, and a gradient routed by the forward
permutation instead of its inverse misses by far more than the bound."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from torch_shuffle_ref import FANOUT, as_torch, fanout_case, grad_errors, torch_net

BOUND = 5e-4


def reference(spec, params, x, dtype=torch.float64, cut=()):
    P = as_torch(params, grad=True, dtype=dtype)
    B = torch_net(spec, P, x, dtype=dtype, cut=cut)
    B["total_loss"].backward()
    return B, P


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(FANOUT))
def test_gradients_against_autograd(gpu, case):
    txt, layer, _typ, acc = FANOUT[case]
    spec, params, x = fanout_case(case)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(proto.parse_text(txt), "TRAIN"), dict(spec.input_shapes),
                      params={k: [np.array(a) for a in v] for k, v in params.items()}, device=0, solver=sp, autotune=False)
    l = next(q for q in spec.layers if q.name == layer)
    n_el = int(np.prod(spec.blob_shapes[l.bottoms[0]]))
    assert [(op.kind, op.name) for op in eng.ops if op.kind == "shuffle"] == [("shuffle", layer)]
    ops = [op for op in eng.bwd_ops if op.kind == "shuffle_bwd"]
    assert [(op.kind, op.name) for op in ops] == [("shuffle_bwd", layer)]
    assert ops[-1].bytes == 4.0 * (2 + acc) * n_el, "the accumulate flag of the launch"
    assert layer not in eng.aux_dev and eng.blobs[l.tops[0]].buf is not eng.blobs[l.bottoms[0]].buf      # nothing kept; the top owns storage
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = eng.step()
    B, P = reference(spec, params, x)
    want = float(B["total_loss"].detach())
    print("SHUFFLEFANOUT %s loss %.6g want %.6g" % (case, out["total_loss"], want))
    assert abs(out["total_loss"] - want) < 1e-4 * abs(want)
    got_y = eng.read_blob(l.tops[0])
    assert rel_err(got_y.reshape(B[l.tops[0]].shape), B[l.tops[0]].detach().numpy()) < 1e-4
    _B32, P32 = reference(spec, params, x, torch.float32)
    got = eng.download_grads()
    seen = 0
    for pl in spec.param_layers():
        errs = grad_errors(got[pl.name], [r.grad.numpy() for r in P[pl.name]], [r.grad.numpy() for r in P32[pl.name]])
        for i, (err, own) in enumerate(errs):
            print("SHUFFLEFANOUT %s %s[%d] %.3g (torch float32: %.3g)" % (case, pl.name, i, err, own))
            assert err < max(BOUND, 4 * own), "gradient %d of %s: %.3g (torch float32: %.3g)" % (i, pl.name, err, own)
            seen += 1
    front = "a" if "a" in got else "x"
    assert seen >= 4 and np.abs(got[front][0]).max() > 0      # the layer in front of the shuffle learns through it
    eng.step()
    again = eng.download_grads()
    assert all(np.array_equal(a, b) for k in got for a, b in zip(got[k], again[k])), "the same step again: the same bits"
    eng.close()


@pytest.mark.parametrize("case", sorted(c for c in FANOUT if c.endswith(("_accumulates", "_writes_first"))))
def test_both_writers_of_the_shared_gradient_count(case):
    """No GPU: a plan that dropped either writer of G[x] - the layer's launch or the other reader's - is far outside the bound."""
    _txt, layer, _typ, _acc = FANOUT[case]
    spec, params, x = fanout_case(case)
    _B, P = reference(spec, params, x)
    front = "a" if "a" in params else "x"
    full = P[front][0].grad.numpy()
    for lost in (layer, "other"):
        _B, Q = reference(spec, params, x, cut=(lost,))
        assert rel_err(Q[front][0].grad.numpy(), full) > 100 * BOUND, (case, lost)


@pytest.mark.parametrize("case", sorted(FANOUT))
def test_a_gradient_routed_by_the_forward_permutation_is_far_off(case, monkeypatch):
    """No GPU: the backward launch with group g instead of C / g (the permutation itself instead of its inverse)."""
    import torch_shuffle_ref as T
    spec, params, x = fanout_case(case)
    _B, P = reference(spec, params, x)

    right = T.shuffle

    class Wrong(torch.autograd.Function):
        @staticmethod
        def forward(ctx, v, g):
            ctx.g = g
            return right(v, g)

        @staticmethod
        def backward(ctx, d):
            return right(d, ctx.g), None      # (the right one is shuffle(d, C / g))
    monkeypatch.setattr(T, "shuffle", Wrong.apply)
    Q = as_torch(params, grad=True)
    T.torch_net(spec, Q, x)["total_loss"].backward()
    front = "a" if "a" in params else "x"
    assert rel_err(Q[front][0].grad.numpy(), P[front][0].grad.numpy()) > 100 * BOUND, case
