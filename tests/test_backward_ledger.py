"""The ledger of the backward planner's layer types (no GPU), like tests/test_guard_coverage.py for the kernels.

Every key of BackwardPlanner.emitters and BackwardPlanner.one_bottom - read from a planner built on a stub engine, not listed by hand -
is in exactly one of three sets:
  cases        the types a case of the fan-out matrix (tests/test_gpu_backward_fanout.CASES) runs as the layer under test;
  NO_GRADIENT  type -> why no launch of it writes a dX;
  REFUSES      type -> the condition (a key of test_gpu_backward_fanout.REFUSALS) under which the planner declines the type's dX: a type
               is here when the matrix cannot give it an accumulate case because accumulating is what it refuses.
A new emitter therefore needs a fan-out case or a stated refusal.  The refusals of types that DO have a case (Eltwise PROD, a learnable
depthwise Deconvolution, ...) are conditions of REFUSALS as well and are raised on the GPU by that file; the three the storage plan keeps
any net from reaching today - Eltwise SUM, Sigmoid and LRN on channel slices - are raised here, on hand-made views."""
import types

import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.engine import Blob
from fcn_object_detector_amd.netspec import DATA_TYPES, Layer
import test_gpu_backward_fanout as F
from test_gpu_backward_fanout import CASES, LEAKY, REFUSALS, VARIANTS
from plan_stub import engine_factory      # (the stub engine of the plan tests: no device, a library that returns 0)

NO_GRADIENT = {
    **{t: "a data layer: it has no bottom" for t in DATA_TYPES},
    "Accuracy": "a metric: nothing is differentiated through it and it has no entry in loss_blobs",
    "Power": "only as the input transform on a net input: nothing upstream of it learns",
    "L1Loss": "a loss: the forward launch writes the gradient of its bottom, the planner only marks it written",
    "EuclideanLoss": "a loss: the forward launch writes the gradient of its bottom, the planner only marks it written",
    "SoftmaxWithLoss": "a loss: the forward launch writes the gradient of its bottom, the planner only marks it written",
    "Slice": "its tops are views of the bottom, and so are their gradients: no launch (a Slice that copies is refused)",
}
REFUSES = {"Dropout": "Dropout into an already written gradient"}


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False)


@pytest.fixture
def planner(monkeypatch):
    monkeypatch.setattr(BW.L, "load", lambda: None)
    eng = types.SimpleNamespace(spec=None, blobs={}, grad_blobs={}, _conv_layer_meta={}, aux_dev={})
    return BW.BackwardPlanner(eng)


def test_the_three_sets_partition_the_planners_tables(planner):
    table = set(planner.emitters) | set(planner.one_bottom)
    assert len(table) >= 20 and {"Convolution", "Pooling", "Upsample", "Input"} <= table
    cases = {t for c in CASES for t in c.types}
    sets = {"cases": cases, "NO_GRADIENT": set(NO_GRADIENT), "REFUSES": set(REFUSES)}
    for name, s in sets.items():
        assert not s - table, "%s names types the planner has no entry for: %s" % (name, sorted(s - table))
    assert not table - cases - set(NO_GRADIENT) - set(REFUSES), "types without a fan-out case or a stated refusal: %s" % sorted(
        table - cases - set(NO_GRADIENT) - set(REFUSES))
    for a, b in (("cases", "NO_GRADIENT"), ("cases", "REFUSES"), ("NO_GRADIENT", "REFUSES")):
        assert not sets[a] & sets[b], "types in both %s and %s: %s" % (a, b, sorted(sets[a] & sets[b]))
    assert all(isinstance(r, str) and len(r) > 20 for r in NO_GRADIENT.values())


def test_every_stated_refusal_is_raised_by_a_test(planner):
    for t, condition in REFUSES.items():
        assert condition in REFUSALS and REFUSALS[condition][0] == t, (t, condition)
    table = set(planner.emitters) | set(planner.one_bottom)
    assert {t for t, _, _ in REFUSALS.values()} <= table


def test_the_matrix_has_the_shape_the_ledger_counts_on():
    assert len({c.name for c in CASES}) == len(CASES) >= 24
    assert ("t_first", False) in VARIANTS and ("s_first", False) in VARIANTS and ("t_first", True) in VARIANTS
    assert all(c.writer[1].split(":")[0] in ("t", "ct") for c in CASES)
    assert {c.c for c in CASES} == {6, 8} and len(LEAKY) >= 4


def _view(name, shape, ptr, coffset=0, cstride=8):
    b = Blob(name, shape)
    b.buf, b.coffset, b.cstride = types.SimpleNamespace(ptr=ptr), coffset, cstride
    return b


def _layer(text):
    return Layer(proto.parse_text(text))


def test_channel_slices_are_refused_by_layer_name(planner):
    """The storage plan hands Eltwise, Sigmoid and LRN whole buffers today (a Concat member or a Slice top that one of them reads or writes
    is copied), so no net reaches these three guards; they hold on views made by hand."""
    shape = (2, 4, 3, 3)
    planner.B.update(x=_view("x", shape, 0x1000), y=_view("y", shape, 0x2000))
    planner.G.update(x=_view("x", shape, 0x3000, coffset=4), y=_view("y", shape, 0x4000))
    planner.mark(planner.G["y"])
    planner.e.aux_dev["n"] = types.SimpleNamespace(ptr=0x5000)
    with pytest.raises(NotImplementedError, match=r"LRN backward on channel slices \(n\)"):
        planner._lrn(_layer('name: "n" type: "LRN" bottom: "x" top: "y"'), planner.G["y"], planner.G["x"], 0)
    planner.skip_sigmoid_of = {"y": "conv"}
    with pytest.raises(NotImplementedError, match=r"sigmoid backward on channel slices \(sg\)"):
        planner._sigmoid(_layer('name: "sg" type: "Sigmoid" bottom: "x" top: "y"'))
    planner.mark(planner.G["x"])
    with pytest.raises(NotImplementedError, match=r"Eltwise SUM backward accumulating into a channel slice \(e\)"):
        planner._eltwise(_layer('name: "e" type: "Eltwise" bottom: "x" bottom: "x" top: "y"'))
    assert planner.ops == []


def test_no_fused_mask_is_built_for_a_relu_with_a_slope(stub):
    """The masks that ride in other launches - CONV_MASK, the BatchNorm chain's, PoolBwd.mask - mean slope 0.  A ReLU with a slope stays
    out of the convolution's epilogue and ends the BatchNorm chain in front of it, so in the backward plan it is a launch of its own with
    its slope, and neither the MAX pooling that writes dc0 nor the BatchNorm apply launch carries a mask."""
    text = F.HEAD + F.conv("c0", "data", 8, "kernel_size: 3 pad: 1") + F.relu("lr0", "c0", None, 0.1) + \
        F.MAXPOOL % ("m", "c0", "m", "", 3, " pad: 1") + F.fc("fa", "m") + (F.BN % "").replace("FAN", "c0") + F.relu("t_relu", "t", None, 0.1) + \
        F.fc("fb", "t") + F.tail(["fa", "fb"])
    e = stub(text, "TRAIN")
    assert e._conv_layer_meta["c0"]["relu"] is False
    assert e._bn_chains["t"].relu is None and e._bn_chains["t"].scale.name == "t_sc"
    assert {"lr0", "t_relu"} <= {t.layer.name for t in e.tasks} and not e._fused_relu_layers()
    seen = {}
    for name in ("fcn_relu_bwd_slope_f32", "fcn_maxpool_bwd_mask_f32", "fcn_batchnorm_bwd_apply_f32"):
        setattr(e.fake, name, lambda *a, name=name: seen.setdefault(name, []).append(a) or 0)
    plan = BW.BackwardPlanner(e)
    plan.run()
    e._adopt_backward(plan)
    kinds = [(op.kind, op.name) for op in plan.ops]
    assert [kn for kn in kinds if kn[0] in ("relu_bwd", "maxpool_bwd", "bn_bwd_apply")] == [
        ("relu_bwd", "t_relu"), ("bn_bwd_apply", "t"), ("maxpool_bwd", "m"), ("relu_bwd", "lr0")]
    assert not plan.relu_ops and not plan.dgrad_records
    for op in plan.ops:
        if op.kind in ("relu_bwd", "maxpool_bwd", "bn_bwd_apply"):
            op.run(None)
    G, B = e.grad_blobs, e.blobs
    # (dy, y, dx, pixels, C, cstride, slope, accumulate, stream): t_relu and lr0 in place, never accumulating
    assert seen["fcn_relu_bwd_slope_f32"] == [(G["t"].ptr, B["t"].ptr, G["t"].ptr, 220, 8, 8, 0.1, 0, None),
                                             (G["c0"].ptr, B["c0"].ptr, G["c0"].ptr, 220, 8, 8, 0.1, 0, None)]
    (pool,), (apply,) = seen["fcn_maxpool_bwd_mask_f32"], seen["fcn_batchnorm_bwd_apply_f32"]
    assert pool[-5] == 1 and pool[-4:] == (None, 0, 0, None)      # adds into what the BatchNorm apply wrote, without a mask
    assert apply[2] is None and apply[-2] == 0
