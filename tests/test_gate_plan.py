"""The gated Scale (csrc/gate.hip) as the forward and backward planners lay it out - without a GPU.

The stub engine of tests/plan_stub.py (a NetSpec built by NetSpec.public's rule, so with scale_gate=True): Engine /
TrainEngine / BackwardPlanner methods run with DeviceBuffer replaced by a counter of addresses and the library by one whose entry points
return 0 (size queries: 64).  Checked: the fused launch list of a TEST engine and its operands, every reason not to fuse, the TRAIN
forward unfused, the backward op order of one SE block, the half-float plan (gate float32, top halves), and that a ResNet - a net
without a two-bottom Scale or an Axpy - has the same launch lists and storage plans with and without the keyword."""
import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import models
from fcn_object_detector_amd import storage as S
from plan_stub import engine_factory


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, public=True, backward=False)


# one SE block on a 12-channel branch: a convolution (the branch), global pooling, squeeze, excite, Sigmoid, the gate, the residual add
BLOCK = """
layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 12 dim: 5 dim: 7 } } }
layer { name: "short" type: "Convolution" bottom: "data" top: "short" convolution_param { num_output: 12 kernel_size: 1 } }
layer { name: "x" type: "Convolution" bottom: "data" top: "x" convolution_param { num_output: 12 kernel_size: 3 pad: 1 } }
layer { name: "pool" type: "Pooling" bottom: "x" top: "pool" pooling_param { pool: AVE global_pooling: true } }
layer { name: "down" type: "InnerProduct" bottom: "pool" top: "down" inner_product_param { num_output: 4 } }
layer { name: "down/relu" type: "ReLU" bottom: "down" top: "down" }
layer { name: "up" type: "InnerProduct" bottom: "down" top: "up" inner_product_param { num_output: 12 } }
layer { name: "gate" type: "Sigmoid" bottom: "up" top: "gate" }
SCALE
ELTWISE
layer { name: "out/relu" type: "ReLU" bottom: "out" top: "out" }
TAIL
"""
SCALE = 'layer { name: "sc" type: "Scale" bottom: "x" bottom: "gate" top: "sc" scale_param { axis: 0 } }'
ELTWISE = 'layer { name: "out" type: "Eltwise" bottom: "sc" bottom: "short" top: "out" }'
TRAIN_TAIL = ('layer { name: "target" type: "Input" top: "target" input_param { shape { dim: 2 dim: 12 dim: 5 dim: 7 } } }\n'
              'layer { name: "loss" type: "EuclideanLoss" bottom: "out" bottom: "target" top: "loss" }')


def block(scale=SCALE, eltwise=ELTWISE, tail=""):
    return BLOCK.replace("SCALE", scale).replace("ELTWISE", eltwise).replace("TAIL", tail)


def gate_ops(e):
    return [(t.layer.name, op) for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind == "scale_gate"]


def run(e, ops):
    del e.fake.calls[:]
    for op in ops:
        op.run(None)
    return list(e.fake.calls)


@pytest.mark.parametrize("f16", [False, True])
def test_the_fused_launch(stub, f16):
    e = stub(block(), f16=f16)
    ops = gate_ops(e)
    assert [(ln, op.name) for ln, op in ops] == [("out", "sc+out+out/relu")]                 # ONE launch, at the Eltwise's place in the order
    names = [t.layer.name for t in e.tasks]
    assert "sc" not in names and "out/relu" not in names and names.index("out") > names.index("short")
    assert not [op for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind in ("eltwise", "relu")]
    B = e.blobs
    x, g, r, y = B["x"], B["gate"], B["short"], B["out"]
    assert g.esize == 4 and all(b.esize == (2 if f16 else 4) for b in (x, r, y, B["sc"]))    # the gate is float32 in both engines
    (name, a), = run(e, [ops[0][1]])
    assert name == ("fcn_scale_gate_fwd_f16" if f16 else "fcn_scale_gate_fwd_f32")
    assert a == (x.buf.ptr, g.ptr, r.buf.ptr, y.buf.ptr, 2, 35, 12, x.cstride, x.coffset, g.cstride, r.cstride, r.coffset, y.cstride, y.coffset, 1, None)
    task = next(t for t in e.tasks if t.layer.name == "out")
    assert sorted(task.reads) == sorted(e._range(b) for b in ("x", "gate", "short")) and task.writes == [e._range("out")]
    # the Scale top owns a buffer that the fused launch leaves alone: read_blob() fills it on demand with the layer's own launch
    (name, a), = run(e, e._lazy_blob_ops["sc"])
    assert a[:4] == (x.buf.ptr, g.ptr, None, B["sc"].buf.ptr) and a[-2] == 0 and a[4:7] == (2, 35, 12)


def test_the_fused_launch_without_a_relu_and_with_the_residual_first(stub):
    e = stub(block(eltwise=ELTWISE.replace('bottom: "sc" bottom: "short"', 'bottom: "short" bottom: "sc"')).replace(
        'layer { name: "out/relu" type: "ReLU" bottom: "out" top: "out" }', ""))
    (ln, op), = gate_ops(e)
    assert (ln, op.name) == ("out", "sc+out")
    (_n, a), = run(e, [op])
    assert a[2] == e.blobs["short"].buf.ptr and a[-2] == 0


NOT_FUSED = {
    "another reader of the Scale top": dict(tail='layer { name: "p2" type: "Pooling" bottom: "sc" top: "p2" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }'),
    "coefficients other than 1": dict(eltwise=ELTWISE.replace("top:", "eltwise_param { coeff: 1 coeff: -1 } top:")),
    "the PROD operation": dict(eltwise=ELTWISE.replace("top:", "eltwise_param { operation: PROD } top:")),
    "the MAX operation": dict(eltwise=ELTWISE.replace("top:", "eltwise_param { operation: MAX } top:")),
    "more than two bottoms": dict(eltwise=ELTWISE.replace('bottom: "short"', 'bottom: "short" bottom: "short"')),
    "the Scale top twice": dict(eltwise=ELTWISE.replace('bottom: "short"', 'bottom: "sc"')),
    "in place on x": dict(scale=SCALE.replace('top: "sc"', 'top: "x"'), eltwise=ELTWISE.replace('bottom: "sc"', 'bottom: "x"')),
}


@pytest.mark.parametrize("why", sorted(NOT_FUSED))
def test_reasons_not_to_fuse(stub, why):
    e = stub(block(**NOT_FUSED[why]))
    ops = gate_ops(e)
    assert [(ln, op.name) for ln, op in ops] == [("sc", "sc")], why
    (_n, a), = run(e, [ops[0][1]])
    assert a[2] is None and a[-2] == 0                                                      # no residual, no ReLU
    assert [op.kind for t in e.tasks if isinstance(t, E.OpTask) and t.layer.name == "out" for op in t.ops] == \
        ["eltwise"] * (2 if why == "more than two bottoms" else 1)
    assert e._lazy_blob_ops == {}


def test_no_fusion_when_the_scale_top_is_an_output_or_fuse_is_off(stub):
    alone = BLOCK.replace("SCALE", SCALE).replace("ELTWISE", "").replace('layer { name: "out/relu" type: "ReLU" bottom: "out" top: "out" }', "")
    e = stub(alone.replace("TAIL", ""))
    assert "sc" in e.outputs and [(ln, op.name) for ln, op in gate_ops(e)] == [("sc", "sc")]
    e = stub(block(), fuse=False)
    assert [(ln, op.name) for ln, op in gate_ops(e)] == [("sc", "sc")]


def test_a_window_the_kernel_refuses_means_no_fusion(stub):
    """storage.plan_blobs makes no window off a 16-byte group, so none can be written as a net: the residual's view is moved by hand."""
    e = stub(block())
    li, sc = next((i, l) for i, l in enumerate(e.spec.layers) if l.name == "sc")
    assert e._gate_fusion(li, sc).name == "out"
    e.blobs["short"].coffset = 2
    assert e._gate_fusion(li, sc) is None
    e.blobs["short"].coffset, e.blobs["out"].esize = 0, 2
    assert e._gate_fusion(li, sc) is None


def test_the_train_forward_is_unfused_and_the_backward_order_of_one_block(stub):
    e = stub(block(tail=TRAIN_TAIL), "TRAIN")
    assert [(ln, op.name) for ln, op in gate_ops(e)] == [("sc", "sc")]
    assert [op.kind for t in e.tasks if isinstance(t, E.OpTask) and t.layer.name == "out" for op in t.ops] == ["eltwise"]
    plan = BW.BackwardPlanner(e)
    plan.run()
    e._adopt_backward(plan)
    kinds = [(op.kind, op.name) for op in plan.ops if op.kind in ("scale_gate_bwd", "avepool_bwd", "sigmoid_bwd", "eltwise_bwd")]
    assert kinds == [("eltwise_bwd", "out:sc"), ("eltwise_bwd", "out:short"), ("scale_gate_bwd", "sc:x"), ("scale_gate_bwd", "sc:gate"),
                     ("sigmoid_bwd", "gate"), ("avepool_bwd", "pool")]
    assert plan.gate_ws is not None and plan.gate_ws.nbytes == 64
    assert [a for n, a in e.fake.calls if n == "fcn_scale_gate_workspace_bytes"] == [(2, 35, 12)]
    B, G = e.blobs, e.grad_blobs
    ops = {op.name: op for op in plan.ops if op.kind in ("scale_gate_bwd", "avepool_bwd")}
    (n1, a1), (n2, a2), (n3, a3) = run(e, [ops["sc:x"], ops["sc:gate"], ops["pool"]])
    assert (n1, n2, n3) == ("fcn_scale_gate_bwd_data_f32", "fcn_scale_gate_bwd_gate_f32", "fcn_avepool_bwd_f32")
    gt, gx, gg = G["sc"], G["x"], G["gate"]
    assert a1 == (gt.buf.ptr, B["gate"].ptr, gx.buf.ptr, 2, 35, 12, gt.cstride, gt.coffset, B["gate"].cstride, gx.cstride, gx.coffset, 0, None)
    assert a2 == (gt.buf.ptr, B["x"].buf.ptr, gg.ptr, 2, 35, 12, gt.cstride, gt.coffset, B["x"].cstride, B["x"].coffset, gg.cstride, 0,
                  plan.gate_ws.ptr, None)
    assert a3[-2] == 1                                                                      # the pooling's backward accumulates into G[x]


def test_a_bottom_without_a_gradient_is_skipped(stub):
    """x comes from a frozen convolution on the data: only the gate's branch learns."""
    text = block(tail=TRAIN_TAIL).replace('top: "x" convolution_param', 'top: "x" param { lr_mult: 0 } param { lr_mult: 0 } convolution_param')
    e = stub(text, "TRAIN")
    plan = BW.BackwardPlanner(e)
    plan.run()
    assert [op.name for op in plan.ops if op.kind == "scale_gate_bwd"] == ["sc:gate"] and "x" not in e.grad_blobs


def test_half_float_refusals_by_layer_name(stub):
    text = ('layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 8 dim: 3 dim: 3 } } }\n'
            'layer { name: "g" type: "Input" top: "g" input_param { shape { dim: 2 dim: 8 } } }\n'
            'layer { name: "x" type: "Convolution" bottom: "data" top: "x" convolution_param { num_output: 8 kernel_size: 1 } }\n'
            'GATE\n'
            'layer { name: "sc" type: "Scale" bottom: "x" bottom: "GNAME" top: "sc" scale_param { axis: 0 } }\n'
            'layer { name: "y" type: "Convolution" bottom: "sc" top: "y" convolution_param { num_output: 8 kernel_size: 1 } }\n')
    with pytest.raises(NotImplementedError, match="Scale sc takes its multiplier g from an input of the net"):
        stub(text.replace("GATE", "").replace("GNAME", "g"), f16=True)
    assert gate_ops(stub(text.replace("GATE", "").replace("GNAME", "g")))                    # (a float32 engine takes it)
    pooled = ('layer { name: "pool" type: "Pooling" bottom: "x" top: "pool" pooling_param { pool: AVE global_pooling: true } }\n'
              'layer { name: "fc" type: "InnerProduct" bottom: "pool" top: "fc" inner_product_param { num_output: 8 } }')
    with pytest.raises(NotImplementedError, match="Scale sc: the multiplier fc is stored as halves"):
        stub(text.replace("GATE", pooled).replace("GNAME", "fc"), f16=True)


def signature(e):
    """What a plan launches and where everything lies: (layer, kinds and names of its ops, reads, writes) per task, and every blob's view."""
    tasks = [(t.layer.name, [(op.kind, op.name) for op in getattr(t, "ops", [])], sorted(t.reads), sorted(t.writes)) for t in e.tasks]
    views = {n: (b.shape, b.esize, b.buf.ptr, b.coffset, b.cstride) for n, b in e.blobs.items()}
    return tasks, views, sorted(e._lazy_blob_ops)


@pytest.mark.parametrize("phase,f16", [("TEST", False), ("TRAIN", False), ("TEST", True)])
def test_a_resnet_plans_the_same_with_and_without_the_keyword(stub, phase, f16):
    text = models.resnet("TRAIN" if phase == "TRAIN" else "DEPLOY", depth=50, width_div=8, size=64, batch=2, num_classes=10)
    sigs, plans, bwd = [], [], []
    for flag in (False, True):
        e = stub(text, phase, f16=f16, scale_gate=flag)
        sigs.append(signature(e))
        plans.append(S.plan_blobs(e.spec, e.shapes, e.inputs, e.outputs, f16, True, True))
        if phase == "TRAIN":
            plan = BW.BackwardPlanner(e)
            plan.run()
            bwd.append(([(op.kind, op.name) for op in plan.ops], plan.gate_ws))
    assert sigs[0] == sigs[1]
    assert plans[0].views == plans[1].views and plans[0].root_bytes == plans[1].root_bytes and plans[0].alias == plans[1].alias
    assert not bwd or (bwd[0] == bwd[1] and bwd[0][1] is None)


@pytest.mark.parametrize("form", ["scale", "axpy"])
def test_se_resnet_plans_one_fused_launch_per_block(stub, form):
    text = models.se_resnet("DEPLOY", depth=50, width_div=8, size=64, batch=2, num_classes=10, reduction=4, form=form)
    for f16 in (False, True):
        e = stub(text, f16=f16)
        ops = gate_ops(e)
        assert len(ops) == 16 and all(op.name == "%s/scale+%s+%s/relu" % (ln, ln, ln) for ln, op in ops)
        assert all(e.blobs[ln + "_prob"].esize == 4 and e.blobs[ln].esize == (2 if f16 else 4) for ln, _op in ops)
    e = stub(models.se_resnet("TRAIN", depth=50, width_div=8, size=64, batch=2, num_classes=10, reduction=4, form=form), "TRAIN")
    assert len(gate_ops(e)) == 16 and all(op.name == ln for ln, op in gate_ops(e))
    plan = BW.BackwardPlanner(e)
    plan.run()
    assert len([op for op in plan.ops if op.kind == "scale_gate_bwd"]) == 32


def bwd_gate_calls(e):
    plan = BW.BackwardPlanner(e)
    plan.run()
    e._adopt_backward(plan)
    ops = [op for op in plan.ops if op.kind == "scale_gate_bwd"]
    return [op.name for op in ops], {op.name: a for op, (_n, a) in zip(ops, run(e, ops))}, plan


FANOUT_TAIL = ('layer { name: "out2" type: "Eltwise" bottom: "out" bottom: "x" top: "out2" }\n' +
               TRAIN_TAIL.replace('bottom: "out" bottom: "target"', 'bottom: "out2" bottom: "target"'))


def test_each_gradient_launch_carries_its_own_accumulate_flag_x_written_first(stub):
    """x has a second reader behind the Scale: its backward writes G[x] first, so the data gradient accumulates and the gate's does not."""
    e = stub(block(tail=FANOUT_TAIL), "TRAIN")
    names, calls, plan = bwd_gate_calls(e)
    assert names == ["sc:x", "sc:gate"]
    order = [op.name for op in plan.ops if op.kind in ("eltwise_bwd", "scale_gate_bwd")]
    assert order.index("out2:x") < order.index("sc:x")
    assert calls["sc:x"][-2] == 1 and calls["sc:gate"][-3] == 0
    data_op = next(op for op in plan.ops if op.name == "sc:x")
    assert data_op.bytes == 4.0 * 3 * 2 * 35 * 12                                            # the estimate and the launch agree: dy, dx read, dx written


def test_each_gradient_launch_carries_its_own_accumulate_flag_gate_written_first(stub):
    """One gate for two Scales: the later one writes G[gate] first, the earlier one accumulates into it - and its data gradient does not."""
    two = SCALE + '\nlayer { name: "sc2" type: "Scale" bottom: "short" bottom: "gate" top: "sc2" scale_param { axis: 0 } }'
    e = stub(block(scale=two, eltwise=ELTWISE.replace('bottom: "short"', 'bottom: "sc2"'), tail=TRAIN_TAIL), "TRAIN")
    names, calls, _plan = bwd_gate_calls(e)
    assert names == ["sc2:short", "sc2:gate", "sc:x", "sc:gate"]
    assert (calls["sc2:short"][-2], calls["sc2:gate"][-3]) == (0, 0)
    assert (calls["sc:x"][-2], calls["sc:gate"][-3]) == (0, 1)
    G = e.grad_blobs
    assert calls["sc:x"][2] == G["x"].buf.ptr and calls["sc2:short"][2] == G["short"].buf.ptr and calls["sc:gate"][2] == calls["sc2:gate"][2] == G["gate"].ptr


LATER_WRITERS = {
    "the Eltwise in place over x": dict(eltwise='layer { name: "out" type: "Eltwise" bottom: "sc" bottom: "x" top: "x" }\n'
                                                'layer { name: "cp" type: "Pooling" bottom: "x" top: "out" pooling_param { pool: MAX kernel_size: 1 stride: 1 } }'),
    "a later layer in place on x": dict(tail='layer { name: "xr" type: "ReLU" bottom: "x" top: "x" }'),
    "a later layer in place on the gate": dict(tail='layer { name: "gr" type: "ReLU" bottom: "gate" top: "gate" }'),
}


@pytest.mark.parametrize("why", sorted(LATER_WRITERS))
def test_no_fusion_when_x_or_the_gate_is_written_behind_the_scale(stub, why):
    """read_blob() would compute the skipped Scale top from what x and the gate hold after the forward pass."""
    e = stub(block(**LATER_WRITERS[why]))
    assert [(ln, op.name) for ln, op in gate_ops(e)] == [("sc", "sc")] and e._lazy_blob_ops == {}


def test_no_fusion_when_x_is_no_nhwc_view(stub):
    e = stub(block())
    li, sc = next((i, l) for i, l in enumerate(e.spec.layers) if l.name == "sc")
    assert e._gate_fusion(li, sc).name == "out"
    e.blobs["x"].shape = (2, 12, 5, 7, 1)
    assert e._gate_fusion(li, sc) is None
