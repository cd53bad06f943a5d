"""The Interp layer as the forward and backward planners lay it out - without a GPU.

As tests/test_dilation_plan.py: Engine / TrainEngine / BackwardPlanner methods run on the stub engine of tests/plan_stub.py with DeviceBuffer replaced by a
counter of addresses and the library by one whose every entry point returns 0 and keeps its arguments; what is checked is which entry
point an op calls with which geometry, the bytes it books, the accumulate flag of a fan-in, and that a label path gets no backward op."""
import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from plan_stub import FakeBuffer, engine_factory

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
TEST_NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 14 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 6 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "up" type: "Interp" bottom: "c0" top: "up" interp_param { zoom_factor: 4 pad_beg: -1 pad_end: -2 } }
""".replace("FILL", FILL)
TRAIN_NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 14 }
input: "target_u" input_shape { dim: 2 dim: 5 dim: 23 dim: 27 }
input: "target" input_shape { dim: 2 dim: 5 dim: 12 dim: 14 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "up" type: "Interp" bottom: "c0" top: "up" interp_param { height: 23 width: 27 } }
layer { name: "cu" type: "Convolution" bottom: "up" top: "cu" convolution_param { num_output: 5 kernel_size: 3 pad: 1 FILL } }
layer { name: "loss_u" type: "EuclideanLoss" bottom: "cu" bottom: "target_u" top: "loss_u" }
layer { name: "c1" type: "Convolution" bottom: "c0" top: "c1" convolution_param { num_output: 5 kernel_size: 3 pad: 1 FILL } }
layer { name: "loss" type: "EuclideanLoss" bottom: "c1" bottom: "target" top: "loss" }
""".replace("FILL", FILL)
LABEL_NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 17 dim: 17 }
input: "label" input_shape { dim: 2 dim: 1 dim: 17 dim: 17 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 5 kernel_size: 1 stride: 8 FILL } }
layer { name: "label_shrink" type: "Interp" bottom: "label" top: "label_shrink" interp_param { shrink_factor: 8 pad_beg: 0 pad_end: 0 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "c0" bottom: "label_shrink" top: "loss" loss_param { ignore_label: 255 } }
""".replace("FILL", FILL)


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False)


def interp_op(e, name):
    ops = [t.ops for t in e.tasks if isinstance(t, E.OpTask) and t.layer.name == name]
    assert len(ops) == 1 and len(ops[0]) == 1
    return ops[0][0]


def test_the_forward_op(stub):
    e = stub(TEST_NET)
    x, y = e.blobs["c0"], e.blobs["up"]
    assert y.shape == (2, 6, 33, 41) and (x.esize, y.esize) == (4, 4)              # 9 x 11 effective -> 9 + 8 * 3, 11 + 10 * 3
    op = interp_op(e, "up")
    assert (op.kind, op.name, op.flops) == ("interp", "up", 0.0)
    assert op.bytes == 4.0 * 2 * 9 * 11 * 6 + 4.0 * 2 * 33 * 41 * 6               # the effective input once, the output once
    op.run(None)
    assert e.fake.names()[-1] == "fcn_interp_fwd_f32"
    assert e.fake.args["fcn_interp_fwd_f32"] == (x.buf.ptr, y.buf.ptr, 2, 12, 14, 6, 8, 0, -1, -2, 33, 41, 8, 0, None)
    t = [t for t in e.tasks if t.layer.name == "up"][0]
    assert t.reads == [e._range("c0")] and t.writes == [e._range("up")]


def test_the_half_float_engine_takes_an_interp_that_writes_the_float32_output(stub):
    e = stub(TEST_NET, f16=True)
    x, y = e.blobs["c0"], e.blobs["up"]
    assert (x.esize, y.esize) == (2, 4) and (x.cstride, y.cstride) == (8, 8)
    op = interp_op(e, "up")
    assert op.bytes == 2.0 * 2 * 9 * 11 * 6 + 4.0 * 2 * 33 * 41 * 6
    op.run(None)
    assert e.fake.names()[-1] == "fcn_interp_fwd_f16"
    assert e.fake.args["fcn_interp_fwd_f16"] == (x.buf.ptr, y.buf.ptr, 2, 12, 14, 6, 8, 0, -1, -2, 33, 41, 8, 0, 1, None)
    # between two half blobs: halves out
    mid = TEST_NET + 'layer { name: "c2" type: "Convolution" bottom: "up" top: "c2" convolution_param { num_output: 4 kernel_size: 1 FILL } }'.replace("FILL", FILL)
    e = stub(mid, f16=True)
    assert (e.blobs["c0"].esize, e.blobs["up"].esize, e.blobs["c2"].esize) == (2, 2, 4)
    interp_op(e, "up").run(None)
    assert e.fake.args["fcn_interp_fwd_f16"][-2] == 0 and interp_op(e, "up").bytes == 2.0 * 2 * 6 * (9 * 11 + 33 * 41)
    # a float32 input (the net's own) into a half blob has no kernel: refused by name
    bad = TEST_NET.replace('bottom: "c0" top: "up"', 'bottom: "data" top: "up"') + \
        'layer { name: "c2" type: "Convolution" bottom: "up" top: "c2" convolution_param { num_output: 4 kernel_size: 1 FILL } }'.replace("FILL", FILL)
    with pytest.raises(NotImplementedError, match="f16 engine: Interp up reads the float32 blob data"):
        stub(bad, f16=True)


def test_no_backward_op_for_the_label(stub):
    e = stub(LABEL_NET, "TRAIN")
    assert e.blobs["label_shrink"].shape == (2, 1, 3, 3) and "label_shrink" not in e.grad_blobs and "label" not in e.grad_blobs
    op = interp_op(e, "label_shrink")
    op.run(None)
    assert e.fake.args["fcn_interp_fwd_f32"][2:14] == (2, 17, 17, 1, 4, 0, 0, 0, 3, 3, 4, 0)
    plan = BW.BackwardPlanner(e)
    by = {l.name: l for l in e.spec.layers}
    assert "Interp" in plan.one_bottom and "Interp" not in plan.emitters
    plan._one_bottom(by["label_shrink"])
    assert plan.ops == []


def test_the_accumulate_flag_of_a_fan_in(stub):
    e = stub(TRAIN_NET, "TRAIN")
    G = e.grad_blobs
    assert {"c0", "up", "cu", "c1"} <= set(G) and G["up"].shape == (2, 8, 23, 27)
    by = {l.name: l for l in e.spec.layers}
    # alone: one launch writes all of dX
    plan = BW.BackwardPlanner(e)
    plan.mark(G["up"])
    plan._one_bottom(by["up"])
    assert [(op.kind, op.name) for op in plan.ops] == [("interp_bwd", "up")] and plan.state(G["c0"]) == "full"
    op = plan.ops[0]
    assert op.bytes == 4.0 * 8 * (2 * 23 * 27 + 2 * 12 * 14)
    op.run(None)
    assert e.fake.args["fcn_interp_bwd_f32"] == (G["up"].buf.ptr, G["c0"].buf.ptr, 2, 12, 14, 8, 8, 0, 0, 0, 23, 27, 8, 0, 0, None)
    # behind another writer of the same gradient (c1's data gradient comes first in the reversed layer list): it adds
    plan = BW.BackwardPlanner(e)
    plan.mark(G["c0"])
    plan.mark(G["up"])
    plan._one_bottom(by["up"])
    op = plan.ops[-1]
    assert op.kind == "interp_bwd" and op.bytes == 4.0 * 8 * (2 * 23 * 27 + 2 * 2 * 12 * 14)
    op.run(None)
    assert e.fake.args["fcn_interp_bwd_f32"][-2] == 1
    # nothing arrived at the top: nothing to hand down
    plan = BW.BackwardPlanner(e)
    plan._one_bottom(by["up"])
    assert plan.ops == []


PYRAMID_NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 12 }
input: "target" input_shape { dim: 2 dim: 4 dim: 12 dim: 12 }
layer { name: "feat" type: "Convolution" bottom: "data" top: "feat" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "pool" type: "Pooling" bottom: "feat" top: "pool" pooling_param { pool: AVE kernel_size: 6 stride: 6 } }
layer { name: "up" type: "Interp" bottom: "pool" top: "up" interp_param { height: 12 width: 12 } }
layer { name: "cat" type: "Concat" bottom: "feat" bottom: "up" top: "cat" }
layer { name: "score" type: "Convolution" bottom: "cat" top: "score" convolution_param { num_output: 4 kernel_size: 3 pad: 1 FILL } }
layer { name: "loss" type: "EuclideanLoss" bottom: "score" bottom: "target" top: "loss" }
""".replace("FILL", FILL)


def test_a_copying_concat_hands_its_gradient_down(stub):
    """The pyramid head's Concat copies (feat has the pooling as a second consumer), so its members' gradients are buffers of their own:
    each gets its channels of dY through the Crop adjoint over the whole extent, and the pooling then adds into feat's."""
    e = stub(PYRAMID_NET, "TRAIN")
    G = e.grad_blobs
    assert "cat" in e.copy_concats and not e.alias
    assert len({G[n].buf.ptr for n in ("feat", "up", "cat")}) == 3
    by = {l.name: l for l in e.spec.layers}
    plan = BW.BackwardPlanner(e)
    plan._concat(by["cat"])
    assert plan.ops == []                                             # nothing arrived yet
    plan.mark(G["cat"])
    plan._concat(by["cat"])
    assert [(op.kind, op.name) for op in plan.ops] == [("concat_bwd", "cat:feat"), ("concat_bwd", "cat:up")]
    for op, name, off in zip(plan.ops, ("feat", "up"), (0, 8)):
        op.run(None)
        assert e.fake.args["fcn_crop_bwd_f32"] == (G["cat"].buf.ptr, G[name].buf.ptr, 2, 12, 12, 8, 8, 0, 0, 0, 12, 12, 16, off, 0, None)
        assert op.bytes == 4.0 * 2 * 12 * 12 * 8 * 2
    plan._one_bottom(by["up"])
    plan._one_bottom(by["pool"])
    assert [(op.kind, op.name) for op in plan.ops[2:]] == [("interp_bwd", "up"), ("avepool_bwd", "pool")]
    plan.ops[2].run(None)
    assert e.fake.args["fcn_interp_bwd_f32"][2:] == (2, 2, 2, 8, 8, 0, 0, 0, 12, 12, 8, 0, 0, None)
    plan.ops[3].run(None)
    assert e.fake.args["fcn_avepool_bwd_f32"][-2] == 1               # feat's gradient already holds the Concat's share


def test_a_fused_relu_below_a_copying_concat_is_masked_after_every_writer(stub):
    """feat's in-place ReLU rides in its convolution.  Its gradient is written by the Concat's hand-down and by the pooling, neither of
    which can take a mask into its epilogue: the mask stays a launch of its own, behind both."""
    text = PYRAMID_NET.replace('layer { name: "pool"', 'layer { name: "relu_feat" type: "ReLU" bottom: "feat" top: "feat" }\nlayer { name: "pool"')
    e = stub(text, "TRAIN")
    assert e._conv_layer_meta["feat"]["relu"] is True and "cat" in e.copy_concats
    G, by = e.grad_blobs, {l.name: l for l in e.spec.layers}
    plan = BW.BackwardPlanner(e)
    plan._plan_banks()
    e._ws, e._bn_chains = FakeBuffer(64), {}
    n0 = len(plan.ops)
    plan.mark(G["cat"])
    for name in ("cat", "up", "pool", "relu_feat", "feat"):
        (plan.emitters.get(by[name].type) or plan._one_bottom)(by[name])
    plan._finish_dgrads()
    assert [(op.kind, op.name) for op in plan.ops[n0:]] == [("concat_bwd", "cat:feat"), ("concat_bwd", "cat:up"), ("interp_bwd", "up"),
                                                            ("avepool_bwd", "pool"), ("relu_bwd", "feat"), ("wgrad", "feat")]
