"""Pooling masks and the Upsample layer as the forward and backward planners lay them out - without a GPU.

As tests/test_interp_plan.py: Engine / TrainEngine / BackwardPlanner methods run on the stub engine of tests/plan_stub.py with DeviceBuffer replaced by a
counter of addresses and the library by one whose every entry point returns 0 and keeps its arguments; what is checked is which entry
point an op calls with which geometry and which argmax buffer, the bytes it books, that a masked pooling stays out of the pool + LRN
fusions, and that the mask gets neither a blob nor a gradient.  The model writers are parsed and inferred at reduced width."""
import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from plan_stub import engine_factory

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
BODY = """
input: "data" input_shape { dim: 2 dim: 3 dim: 11 dim: 14 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "pool1" type: "Pooling" bottom: "c0" top: "pool1" top: "pool1_mask" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
layer { name: "c1" type: "Convolution" bottom: "pool1" top: "c1" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "up1" type: "Upsample" bottom: "c1" bottom: "pool1_mask" top: "up1" upsample_param { upsample_h: 11 upsample_w: 14 } }
""".replace("FILL", FILL)
SCORE = 'layer { name: "score" type: "Convolution" bottom: "up1" top: "score" convolution_param { num_output: 5 kernel_size: 1 FILL } }\n'.replace("FILL", FILL)
TRAIN_NET = 'input: "target" input_shape { dim: 2 dim: 5 dim: 11 dim: 14 }\n' + BODY + SCORE + \
    'layer { name: "loss" type: "EuclideanLoss" bottom: "score" bottom: "target" top: "loss" }\n'
LRN = 'layer { name: "NAME" type: "LRN" bottom: "BOT" top: "NAME" lrn_param { local_size: 5 alpha: 0.0001 beta: 0.75 } }\n'
POOL = 'layer { name: "pool1" type: "Pooling" bottom: "BOT" top: "pool1"MASK pooling_param { pool: MAX kernel_size: 3 stride: 2 } }\n'
HEAD = 'input: "data" input_shape { dim: 2 dim: 8 dim: 13 dim: 15 }\n'
UP = 'layer { name: "up1" type: "Upsample" bottom: "BOT" bottom: "pool1_mask" top: "up1" upsample_param { upsample_h: 13 upsample_w: 15 } }\n'


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False)


def task_of(e, name):
    ts = [t for t in e.tasks if isinstance(t, E.OpTask) and t.layer.name == name]
    assert len(ts) == 1
    return ts[0]


def only_op(e, name):
    t = task_of(e, name)
    assert len(t.ops) == 1
    return t.ops[0]


def test_the_mask_is_the_argmax_buffer_not_a_blob(stub):
    e = stub(BODY + SCORE)
    assert "pool1_mask" in e.shapes and "pool1_mask" not in e.blobs and "pool1_mask" not in e.outputs
    assert e.shapes["pool1_mask"] == e.shapes["pool1"] == (2, 8, 6, 7)
    idx = e.aux_dev["pool1"]                                              # allocated in TEST too: the layer has a mask top
    assert idx.nbytes == 2 * 6 * 7 * 8 * 4
    assert e._range("pool1_mask") == (idx.ptr, 0, 8)
    pool, up = task_of(e, "pool1"), task_of(e, "up1")
    assert pool.writes == [e._range("pool1"), (idx.ptr, 0, 8)] and up.reads == [e._range("c1"), (idx.ptr, 0, 8)]
    assert E.task_waits(up, pool)
    # float32: the pooling may ride in a convolution launch, whose pooling form writes idx
    assert pool.pool_desc is not None and pool.pool_desc.idx == idx.ptr
    op = only_op(e, "pool1")
    assert op.kind == "maxpool" and op.bytes == 4.0 * 8 * (2 * 11 * 14 + 2 * 6 * 7) + 4.0 * 2 * 6 * 7 * 8
    op.run(None)
    x, y = e.blobs["c0"], e.blobs["pool1"]
    assert e.fake.args["fcn_maxpool_fwd_f32"] == (x.ptr, y.buf.ptr, idx.ptr, 2, 11, 14, 8, 8, 2, 2, 0, 6, 7, 8, 0, None)


def test_one_unpool_op_in_the_float32_engine(stub):
    e = stub(BODY + SCORE)
    x, y, idx = e.blobs["c1"], e.blobs["up1"], e.aux_dev["pool1"]
    assert y.shape == (2, 8, 11, 14)
    op = only_op(e, "up1")
    assert (op.kind, op.name, op.flops) == ("unpool", "up1", 0.0)
    assert op.bytes == (4.0 + 4.0) * 2 * 6 * 7 * 8 + 4.0 * 2 * 11 * 14 * 8          # x + idx + y
    op.run(None)
    assert e.fake.names()[-1] == "fcn_unpool_fwd_f32"
    assert e.fake.args["fcn_unpool_fwd_f32"] == (x.buf.ptr, idx.ptr, y.buf.ptr, 2, 6, 7, 8, 8, 0, 2, 2, 0, 11, 14, 8, 0, None)
    assert [t.layer.name for t in e.tasks if any(o.kind == "unpool" for o in getattr(t, "ops", []))] == ["up1"]


def test_one_unpool_op_in_the_half_engine(stub):
    e = stub(BODY + SCORE, f16=True)
    x, y, idx = e.blobs["c1"], e.blobs["up1"], e.aux_dev["pool1"]
    assert (x.esize, y.esize, e.blobs["score"].esize) == (2, 2, 4) and "pool1_mask" not in e.blobs
    assert idx.nbytes == 2 * 6 * 7 * 8 * 4                                           # the argmax stays int32
    pool = task_of(e, "pool1")
    assert pool.pool_desc is None                                                    # a masked pooling of halves has its own kernel
    pool.ops[0].run(None)
    xb, yb = e.blobs["c0"], e.blobs["pool1"]
    assert e.fake.names()[-1] == "fcn_maxpool_idx_fwd_f16"
    assert e.fake.args["fcn_maxpool_idx_fwd_f16"] == (xb.ptr, yb.buf.ptr, idx.ptr, 2, 11, 14, 8, 8, 2, 2, 0, 6, 7, 8, 0, None)
    assert pool.ops[0].bytes == 2.0 * 8 * (2 * 11 * 14 + 2 * 6 * 7) + 4.0 * 2 * 6 * 7 * 8
    op = only_op(e, "up1")
    assert op.kind == "unpool" and op.bytes == (2.0 + 4.0) * 2 * 6 * 7 * 8 + 2.0 * 2 * 11 * 14 * 8
    op.run(None)
    assert e.fake.names()[-1] == "fcn_unpool_fwd_f16"
    assert e.fake.args["fcn_unpool_fwd_f16"] == (x.buf.ptr, idx.ptr, y.buf.ptr, 2, 6, 7, 8, 8, 0, 2, 2, 0, 11, 14, 8, 0, 0, None)
    # the net's output behind the layer: halves in, float32 out
    e = stub(BODY, f16=True)
    assert (e.blobs["c1"].esize, e.blobs["up1"].esize) == (2, 4) and e.outputs == ["up1"]
    op = only_op(e, "up1")
    op.run(None)
    assert e.fake.args["fcn_unpool_fwd_f16"][-2] == 1 and op.bytes == (2.0 + 4.0) * 2 * 6 * 7 * 8 + 4.0 * 2 * 11 * 14 * 8
    # an unmasked pooling of halves is what it was
    plain = stub((BODY + SCORE).replace(' top: "pool1_mask"', "").replace('bottom: "pool1_mask" ', "").replace('"Upsample"', '"ReLU"'), f16=True)
    assert "pool1" not in plain.aux_dev
    task_of(plain, "pool1").ops[0].run(None)
    assert plain.fake.names()[-1] == "fcn_maxpool_fwd_f16"


@pytest.mark.parametrize("f16", [False, True])
def test_a_masked_pooling_stays_out_of_the_pool_lrn_fusions(stub, f16):
    tail = UP.replace("BOT", "c1") + SCORE
    conv = 'layer { name: "c1" type: "Convolution" bottom: "BOT" top: "c1" convolution_param { num_output: 8 kernel_size: 1 FILL } }\n'.replace("FILL", FILL)
    pool_lrn = HEAD + POOL.replace("BOT", "data") + LRN.replace("NAME", "norm1").replace("BOT", "pool1") + conv.replace("BOT", "norm1")
    lrn_pool = HEAD + LRN.replace("NAME", "norm1").replace("BOT", "data") + POOL.replace("BOT", "norm1") + conv.replace("BOT", "pool1")
    first = 'layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 1 FILL } }\n'.replace("FILL", FILL)
    if f16:      # (a net input stays float32: the pair must sit behind a convolution to hold halves)
        pool_lrn = pool_lrn.replace(HEAD, HEAD + first).replace('bottom: "data" top: "pool1"', 'bottom: "c0" top: "pool1"')
        lrn_pool = lrn_pool.replace(HEAD, HEAD + first).replace('bottom: "data" top: "norm1"', 'bottom: "c0" top: "norm1"')
    for text in (pool_lrn, lrn_pool):
        plain = stub(text.replace("MASK", "") + SCORE.replace('"up1"', '"c1"'), f16=f16)
        kinds = [op.kind for t in plain._fuse_pool_lrn(plain.tasks) for op in getattr(t, "ops", [])]
        assert "pool_lrn" in kinds and "maxpool" not in kinds, "the control: without a mask the pair is one launch"
        masked = stub(text.replace("MASK", ' top: "pool1_mask"') + tail, f16=f16)
        kinds = [op.kind for t in masked._fuse_pool_lrn(masked.tasks) for op in getattr(t, "ops", [])]
        assert "pool_lrn" not in kinds and "pool_lrn_conv" not in kinds and kinds.count("maxpool") == 1 and kinds.count("lrn") == 1 and "unpool" in kinds
        assert "pool1" in masked.aux_dev


def test_backward_goes_to_the_first_bottom_only(stub):
    e = stub(TRAIN_NET, "TRAIN")
    G, idx = e.grad_blobs, e.aux_dev["pool1"]
    assert {"c0", "pool1", "c1", "up1", "score"} <= set(G) and "pool1_mask" not in G and "pool1_mask" not in e.blobs
    by = {l.name: l for l in e.spec.layers}
    plan = BW.BackwardPlanner(e)
    assert "Upsample" in plan.one_bottom and "Upsample" not in plan.emitters
    plan._one_bottom(by["up1"])
    assert plan.ops == []                                                 # nothing arrived at the top yet
    plan.mark(G["up1"])
    plan._one_bottom(by["up1"])
    assert [(op.kind, op.name) for op in plan.ops] == [("unpool_bwd", "up1")] and plan.state(G["c1"]) == "full"
    op = plan.ops[0]
    assert op.bytes == 4.0 * 2 * 6 * 7 * 8 * 3                            # dY gathered + idx + dX
    op.run(None)
    assert e.fake.args["fcn_unpool_bwd_f32"] == (G["up1"].buf.ptr, idx.ptr, G["c1"].buf.ptr, 2, 6, 7, 8, 8, 0, 2, 2, 0, 11, 14, 8, 0, 0, None)
    # behind another writer of the same gradient: it adds
    plan = BW.BackwardPlanner(e)
    plan.mark(G["c1"])
    plan.mark(G["up1"])
    plan._one_bottom(by["up1"])
    plan.ops[-1].run(None)
    assert e.fake.args["fcn_unpool_bwd_f32"][-2] == 1 and plan.ops[-1].bytes == 4.0 * 2 * 6 * 7 * 8 * 4
    # the masked pooling's own backward is what every MAX pooling's is, by the same buffer
    plan = BW.BackwardPlanner(e)
    plan.mark(G["pool1"])
    plan._one_bottom(by["pool1"])
    assert [(op.kind, op.name) for op in plan.ops] == [("maxpool_bwd", "pool1")]
    plan.ops[0].run(None)
    assert e.fake.args["fcn_maxpool_bwd_mask_f32"][1] == idx.ptr


def test_the_mask_does_not_pull_the_backward_pass(stub):
    """A frozen encoder: nothing below the pooling learns, so neither of its tops needs a gradient - and the mask bottom of the Upsample
    does not make one flow (Caffe: the layer propagates to bottom 0 only)."""
    frozen = TRAIN_NET.replace('name: "c0" type: "Convolution" bottom: "data" top: "c0"',
                               'name: "c0" type: "Convolution" bottom: "data" top: "c0" param { lr_mult: 0 } param { lr_mult: 0 }')
    e = stub(frozen, "TRAIN")
    assert "pool1" not in e.need_grad and "pool1_mask" not in e.need_grad and {"c1", "up1", "score"} <= e.need_grad
    only = frozen.replace('bottom: "c1" bottom: "pool1_mask"', 'bottom: "pool1" bottom: "pool1_mask"')
    e = stub(only, "TRAIN")
    assert "up1" not in e.need_grad and "score" in e.need_grad


@pytest.mark.parametrize("phase", ["DEPLOY", "TRAIN", "TEST"])
def test_the_writers_parse_and_infer(phase):
    net_phase = "TRAIN" if phase == "TRAIN" else "TEST"
    spec = NetSpec(proto.parse_text(models.segnet_basic(phase, classes=5, batch=2, size=(32, 48), width_div=8)), net_phase)
    shapes = spec.infer()
    assert list(spec.mask_blobs) == ["pool%d_mask" % i for i in (1, 2, 3, 4)]
    assert shapes["pool4"] == shapes["pool4_mask"] == (2, 8, 2, 3) and shapes["upsample1"] == (2, 8, 32, 48) and shapes["conv_classifier"] == (2, 5, 32, 48)
    assert sum(l.type == "Upsample" for l in spec.layers) == 4 and sum(l.type == "Convolution" for l in spec.layers) == 9
    assert spec.param_shapes["conv1"][0] == (8, 3, 7, 7) and spec.param_shapes["conv_decode4"][0] == (8, 8, 7, 7)
    assert spec.output_blobs() == {"DEPLOY": ["prob"], "TRAIN": ["loss"], "TEST": ["accuracy", "loss"]}[phase]
    spec = NetSpec(proto.parse_text(models.segnet(phase, classes=5, batch=1, size=64, width_div=8)), net_phase)
    shapes = spec.infer()
    assert list(spec.mask_blobs) == ["pool%d_mask" % i for i in (1, 2, 3, 4, 5)]
    assert sum(l.type == "Convolution" for l in spec.layers) == 26 and sum(l.type == "Upsample" for l in spec.layers) == 5
    assert shapes["pool5"] == (1, 64, 2, 2) and shapes["upsample5"] == (1, 64, 4, 4) and shapes["conv4_1_D"] == (1, 32, 8, 8)
    assert shapes["conv1_2_D"] == (1, 8, 64, 64) and shapes["conv1_1_D"] == (1, 5, 64, 64)
    names = [l.name for l in spec.layers]
    assert names.index("pool5") < names.index("upsample5") < names.index("conv5_3_D") < names.index("conv5_1_D") < names.index("upsample4")
    assert "conv1_1_D_bn" not in names and "relu1_2_D" in names and "conv1_1_bn" in names and "conv1_1_scale" in names


def test_the_writers_at_odd_sizes_carry_the_extents():
    text = models.segnet_basic("DEPLOY", classes=5, batch=1, size=(45, 31), width_div=8)
    assert "upsample_h: 45 upsample_w: 31" in text and "upsample_h: 23 upsample_w: 16" in text and text.count("upsample_h") == 2
    assert text.count("scale: 2") == 2                                    # 12 x 8 and 6 x 4, the even planes
    shapes = NetSpec(proto.parse_text(text), "TEST").infer()
    assert shapes["pool4"] == (1, 8, 3, 2) and shapes["upsample4"] == (1, 8, 6, 4) and shapes["prob"] == (1, 5, 45, 31)
    assert "scale: 2" in models.segnet("DEPLOY", size=64, width_div=8) and "upsample_h" not in models.segnet("DEPLOY", size=64, width_div=8)
    with pytest.raises(ValueError, match="phase must be"):
        models.segnet_basic("VAL")
