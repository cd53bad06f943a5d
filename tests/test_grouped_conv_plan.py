"""Grouped Convolution as the planners lay it out, and the text of the CaffeNet / GOTURN / BVLC GoogLeNet writers - without a GPU.

The planner cases run Engine / TrainEngine / BackwardPlanner methods on the stub engine of tests/plan_stub.py with
DeviceBuffer replaced by a counter of addresses and the library by one whose every entry point returns 0: what is checked is pure
arithmetic - the g descriptors of a grouped layer (pointers, offsets, extents), its g flip segments, its g weight-gradient items -
against the layout rule written out by hand below (storage.conv_groups: group i's bank is rows i*Cout/g .. of [Cout][kh][kw][Cin/g])."""
import hashlib

import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd import storage as S
from fcn_object_detector_amd.netspec import NetSpec
from plan_stub import engine_factory

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 12 }
%s
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 16 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "g2" type: "Convolution" bottom: "c0" top: "g2" convolution_param { num_output: 32 group: 2 kernel_size: 3 pad: 1 FILL } }
layer { name: "r2" type: "ReLU" bottom: "g2" top: "g2" }
layer { name: "gs" type: "Convolution" bottom: "g2" top: "gs" convolution_param { num_output: 32 group: 4 kernel_size: 3 stride: 2 pad: 1 FILL } }
%s
""".replace("FILL", FILL)
TEST_NET = NET % ("", "")
TRAIN_NET = NET % ('input: "target" input_shape { dim: 2 dim: 32 dim: 6 dim: 6 }',
                   'layer { name: "loss" type: "EuclideanLoss" bottom: "gs" bottom: "target" top: "loss" }')


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False)


@pytest.mark.parametrize("f16", [False, True])
def test_forward_descriptors_of_a_grouped_layer(stub, f16):
    e = stub(TEST_NET, f16=f16)
    es = 2 if f16 else 4
    assert e.blobs["c0"].esize == es and e.blobs["g2"].esize == es
    tasks = [t for t in e.tasks if isinstance(t, E.ConvTask)]
    assert [t.layer.name for t in tasks] == ["c0", "g2", "g2", "gs", "gs", "gs", "gs"]
    x, y, (w, b) = e.blobs["c0"], e.blobs["g2"], e.params_dev["g2"]
    assert e.param_segs[("g2", 0)].shape == (32, 3, 3, 8) and e.param_segs[("g2", 0)].esize == es
    dense = 2.0 * 2 * 32 * 12 * 12 * 16 * 9
    for i, t in enumerate(tasks[1:3]):
        d = t.desc
        assert (d.x, d.Cin, d.x_cstride) == (x.buf.ptr + es * 8 * i, 8, 16)
        assert (d.y, d.Cout, d.y_coffset, d.y_cstride) == (y.buf.ptr, 16, 16 * i, 32)
        assert (d.w, d.bias) == (w.ptr + es * i * 16 * 3 * 3 * 8, b.ptr + 4 * 16 * i)
        assert (d.N, d.H, d.W, d.OH, d.OW, d.kh, d.kw, d.pad, d.stride) == (2, 12, 12, 12, 12, 3, 3, 1, 1)
        assert d.flags & L.CONV_RELU and bool(d.flags & L.CONV_F16) == f16
        assert t.reads == [(x.buf.ptr, 8 * i, 8 * i + 8)] and t.writes == [(y.buf.ptr, 16 * i, 16 * i + 16)]
        assert t.flops == dense / 4      # two groups, each a quarter of the dense layer: together 1/g of it
        assert t.bytes == 4.0 * (2 * 8 * 144 + 2 * 16 * 144 + 16 * 8 * 9 + 16)
    # the two groups are independent of each other and share one level: one grouped launch carries both
    levels = E.task_levels(e.tasks)
    assert levels[e.tasks.index(tasks[1])] == levels[e.tasks.index(tasks[2])] == levels[e.tasks.index(tasks[0])] + 1
    ys, (ws, bs) = e.blobs["gs"], e.params_dev["gs"]
    for i, t in enumerate(tasks[3:]):
        d = t.desc
        assert (d.x, d.Cin, d.Cout, d.y_coffset, d.stride, d.OH) == (y.buf.ptr + es * 8 * i, 8, 8, 8 * i, 2, 6)
        assert (d.w, d.bias, d.y) == (ws.ptr + es * i * 8 * 9 * 8, bs.ptr + 4 * 8 * i, ys.buf.ptr)


def test_backward_banks_descriptors_and_weight_gradient_items(stub):
    e = stub(TRAIN_NET, "TRAIN")
    assert set(e.grad_blobs) == {"c0", "g2", "gs"}
    plan = BW.BackwardPlanner(e)
    plan._plan_banks()
    g2, gs = [next(l for l in e.spec.layers if l.name == n) for n in ("g2", "gs")]
    # one flip segment per group of the stride-1 layer (c0 has no gradient below it, gs is strided: one tap-major bank per group)
    raw = [data for dst, data in e.copies if dst == plan.flip_segs_dev.ptr][-1]
    segs = (L.FlipSeg * 2).from_buffer_copy(raw)
    w_off = (e.params_dev["g2"][0].ptr - e.param_flat.ptr) // 4
    for i, s in enumerate(segs):
        assert (s.w_offset, s.wt_offset) == (w_off + i * 16 * 9 * 8, i * 8 * 9 * 16)
        assert (s.Cout, s.kh, s.kw, s.Cin, s.Cin4, s.Cout4) == (16, 3, 3, 8, 8, 16)
    assert plan.flip_flat.nbytes == 4 * 2 * 8 * 9 * 16 and sorted(plan.tbank) == ["gs", "gs#1", "gs#2", "gs#3"]
    B, G = e.blobs, e.grad_blobs
    for i in range(2):
        d, flops = plan.dgrad_desc(g2, G["g2"], G["c0"], False, i)
        assert (d.x, d.Cin, d.x_cstride) == (G["g2"].buf.ptr + 4 * 16 * i, 16, 32)      # the group's 16 channels of dY ...
        assert (d.y, d.Cout, d.y_coffset, d.y_cstride) == (G["c0"].buf.ptr, 8, 8 * i, 16)      # ... make its 8 channels of dX
        assert (d.w, d.pad, d.stride, d.kh) == (plan.flip_flat.ptr + 4 * i * 8 * 9 * 16, 1, 1, 3) and d.flags == 0
        assert flops == 2.0 * 2 * 32 * 144 * 16 * 9 / 4
    assert plan.dgrad_desc(g2, G["g2"], G["c0"], True, 1)[0].flags == L.CONV_ACCUM
    items = plan.wgrad_items(g2, G["g2"])
    assert len(items) == 2
    dw0, db0 = e._grad_view("g2", 0), e._grad_view("g2", 1)
    for i, (d, dw, db, flops) in enumerate(items):
        assert (d.x, d.Cin, d.x_cstride) == (B["c0"].ptr + 4 * 8 * i, 8, 16)
        assert (d.y, d.Cout, d.y_coffset, d.y_cstride) == (G["g2"].buf.ptr, 16, 16 * i, 32)
        assert (dw.ptr, dw.nbytes, db.ptr, db.nbytes) == (dw0.ptr + 4 * i * 16 * 9 * 8, 4 * 16 * 9 * 8, db0.ptr + 4 * 16 * i, 4 * 16)
    # the strided layer: group i reads its 8 channels of dY through its own bank and writes its 8 channels of dX
    for i in range(4):
        rec = plan.emit_tdgrad(gs, G["gs"], G["g2"], False, i)
        d = rec.descs[0]
        assert (d.a, d.Ca, d.a_cstride, d.w) == (G["gs"].buf.ptr + 4 * 8 * i, 8, 32, plan.tbank["gs" if i == 0 else "gs#%d" % i].ptr)
        assert (d.b, d.Cb, d.b_coffset, d.b_cstride, d.stride, d.OH) == (G["g2"].buf.ptr, 8, 8 * i, 32, 2, 12)


def test_group_two_weight_gradients_share_one_grouped_launch(stub):
    e = stub(TRAIN_NET, "TRAIN")
    plan = BW.BackwardPlanner(e)
    plan._plan_banks()
    n0 = len(plan.ops)
    gs = next(l for l in e.spec.layers if l.name == "gs")
    plan.emit_wgrads([gs], [e.grad_blobs["gs"]])
    ops = plan.ops[n0:]
    assert [(op.kind, op.name, op.layers) for op in ops] == [("wgrad", "gs", ["gs"])] and "gs" in plan.wgrad_done      # four items, one launch
    assert ops[0].flops == 2.0 * 2 * 32 * 36 * 32 * 9 / 4


BAD = """
input: "data" input_shape { dim: 1 dim: %d dim: 8 dim: 8 }
layer { name: "g" type: "Convolution" bottom: "data" top: "g" convolution_param { num_output: %d group: %d kernel_size: 3 } }
"""


@pytest.mark.parametrize("cin,cout,group,f16,message", [
    (6, 8, 2, False, "grouped Convolution g: group 2 leaves 3 input and 4 output channels per group, not whole 16-byte segments \\(4 floats\\)"),
    (8, 8, 8, False, "grouped Convolution g: group 8 leaves 1 input and 1 output channels per group.*depthwise convolution has no kernel here"),
    (8, 6, 2, False, "grouped Convolution g: group 2 leaves 4 input and 3 output channels"),
])
def test_refusals_name_the_layer(cin, cout, group, f16, message):
    spec = NetSpec(proto.parse_text(BAD % (cin, cout, group)), "TEST")
    shapes = spec.infer()
    plan = S.plan_blobs(spec, shapes, spec.data_tops(), ["g"], f16, True, True)
    with pytest.raises(NotImplementedError, match=message):
        S.param_layout(spec, plan.views, f16)


def test_half_float_groups_need_eight_channels():
    """16 -> 24 channels in two groups: 8 in / 12 out per group are whole segments of floats, but 12 halves are a segment and a half."""
    text = NET.split('layer { name: "gs"')[0].replace("num_output: 32 group: 2", "num_output: 24 group: 2") % ""
    spec = NetSpec(proto.parse_text(text), "TEST")
    shapes = spec.infer()
    for f16 in (False, True):
        plan = S.plan_blobs(spec, shapes, spec.data_tops(), [], f16, True, True)      # (g2 taken as an interior blob: halves in the f16 engine)
        if f16:
            with pytest.raises(NotImplementedError, match="grouped Convolution g2: group 2 leaves 8 input and 12 output channels.*8 halves"):
                S.param_layout(spec, plan.views, f16)
        else:
            assert [s.shape for s in S.param_layout(spec, plan.views, f16)[0] if s.layer == "g2"] == [(24, 3, 3, 8), (24,)]


# ---------------------------------------------------------------------- the writers
def _spec(text, phase):
    spec = NetSpec(proto.parse_text(text), phase)
    spec.infer()
    return spec


def test_caffenet_text():
    for phase, tail in (("TRAIN", ["loss"]), ("TEST", ["accuracy", "loss"]), ("DEPLOY", ["prob"])):
        spec = _spec(models.caffenet(phase, batch=10), "TRAIN" if phase == "TRAIN" else "TEST")
        bs, ps = spec.blob_shapes, spec.param_shapes
        assert bs["conv1"] == (10, 96, 55, 55) and bs["pool5"] == (10, 256, 6, 6) and bs["fc8"] == (10, 1000)
        assert ps["conv2"][0] == (256, 48, 5, 5) and ps["conv3"][0] == (384, 256, 3, 3) and ps["conv4"][0] == (384, 192, 3, 3)
        assert ps["conv5"][0] == (256, 192, 3, 3) and ps["fc6"][0] == (4096, 9216) and ps["fc7"][0] == (4096, 4096)
        assert [l.name for l in spec.layers][-len(tail):] == tail
        assert [l.name for l in spec.layers if l.type == "Dropout"] == ["drop6", "drop7"]
        assert (bs.get("label") == (10,)) == (phase != "DEPLOY")
    assert "_filler" not in models.caffenet("TRAIN", fillers=False) and "gaussian" in models.caffenet("TRAIN")
    small = _spec(models.caffenet("TRAIN", batch=2, num_classes=10, width_div=2, fc_div=32, size=99), "TRAIN")
    assert small.param_shapes["conv2"][0] == (128, 24, 5, 5) and small.param_shapes["fc6"][0] == (128, 512)


def test_goturn_text():
    spec = _spec(models.goturn_tracker("TRAIN", batch=1), "TRAIN")
    bs, ps = spec.blob_shapes, spec.param_shapes
    assert bs["pool5"] == bs["pool5_p"] == (1, 256, 6, 6) and bs["pool5_concat"] == (1, 512, 6, 6)
    assert ps["fc6-new"][0] == (4096, 18432) and ps["fc7-newb"][0] == (4096, 4096) and bs["fc8-shapes"] == (1, 4) and bs["bbox"] == (1, 4)
    towers = [l for l in spec.param_layers() if l.type == "Convolution"]
    assert [l.name for l in towers] == ["conv1", "conv2", "conv3", "conv4", "conv5"] + ["conv%d_p" % i for i in range(1, 6)]
    assert all(list(l.lr_mult) == [0.0, 0.0] for l in towers)
    assert all(list(l.lr_mult) == [1.0, 2.0] for l in spec.param_layers() if l.type == "InnerProduct")
    assert spec.layers[-1].type == "L1Loss" and spec.layers[-1].bottoms == ["fc8-shapes", "bbox"]
    assert _spec(models.goturn_tracker("DEPLOY"), "TEST").output_blobs() == ["fc8-shapes"]


def test_bvlc_googlenet_text():
    spec = _spec(models.bvlc_googlenet("TRAIN", batch=2), "TRAIN")
    bs, ps = spec.blob_shapes, spec.param_shapes
    assert bs["inception_4a/output"] == (2, 512, 14, 14) and bs["loss1/ave_pool"] == (2, 512, 4, 4) and bs["loss2/ave_pool"] == (2, 528, 4, 4)
    assert bs["pool4/3x3_s2"] == (2, 832, 7, 7) and bs["pool5/7x7_s1"] == (2, 1024, 1, 1) and bs["loss3/classifier"] == (2, 1000)
    assert ps["loss1/conv"][0] == (128, 512, 1, 1) and ps["loss1/fc"][0] == (1024, 2048) and ps["loss2/classifier"][0] == (1000, 1024)
    losses = [(l.name, list(l.loss_weight)) for l in spec.layers if l.type == "SoftmaxWithLoss"]
    assert losses == [("loss1/loss", [0.3]), ("loss2/loss", [0.3]), ("loss3/loss3", [1.0])]
    drops = {l.name: float(l.sub("dropout_param").get("dropout_ratio")) for l in spec.layers if l.type == "Dropout"}
    assert drops == {"loss1/drop_fc": 0.7, "loss2/drop_fc": 0.7, "pool5/drop_7x7_s1": 0.4}
    assert not any(l.type == "Power" for l in spec.layers)
    test = _spec(models.bvlc_googlenet("TEST", batch=2), "TEST")
    assert not any(l.name.startswith(("loss1/", "loss2/")) for l in test.layers)
    assert [(l.name, int(l.sub("accuracy_param").get("top_k", 1))) for l in test.layers if l.type == "Accuracy"] == [("loss3/top-1", 1), ("loss3/top-5", 5)]
    noaux = _spec(models.bvlc_googlenet("TRAIN", batch=2, aux=False), "TRAIN")
    assert [l.name for l in noaux.layers if l.type == "SoftmaxWithLoss"] == ["loss3/loss3"]
    # the body is the detector's: the same layers to inception_5b, plus pool4, minus the input shift and its Dropout
    det = _spec(models.googlenet_detectnet_deploy(2, 224, 224), "TEST")
    mine = [l.name for l in spec.layers if not l.name.startswith(("loss", "pool5/", "data", "label"))]
    assert [n for n in mine if n != "pool4/3x3_s2"] == [l.name for l in det.layers if l.name.split("/")[0] not in ("deploy_transform", "pool5", "cvg", "coverage", "bbox")]


# the text the existing builders emit, recorded from the parent commit (sha256, first 16 hex digits)
OLD_BUILDERS = {
    "googlenet_detectnet_deploy": (lambda: models.googlenet_detectnet_deploy(), "a2c34ab12e85b662"),
    "googlenet_detectnet_deploy_b2": (lambda: models.googlenet_detectnet_deploy(2, 224, 320, 3), "53b527b721f74da3"),
    "googlenet_detectnet_train": (lambda: models.googlenet_detectnet_train("mod", "Layer", "'a': 1", 2), "1fe3274c33a1b501"),
    "googlenet_detectnet_train_lmdb": (lambda: models.googlenet_detectnet_train_lmdb(), "8b0579915b4cc221"),
    "vgg16_fcn_bbox_deploy": (lambda: models.vgg16_fcn_bbox_deploy(), "8cdf1b51587fec8e"),
    "vgg16_bounding_box_deploy": (lambda: models.vgg16_bounding_box_deploy(), "ccbde518d7449e56"),
    "voc_fcn8s": (lambda: models.voc_fcn8s("TRAIN", fillers=True), "00c2e3610968150c"),
}


@pytest.mark.parametrize("name", sorted(OLD_BUILDERS))
def test_existing_builders_emit_the_same_text(name):
    fn, digest = OLD_BUILDERS[name]
    assert hashlib.sha256(fn().encode()).hexdigest()[:16] == digest
