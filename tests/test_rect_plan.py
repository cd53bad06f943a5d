"""Rectangular Convolution as the forward and backward planners lay it out - without a GPU.

Engine / TrainEngine / BackwardPlanner methods run on the stub engine of tests/plan_stub.py (a bare NetSpec), with DeviceBuffer replaced
by a counter of addresses and the library by one whose every entry point returns 0; what is checked is the arithmetic of the descriptors
(pointers, extents, per-axis pads of the data gradient, flags), which launches share a plan, how the weight gradient is booked, that
every refusal names its layer - and that nets without a rectangular layer plan exactly as they did before the rectangular path
existed (tests/golden/rect_plan_square_tasks.json, recorded with plan_signature() below on the commit before it)."""
import json
import os

import pytest

from conftest import ROOT
from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models
from fcn_object_detector_amd.netspec import is_rectangular
from plan_stub import FakeBuffer, engine_factory

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 14 }
%s
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 6 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "a17" type: "Convolution" bottom: "c0" top: "a17" convolution_param { num_output: 8 kernel_h: 1 kernel_w: 7 pad_h: 0 pad_w: 3 FILL } }
layer { name: "ra17" type: "ReLU" bottom: "a17" top: "a17" }
layer { name: "a71" type: "Convolution" bottom: "c0" top: "a71" convolution_param { num_output: 8 kernel_h: 7 kernel_w: 1 pad_h: 3 pad_w: 0 bias_term: false FILL } }
layer { name: "sum" type: "Eltwise" bottom: "a17" bottom: "a71" top: "sum" }
layer { name: "b31" type: "Convolution" bottom: "sum" top: "b31" convolution_param { num_output: 5 kernel_h: 3 kernel_w: 1 pad_h: 2 pad_w: 0 dilation: 2 EXTRA FILL } }
%s
""".replace("FILL", FILL)
TEST_NET = (NET % ("", "")).replace("EXTRA", "stride_h: 2 stride_w: 1")
TRAIN_NET = (NET % ('input: "target" input_shape { dim: 2 dim: 5 dim: 12 dim: 14 }',
                    'layer { name: "loss" type: "EuclideanLoss" bottom: "b31" bottom: "target" top: "loss" }')).replace("EXTRA", "")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rect_plan_square_tasks.json")


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False)


def test_forward_tasks_and_the_shared_launch(stub):
    e = stub(TEST_NET)
    assert [t.layer.name for t in e.tasks if isinstance(t, E.ConvTask)] == ["c0"]          # never a ConvTask: no grouped launch, no tuner
    rt = {t.layer.name: t for t in e.tasks if isinstance(t, E.OpTask) and t.rconv is not None}
    assert sorted(rt) == ["a17", "a71", "b31"] and all(t.ops == [] for t in rt.values())
    assert "ra17" not in [t.layer.name for t in e.tasks]                    # the in-place ReLU rides in a17's epilogue
    assert e._conv_layer_meta["a17"] == dict(relu=True, sigmoid_top=None) and e._conv_layer_meta["a71"]["relu"] is False
    x = e.blobs["c0"]
    for nm, (kh, kw, ph, pw), relu in (("a17", (1, 7, 0, 3), True), ("a71", (7, 1, 3, 0), False)):
        d, y, pd = rt[nm].rconv, e.blobs[nm], e.params_dev[nm]
        assert isinstance(d, L.RConvDesc)
        assert (d.x, d.Cin, d.x_cstride, d.N, d.H, d.W) == (x.ptr, 6, 8, 2, 12, 14)
        assert (d.y, d.Cout, d.y_coffset, d.y_cstride, d.OH, d.OW) == (y.buf.ptr, 8, y.coffset, y.cstride, 12, 14)
        assert (d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.dilation) == (kh, kw, ph, pw, 1, 1, 1)
        assert d.w == pd[0].ptr and d.bias == (pd[1].ptr if len(pd) > 1 else None)      # the parameter blob where it lies: no repacking
        assert d.flags == (L.CONV_RELU if relu else 0)
        assert e.param_segs[(nm, 0)].shape == (8, kh, kw, 8)                             # [Cout][kh][kw][round4(Cin)]
    d = rt["b31"].rconv      # dilation 2: (12 + 4 - 5) // 2 + 1 rows, 14 columns
    assert (d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.dilation, d.OH, d.OW, d.Cin, d.Cout) == (3, 1, 2, 0, 2, 1, 2, 6, 14, 8, 5)
    # a17 and a71 read one blob and wait for the same launch: one level, ONE prepare and one op; b31 waits for both
    lv = dict(zip([t.layer.name for t in e.tasks], E.task_levels(e.tasks)))
    assert lv["a17"] == lv["a71"] == lv["c0"] + 1 and lv["b31"] > lv["sum"] > lv["a17"]
    del e.fake.calls[:]
    e._emit_rconvs([rt["a17"], rt["a71"]])
    assert e.fake.names().count("fcn_rconv2d_prepare") == 1 and len(e.ops) == 1
    op = e.ops[0]
    assert op.kind == "rconv" and op.name.startswith("a17+a71 [1x7,7x1 ")
    assert op.flops == 2 * (2.0 * 2 * 12 * 14 * 6 * 8 * 7)                               # 2 N OH OW Cin Cout kh kw, each
    assert op.bytes == 4.0 * (2 * (2 * 6 * 168 + 2 * 8 * 168 + 8 * 6 * 7) + 8 + 8)      # (booked as a dilated layer's: Cout floats of bias each)
    op.run(None)
    assert e.fake.names()[-1] == "fcn_rconv2d_f32"
    e._emit_rconvs([rt["b31"]])
    assert len(e.ops) == 2 and e.ops[1].flops == 2.0 * 2 * 6 * 14 * 8 * 5 * 3


def test_the_whole_forward_plan_emits_one_launch_per_shared_bottom(stub):
    e = stub(TEST_NET)
    e.tuner = None
    e._build_ops()
    assert [(op.kind, op.name.split(" ")[0]) for op in e.ops if op.kind == "rconv"] == [("rconv", "a17+a71"), ("rconv", "b31")]
    assert e.fake.names().count("fcn_rconv2d_prepare") == 2


def test_backward_plan_of_rectangular_layers(stub):
    e = stub(TRAIN_NET, "TRAIN")
    B, G = e.blobs, e.grad_blobs
    assert {"c0", "a17", "a71", "sum", "b31"} <= set(G)
    plan = BW.BackwardPlanner(e)
    plan._plan_banks()
    # the flip launch takes kh and kw separately: a17, a71 and b31 are three more segments of it (c0 has no gradient below it)
    raw = [data for dst, data in e.copies if dst == plan.flip_segs_dev.ptr][-1]
    segs = (L.FlipSeg * 3).from_buffer_copy(raw)
    assert [(s.Cout, s.kh, s.kw, s.Cin, s.Cin4, s.Cout4) for s in segs] == [(8, 1, 7, 6, 8, 8), (8, 7, 1, 6, 8, 8), (5, 3, 1, 8, 8, 8)]
    assert plan.flip_layout == {"a17": 0, "a71": 6 * 7 * 8, "b31": 2 * 6 * 7 * 8} and not plan.tbank
    by = {l.name: l for l in e.spec.layers}
    e._ws = FakeBuffer(64)
    plan.mark(G["b31"])                                                        # (what the loss layer does)
    plan._convolution(by["b31"])
    kinds = [(op.kind, op.name) for op in plan.ops if op.kind != "flip"]
    assert kinds == [("wgrad", "b31"), ("rconv_dgrad", "b31")]                 # no ReLU behind b31
    wop = plan.ops[-2]
    assert wop.layers == ["b31"] and wop.sel is None and "b31" in plan.wgrad_done
    assert wop.flops == 2.0 * 2 * 12 * 14 * 8 * 5 * 3                              # b31: 3x1, pad_h 2, dilation 2 keeps 12 x 14
    rec = plan.last_writer("sum")
    assert isinstance(rec.launch, L.RConvPlan) and rec.targets == ["sum"]
    d = rec.descs[0]
    assert (d.x, d.Cin, d.x_cstride, d.H, d.W) == (G["b31"].ptr, 5, 8, 12, 14)           # dY of b31
    assert (d.y, d.Cout, d.y_coffset, d.y_cstride, d.OH, d.OW) == (G["sum"].buf.ptr, 8, 0, 8, 12, 14)
    assert (d.w, d.kh, d.kw, d.stride_h, d.stride_w, d.dilation, d.flags) == (plan.flip_flat.ptr + 4 * 2 * 6 * 7 * 8, 3, 1, 1, 1, 2, 0)
    assert (d.pad_h, d.pad_w) == (2 * 2 - 2, 0)                                          # pad' = dil (k-1) - pad, per axis
    wop.run(None)
    assert e.fake.names()[-1] == "fcn_rconv2d_wgrad_f32"
    # a17 (fused ReLU: its mask first) and a71 both write the gradient of c0: the second one accumulates
    plan._eltwise(by["sum"])
    n0 = len(plan.ops)
    plan._convolution(by["a71"])
    plan._convolution(by["a17"])
    assert [(op.kind, op.name) for op in plan.ops[n0:]] == [("wgrad", "a71"), ("rconv_dgrad", "a71"), ("relu_bwd", "a17"), ("wgrad", "a17"),
                                                            ("rconv_dgrad", "a17")]
    first, last = plan.writers["c0"]
    assert (first.descs[0].kh, first.descs[0].kw, first.descs[0].pad_h, first.descs[0].pad_w, first.descs[0].flags) == (7, 1, 3, 0, 0)
    assert (last.descs[0].kh, last.descs[0].kw, last.descs[0].pad_h, last.descs[0].pad_w, last.descs[0].flags) == (1, 7, 0, 3, L.CONV_ACCUM)
    # c0's own ReLU mask is folded into the LAST pass that writes its gradient, as for a dense pass
    plan._convolution(by["c0"])
    del e.fake.calls[:]
    plan._finish_dgrads()
    assert e.fake.names().count("fcn_rconv2d_prepare") == 3
    dl = last.descs[0]
    assert dl.flags == L.CONV_ACCUM | L.CONV_MASK and (dl.y2, dl.y2_cstride, dl.y2_coffset) == (B["c0"].buf.ptr, B["c0"].cstride, B["c0"].coffset)
    assert first.descs[0].flags == 0 and ("relu_bwd", "c0") not in [(op.kind, op.name) for op in plan.ops]
    assert last.op.name.startswith("a17 [1x7 ")


ONE = """
input: "data" input_shape { dim: 1 dim: 4 dim: 16 dim: 16 }
%s
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "rect" type: "Convolution" bottom: "%s" top: "rect" convolution_param { num_output: 8 %s FILL } }
%s
""".replace("FILL", FILL)


def one(extra, bottom="c0", train=None):
    if train is None:
        return ONE % ("", bottom, extra, "")
    return ONE % ('input: "target" input_shape { dim: 1 dim: 8 dim: %d dim: %d }' % train, bottom, extra,
                  'layer { name: "loss" type: "EuclideanLoss" bottom: "rect" bottom: "target" top: "loss" }')


def test_refusals_name_the_layer(stub):
    with pytest.raises(NotImplementedError, match=r"f16 engine: rectangular Convolution rect \(1x3 stride 1x1 pad 0x1\)"):
        stub(one("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1"), f16=True)
    with pytest.raises(NotImplementedError, match=r"rectangular Convolution rect \(1x3 stride 1x1 pad 0x1\): group 2"):
        stub(one("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1 group: 2"))
    stub(one("kernel_h: 3 kernel_w: 3 pad_h: 1 pad_w: 1 group: 2"))            # axes that agree stay the dense grouped layer
    # TRAIN, the bottom needs a gradient: a stride above 1 on either axis and a pad above d (k-1) on its axis have no data-gradient pass
    e = stub(one("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1 stride_h: 1 stride_w: 2", train=(16, 8)), "TRAIN")
    with pytest.raises(NotImplementedError, match=r"rectangular Convolution rect: .*stride 1x2 .*bottom c0 needs a gradient"):
        BW.BackwardPlanner(e)._plan_banks()
    e = stub(one("kernel_h: 3 kernel_w: 1 pad_h: 1 pad_w: 0 stride_h: 2 stride_w: 1", train=(8, 16)), "TRAIN")
    with pytest.raises(NotImplementedError, match=r"rectangular Convolution rect: .*stride 2x1 .*bottom c0 needs a gradient"):
        BW.BackwardPlanner(e)._plan_banks()
    e = stub(one("kernel_h: 1 kernel_w: 3 pad_h: 1 pad_w: 1", train=(18, 16)), "TRAIN")
    with pytest.raises(NotImplementedError, match=r"rectangular Convolution rect: .*pad_h 1 above dilation \* \(kernel_h - 1\) = 0"):
        BW.BackwardPlanner(e)._plan_banks()
    e = stub(one("kernel_h: 3 kernel_w: 2 pad_h: 2 pad_w: 3 dilation: 2", train=(16, 20)), "TRAIN")
    with pytest.raises(NotImplementedError, match=r"rectangular Convolution rect: .*pad_w 3 above dilation \* \(kernel_w - 1\) = 2"):
        BW.BackwardPlanner(e)._plan_banks()
    # ... and all are fine where nothing below learns (the bottom is the data blob), and in a forward-only net
    for extra, hw in (("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1 stride_h: 1 stride_w: 2", (16, 8)), ("kernel_h: 1 kernel_w: 3 pad_h: 1 pad_w: 1", (18, 16))):
        e = stub(one(extra, "data", train=hw).replace("num_output: 8 kernel_size: 3 pad: 1", "num_output: 4 kernel_size: 3 pad: 1"), "TRAIN")
        BW.BackwardPlanner(e)._plan_banks()
        stub(one(extra))


# ---------------------------------------------------------------- nets without a rectangular layer plan as before
SQUARE_DILATED = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 14 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "a2" type: "Convolution" bottom: "c0" top: "a2" convolution_param { num_output: 8 kernel_size: 3 pad: 2 dilation: 2 FILL } }
layer { name: "ra2" type: "ReLU" bottom: "a2" top: "a2" }
layer { name: "g2" type: "Convolution" bottom: "c0" top: "g2" convolution_param { num_output: 8 kernel_size: 5 pad: 2 group: 2 FILL } }
layer { name: "sum" type: "Eltwise" bottom: "a2" bottom: "g2" top: "sum" }
layer { name: "p" type: "Pooling" bottom: "sum" top: "p" pooling_param { pool: MAX kernel_size: 3 stride: 2 } }
layer { name: "s2" type: "Convolution" bottom: "p" top: "s2" convolution_param { num_output: 5 kernel_size: 3 stride: 2 FILL } }
""".replace("FILL", FILL)


def square_nets():
    return {"hand": SQUARE_DILATED,
            "googlenet_detectnet": models.googlenet_detectnet_deploy(batch=1, height=96, width=128, num_classes=2),
            "resnet50": models.resnet("DEPLOY", depth=50, batch=1, num_classes=10, width_div=8, size=64),
            "deeplab_aspp": models.deeplab_aspp("DEPLOY", batch=1, num_classes=5, width_div=8, fc_div=8, size=65)}


def _fields(d):
    return None if d is None else {n: getattr(d, n) for n, _ in d._fields_}


def plan_signature(e):
    """What the forward planner decided, in task order: the kind of every task, its layer, its read / write ranges, its level, and the
    descriptor (every field, addresses of the counting allocator included) it hands to the launch."""
    out = []
    for t, lv in zip(e.tasks, E.task_levels(e.tasks, e.group_convs)):
        rec = {"task": type(t).__name__, "layer": t.layer.name, "level": lv, "reads": [list(r) for r in t.reads], "writes": [list(r) for r in t.writes]}
        if isinstance(t, E.ConvTask):
            rec.update(desc=_fields(t.desc), flops=t.flops, bytes=t.bytes)
        else:
            rec.update(ops=[[op.kind, op.name, op.flops, op.bytes] for op in t.ops], pool=_fields(t.pool_desc), rconv=_fields(t.rconv))
        out.append(rec)
    return out


def widened(rec):
    """A task record of the golden file, written when square dilated layers had a descriptor with one pad and one stride (`dconv`), as
    plan_signature() writes it now: the same fields in `rconv`, pad and stride once per axis."""
    if "dconv" not in rec:
        return rec
    rec = dict(rec)
    d = rec["rconv"] = rec.pop("dconv")
    if d is not None:
        pad, stride = d.pop("pad"), d.pop("stride")
        d.update(pad_h=pad, pad_w=pad, stride_h=stride, stride_w=stride)
    return rec


def test_nets_of_square_layers_plan_as_before(stub):
    golden = json.load(open(GOLDEN))
    for name, text in square_nets().items():
        e = stub(text)
        assert not any(is_rectangular(t.layer) for t in e.tasks if t.layer.type == "Convolution"), name
        got = json.loads(json.dumps(plan_signature(e)))
        assert len(got) == len(golden[name]), name
        for a, b in zip(got, golden[name]):
            assert a == widened(b), (name, a["layer"])
        # one launch for the dilated layers of a level that read one bottom
        groups = {(b["level"], tuple(b["reads"][0])) for b in golden[name] if b.get("dconv") is not None}
        e.tuner = None
        del e.fake.calls[:]
        e._build_ops()
        assert e.fake.names().count("fcn_rconv2d_prepare") == len(groups), name
