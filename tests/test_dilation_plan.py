"""Dilated Convolution as the forward and backward planners lay it out - without a GPU.

As tests/test_grouped_conv_plan.py: Engine / TrainEngine / BackwardPlanner methods run on the stub engine of tests/plan_stub.py with DeviceBuffer replaced by
a counter of addresses and the library by one whose every entry point returns 0; what is checked is the arithmetic of the
descriptors (pointers, extents, pad' = dil (k-1) - pad, flags), which launches share a plan, how the weight gradient is booked, and
that every refusal names its layer."""
import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from plan_stub import FakeBuffer, engine_factory

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 14 }
%s
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 6 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "a2" type: "Convolution" bottom: "c0" top: "a2" convolution_param { num_output: 8 kernel_size: 3 pad: 2 dilation: 2 FILL } }
layer { name: "ra2" type: "ReLU" bottom: "a2" top: "a2" }
layer { name: "a4" type: "Convolution" bottom: "c0" top: "a4" convolution_param { num_output: 8 kernel_size: 3 pad: 4 dilation: 4 bias_term: false FILL } }
layer { name: "sum" type: "Eltwise" bottom: "a2" bottom: "a4" top: "sum" }
layer { name: "b3" type: "Convolution" bottom: "sum" top: "b3" convolution_param { num_output: 5 kernel_size: 3 pad: 1 dilation: 3 EXTRA FILL } }
%s
""".replace("FILL", FILL)
TEST_NET = (NET % ("", "")).replace("EXTRA", "stride: 2")
TRAIN_NET = (NET % ('input: "target" input_shape { dim: 2 dim: 5 dim: 8 dim: 10 }',
                    'layer { name: "loss" type: "EuclideanLoss" bottom: "b3" bottom: "target" top: "loss" }')).replace("EXTRA", "")


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False)


def test_forward_tasks_and_the_shared_launch(stub):
    e = stub(TEST_NET)
    assert [t.layer.name for t in e.tasks if isinstance(t, E.ConvTask)] == ["c0"]
    dt = {t.layer.name: t for t in e.tasks if isinstance(t, E.OpTask) and t.rconv is not None}
    assert sorted(dt) == ["a2", "a4", "b3"] and all(t.ops == [] for t in dt.values())
    assert "ra2" not in [t.layer.name for t in e.tasks]                     # the in-place ReLU rides in a2's epilogue
    assert e._conv_layer_meta["a2"] == dict(relu=True, sigmoid_top=None) and e._conv_layer_meta["a4"]["relu"] is False
    x = e.blobs["c0"]
    for nm, dil, relu in (("a2", 2, True), ("a4", 4, False)):
        d, y, pd = dt[nm].rconv, e.blobs[nm], e.params_dev[nm]
        assert (d.x, d.Cin, d.x_cstride, d.N, d.H, d.W) == (x.ptr, 6, 8, 2, 12, 14)
        assert (d.y, d.Cout, d.y_coffset, d.y_cstride, d.OH, d.OW) == (y.buf.ptr, 8, y.coffset, y.cstride, 12, 14)
        assert (d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.dilation) == (3, 3, dil, dil, 1, 1, dil)
        assert d.w == pd[0].ptr and d.bias == (pd[1].ptr if len(pd) > 1 else None)      # the parameter blob where it lies: no repacking
        assert d.flags == (L.CONV_RELU if relu else 0)
        assert e.param_segs[(nm, 0)].shape == (8, 3, 3, 8)                               # [Cout][kh][kw][round4(Cin)]
    d = dt["b3"].rconv
    assert (d.stride_h, d.stride_w, d.dilation, d.pad_h, d.pad_w, d.OH, d.OW, d.Cin, d.Cout) == (2, 2, 3, 1, 1, 4, 5, 8, 5)      # (12 + 2 - 7) // 2 + 1, (14 + 2 - 7) // 2 + 1
    # a2 and a4 read one blob and wait for the same launch: one level, ONE prepare and one op; b3 waits for both
    lv = dict(zip([t.layer.name for t in e.tasks], E.task_levels(e.tasks)))
    assert lv["a2"] == lv["a4"] == lv["c0"] + 1 and lv["b3"] > lv["sum"] > lv["a2"]
    del e.fake.calls[:]
    e._emit_rconvs([dt["a2"], dt["a4"]])
    assert e.fake.names().count("fcn_rconv2d_prepare") == 1 and len(e.ops) == 1
    op = e.ops[0]
    assert op.kind == "dconv" and op.name.startswith("a2+a4 [d2,4 ")
    assert op.flops == 2 * (2.0 * 2 * 12 * 14 * 6 * 8 * 9)                               # 2 N OH OW Cin Cout k k, each
    assert op.bytes == 4.0 * (2 * (2 * 6 * 168 + 2 * 8 * 168 + 8 * 6 * 9) + 8 + 8)
    op.run(None)
    assert e.fake.names()[-1] == "fcn_rconv2d_f32"
    e._emit_rconvs([dt["b3"]])
    assert len(e.ops) == 2 and e.ops[1].flops == 2.0 * 2 * 4 * 5 * 8 * 5 * 9


def test_backward_plan_of_dilated_layers(stub):
    e = stub(TRAIN_NET, "TRAIN")
    B, G = e.blobs, e.grad_blobs
    assert {"c0", "a2", "a4", "sum", "b3"} <= set(G)
    plan = BW.BackwardPlanner(e)
    plan._plan_banks()
    # the flip does not depend on the dilation: a2, a4 and b3 are three ordinary segments of the one flip launch (c0 has no gradient below it)
    raw = [data for dst, data in e.copies if dst == plan.flip_segs_dev.ptr][-1]
    segs = (L.FlipSeg * 3).from_buffer_copy(raw)
    assert [(s.Cout, s.kh, s.Cin, s.Cin4, s.Cout4) for s in segs] == [(8, 3, 6, 8, 8), (8, 3, 6, 8, 8), (5, 3, 8, 8, 8)]
    assert plan.flip_layout == {"a2": 0, "a4": 6 * 9 * 8, "b3": 2 * 6 * 9 * 8} and not plan.tbank
    by = {l.name: l for l in e.spec.layers}
    e._ws = FakeBuffer(64)
    plan.mark(G["b3"])                                                         # (what the loss layer does)
    plan._convolution(by["b3"])
    kinds = [(op.kind, op.name) for op in plan.ops if op.kind != "flip"]
    assert kinds == [("wgrad", "b3"), ("dconv_dgrad", "b3")]                   # no ReLU behind b3
    wop = plan.ops[-2]
    assert wop.layers == ["b3"] and wop.sel is None and "b3" in plan.wgrad_done
    assert wop.flops == 2.0 * 2 * 8 * 10 * 8 * 5 * 9                               # b3: pad 1, dilation 3 on 12 x 14 gives 8 x 10
    rec = plan.last_writer("sum")
    assert isinstance(rec.launch, L.RConvPlan) and rec.targets == ["sum"]
    d = rec.descs[0]
    assert (d.x, d.Cin, d.x_cstride, d.H, d.W) == (G["b3"].ptr, 5, 8, 8, 10)             # dY of b3
    assert (d.y, d.Cout, d.y_coffset, d.y_cstride, d.OH, d.OW) == (G["sum"].buf.ptr, 8, 0, 8, 12, 14)
    assert (d.w, d.kh, d.kw, d.stride_h, d.stride_w, d.dilation, d.pad_h, d.pad_w, d.flags) == \
        (plan.flip_flat.ptr + 4 * 2 * 6 * 9 * 8, 3, 3, 1, 1, 3, 3 * 2 - 1, 3 * 2 - 1, 0)      # pad' = dil (k-1) - pad
    wop.run(None)
    assert e.fake.names()[-1] == "fcn_rconv2d_wgrad_f32"
    # a2 (fused ReLU: its mask first) and a4 both write the gradient of c0: the second one accumulates
    plan._eltwise(by["sum"])
    n0 = len(plan.ops)
    plan._convolution(by["a4"])
    plan._convolution(by["a2"])
    assert [(op.kind, op.name) for op in plan.ops[n0:]] == [("wgrad", "a4"), ("dconv_dgrad", "a4"), ("relu_bwd", "a2"), ("wgrad", "a2"),
                                                            ("dconv_dgrad", "a2")]
    first, last = plan.writers["c0"]
    assert (first.descs[0].dilation, first.descs[0].pad_h, first.descs[0].pad_w, first.descs[0].flags) == (4, 4, 4, 0)
    assert (last.descs[0].dilation, last.descs[0].pad_h, last.descs[0].pad_w, last.descs[0].flags) == (2, 2, 2, L.CONV_ACCUM)
    # c0's own ReLU mask is folded into the LAST pass that writes its gradient, as for a dense pass
    plan._convolution(by["c0"])
    del e.fake.calls[:]
    plan._finish_dgrads()
    assert e.fake.names().count("fcn_rconv2d_prepare") == 3
    dl = last.descs[0]
    assert dl.flags == L.CONV_ACCUM | L.CONV_MASK and (dl.y2, dl.y2_cstride, dl.y2_coffset) == (B["c0"].buf.ptr, B["c0"].cstride, B["c0"].coffset)
    assert first.descs[0].flags == 0 and ("relu_bwd", "c0") not in [(op.kind, op.name) for op in plan.ops]
    assert last.op.name.startswith("a2 [d2 ")


ONE = """
input: "data" input_shape { dim: 1 dim: 4 dim: 16 dim: 16 }
%s
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "atrous" type: "Convolution" bottom: "%s" top: "atrous" convolution_param { num_output: 8 kernel_size: 3 %s FILL } }
%s
""".replace("FILL", FILL)


def one(extra, bottom="c0", train=None):
    if train is None:
        return ONE % ("", bottom, extra, "")
    return ONE % ('input: "target" input_shape { dim: 1 dim: 8 dim: %d dim: %d }' % train, bottom, extra,
                  'layer { name: "loss" type: "EuclideanLoss" bottom: "atrous" bottom: "target" top: "loss" }')


def test_refusals_name_the_layer(stub):
    with pytest.raises(NotImplementedError, match=r"f16 engine: Convolution atrous with dilation 2"):
        stub(one("dilation: 2 pad: 2"), f16=True)
    with pytest.raises(NotImplementedError, match=r"Convolution atrous: group 2 together with dilation 2"):
        stub(one("dilation: 2 pad: 2 group: 2"))
    stub(one("dilation: 1 pad: 1 group: 2"))                                   # dilation 1 stays the dense grouped layer
    # TRAIN, the bottom needs a gradient: stride > 1 and pad > dil (k-1) have no data-gradient pass
    e = stub(one("dilation: 2 pad: 2 stride: 2", train=(8, 8)), "TRAIN")
    with pytest.raises(NotImplementedError, match=r"dilated Convolution atrous: .*stride 2 .*bottom c0 needs a gradient"):
        BW.BackwardPlanner(e)._plan_banks()
    e = stub(one("dilation: 2 pad: 5", train=(22, 22)), "TRAIN")
    with pytest.raises(NotImplementedError, match=r"dilated Convolution atrous: .*pad 5 above dilation \* \(kernel - 1\) = 4"):
        BW.BackwardPlanner(e)._plan_banks()
    # ... and both are fine where nothing below learns (the bottom is the data blob), and in a forward-only net
    for extra, hw in (("dilation: 2 pad: 2 stride: 2", (8, 8)), ("dilation: 2 pad: 5", (22, 22))):
        e = stub(one(extra, "data", train=hw).replace("num_output: 8 kernel_size: 3 pad: 1", "num_output: 4 kernel_size: 3 pad: 1"), "TRAIN")
        BW.BackwardPlanner(e)._plan_banks()
        stub(one(extra))
