"""InnerProduct above FCN_IP_MAX_ROWS rows as the forward and backward planners lay it out - without a GPU.

As tests/test_region_plan.py: Engine / TrainEngine / BackwardPlanner methods run on the stub engine of tests/plan_stub.py with DeviceBuffer replaced by a counter
of addresses and the library by one whose entry points return 0 (size queries: 64).  Checked: at 32 rows the plan is the streaming one
whatever the NetSpec's ip_gemm says (same op kinds, same entry points, same arguments); at 33 rows a bare NetSpec is refused by layer
name with the words that say how to opt in, and one built with ip_gemm=True plans ip_gemm / ip_gemm_bwd / wgrad ops on the
fcn_ip_gemm_* entry points with the streaming call's operands, the forward workspace per layer from the new query, bwd_data's through
e._ip_ws and the weight gradient's a buffer of its own."""
import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import models
from plan_stub import engine_factory

RELU, ACCUM, OUT_F32, NT = 1, 4, 8, 256


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False, depthwise=True)


def net(m, train=False):
    tail = ('layer { name: "label" type: "Input" top: "label" input_param { shape { dim: %d } } }\n'
            'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc2" bottom: "label" top: "loss" }\n' % m) if train else \
        'layer { name: "prob" type: "Softmax" bottom: "fc2" top: "prob" }\n'
    return ('layer { name: "data" type: "Input" top: "data" input_param { shape { dim: %d dim: 3 dim: 6 dim: 6 } } }\n'
            'layer { name: "conv" type: "Convolution" bottom: "data" top: "conv" convolution_param { num_output: 6 kernel_size: 3 stride: 2 } }\n'
            'layer { name: "relu" type: "ReLU" bottom: "conv" top: "conv" }\n'
            'layer { name: "fc1" type: "InnerProduct" bottom: "conv" top: "fc1" inner_product_param { num_output: 12 } }\n'
            'layer { name: "relu1" type: "ReLU" bottom: "fc1" top: "fc1" }\n'
            'layer { name: "fc2" type: "InnerProduct" bottom: "fc1" top: "fc2" inner_product_param { num_output: 5 bias_term: false } }\n' % m) + tail


IP_KINDS = ("inner_product", "ip_gemm")


def fwd_ops(e):
    return [op for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind in IP_KINDS]


def run(e, ops):
    del e.fake.calls[:]
    for op in ops:
        op.run(None)
    return list(e.fake.calls)


@pytest.mark.parametrize("ip_gemm", [False, True])
def test_32_rows_plan_the_streaming_kernels_whatever_the_keyword(stub, ip_gemm):
    e = stub(net(32), ip_gemm=ip_gemm)
    ops = fwd_ops(e)
    assert [(op.kind, op.name) for op in ops] == [("inner_product", "fc1"), ("inner_product", "fc2")]
    assert not [n for n, _a in e.fake.calls if "ip_gemm" in n]                       # not even the size query
    B, P = e.blobs, e.params_dev
    calls = run(e, ops)
    assert [n for n, _a in calls] == ["fcn_inner_product_fwd_f32"] * 2
    a = calls[0][1]      # conv is 2 x 2 pixels of 8 channels (6 padded to 8): K = 32
    assert a[:11] == (B["conv"].buf.ptr, 32, P["fc1"][0].ptr, P["fc1"][1].ptr, B["fc1"].buf.ptr, B["fc1"].cstride, B["fc1"].coffset, 32, 32, 12,
                      RELU | NT)
    assert calls[1][1][3] is None and calls[1][1][7:11] == (32, 12, 5, NT)


def test_33_rows_are_refused_by_layer_name_without_the_keyword(stub):
    with pytest.raises(NotImplementedError, match=r"InnerProduct fc1: a batch of 33 rows \(the streaming kernels take at most 32\).*"
                                                  r"NetSpec built with ip_gemm=True \(caffe.Net, the solvers and the caffe tool pass it\)"):
        stub(net(33))
    with pytest.raises(NotImplementedError, match="InnerProduct fc1: a batch of 33 rows"):
        stub(net(33), f16=True)


def test_33_rows_plan_the_gemm(stub):
    e = stub(net(33), ip_gemm=True)
    ops = fwd_ops(e)
    assert [(op.kind, op.name) for op in ops] == [("ip_gemm", "fc1"), ("ip_gemm", "fc2")]
    queries = [a for n, a in e.fake.calls if n == "fcn_ip_gemm_workspace_bytes"]
    assert queries == [(33, 32, 12, 4), (33, 12, 5, 4)]
    assert not [n for n, _a in e.fake.calls if n.startswith("fcn_inner_product")]
    B, P = e.blobs, e.params_dev
    # the layer's FLOPs (over its real channels) and bytes: `caffe time` lists them
    assert ops[0].flops == 2.0 * 33 * 6 * 2 * 2 * 12 and ops[0].bytes == 4.0 * (12 * 32 + 33 * 32) + 4.0 * 33 * 12
    calls = run(e, ops)
    assert [n for n, _a in calls] == ["fcn_ip_gemm_fwd_f32"] * 2
    a = calls[0][1]
    assert a[:11] == (B["conv"].buf.ptr, 32, P["fc1"][0].ptr, P["fc1"][1].ptr, B["fc1"].buf.ptr, B["fc1"].cstride, B["fc1"].coffset, 33, 32, 12,
                      RELU)                                                             # (no non-temporal flag: the GEMM has none)
    assert a[11] is not None and a[11] != calls[1][1][11]                                # a workspace per layer, allocated at plan time
    assert calls[1][1][3] is None and calls[1][1][7:11] == (33, 12, 5, 0)


def test_33_rows_in_the_half_float_engine(stub):
    e = stub(net(33), f16=True, ip_gemm=True)
    ops = fwd_ops(e)
    assert [(op.kind, op.name) for op in ops] == [("ip_gemm", "fc1"), ("ip_gemm", "fc2")]
    assert [a[3] for n, a in e.fake.calls if n == "fcn_ip_gemm_workspace_bytes"] == [2, 2]
    calls = run(e, ops)
    assert [n for n, _a in calls] == ["fcn_ip_gemm_fwd_f16"] * 2
    for (_n, a), top in zip(calls, ("fc1", "fc2")):      # the CONV_OUT_F32 rule of the streaming call: float32 where the top blob is
        assert bool(a[10] & OUT_F32) == (e.blobs[top].esize == 4)
        assert not a[10] & NT


def backward_plan(e):
    plan = BW.BackwardPlanner(e)
    plan.run()
    e._adopt_backward(plan)
    return plan


IP_BWD = ("wgrad", "inner_product_bwd", "ip_gemm_bwd")


def test_backward_plan_at_32_rows_is_the_streaming_one(stub):
    e = stub(net(32, train=True), "TRAIN", ip_gemm=True)
    plan = backward_plan(e)
    ops = [op for op in plan.ops if op.kind in IP_BWD and op.name in ("fc1", "fc2")]
    assert [(op.kind, op.name) for op in ops] == [("wgrad", "fc2"), ("inner_product_bwd", "fc2"), ("wgrad", "fc1"), ("inner_product_bwd", "fc1")]
    assert plan.ip_wgrad_ws is None and not [n for n, _a in e.fake.calls if "ip_gemm" in n]
    names = [n for n, _a in run(e, ops)]
    assert names == ["fcn_inner_product_bwd_weights_f32", "fcn_inner_product_bwd_data_f32"] * 2


def test_backward_plan_at_40_rows(stub):
    e = stub(net(40, train=True), "TRAIN", ip_gemm=True)
    plan = backward_plan(e)
    ops = [op for op in plan.ops if op.kind in IP_BWD and op.name in ("fc1", "fc2")]
    assert [(op.kind, op.name) for op in ops] == [("wgrad", "fc2"), ("ip_gemm_bwd", "fc2"), ("wgrad", "fc1"), ("ip_gemm_bwd", "fc1")]
    assert all(op.flops > 0 and op.bytes > 0 for op in ops)
    # two workspaces, both allocated by the planner: the weight gradients run on the second stream beside bwd_data
    assert plan.ip_ws is not None and plan.ip_wgrad_ws is not None and plan.ip_ws.ptr != plan.ip_wgrad_ws.ptr
    assert plan.ip_ws.nbytes == plan.ip_wgrad_ws.nbytes == 64
    B, G, P = e.blobs, e.grad_blobs, e.params_dev
    calls = run(e, ops)
    assert [n for n, _a in calls] == ["fcn_ip_gemm_bwd_weights_f32", "fcn_ip_gemm_bwd_data_f32"] * 2
    w1, d1 = calls[2][1], calls[3][1]
    gw, gb = e._grad_view("fc1", 0), e._grad_view("fc1", 1)
    assert w1 == (B["conv"].buf.ptr, 32, G["fc1"].buf.ptr, G["fc1"].cstride, G["fc1"].coffset, gw.ptr, gb.ptr, 40, 32, 12, 0, plan.ip_wgrad_ws.ptr,
                  None)
    assert d1 == (G["fc1"].buf.ptr, G["fc1"].cstride, G["fc1"].coffset, P["fc1"][0].ptr, G["conv"].buf.ptr, 32, 40, 32, 12, 0, plan.ip_ws.ptr, None)
    assert calls[0][1][6] is None                                                        # fc2 has no bias: db is NULL


def test_backward_plan_refuses_without_the_keyword(stub):
    with pytest.raises(NotImplementedError, match="InnerProduct fc1: a batch of 40 rows"):
        stub(net(40, train=True), "TRAIN")


def test_the_full_size_faster_rcnn_head_plans_the_gemm_over_all_rois(stub):
    e = stub(models.faster_rcnn_vgg16(fillers=False), ip_gemm=True)
    ops = fwd_ops(e)
    assert [(op.kind, op.name) for op in ops] == [("ip_gemm", n) for n in ("fc6", "fc7", "cls_score", "bbox_pred")]
    assert ops[0].flops == 2.0 * 300 * 25088 * 4096
    assert [a for n, a in e.fake.calls if n == "fcn_ip_gemm_workspace_bytes"][0] == (300, 25088, 4096, 4)
    with pytest.raises(NotImplementedError, match="InnerProduct fc6: a batch of 300 rows"):
        stub(models.faster_rcnn_vgg16(fillers=False))
