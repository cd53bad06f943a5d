"""The region stage as the forward planner lays it out - without a GPU.

As tests/test_ssd_plan.py: Engine methods run on the stub engine of tests/plan_stub.py with DeviceBuffer replaced by a counter of addresses and the library by one
whose entry points return 0 (size queries: 64).  Checked: one op per layer of the region stage and none for the two Reshape layers of the
RPN softmax chain, the arguments of each launch, that the chain's middle blobs own nothing, the order of the ops, the blobs on the ROI
axis, and the refusals that the planner makes (the half-float engine, a TRAIN net, other Reshape forms, a chain with another reader)."""

import numpy as np
import pytest

import ref_region64 as R
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models
from plan_stub import engine_factory


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False, depthwise=True)


KINDS = ("pair_softmax", "proposal", "roi_pool", "psroi_pool")


def region_ops(e):
    return [(op.kind, op.name) for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind in KINDS]


def run_region_ops(e):
    for t in e.tasks:
        if isinstance(t, E.OpTask):
            for op in t.ops:
                if op.kind in KINDS:
                    op.run(None)
    return {n: a for n, a in e.fake.calls}


def small_rfcn(**kw):
    return models.rfcn_resnet(depth=50, width_div=8, size=96, classes=5, pre_nms_topn=60, post_nms_topn=12, scales=(1, 2, 4), **kw)


def test_rfcn_plan(stub):
    e = stub(small_rfcn())
    B = e.blobs
    assert region_ops(e) == [("pair_softmax", "rpn_cls_prob"), ("proposal", "proposal"), ("psroi_pool", "psroipooled_cls_rois"),
                             ("psroi_pool", "psroipooled_loc_rois")]
    emitting = {t.layer.name for t in e.tasks if isinstance(t, E.OpTask) and t.ops}
    assert not emitting & {"rpn_cls_score_reshape", "rpn_cls_prob_reshape"}
    # the chain's middle blobs own nothing; they are read from their neighbours
    assert "rpn_cls_score_reshape" not in B and "rpn_cls_prob" not in B
    assert e.rpn_views == {"rpn_cls_score_reshape": "rpn_cls_score", "rpn_cls_prob": "rpn_cls_prob_reshape"}
    assert e.pair_softmax == {"rpn_cls_prob": ("rpn_cls_score", "rpn_cls_prob_reshape", 9)}
    calls = run_region_ops(e)
    sc, pr, dl, rois, im = B["rpn_cls_score"], B["rpn_cls_prob_reshape"], B["rpn_bbox_pred"], B["rois"], B["im_info"]
    assert calls["fcn_pair_softmax_f32"][:8] == (sc.buf.ptr, pr.buf.ptr, 36, 9, 20, 0, 20, 0)
    p = calls["fcn_proposal_f32"]
    assert (p[0], p[1], p[2], p[4], p[5]) == (pr.buf.ptr, dl.buf.ptr, im.buf.ptr, rois.buf.ptr, None)
    assert p[6] == e.roi_counts["proposal"].ptr and p[8] == 64
    par = next(k for k in e._keep if isinstance(k, L.ProposalParams))
    assert (par.H, par.W, par.A, par.feat_stride, par.pre_nms_topn, par.post_nms_topn) == (6, 6, 9, 16, 60, 12)
    assert (par.score_cstride, par.delta_cstride, par.rois_cstride, par.rois_coffset, par.top_score_cstride) == (20, 36, 8, 0, 0)
    assert abs(par.min_size - 16) < 1e-9 and abs(par.nms_thresh - 0.7) < 1e-7
    assert np.array_equal(np.array(par.anchors[:36]).reshape(9, 4), R.anchors(16, (0.5, 1, 2), (1, 2, 4)))
    ps = [a for n, a in e.fake.calls if n == "fcn_psroi_pool_fwd_f32"]
    cls, box = B["rfcn_cls"], B["rfcn_bbox"]
    assert ps[0][:3] == (cls.buf.ptr, rois.buf.ptr, B["psroipooled_cls_rois"].buf.ptr) and ps[0][3:9] == (1, 6, 6, 245, cls.cstride, 0)
    assert ps[0][9:14] == (12, 8, 0, 5, 7) and abs(ps[0][14] - 0.0625) < 1e-9 and ps[0][15:17] == (8, 0)
    assert ps[1][:3] == (box.buf.ptr, rois.buf.ptr, B["psroipooled_loc_rois"].buf.ptr) and ps[1][6] == 392 and ps[1][12:14] == (8, 7)
    # order: every task waits for what it reads
    lv = dict(zip([t.layer.name for t in e.tasks], E.task_levels(e.tasks)))
    assert lv["rpn_cls_score"] < lv["rpn_cls_prob"] < lv["proposal"] < lv["psroipooled_cls_rois"] < lv["ave_cls_score_rois"] < lv["cls_prob"]
    assert lv["rpn_bbox_pred"] < lv["proposal"] and lv["rfcn_bbox"] < lv["psroipooled_loc_rois"]
    # the ROI axis: the Proposal top and everything behind it; before any forward the shapes are the capacity
    assert set(e.spec.roi_blobs) == {"rois", "psroipooled_cls_rois", "psroipooled_loc_rois", "cls_score", "bbox_pred", "cls_prob"}
    assert e.blob_shape("rois") == (12, 5) and e.blob_shape("cls_prob") == (12, 5, 1, 1)


FAST = """input: "data" input_shape { dim: 2 dim: 3 dim: 16 dim: 20 }
input: "rois" input_shape { dim: 8 dim: 5 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv" convolution_param { num_output: 6 kernel_size: 3 pad: 1 stride: 2 } }
layer { name: "pool" type: "ROIPooling" bottom: "conv" bottom: "rois" top: "pool" roi_pooling_param { pooled_h: 3 pooled_w: 2 spatial_scale: 0.5 } }
layer { name: "fc" type: "InnerProduct" bottom: "pool" top: "fc" inner_product_param { num_output: 4 } }
layer { name: "prob" type: "Softmax" bottom: "fc" top: "prob" }
"""


def test_fast_rcnn_fragment_plan(stub):
    """rois through an Input layer: all R rows are real, no blob is on a ROI axis and nothing is cut."""
    e = stub(FAST)
    B = e.blobs
    assert region_ops(e) == [("roi_pool", "pool")] and e.spec.roi_blobs == {} and e.roi_counts == {}
    a = run_region_ops(e)["fcn_roi_pool_fwd_f32"]
    assert a[:4] == (B["conv"].buf.ptr, B["rois"].buf.ptr, B["pool"].buf.ptr, None)
    assert a[4:15] == (2, 8, 10, 6, 8, 0, 8, 8, 0, 3, 2) and abs(a[15] - 0.5) < 1e-9 and a[16:18] == (8, 0)
    assert e.shapes["pool"] == (8, 6, 3, 2) and e.shapes["prob"] == (8, 4) and e.blob_shape("pool") == (8, 6, 3, 2)


PROPOSAL = """input: "s" input_shape { dim: 1 dim: 18 dim: 4 dim: 5 }
input: "d" input_shape { dim: 1 dim: 36 dim: 4 dim: 5 }
input: "im_info" input_shape { dim: 1 dim: 3 }
input: "rois0" input_shape { dim: 4 dim: 5 }
layer { name: "prop" type: "Proposal" bottom: "s" bottom: "d" bottom: "im_info" top: "rois" proposal_param { post_nms_topn: 7 } }
"""


def test_the_half_float_engine_refuses_by_layer_name(stub):
    with pytest.raises(NotImplementedError, match=r"f16 engine: layer type ROIPooling \(pool\) has no half-float kernel"):
        stub(FAST, f16=True)
    with pytest.raises(NotImplementedError, match=r"f16 engine: layer type Proposal \(prop\) has no half-float kernel"):
        stub(PROPOSAL, f16=True)
    with pytest.raises(NotImplementedError, match=r"f16 engine: layer type PSROIPooling \(ps\) has no half-float kernel"):
        stub('input: "s" input_shape { dim: 1 dim: 18 dim: 4 dim: 5 }\ninput: "rois0" input_shape { dim: 4 dim: 5 }\nlayer { name: "ps" '
             'type: "PSROIPooling" bottom: "s" bottom: "rois0" top: "ps" psroi_pooling_param { spatial_scale: 0.5 output_dim: 2 group_size: 3 } }', f16=True)


def test_a_train_net_refuses_the_stage_by_layer_name(stub):
    text = FAST.replace('layer { name: "prob" type: "Softmax" bottom: "fc" top: "prob" }',
                        'input: "label" input_shape { dim: 8 }\nlayer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }')
    with pytest.raises(NotImplementedError, match="layer pool: ROIPooling below a layer that learns in a TRAIN-phase net"):
        stub(text, phase="TRAIN")


CHAIN = """input: "d" input_shape { dim: 1 dim: 3 dim: 4 dim: 5 }
layer { name: "c" type: "Convolution" bottom: "d" top: "c" convolution_param { num_output: 6 kernel_size: 1 } }
layer { name: "r1" type: "Reshape" bottom: "c" top: "r1" reshape_param { shape { %s } } }
layer { name: "sm" type: "Softmax" bottom: "r1" top: "sm" }
layer { name: "r2" type: "Reshape" bottom: "sm" top: "r2" reshape_param { shape { dim: 0 dim: 6 dim: -1 dim: 0 } } }
%s"""


def test_only_the_rpn_form_of_a_4d_reshape_is_taken(stub):
    rpn = "dim: 0 dim: 2 dim: -1 dim: 0"
    e = stub(CHAIN % (rpn, ""))
    assert region_ops(e) == [("pair_softmax", "sm")] and e.pair_softmax == {"sm": ("c", "r2", 3)}
    # another 4-d form: three groups of two channels
    with pytest.raises(NotImplementedError, match=r"layer r1: Reshape of \(1, 6, 4, 5\) to \(1, 3, 8, 5\)"):
        stub(CHAIN % ("dim: 0 dim: 3 dim: -1 dim: 0", ""))
    # a middle blob with another reader
    for extra in ('layer { name: "x" type: "ReLU" bottom: "r1" top: "x" }', 'layer { name: "x" type: "ReLU" bottom: "sm" top: "x" }'):
        with pytest.raises(NotImplementedError, match=r"layer r1: Reshape of \(1, 6, 4, 5\) to \(1, 2, 12, 5\)"):
            stub(CHAIN % (rpn, extra))
