"""Shape inference and the refusals of the region stage's layers (Proposal, ROIPooling, PSROIPooling, the Python spelling of Proposal,
the R-FCN writer) - no GPU."""
import pytest

from fcn_object_detector_amd import models, proto, region
from fcn_object_detector_amd.netspec import NetSpec


def spec_of(text, phase="TEST"):
    s = NetSpec(proto.parse_text(text), phase, depthwise=True)
    s.infer()
    return s


def test_rfcn_shapes_at_full_size():
    """ResNet-101 R-FCN at 600 x 1000: a 38 x 63 map at stride 16 under the RPN and, res5 running at stride 1 with dilation 2, under the
    region stage; 9 anchors, 300 rois, 21 classes and 8 box values over 7 x 7 groups."""
    s = spec_of(models.rfcn_resnet(depth=101))
    b = s.blob_shapes
    assert b["data"] == (1, 3, 600, 1000) and b["im_info"] == (1, 3)
    assert b["res4b22"] == (1, 1024, 38, 63) and b["res5c"] == (1, 2048, 38, 63) and b["conv_new_1"] == (1, 1024, 38, 63)
    assert b["rpn_cls_score"] == (1, 18, 38, 63) and b["rpn_bbox_pred"] == (1, 36, 38, 63)
    assert b["rpn_cls_score_reshape"] == b["rpn_cls_prob"] == (1, 2, 9 * 38, 63) and b["rpn_cls_prob_reshape"] == (1, 18, 38, 63)
    assert b["rois"] == (300, 5) and b["rfcn_cls"] == (1, 21 * 49, 38, 63) and b["rfcn_bbox"] == (1, 8 * 49, 38, 63)
    assert b["psroipooled_cls_rois"] == (300, 21, 7, 7) and b["psroipooled_loc_rois"] == (300, 8, 7, 7)
    assert b["cls_score"] == b["cls_prob"] == (300, 21, 1, 1) and b["bbox_pred"] == (300, 8, 1, 1)
    assert s.output_blobs() == ["bbox_pred", "cls_prob"] and s.data_tops() == ["data", "im_info"]
    dil = [l for l in s.layers if l.type == "Convolution" and int(l.sub("convolution_param").get("dilation", 1)) == 2]
    assert [l.name for l in dil] == ["res5a_branch2b", "res5b_branch2b", "res5c_branch2b"]
    # the proposal layer is written as the published files write it and is the built-in layer all the same
    prop = next(l for l in s.layers if l.name == "proposal")
    assert 'type: "Python"' in models.rfcn_resnet(depth=101) and "rpn.proposal_layer" in models.rfcn_resnet(depth=101)
    assert prop.type == "Proposal" and prop.python_alias and region.proposal_params(prop) == region.ProposalParams(
        16, 16, 16.0, (0.5, 1.0, 2.0), (8.0, 16.0, 32.0), 6000, 300, 0.7)
    assert set(s.roi_blobs) == {"rois", "psroipooled_cls_rois", "psroipooled_loc_rois", "cls_score", "bbox_pred", "cls_prob"}
    assert all(l is prop for l in s.roi_blobs.values())


def test_rfcn_shapes_at_a_reduced_size():
    s = spec_of(models.rfcn_resnet(depth=50, width_div=8, size=96, classes=5, pre_nms_topn=60, post_nms_topn=12, scales=(1, 2, 4)))
    b = s.blob_shapes
    assert b["res4f"] == (1, 128, 6, 6) and b["res5c"] == (1, 256, 6, 6) and b["rpn_conv/3x3"] == (1, 64, 6, 6)
    assert b["rois"] == (12, 5) and b["psroipooled_cls_rois"] == (12, 5, 7, 7) and b["cls_prob"] == (12, 5, 1, 1) and b["bbox_pred"] == (12, 8, 1, 1)
    prop = next(l for l in s.layers if l.name == "proposal")
    assert not prop.python_alias and region.proposal_params(prop).scales == (1.0, 2.0, 4.0) and region.proposal_params(prop).pre_nms_topn == 60
    assert spec_of(models.rfcn_resnet(size=(64, 96), width_div=16)).blob_shapes["res5c"] == (1, 128, 4, 6)


def test_the_writer_is_deploy_only():
    for phase in ("TRAIN", "TEST"):
        with pytest.raises(NotImplementedError, match="AnchorTarget / ProposalTarget"):
            models.rfcn_resnet(phase)
    with pytest.raises(ValueError, match="depth must be 50 or 101"):
        models.rfcn_resnet(depth=152)
    with pytest.raises(NotImplementedError, match="one image a forward"):
        models.rfcn_resnet(batch=2)


HEAD = """input: "s" input_shape { dim: %d dim: 18 dim: 4 dim: 5 }
input: "d" input_shape { dim: %d dim: 36 dim: 4 dim: 5 }
input: "im_info" input_shape { dim: 1 dim: 3 }
input: "f" input_shape { dim: 2 dim: 18 dim: 4 dim: 5 }
"""
PROPOSAL = 'layer { name: "prop" type: "Proposal" bottom: "s" bottom: "d" bottom: "im_info" top: "rois" %s %s }\n'


def test_the_two_spellings_of_proposal():
    s = spec_of(HEAD % (1, 1) + PROPOSAL % ('top: "scores"', "proposal_param { post_nms_topn: 7 pre_nms_topn: 50 nms_thresh: 0.5 min_size: 4 }"))
    assert s.blob_shapes["rois"] == (7, 5) and s.blob_shapes["scores"] == (7, 1) and set(s.roi_blobs) == {"rois", "scores"}
    p = region.proposal_params(s.layers[-1])
    assert (p.feat_stride, p.base_size, p.min_size, p.ratios, p.scales, p.pre_nms_topn, p.post_nms_topn, p.nms_thresh) == (
        16, 16, 4.0, (0.5, 1.0, 2.0), (8.0, 16.0, 32.0), 50, 7, 0.5)
    python = ("layer { name: 'prop' type: 'Python' bottom: 's' bottom: 'd' bottom: 'im_info' top: 'rois' python_param { module: 'rpn.proposal_layer' "
              "layer: 'ProposalLayer' param_str: \"%s\" } }\n")
    s = spec_of(HEAD % (1, 1) + python % "'feat_stride': 16")
    assert s.layers[-1].type == "Proposal" and s.blob_shapes["rois"] == (300, 5) and s.data_tops() == ["s", "d", "im_info", "f"]
    s = spec_of((HEAD % (1, 1)).replace("dim: 18", "dim: 12").replace("dim: 36", "dim: 24") + python % "'feat_stride': 8, 'scales': [4, 8]")
    p = region.proposal_params(s.layers[-1])
    assert p.feat_stride == 8 and p.scales == (4.0, 8.0) and s.blob_shapes["rois"] == (300, 5)
    with pytest.raises(ValueError, match="layer prop: ProposalLayer param_str names 'stride'"):
        spec_of(HEAD % (1, 1) + python % "'stride': 16")
    # any other Python layer that has bottoms keeps today's behaviour: a data layer whose tops need shapes from outside
    other = python.replace("rpn.proposal_layer", "rpn.anchor_target_layer").replace("ProposalLayer", "AnchorTargetLayer") % "'feat_stride': 16"
    with pytest.raises(KeyError, match=r"shape of data blob 'rois' \(layer prop\) was not provided"):
        spec_of(HEAD % (1, 1) + other)
    assert NetSpec(proto.parse_text(HEAD % (1, 1) + other), "TEST").layers[-1].type == "Python"


def test_proposal_refusals():
    with pytest.raises(NotImplementedError, match="layer prop: Proposal at a batch of 2"):
        spec_of(HEAD % (2, 2) + PROPOSAL % ("", ""))
    with pytest.raises(ValueError, match=r"layer prop: Proposal with 6 anchors needs scores \(1, 12, H, W\)"):
        spec_of(HEAD % (1, 1) + PROPOSAL % ("", "proposal_param { scale: 8 scale: 16 }"))
    with pytest.raises(ValueError, match="layer prop: Proposal takes three bottoms"):
        spec_of(HEAD % (1, 1) + (PROPOSAL % ("", "")).replace('bottom: "im_info" ', ""))
    with pytest.raises(ValueError, match="layer prop: Proposal with feat_stride 0"):
        spec_of(HEAD % (1, 1) + PROPOSAL % ("", "proposal_param { feat_stride: 0 }"))
    # the capacity limits of the kernel, by layer name
    big = HEAD.replace("dim: 4 dim: 5", "dim: 90 dim: 90") % (1, 1)
    with pytest.raises(NotImplementedError, match=r"layer prop: Proposal over 72900 candidates \(90 x 90 x 9 anchors\): the kernel ranks at most 65536"):
        spec_of(big + PROPOSAL % ("", ""))
    mid = HEAD.replace("dim: 4 dim: 5", "dim: 38 dim: 63") % (1, 1)
    with pytest.raises(NotImplementedError, match="layer prop: Proposal with pre_nms_topn 7000 / post_nms_topn 300 over 21546 candidates: the NMS kernel holds at most 6144"):
        spec_of(mid + PROPOSAL % ("", "proposal_param { pre_nms_topn: 7000 }"))
    with pytest.raises(NotImplementedError, match="post_nms_topn 6145"):
        spec_of(mid + PROPOSAL % ("", "proposal_param { post_nms_topn: 6145 }"))
    assert spec_of(mid + PROPOSAL % ("", "")).blob_shapes["rois"] == (300, 5)                      # R-FCN at 600 x 1000 fits
    assert spec_of(HEAD % (1, 1) + PROPOSAL % ("", "proposal_param { pre_nms_topn: 7000 }")).blob_shapes["rois"] == (300, 5)      # 180 candidates count
    many = HEAD.replace("dim: 18", "dim: 72").replace("dim: 36", "dim: 144") % (1, 1)
    with pytest.raises(NotImplementedError, match="layer prop: Proposal with 36 anchors"):
        spec_of(many + PROPOSAL % ("", "proposal_param { %s }" % " ".join("scale: %d" % (i + 1) for i in range(12))))
    for t in ("AnchorTarget", "ProposalTarget"):
        with pytest.raises(NotImplementedError, match=r"layer type '%s' \(layer t\): training the region stage" % t):
            spec_of(HEAD % (1, 1) + 'layer { name: "t" type: "%s" bottom: "s" top: "t" }' % t)


ROI = 'input: "rois" input_shape { dim: 6 dim: 5 }\nlayer { name: "pool" type: "ROIPooling" bottom: "f" bottom: "rois" top: "pool" roi_pooling_param { %s } }\n'
PSROI = 'input: "rois" input_shape { dim: 6 dim: 5 }\nlayer { name: "ps" type: "PSROIPooling" bottom: "f" bottom: "rois" top: "ps" psroi_pooling_param { %s } }\n'


def test_pooling_shapes_and_refusals():
    s = spec_of(HEAD % (1, 1) + ROI % "pooled_h: 3 pooled_w: 2 spatial_scale: 0.0625")
    assert s.blob_shapes["pool"] == (6, 18, 3, 2) and s.roi_blobs == {}          # rois through an Input: no count governs them
    s = spec_of(HEAD % (1, 1) + PSROI % "spatial_scale: 0.0625 output_dim: 2 group_size: 3")
    assert s.blob_shapes["ps"] == (6, 2, 3, 3)
    for body, msg in (("pooled_h: 0 pooled_w: 2 spatial_scale: 1", r"layer pool: ROIPooling with pooled_h 0, pooled_w 2 \(both at least 1\)"),
                      ("pooled_h: 2 spatial_scale: 1", "layer pool: ROIPooling with pooled_h 2, pooled_w 0"),
                      ("pooled_h: 2 pooled_w: 2 spatial_scale: 0", "layer pool: ROIPooling with spatial_scale 0"),
                      ("pooled_h: 2 pooled_w: 2 spatial_scale: -0.5", "layer pool: ROIPooling with spatial_scale -0.5")):
        with pytest.raises(ValueError, match=msg):
            spec_of(HEAD % (1, 1) + ROI % body)
    for body, msg in (("spatial_scale: 0.0625 output_dim: 2 group_size: 0", "layer ps: PSROIPooling with output_dim 2, group_size 0"),
                      ("spatial_scale: 0 output_dim: 2 group_size: 3", "layer ps: PSROIPooling with spatial_scale 0"),
                      ("output_dim: 2 group_size: 3", "layer ps: PSROIPooling with spatial_scale 0"),
                      ("spatial_scale: 0.0625 output_dim: 3 group_size: 3",
                       "layer ps: PSROIPooling with output_dim 3 and group_size 3 needs a bottom of 27 channels, f has 18")):
        with pytest.raises(ValueError, match=msg):
            spec_of(HEAD % (1, 1) + PSROI % body)
    with pytest.raises(ValueError, match=r"layer pool: ROIPooling takes a 4-d feature blob and rois \(R, 5\)"):
        spec_of(HEAD % (1, 1) + (ROI % "pooled_h: 2 pooled_w: 2").replace("dim: 6 dim: 5", "dim: 6 dim: 4"))
