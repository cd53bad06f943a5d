"""The decision margin of the small Faster R-CNN net of tests/test_gpu_ip_gemm_nets.py, on the CPU (no GPU): the float64 reference of
tests/faster_rcnn_case.py keeps every NMS overlap, every gap between neighbouring scores, every min_size comparison and every bin edge of
roi_pool5 at least region_cases.MARGIN from its threshold, so a float32 net decides as the reference does and a tie cannot hide a
failure; the NMS keeps fewer boxes than post_nms_topn and drops some, so the zero rows that fc6 multiplies are there."""
import numpy as np

import faster_rcnn_case as FR
import region_cases as RC


def test_margin_count_and_shapes():
    c = FR.case()
    B, count, prop = c["ref"], c["count"], c["prop"]
    print("faster_rcnn case: margin %.3g count %d suppressed %d filtered %d" % (c["margin"], count, prop["suppressed"], prop["filtered"]))
    assert c["margin"] >= RC.MARGIN
    assert 8 <= count < FR.NET["post_nms_topn"] and prop["suppressed"] > 0
    assert FR.NET["post_nms_topn"] > 32                                   # fc6 is past the streaming kernels whatever the count
    assert c["spec"].blob_shapes["roi_pool5"] == (48, 64, 7, 7) and c["spec"].param_shapes["fc6"][0] == (128, 64 * 49)
    assert B["rois"].shape == (count, 5) and B["roi_pool5"].shape == (count, 64, 7, 7)
    assert B["cls_prob"].shape == (count, 5) and B["bbox_pred"].shape == (count, 20)
    assert np.allclose(B["cls_prob"].sum(axis=1), 1.0)
    # the head is not degenerate: both signs in front of relu6 / relu7, rows that differ
    for nm in ("fc6", "fc7"):
        assert 0.2 < (B[nm] > 0).mean() < 0.8, nm
    assert np.ptp(B["cls_prob"], axis=0).max() > 1e-3
