"""tests/ref_ssd64.py held to cases worked by hand, and the decision margin of every GPU DetectionOutput case (no GPU)."""
import math

import numpy as np
import pytest

import ref_ssd64 as R
import ssd_cases


def test_priorbox_of_the_first_ssd300_head():
    """38 x 38 map of a 300 image, min_size 30, max_size 60, aspect ratio 2 with flip: ratios 1, 2, 1/2 -> 3 + 1 = 4 priors per cell."""
    top = R.prior_box(38, 38, 300, 300, [30.0], [60.0], [2.0], flip=True, variance=(0.1, 0.1, 0.2, 0.2), step=8)
    assert top.shape == (1, 2, 23104) and 23104 == 38 * 38 * 4 * 4
    b = top[0, 0].reshape(38, 38, 4, 4)
    np.testing.assert_allclose(b[0, 0, 0], [(4 - 15) / 300, (4 - 15) / 300, (4 + 15) / 300, (4 + 15) / 300], rtol=0, atol=1e-15)
    side = (b[0, 0, 1, 2] - b[0, 0, 1, 0]) * 300
    assert abs(side - math.sqrt(1800)) < 1e-12 and abs((b[0, 0, 1, 3] - b[0, 0, 1, 1]) * 300 - math.sqrt(1800)) < 1e-12
    # ratio 2: 30 sqrt(2) wide, 30 / sqrt(2) high; then its flip
    np.testing.assert_allclose((b[0, 0, 2, 2:] - b[0, 0, 2, :2]) * 300, [30 * math.sqrt(2), 30 / math.sqrt(2)], atol=1e-12)
    np.testing.assert_allclose((b[0, 0, 3, 2:] - b[0, 0, 3, :2]) * 300, [30 / math.sqrt(2), 30 * math.sqrt(2)], atol=1e-12)
    # the cell (h = 2, w = 5): centre ((5 + .5) 8, (2 + .5) 8)
    np.testing.assert_allclose(b[2, 5, 0], [(44 - 15) / 300, (20 - 15) / 300, (44 + 15) / 300, (20 + 15) / 300], atol=1e-15)
    assert np.array_equal(top[0, 1].reshape(-1, 4), np.tile([0.1, 0.1, 0.2, 0.2], (23104 // 4, 1)))
    one = R.prior_box(2, 2, 10, 10, [4.0], variance=(0.3,))
    assert one.shape == (1, 2, 16) and np.all(one[0, 1] == 0.3)
    assert R.prior_box(1, 1, 10, 10, [30.0], clip=True)[0, 0].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert R.expand_ratios([2.0, 2.0, 0.5, 3.0]) == [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0] and R.expand_ratios([2.0], flip=False) == [1.0, 2.0]
    for bad in (dict(max_sizes=[60.0, 70.0]), dict(max_sizes=[30.0]), dict(variance=(0.1, 0.2))):
        with pytest.raises(ValueError):
            R.prior_box(2, 2, 10, 10, [30.0], **bad)


def three_boxes():
    """Priors A = (0, 0, 1, 1) / 2, B = A shifted by 0.1 (overlap 0.4 * 0.5 / (0.5 - 0.2) ...), C far away; CORNER code with loc 0."""
    boxes = np.array([[0.0, 0.0, 0.5, 0.5], [0.1, 0.0, 0.6, 0.5], [0.7, 0.7, 0.9, 0.9]])
    priors = np.stack([boxes.reshape(-1), np.full(12, 0.1)])[None]
    return boxes, priors, np.zeros((1, 12))


def test_three_box_nms_by_hand():
    boxes, priors, loc = three_boxes()
    # A and B: intersection 0.4 x 0.5 = 0.2, union 0.25 + 0.25 - 0.2 = 0.3, overlap 2/3; C meets neither
    assert abs(R.jaccard(boxes[0], boxes[1]) - 2.0 / 3.0) < 1e-15 and R.jaccard(boxes[0], boxes[2]) == 0.0
    conf = np.array([[0.1, 0.9, 0.2, 0.8, 0.3, 0.7]])      # (prior, class): class 1 scores .9 .8 .7
    rows, margin, count = R.detection_output(loc, conf, priors, 2, 0, nms_threshold=0.5, top_k=10, keep_top_k=10, confidence_threshold=0.5)
    assert count == 2 and rows[:, :3].tolist() == [[0, 1, 0.9], [0, 1, 0.7]] and rows[1, 3:].tolist() == [0.7, 0.7, 0.9, 0.9]
    assert abs(margin - (2.0 / 3.0 - 0.5)) < 1e-12                 # the nearest decision: B's overlap with A against the threshold
    rows, margin, count = R.detection_output(loc, conf, priors, 2, 0, nms_threshold=0.7, top_k=10, keep_top_k=10, confidence_threshold=0.5)
    assert count == 3 and abs(margin - (0.7 - 2.0 / 3.0)) < 1e-12
    # a box turned inside out has area 0; touching boxes do not overlap
    assert R.area([0.5, 0.0, 0.4, 1.0]) == 0.0 and R.jaccard([0, 0, 0.5, 0.5], [0.5, 0, 1, 0.5]) == 0.0


def test_top_k_and_keep_top_k_cuts():
    boxes, priors, loc = three_boxes()
    conf = np.array([[0.0, 0.9, 0.6, 0.0, 0.8, 0.65, 0.0, 0.7, 0.55]])      # 3 classes: class 1 .9 .8 .7, class 2 .6 .65 .55
    rows, margin, count = R.detection_output(loc, conf, priors, 3, 0, nms_threshold=0.9, top_k=2, keep_top_k=-1, confidence_threshold=0.5)
    assert rows[:, :3].tolist() == [[0, 1, 0.9], [0, 1, 0.8], [0, 2, 0.65], [0, 2, 0.6]]      # label ascending, NMS (score) order within
    assert abs(margin - 0.05) < 1e-12                                                          # .6 against .55 at class 2's cut
    rows, margin, count = R.detection_output(loc, conf, priors, 3, 0, nms_threshold=0.9, top_k=-1, keep_top_k=4, confidence_threshold=0.5)
    assert rows[:, :3].tolist() == [[0, 1, 0.9], [0, 1, 0.8], [0, 1, 0.7], [0, 2, 0.65]] and abs(margin - 0.05) < 1e-12


def test_equal_scores_go_by_prior_index_then_label():
    boxes, priors, loc = three_boxes()
    conf = np.array([[0.0, 0.8, 0.8, 0.0, 0.8, 0.8, 0.0, 0.8, 0.8]])
    rows, _m, count = R.detection_output(loc, conf, priors, 3, 0, nms_threshold=0.9, top_k=2, keep_top_k=-1, confidence_threshold=0.5)
    assert count == 4 and rows[:, 1].tolist() == [1, 1, 2, 2]
    assert rows[:, 3:].tolist() == [boxes[0].tolist(), boxes[1].tolist()] * 2          # priors 0 and 1: the lower indices win the tie
    rows, _m, count = R.detection_output(loc, conf, priors, 3, 0, nms_threshold=0.9, top_k=-1, keep_top_k=4, confidence_threshold=0.5)
    assert rows[:, 1].tolist() == [1, 1, 1, 2] and rows[3, 3:].tolist() == boxes[0].tolist()      # label 1 first, then label 2's prior 0


def test_no_detection_at_all():
    boxes, priors, loc = three_boxes()
    rows, _m, count = R.detection_output(np.zeros((2, 12)), np.zeros((2, 6)), priors, 2, 0, top_k=5, confidence_threshold=0.5)
    assert count == 0 and rows.tolist() == [[0, -1, -1, -1, -1, -1, -1], [1, -1, -1, -1, -1, -1, -1]]
    rows, _m, count = R.detection_output(loc, np.array([[0.9, 0.1] * 3]), priors, 2, 0, top_k=5, confidence_threshold=0.5)
    assert count == 0                                               # the background label is never emitted


def test_both_code_types():
    prior = np.array([[[0.2, 0.2, 0.6, 0.4], [0.1, 0.1, 0.2, 0.2]]]).reshape(1, 2, 4)
    loc = np.array([1.0, -2.0, 0.5, 0.25])
    np.testing.assert_allclose(R.decode(loc, prior[0], R.CORNER, False), [[0.3, 0.0, 0.7, 0.45]], atol=1e-15)
    np.testing.assert_allclose(R.decode(loc, prior[0], R.CORNER, True), [[1.2, -1.8, 1.1, 0.65]], atol=1e-15)
    # centre (.4, .3), size (.4, .2): cx = .1 * 1 * .4 + .4, cy = .1 * -2 * .2 + .3, w = exp(.1) .4, h = exp(.05) .2
    cx, cy, w, h = 0.44, 0.26, math.exp(0.1) * 0.4, math.exp(0.05) * 0.2
    np.testing.assert_allclose(R.decode(loc, prior[0], R.CENTER_SIZE, False), [[cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]], atol=1e-15)
    cx, cy, w, h = 0.8, -0.1, math.exp(0.5) * 0.4, math.exp(0.25) * 0.2
    np.testing.assert_allclose(R.decode(loc, prior[0], R.CENTER_SIZE, True), [[cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]], atol=1e-15)


def test_normalize_gather_and_row_softmax():
    x = np.array([3.0, 4.0]).reshape(1, 2, 1, 1)
    np.testing.assert_allclose(R.normalize(x, [20.0], eps=0.0).reshape(-1), [12.0, 16.0], atol=1e-12)
    np.testing.assert_allclose(R.normalize(x, [1.0, 2.0], eps=0.0).reshape(-1), [0.6, 1.6], atol=1e-12)
    a, b = np.arange(12.0).reshape(1, 3, 2, 2), np.arange(100.0, 102.0).reshape(1, 2, 1, 1)
    assert R.gather([a, b]).tolist() == [[0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11, 100, 101]]
    np.testing.assert_allclose(R.row_softmax(np.array([[[0.0, math.log(3.0)]]])), [[[0.25, 0.75]]], atol=1e-15)


@pytest.mark.parametrize("name", list(ssd_cases.CASES))
def test_margin_of_the_gpu_cases(name):
    """Every DetectionOutput case the GPU test runs decides, in float64, at least MARGIN away from each of its thresholds and cuts: the
    float32 kernel, off by rounding of order 1e-6, then has to decide the same.  A condition on the inputs (the seeds), not a skip."""
    c, _loc, _conf, _priors, rows, margin, count = ssd_cases.reference(name)
    assert margin >= ssd_cases.MARGIN, "case %s: margin %.3g" % (name, margin)
    per_image = [int((rows[:, 0] == i).sum()) if count else 0 for i in range(c["N"])]
    if name == "p70_nothing":
        assert count == 0
    elif name == "p300_one_empty":
        assert per_image == [8, 0]
    elif name == "p300_corner_enc":
        assert [int(((rows[:, 0] == i) & (rows[:, 1] == 1)).sum()) for i in range(2)] == [1, 1]      # the smothered class: one box survives
    elif name in ("p2000_multipass", "ssd300_shape", "p1200_full_tile"):
        assert per_image == [c["keep_top_k"]] * c["N"]                                                # keep_top_k cuts
    elif name == "logits":
        negative = rows[rows[:, 2] < 0]
        print("DETOUT-REF logits: %d of %d rows have a negative score" % (len(negative), count))
        assert c["thr"] < 0 and len(negative) >= 10 and per_image == [c["keep_top_k"]] * 2
        conf = _conf.reshape(2, c["P"], c["classes"])
        assert all(int((conf[i, :, cl] > c["thr"]).sum()) > c["top_k"] for i in range(2) for cl in (1, 2, 3))      # top_k cuts, among negative scores
    elif name == "no_threshold":
        conf = _conf.reshape(2, c["P"], c["classes"])
        assert c["thr"] == -float(np.finfo(np.float32).max) and np.all(conf > c["thr"]) and c["top_k"] < c["P"]      # every prior is a candidate
        for i in range(2):
            for cl in (1, 2):
                z = np.nonzero(conf[i, :, cl] == 0)[0]
                assert len(z) == 2 and sorted(np.signbit(conf[i, z, cl]).tolist()) == [False, True]
                assert int((conf[i, :, cl] > 0).sum()) + 2 <= c["top_k"]                              # both zeros inside the top_k
        zero_rows = rows[rows[:, 2] == 0]
        assert np.any(np.signbit(zero_rows[:, 2])) and np.any(~np.signbit(zero_rows[:, 2])) and int((rows[:, 2] < 0).sum()) >= 10
    elif name == "no_background":
        assert c["bg"] == -1 and np.any(rows[:, 1] == 0)
    elif name == "c300":
        # before the keep_top_k cut: at least 260 classes of image 0 have a survivor, image 1 has survivors in classes >= 256 only
        uncut, _m, _n = R.detection_output(_loc, _conf, _priors, c["classes"], c["bg"], c["nms"], c["top_k"], c["code"], c["var_enc"], -1, c["thr"])
        lab0, lab1 = uncut[uncut[:, 0] == 0, 1], uncut[uncut[:, 0] == 1, 1]
        print("DETOUT-REF c300: survivors %d in %d classes (image 0), %d in %d classes (image 1)" % (len(lab0), len(set(lab0)), len(lab1), len(set(lab1))))
        assert c["classes"] == 300 and len(set(lab0)) >= 260 and len(lab0) > c["keep_top_k"] and len(lab1) > 0 and lab1.min() >= 256
        cut0 = rows[rows[:, 0] == 0, 1]
        assert len(cut0) == c["keep_top_k"] and np.any(cut0 < 256) and np.any(cut0 >= 256) and c["bg"] not in set(uncut[:, 1])
    else:
        assert count > 0


@pytest.mark.parametrize("name", ["mobilenet_ssd", "ssd300_vgg"])
def test_margin_of_the_gpu_net_cases(name):
    """The same for the detection tails of the two test nets of tests/test_gpu_ssd_nets.py: the nets' own float64 scores and boxes decide
    at least MARGIN away from every threshold, some candidates clear the confidence threshold and the NMS suppresses some of them."""
    import ssd_net_ref as N
    _text, spec, params, x = N.build(name)
    B, margin, count = N.reference(name, spec, params, x)
    assert margin >= ssd_cases.MARGIN, "net %s: margin %.3g" % (name, margin)
    fg = B["mbox_conf_flatten"].reshape(2, -1, 21)[:, :, 1:]
    assert 0 < count < int((fg > N.NETS[name]["thr"]).sum())
