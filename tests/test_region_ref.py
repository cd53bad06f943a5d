"""tests/ref_region64.py held to cases worked by hand, the package's anchors held to the published table, and the decision margin of
every GPU case of the region stage (no GPU)."""
import math

import numpy as np
import pytest

import ref_region64 as R
import region_cases as RC
from fcn_object_detector_amd import region

# py-faster-rcnn's nine anchors for base 16, ratios .5 1 2, scales 8 16 32 (ratio-major, scale-minor)
TABLE = [[-84, -40, 99, 55], [-176, -88, 191, 103], [-360, -184, 375, 199], [-56, -56, 71, 71], [-120, -120, 135, 135], [-248, -248, 263, 263],
         [-36, -80, 51, 95], [-80, -168, 95, 183], [-168, -344, 183, 359]]


def test_the_anchor_table():
    assert R.anchors().tolist() == TABLE
    got = region.anchors()
    assert got.dtype == np.float64 and got.tolist() == TABLE
    # other parameters: the reference and the package agree, and the index is ratio-major
    for base, ratios, scales in ((16, (0.5, 1.0, 2.0), (1.0, 2.0, 4.0)), (8, (1.0, 3.0), (2.0,)), (16, (0.333, 1.0), (3.0, 6.0, 12.0))):
        assert np.array_equal(region.anchors(base, ratios, scales), R.anchors(base, ratios, scales))
    a = R.anchors(16, (1.0, 2.0), (1.0, 4.0))
    assert a.tolist() == [[0, 0, 15, 15], [-24, -24, 39, 39], [2.5, -3, 12.5, 18], [-14, -36, 29, 51]]      # ratio 2: 11 wide, 22 high about the centre 7.5


def test_a_proposal_by_hand():
    """One anchor [0, 0, 15, 15] on a 1 x 3 map at stride 16 of a 20 x 48 image: boxes [0..15], [16..31], [32..47] in x.  The middle one is
    moved left by dx = -0.5 (8 pixels: [8, 24] by the decode; overlap with the first 9 x 17 / (2 x 289 - 153) = 0.36 with the +1 extents), the last one is shrunk by
    dw = log(0.5) to 8 pixels and dropped by min_size 16."""
    base = np.array([[0.0, 0.0, 15.0, 15.0]])
    scores = np.zeros((1, 2, 1, 3))
    scores[0, 1, 0] = [0.6, 0.9, 0.8]
    deltas = np.zeros((1, 4, 1, 3))
    deltas[0, 0, 0, 1] = -0.5
    deltas[0, 2, 0, 2] = math.log(0.5)
    out = R.proposal(scores, deltas, [[20, 48, 1.0]], base, 16, 10, 4, 0.3, 16)
    assert out["count"] == 1 and out["filtered"] == 1 and out["suppressed"] == 1 and out["index"] == [1]
    assert out["rois"].tolist() == [[0, 8, 0, 24, 16]] + [[0] * 5] * 3 and out["scores"][:, 0].tolist() == [0.9, 0, 0, 0]
    # decode: w = 16, cx = 8 (+ 16 x), pcx = cx - 8, corners pcx -+ 8: the box is [8, 24] wide 17 by the +1 convention
    inter = (16 - 8 + 1) * 17.0
    ov = inter / (17 * 17 + 17 * 17 - inter)
    assert abs(out["margin"] - min(abs(ov - 0.3), 0.9 - 0.6)) < 1e-12
    assert out["margin"] == pytest.approx(0.06)                   # 153 / 425 = 0.36 against 0.3
    # a higher threshold keeps both; the rows come in score order
    out = R.proposal(scores, deltas, [[20, 48, 1.0]], base, 16, 10, 4, 0.4, 16)
    assert out["count"] == 2 and out["index"] == [1, 0] and out["rois"][:2].tolist() == [[0, 8, 0, 24, 16], [0, 0, 0, 16, 16]]
    # clipping: the image is 20 high and 48 wide; a box moved up and left ends on the borders
    deltas[0, 0, 0, 0] = deltas[0, 1, 0, 0] = -1.0
    out = R.proposal(scores, deltas, [[20, 48, 1.0]], base, 16, 10, 4, 0.4, 1)
    assert out["boxes"][0].tolist() == [0, 0, 0, 0] and out["boxes"][2].tolist() == [36, 0, 44, 16]
    # ties go to the smaller candidate index; pre_nms_topN cuts the order, post_nms_topN the survivors
    scores[0, 1, 0] = [0.7, 0.7, 0.7]
    out = R.proposal(scores, np.zeros((1, 4, 1, 3)), [[20, 48, 1.0]], base, 16, 2, 4, 0.4, 16)
    assert out["index"] == [0, 1]
    assert R.proposal(scores, np.zeros((1, 4, 1, 3)), [[20, 48, 1.0]], base, 16, 3, 1, 0.4, 16)["index"] == [0]


def test_roi_pooling_bins_by_hand():
    """A 6 x 8 map, one ROI [0, 2, 2, 11, 9] at scale 0.5: start (1, 1), end (round(5.5) = 6, round(4.5) = 5: halves away from zero), 6 wide
    and 5 high.  pooled 2 x 3: bin_h 2.5 -> rows [1, 4) and [3, 6); bin_w 2 -> columns [1, 3), [3, 5), [5, 7)."""
    x = np.arange(48.0).reshape(1, 1, 6, 8)
    y, arg, margin = R.roi_pool(x, [[0, 2, 2, 11, 9]], 2, 3, 0.5)
    assert y[0, 0].tolist() == [[26, 28, 30], [42, 44, 46]] and arg[0, 0].tolist() == [[26, 28, 30], [42, 44, 46]]
    assert margin == np.inf                                  # every argument is exact in float32 as well
    # hanging over the lower right corner: rows and columns are clipped to the map, bins outside are empty (0, argmax -1)
    y, arg, _m = R.roi_pool(x, [[0, 12, 8, 30, 22]], 2, 2, 0.5)      # start (6, 4), end (15, 11): 10 x 8, bins of 5 x 4
    assert y[0, 0].tolist() == [[47, 0], [0, 0]] and arg[0, 0].tolist() == [[47, -1], [-1, -1]]
    # the first maximum in raster order wins a tie
    _y, arg, _m = R.roi_pool(np.ones((1, 1, 6, 8)), [[0, 2, 2, 11, 9]], 1, 1, 0.5)
    assert arg[0, 0, 0, 0] == 9
    # an argument float32 does not reproduce counts: 0.3 * 7 in float64 is 2.1 - 4e-16, its distance from the breakpoint 2.5 is 0.4
    _y, _a, m = R.roi_pool(x, [[0, 7, 0, 7, 0]], 1, 1, 0.3)
    assert abs(m - 0.4) < 1e-6


def test_psroi_pooling_bins_by_hand():
    """group_size 2, output_dim 1 (4 channels), a 4 x 4 map at scale 0.25, ROI [0, 0, 0, 15, 7]: start (0, 0), end ((15 + 1) / 4, (7 + 1) / 4) =
    (4, 2); bins 2 wide and 1 high.  Bin (ph, pw) reads channel ph * 2 + pw."""
    x = np.stack([np.full((4, 4), 10.0 * c) + np.arange(16.0).reshape(4, 4) for c in range(4)])[None]
    y, mag, largest, margin = R.psroi_pool(x, [[0, 0, 0, 15, 7]], 1, 2, 0.25)
    assert y[0, 0].tolist() == [[0.5, 12.5], [24.5, 36.5]] and largest == 2 and margin == np.inf
    # a ROI of no extent still covers max(.., 0.1) of a cell; one outside the map gives zeros
    y, _mag, _l, _m = R.psroi_pool(x, [[0, 5, 5, 4, 4], [0, 40, 40, 50, 50]], 1, 2, 0.25)
    assert y[0, 0].tolist() == [[5.0, 15.0], [25.0, 35.0]] and np.all(y[1] == 0)
    np.testing.assert_allclose(R.pair_softmax(np.array([0.0, 1.0, math.log(3.0), 1.0]).reshape(1, 4, 1, 1)).reshape(-1), [0.25, 0.5, 0.75, 0.5], atol=1e-15)


@pytest.mark.parametrize("name", list(RC.PROPOSALS))
def test_margin_of_the_gpu_proposal_cases(name):
    """Every Proposal case the GPU test runs decides, in float64, at least MARGIN away from each threshold, bound and neighbouring score: the
    float32 kernel, off by rounding, then has to decide the same.  A condition on the inputs (the seeds), not a skip.

    Beside each case stands what it is for, computed from the reference's order, places, suppressors and scores: the depth of the walk
    (the last place of the order the greedy NMS looks at), boxes kept and dropped in the upper half of the sweep's suppressed set (places
    from 4096 on), a full matrix, a cut that hides leaders, an image that is not the map's extent ...  An edit of a seed that moves a case
    off its path fails here."""
    c, base, scores, deltas, im, out = RC.proposal_reference(name)
    assert out["margin"] >= RC.MARGIN, "case %s: margin %.3g" % (name, out["margin"])
    m = scores.shape[2] * scores.shape[3] * len(base)
    assert float(np.nanmax(np.abs(out["boxes"]))) < 2 * max(c["H"], c["W"]) * RC.FEAT_STRIDE
    places = np.array(out["places"], np.int64)
    drops = np.array(out["suppressors"], np.int64).reshape(-1, 2)            # (place of the dropped box, place of the kept box that dropped it)
    depth, k, fg = RC.depth(out), len(out["order"]), scores[0, len(base):].transpose(1, 2, 0).reshape(-1)
    print("PROPOSAL-REF %s: %d candidates, %d into the NMS (%d words), count %d, depth %d, %d kept at places >= 4096"
          % (name, m, k, (k + 63) // 64, out["count"], depth, int((places >= 4096).sum())))
    # the corner tolerance of the GPU test (32 float32 ulps of the larger image extent) is justified here, against the reference and not
    # against the kernel: the contract's decode in numpy float32 is off by at most a quarter of it
    number = ~np.isnan(out["boxes"]).any(axis=1)
    err = float(np.max(np.abs(RC.decode32(c, base, deltas, im)[number].astype(np.float64) - out["boxes"][number])))
    limit = 32 * float(np.spacing(np.float32(max(im[0, 0], im[0, 1]))))
    print("PROPOSAL-REF %s: a float32 decode is off by at most %.3g, the tolerance is %.3g" % (name, err, limit))
    assert err <= 0.25 * limit
    if "placed" in c:
        assert np.array_equal(out["boxes"], out["raw"]) and float(np.abs(deltas).max()) > 50, "every box inside the image; deltas far above 1"
        assert drops.size and np.all(fg[out["order"][:-1]] >= fg[out["order"][1:]])
    if name == "deep_sweep":
        assert k == m == 5184 and out["count"] == c["post"] and depth >= 4096 + 128 and int((places >= 4096).sum()) >= 64
        late = drops[drops[:, 0] >= 4096]
        assert np.any(late[:, 1] < 4096), "a box in the upper half of the set dropped by a box kept in the lower half"
        assert np.any(late[:, 1] >= 4096), "... and one dropped by a box kept in the upper half"
        assert np.any(places % 64 == 63) and np.any(places[places % 64 == 63] >= 4096), "a kept box at bit 63 of its word"
        assert int((out["scores"][:out["count"], 0] < 0).sum()) >= 64 and np.all(fg != 0)
    elif name == "pre_6144":
        assert m == 26 * 27 * 9 > c["pre"] == k == 6144 and (k + 63) // 64 == 96 and places[-1] > 6080 and out["count"] < c["post"]
        # past the cut lie leaders of sites the order has not seen: with them the count would be another one
        more = R.proposal(scores, deltas, im, base, RC.FEAT_STRIDE, m, c["post"], c["nms"], c["min_size"])
        assert more["count"] > out["count"] + 10 and more["index"][:out["count"]] == out["index"]
        # the tie across the cut: the two candidates have one score, both are leaders, the smaller index is in
        order_all = more["order"]
        inside, outside = int(order_all[c["pre"] - 1]), int(order_all[c["pre"]])
        assert fg[inside] == fg[outside] and inside < outside and out["index"][-1] == inside and outside in more["index"]
    elif name in ("keep_everything", "suppress_everything"):
        assert k == m >= 4200 and out["filtered"] == 0 and c["post"] == 6144 and (k + 63) // 64 > 64
        assert out["count"] == (k if name == "keep_everything" else 1)
        if name == "suppress_everything":
            far = R.overlaps(out["boxes"][out["index"][0]], out["boxes"])
            assert int((far == 0).sum()) > 1000, "pairs that do not meet at all are dropped as well: 0 > -1"
    elif name == "max_candidates":
        assert m == 65536 and len(base) == 16 and m - out["filtered"] > c["pre"] == k and out["filtered"] > 0 and out["count"] == c["post"]
        assert out["index"][:4] == [2047, 2048, 8191, 8192] and fg[2047] == fg[2048] > fg[8191] == fg[8192] > np.delete(fg, [2047, 2048, 8191, 8192]).max()
    elif name == "a32":
        assert (m, len(base)) == (480, 32) and out["count"] > 0 and out["suppressed"] > 0 and out["filtered"] > 0
    elif name == "a1":
        assert (m, len(base)) == (63, 1) and out["count"] > 0 and out["suppressed"] > 0
    elif name == "one":
        assert m == 1 and (c["pre"], c["post"], out["count"], out["index"]) == (1, 1, 1, [0])
    elif name == "one_filtered":
        assert m == 1 and (out["count"], out["filtered"]) == (0, 1) and np.all(out["rois"] == 0)
    elif name == "none_survive":
        assert (out["count"], out["filtered"], k) == (0, m, 0) and np.all(out["rois"] == 0) and np.all(out["scores"] == 0)
    elif name == "scaled_image":
        assert tuple(im[0]) == (43, 91, np.float32(1.6)) and out["count"] > 0 and out["suppressed"] > 0
        unit = R.proposal(scores, deltas, [im[0, 0], im[0, 1], 1.0], base, RC.FEAT_STRIDE, c["pre"], c["post"], c["nms"], c["min_size"])
        ext = np.stack([out["boxes"][:, 2] - out["boxes"][:, 0] + 1, out["boxes"][:, 3] - out["boxes"][:, 1] + 1], axis=1).min(axis=1)
        fate = int(((ext >= 16) & (ext < 16 * 1.6)).sum())                  # alive at scale 1, dropped at scale 1.6
        assert fate >= 10 and unit["filtered"] == out["filtered"] - fate and unit["index"] != out["index"]
        raw, box = out["raw"], out["boxes"]
        by_image = int(((raw[:, 2] > 90) & (raw[:, 2] <= 7 * 16 - 1)).sum()) + int(((raw[:, 3] > 42) & (raw[:, 3] <= 5 * 16 - 1)).sum())
        assert by_image >= 10 and np.any(box[:, 2] == 90) and np.any(box[:, 3] == 42), "corners the image clips and the map's extent would not"
        on_map = R.proposal(scores, deltas, [5 * 16, 7 * 16, im[0, 2]], base, RC.FEAT_STRIDE, c["pre"], c["post"], c["nms"], c["min_size"])
        assert on_map["index"] != out["index"]
    elif name == "signed_scores":
        s = out["scores"][:out["count"], 0]
        assert s[0] == np.inf and s[-1] == -np.inf and np.all(np.isfinite(s[1:-1])) and out["count"] <= c["post"] and k < c["pre"]
        assert int(((s < 0) & (s > -1e30)).sum()) >= 10 and np.any((s > 0) & (s < 1e-38)) and np.any((s < 0) & (s > -1e-38))
        zero = np.nonzero(s == 0)[0]
        assert np.any(np.signbit(s[zero])) and np.any(~np.signbit(s[zero]))
        tied = np.array(out["index"])[zero]
        assert len(zero) >= 2 and np.all(np.diff(zero) == 1) and np.all(np.diff(tied) > 0), "the zeros are one score: smaller index first"
        assert np.any(np.diff(np.signbit(s[zero]).astype(int)) < 0), "a -0.0 in front of a +0.0: the sign does not order them"
    elif name in ("nan_inputs", "nan_min0"):
        clean = c["clean"]
        assert int(np.isnan(fg).sum()) == 5 and int(np.isnan(deltas).sum()) == 5 and int(np.isnan(out["raw"]).any(axis=1).sum()) == 5
        lost = set(c["no_score"] + c["no_delta"])
        assert len(lost & set(clean["index"])) >= 6 and not lost & set(out["index"]) and not lost & set(out["order"].tolist())
        assert out["index"] != clean["index"] and out["count"] == c["post"]
        assert out["filtered"] == m - len(set(clean["alive"].tolist()) - lost) > clean["filtered"], "`filtered` counts them"
        if name == "nan_min0":
            assert c["min_size"] == 0 and clean["filtered"] == 0 and out["filtered"] == 10, "no size bound drops a box here: the NaN rule alone does"
    elif name == "m12x10_tiles":
        assert m == 1080 and c["pre"] == 150 and out["suppressed"] > 0            # more than one ranking tile, three words of NMS matrix
    elif name == "filter_clip":
        assert out["filtered"] > m // 2 and np.any(out["boxes"] == 0) and np.any(out["boxes"][:, 2] == c["W"] * RC.FEAT_STRIDE - 1)
    elif name == "few_survive":
        assert 0 < out["count"] < c["post"] and np.all(out["rois"][out["count"]:] == 0)
    elif name == "post_cut":
        assert out["count"] == c["post"] and m - out["filtered"] > c["post"]
    elif name == "pre_above":
        assert c["pre"] > m and out["suppressed"] > 0
    elif name == "rfcn_full":
        assert (m, c["pre"], c["post"], out["count"]) == (38 * 63 * 9, 6000, 300, 300) and m - out["filtered"] > 6000 and out["suppressed"] > 0
    else:
        assert out["count"] > 0 and out["suppressed"] > 0


def test_margin_of_the_gpu_pooling_cases():
    for name in RC.ROI_POOLS:
        _x, y, arg, margin = RC.roi_pool_reference(name)
        assert margin >= RC.MARGIN and 0 < int((arg < 0).sum()) < arg.size, name      # some bins are empty, not all
        assert np.all(y[5] == 0) and np.all(arg[5] == -1) and len({v for v in y[3, 0].reshape(-1)}) == 1      # outside; the one-cell ROI
    for name, (_n, od, g, _cs, _co) in RC.PS_POOLS.items():
        _x, y, _mag, largest, margin = RC.psroi_pool_reference(name)
        assert margin >= RC.MARGIN and largest > 1 and np.all(y[5] == 0) and np.any(y[2] != 0), name


@pytest.mark.parametrize("name", ["fast", "rfcn"])
def test_margin_of_the_gpu_net_cases(name):
    """The same for the two test nets of tests/test_gpu_region_nets.py: the nets' own float64 scores, boxes and rois decide at least MARGIN
    away from every threshold and breakpoint; the R-FCN net's RPN keeps some boxes and suppresses some."""
    import region_net_ref as N
    _text, spec, params, inputs = N.build(name)
    B, margin, count, prop = N.reference(name, spec, params, inputs)
    assert margin >= RC.MARGIN, "net %s: margin %.3g" % (name, margin)
    if name == "rfcn":
        assert 0 < count < N.RFCN["post_nms_topn"] and prop["suppressed"] > 0 and B["rois"].shape == (count, 5) and B["cls_prob"].shape == (count, 5, 1, 1)
    else:
        assert count is None and B["prob"].shape == (8, 6)
