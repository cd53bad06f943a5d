"""The references and inputs of the guarded byte / integer tests, checked without a GPU: every independent reference of tests/ref_bytes.py
agrees with the oracle on exactly the inputs the GPU tests use (tests/byte_cases.py), and those inputs reach the paths they were built for."""
import math

import numpy as np
import pytest

import byte_cases as B
import ref_bytes as RB
from oracle import detect_ref as D
from oracle import mask_ref as M
from oracle import scene_ref as S


@pytest.mark.parametrize("hw", B.IMAGE_SIZES + [(1, 7), (3, 2), (13, 17)], ids=str)
def test_box_and_median_references_equal_the_oracle(hw):
    """Down to images smaller than the kernel, where the reflected border folds several times."""
    img = B.image(hw)
    for k in B.BOX_KS:
        assert np.array_equal(RB.blur_box(img, k), S.blur_box(img, k)), k
    for k in B.MEDIAN_KS:
        assert np.array_equal(RB.blur_median(img, k), S.blur_median(img, k)), k


def test_gauss_and_colour_inputs():
    assert [len(t) - 1 for t in B.GAUSS.values()] == [1, 3, 10, 0, 15]
    for t in B.GAUSS.values():
        assert t.dtype == np.float32 and abs(float(t[0]) + 2.0 * float(t[1:].sum()) - 1.0) < 1e-6
    for hw in B.IMAGE_SIZES:
        img = B.image(hw)
        assert np.array_equal(S.blur_gauss(img, B.GAUSS["radius0"]), img)          # the identity cases need no oracle: it agrees with them
        assert np.array_equal(S.color_point_ops(img, (0.0, 1.0), [0] * 3, [1.0] * 3, 0.0), img)
    assert B.colour_fields(dict(sharpen=(0.0, 1.0), add=[0] * 3, mul=[1.0] * 3, gray=0.0))[:2] == (1.0, -0.0)
    big = B.image((17, 19))
    sat = [B.colour_expected(big, B.COLOUR[n]) for n in ("add+300", "add-300-grey", "mul0", "mul3-grey")]
    assert sat[0].min() == 255 and sat[1].max() == 0 and sat[2].max() == 0 and sat[3].max() == 255 and sat[3].min() < 255


def test_compose_inputs_reach_their_paths():
    W, H = B.SCENE_W, B.SCENE_H
    _, mask = S.render_scene(B.StandInLayer, B.plan(final_flip=2))
    assert set(np.unique(mask)) == {0, 1, 2, 3, 4}, "at least one output pixel comes from each object"
    left = any(o["pos"][0] < 0 for o in B.OBJECTS)
    top = any(o["pos"][1] < 0 for o in B.OBJECTS)
    right = any(o["pos"][0] + o["out"][0] > W for o in B.OBJECTS)
    bottom = any(o["pos"][1] + o["out"][1] > H for o in B.OBJECTS)
    assert left and top and right and bottom
    # the value-1 mask under the bilinear enlargement: blends in (0, 0.5] round to 0 inside the object's footprint, visible in the scene
    o = B.OBJECTS[1]
    x, y, w, h = o["roi"]
    m = RB.flip(B.SOURCES[o["idx"]][1], o["flip"])[y:y + h, x:x + w]
    blend = S.resize_bilinear(m.astype(np.float64), *o["out"])
    hole = (blend > 0) & (np.rint(blend) == 0)
    assert hole.any() and (np.rint(blend) == 1).any()
    cx, cy = o["pos"]
    assert cx >= 0 and cy >= 0 and cx + o["out"][0] <= W and cy + o["out"][1] <= H
    only = S.render_scene(B.StandInLayer, B.plan(objects=[o], final_flip=2))[1][cy:cy + o["out"][1], cx:cx + o["out"][0]]
    assert np.array_equal(only == 0, np.rint(blend) == 0)
    # the last object overlaps the second one and wins where its own mask is nonzero
    both = S.render_scene(B.StandInLayer, B.plan(objects=[B.OBJECTS[1], B.OBJECTS[3]], final_flip=2))[1]
    assert ((both == 4) & (S.render_scene(B.StandInLayer, B.plan(objects=[B.OBJECTS[1]], final_flip=2))[1] == 2)).any()
    for crop in [B.MAIN_CROP] + B.OTHER_CROPS:
        assert crop[0] + crop[2] <= B.BG_W and crop[1] + crop[3] <= B.BG_H
    assert B.SAME_SIZE_CROP[2:] == (W, H) and B.OTHER_CROPS[3][0] + B.OTHER_CROPS[3][2] == B.BG_W and B.OTHER_CROPS[3][1] + B.OTHER_CROPS[3][3] == B.BG_H
    assert any(o["roi"][0] + o["roi"][2] == B.SRC_W and o["roi"][1] + o["roi"][3] == B.SRC_H for o in B.OBJECTS)
    assert {o["flip"] for o in B.OBJECTS} == {0, 1, -1, 2}


def test_permutation_scenes_equal_the_oracle():
    n = 0
    for name, (p, _outs, _entry, perm) in B.compose_cases().items():
        if not perm:
            continue
        assert p["bg_crop"][2:] == (B.SCENE_W, B.SCENE_H) and all(o["out"] == o["roi"][2:] for o in p["objects"])
        img, mask = RB.compose_permutation(B.BACKGROUND, p["bg_crop"][:2], B.SCENE_H, B.SCENE_W, B.SOURCES, p["objects"], p["final_flip"])
        if p["view"]:
            vx, vy, vw, vh = p["view"]
            img, mask = img[vy:vy + vh, vx:vx + vw], mask[vy:vy + vh, vx:vx + vw]
        want = B.compose_expected(p)
        assert np.array_equal(img, want[0]) and np.array_equal(mask, want[1]), name
        n += 1
    assert n == 5


def test_label_references():
    assert np.array_equal(RB.label_repeat(B.LABEL_MASK, 2, 2), B.label_expected((14, 18)))
    assert np.array_equal(B.label_expected((7, 9)), B.LABEL_MASK.astype(np.float32))
    assert len(np.unique(B.LABEL_MASK)) == 5 and B.label_expected((5, 4)).shape == (5, 4)


def test_analytic_masks_equal_the_oracle():
    fm, masks = B.analytic_scores()
    pmap, out = B.analytic_expected()
    assert M.create_mask_labels(masks[0]) == (8, 6, 6, 3)
    assert out.tolist() == [[1, 8, 6, 6, 3], [1, 9, 5, 3, 4], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    opmap, oout = B.score_expected(fm, B.ANALYTIC_RECTS, B.ANALYTIC_FRAME)
    assert np.array_equal(pmap, opmap) and np.array_equal(out, oout)
    assert pmap[-1, -1] == 0 and pmap.size % 4 != 0 and set(np.unique(pmap)) == {0, 126, 255}


@pytest.mark.parametrize("win", B.SCORE_WINDOWS, ids=str)
def test_score_inputs_reach_their_paths(win):
    fm, rects = B.score_case(win)
    pmap, out = B.score_expected(fm, rects, B.SCORE_FRAME)
    assert pmap.size == 130 and pmap[-1, -1] != 0, "the map's last byte is written"
    assert out[3].tolist() == [0] * 5 and out[:, 0].sum() >= 2, "an empty class, and classes with contours"
    assert rects[1][0] + win[0] == 13 and rects[1][1] + win[1] == 10 and fm.max() > 1.0
    if win == (7, 6):
        assert fm[0, 1, 0, 0] == 1.5 and M.to_uint8(np.array([np.float32(1.5) * np.float32(255)]))[0] == 126          # 382.5 -> 382 & 0xFF


def test_a_huge_score_reads_as_foreground():
    """The oracle's cast on the poison of the score maps, 3e38 (the whole chain, and what a NaN gives, is pinned on numpy stand-ins in
    test_guard_harness.py)."""
    assert M.to_uint8(np.array([np.clip(np.float32(3e38) * np.float32(255), -2147483648.0, 2147483520.0)]))[0] == 128


@pytest.mark.parametrize("mode", ["nearest_even", "trunc"])
@pytest.mark.parametrize("seed", B.DENSE_SEEDS)
def test_dense_detect_scene_reaches_every_filter(seed, mode):
    cvg, bb = B.detect_scene("dense%d" % seed)
    prop, mask = D.gridbox_to_boxes(cvg[0, 0], bb[0, :4], B.DET_THRESH, 17 * 16, 15 * 16, 16)
    assert mask.all() and len(prop) == 255 > B.SLICE_MIN_CANDIDATES
    assert (prop != np.floor(prop)).any(), "half-integer coordinates: the rounding modes differ"
    rects = [D.to_rect(b, mode) for b in prop.tolist()]
    labels, ncls = D.partition(rects, B.DET_EPS)
    flabels, fncls = D.partition_fast(np.asarray(rects), B.DET_EPS)
    assert ncls == fncls and np.array_equal(np.asarray(labels), flabels), "the literal cv::partition and the vectorised one"
    sizes = np.bincount(labels)
    assert (sizes <= 3).any(), "a class at or below the group threshold"
    grouped, weights = D.group_rectangles(rects, 3, B.DET_EPS)
    assert len(grouped) < (sizes > 3).sum(), "a class removed by containment"
    kept, kw = B.vote_slot(prop, 3, B.DET_EPS, mode)
    assert 2 <= len(kept) < len(grouped), "a class removed by min_height, at least two survivors"
    votes = D.vote_boxes(prop, 3, B.DET_EPS, mode, B.DET_MIN_HEIGHT, fast=False)
    assert [list(r) + [math.log(w)] for r, w in zip(kept, kw)] == votes
    assert B.detect_expected("dense%d" % seed, mode)[0] == (len(kept), kept, kw)


def test_other_detect_scenes():
    for name in ("small", "batch2", "batch43", "three", "overflow"):
        for mode in ("nearest_even", "trunc"):
            slow, fast = B.detect_expected(name, mode), B.detect_expected(name, mode, fast=True)
            assert slow == fast, name
    cvg, _ = B.detect_scene("small")
    assert (cvg >= 0.5).sum() == 90 <= B.SLICE_MIN_CANDIDATES
    b2 = B.detect_expected("batch2")
    assert len(b2) == 50 and b2[25 + 7] == B.detect_expected("dense%d" % B.DENSE_SEEDS[0])[0]
    assert b2[0][0] >= 1 and b2[1][0] == 0 and b2[2][0] == 0 and b2[3][0] >= 1
    cvg2, bb2 = B.detect_scene("batch2")
    assert (cvg2[0, 2] >= 0.5).sum() == 1 and not bb2[0, 8:12, 0, 0].any(), "one candidate, an all-zero box"
    assert (cvg2[0, 1] >= 0.5).sum() == 0
    b43 = B.detect_expected("batch43")
    assert len(b43) == 129 and sum(s[0] > 0 for s in b43) > 40 and sum(s[0] == 0 for s in b43) > 40
    three = B.detect_expected("three")
    assert [s[0] for s in three] == [3, 0, 3] and (B.detect_scene("three")[0][0, 1] >= 0.5).sum() == 0
    assert three[0][1] != three[2][1]
    over = B.detect_expected("overflow")
    assert over[0] == (-1, [], []) and over[1][0] == 1
    thr0 = B.detect_expected("small", "nearest_even", 0)
    assert 5 < thr0[0][0] < 90 and set(thr0[0][2]) == {1}, "group_thresh 0 passes the candidates through, min_height still filters"
    cvg, bb = B.detect_scene("small")
    prop, _ = D.gridbox_to_boxes(cvg[0, 0], bb[0, :4], B.DET_THRESH, 160, 144, 16)
    assert [D.to_rect(b, "trunc") for b in prop.tolist()] != [D.to_rect(b) for b in prop.tolist()], "the rounding modes see different candidates"


def test_target_inputs_reach_their_paths():
    t = B.TGT
    fg, bl, sl, ol, cl = B.targets_expected()
    assert fg.shape == (3, 3, 5, 6) and bl.shape == (3, 12, 5, 6)
    assert not fg[0].any() and fg[1, 0].any() and fg[1, 1].any() and fg[2, 1].any() and not fg[:, 2].any()
    im_h, im_w = t["gy"] * t["stride"], t["gx"] * t["stride"]
    first = D.bounding_box_parameterized_labels(im_h, im_w, t["rects"][1][:1], [0], t["stride"], t["C"], t["iou"])
    replaced = (first[0][0] == 1) & (bl[1, 0] != first[1][0])
    assert replaced.any(), "a cell where the later box replaced an earlier one"
    kept = (first[0][0] == 1) & (bl[1, 0] == first[1][0])
    assert kept.any(), "and a cell the later box does not reach"
    outside = D.bounding_box_parameterized_labels(im_h, im_w, t["rects"][2][1:], [1], t["stride"], t["C"], t["iou"])
    assert not outside[0].any() and t["rects"][2][0][0] < 0
    assert all(r[2] >= 1 and r[3] >= 1 for rs in t["rects"] for r in rs)
