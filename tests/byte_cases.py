"""The inputs and expected results of the guarded byte / integer tests, in ONE place: tests/test_byte_refs.py checks them on the CPU (the
independent references of tests/ref_bytes.py against the oracle, and that every input reaches the path it was built for) and the
tests/test_gpu_guarded_{augment,scene,masks,detect}.py files feed exactly these to the kernels.  Everything is deterministic."""
import functools

import numpy as np

from fcn_object_detector_amd.data_layer import gauss_taps, plan_color
from oracle import detect_ref as D
from oracle import mask_ref as M
from oracle import scene_ref as S

# ------------------------------------------------------------------------------------------------------------ colour kernels
IMAGE_SIZES = [(1, 1), (2, 9), (7, 5), (17, 19)]          # 17 x 19 = 323 pixels: more than one 256-lane workgroup
BOX_KS = list(range(1, 16))
MEDIAN_KS = [3, 5, 7]


def image(hw):
    h, w = hw
    return np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _radius15():
    w = np.exp(-0.5 * np.arange(16, dtype=np.float64) ** 2 / 25.0)
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


GAUSS = {"sigma0.05": gauss_taps(0.05), "sigma0.7": gauss_taps(0.7), "sigma3.0": gauss_taps(3.0), "radius0": np.array([1.0], np.float32),
         "radius15": _radius15()}


def _colour_cases():
    rng = np.random.default_rng(2025)
    cases = {}
    for i in range(6):
        c = plan_color(rng)
        cases["draw%d" % i] = dict(sharpen=c["sharpen"], add=c["add"], mul=c["mul"], gray=c["gray"])
    cases["add+300"] = dict(sharpen=(0.0, 1.0), add=[300] * 3, mul=[1.0] * 3, gray=0.0)
    cases["add-300-grey"] = dict(sharpen=(0.0, 1.0), add=[-300] * 3, mul=[1.0] * 3, gray=1.0)
    cases["mul0"] = dict(sharpen=(0.0, 1.0), add=[0] * 3, mul=[0.0] * 3, gray=0.0)
    cases["mul3-grey"] = dict(sharpen=(0.0, 1.0), add=[0] * 3, mul=[3.0] * 3, gray=1.0)
    cases["mixed-sharp"] = dict(sharpen=(1.0, 1.5), add=[300, -300, 0], mul=[3.0, 0.0, 1.0], gray=1.0)
    return cases


COLOUR = _colour_cases()
COLOUR_IDENTITY = (1.0, 0.0, [0, 0, 0], [1.0, 1.0, 1.0], 0.0, 1.0)      # centre, off, add, mul, gray_alpha, gray_keep


def colour_fields(case):
    """The fcn_color_params of a case, rounded to float32 as the data layer does it."""
    al, light = case["sharpen"]
    ga = np.float32(case["gray"])
    return (float(np.float32((1.0 - al) + al * (8.0 + light))), float(np.float32(-al)), list(case["add"]), list(case["mul"]), float(ga),
            float(np.float32(1.0) - ga))


def colour_expected(img, case):
    return S.color_point_ops(img, case["sharpen"], case["add"], case["mul"], case["gray"])


# ------------------------------------------------------------------------------------------------------------ scene compose
BG_H, BG_W, SCENE_H, SCENE_W = 11, 13, 10, 12
SRC_H, SRC_W = 6, 7


def _sources():
    rng = np.random.default_rng(77)
    imgs = [rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(3)]
    m0 = np.full((SRC_H, SRC_W), 255, np.uint8)
    m0[0, 0] = m0[2, 3] = m0[4, 5] = 0                        # zeros and 255
    m1 = np.ones((SRC_H, SRC_W), np.uint8)
    m1[::2, ::2] = 0                                           # zeros and 1: an enlargement blends them, and <= 0.5 rounds to 0
    m2 = np.full((SRC_H, SRC_W), 255, np.uint8)
    return [(imgs[0], m0), (imgs[1], m1), (imgs[2], m2)]


SOURCES = _sources()
BACKGROUND = np.random.default_rng(78).integers(0, 256, (BG_H, BG_W, 3), dtype=np.uint8)


class StandInLayer:
    """What oracle.scene_ref.render_scene needs of a data layer."""
    background, SCENE_W, SCENE_H = BACKGROUND, SCENE_W, SCENE_H

    @staticmethod
    def _source(idx):
        return SOURCES[idx][0], SOURCES[idx][1], 0, None


# roi in the interior / touching the source's last row and column; out == roi, enlarged, reduced; paste positions negative and hanging over
# the right and bottom edges; the last object overlaps the second one
OBJECTS = [dict(idx=0, flip=0, roi=(1, 1, 4, 3), out=(4, 3), pos=(-2, -1), label=0),
           dict(idx=1, flip=1, roi=(3, 2, 4, 4), out=(7, 6), pos=(3, 2), label=1),
           dict(idx=2, flip=-1, roi=(0, 0, 7, 6), out=(4, 3), pos=(10, 8), label=2),
           dict(idx=0, flip=2, roi=(2, 1, 3, 4), out=(3, 4), pos=(5, 4), label=3)]
PERM_OBJECTS = [dict(idx=0, flip=0, roi=(1, 1, 4, 3), out=(4, 3), pos=(-2, -1), label=0),
                dict(idx=1, flip=1, roi=(3, 2, 4, 4), out=(4, 4), pos=(3, 2), label=1),
                dict(idx=2, flip=-1, roi=(2, 1, 5, 4), out=(5, 4), pos=(9, 7), label=2),
                dict(idx=0, flip=2, roi=(2, 1, 3, 4), out=(3, 4), pos=(5, 4), label=3)]
MAIN_CROP, SAME_SIZE_CROP = (2, 1, 9, 7), (1, 1, 12, 10)
OTHER_CROPS = [SAME_SIZE_CROP, (5, 2, 1, 6), (3, 4, 8, 1), (4, 3, 9, 8)]      # n_in == n_out; width 1; height 1; last row and column
VIEW = (3, 2, 5, 4)
FLIPS = [0, 1, -1, 2]


def plan(crop=MAIN_CROP, objects=OBJECTS, final_flip=2, view=None):
    return dict(bg_crop=crop, objects=objects, final_flip=final_flip, view=view)


def compose_expected(p):
    """(image, mask) of the view: the oracle's renderer crops the image only, the kernel's window applies to both."""
    img, mask = S.render_scene(StandInLayer, p)
    if p["view"]:
        vx, vy, vw, vh = p["view"]
        mask = mask[vy:vy + vh, vx:vx + vw].copy()
    return img, mask


def compose_cases():
    """name -> (plan, outputs in 'img' / 'mask' / 'both', entry point 'view' / 'plain', permutation-only?)."""
    cases = {}
    for ff in FLIPS:
        for vname, view in (("whole", None), ("view", VIEW)):
            for outs in ("img", "mask", "both"):
                cases["main-flip%d-%s-%s" % (ff, vname, outs)] = (plan(final_flip=ff, view=view), outs, "view", False)
    for crop in OTHER_CROPS:
        cases["crop-%d-%d-%d-%d" % crop] = (plan(crop=crop), "both", "view", False)
    cases["no-objects"] = (plan(objects=[], final_flip=1), "both", "view", False)
    cases["plain-both"] = (plan(final_flip=-1), "both", "plain", False)
    cases["plain-img"] = (plan(final_flip=0), "img", "plain", False)
    for ff in FLIPS:
        cases["perm-flip%d" % ff] = (plan(crop=SAME_SIZE_CROP, objects=PERM_OBJECTS, final_flip=ff), "both", "view", True)
    cases["perm-view"] = (plan(crop=SAME_SIZE_CROP, objects=PERM_OBJECTS, final_flip=1, view=VIEW), "both", "view", True)
    return cases


# ------------------------------------------------------------------------------------------------------------ mask -> label
LABEL_MASK = np.random.default_rng(79).integers(0, 5, (7, 9), dtype=np.uint8)
LABEL_SIZES = [(7, 9), (14, 18), (5, 4)]                     # (H, W)


def label_expected(hw):
    return S.resize_nearest(LABEL_MASK, hw[1], hw[0]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ score masks
SCORE_FRAME = (10, 13)                                       # 130 bytes: not a multiple of 4
SCORE_WINDOWS = [(7, 6), (11, 9), (5, 4)]                    # (w, h): identity, up, down of the 6 x 7 score maps
SCORE_THRESH = 0.5


def score_case(win):
    """fm (2, 3, 6, 7) float32 (class 0 is never read: zeros here, poison on the device), the two windows: one at (0, 0), one ending on
    the frame's last row and column."""
    from scipy import ndimage as ndi
    w, h = win
    rng = np.random.default_rng(w * 10 + h)
    fm = np.stack([[ndi.gaussian_filter(rng.random((6, 7)), 0.9) for _ in range(3)] for _ in range(2)])
    fm = ((fm - fm.min()) / (fm.max() - fm.min()) * 1.6).astype(np.float32)          # scores above 1 wrap
    fm[:, 0] = 0
    fm[1, 2] = 0.2                                           # an empty class
    fm[1, 1, -2:, -2:] = 1.0                                 # the frame's last byte is written
    fm[0, 1, 0, 0] = 1.5                                     # 382 -> 126
    rects = [(0, 0, w, h), (SCORE_FRAME[1] - w, SCORE_FRAME[0] - h, w, h)]
    return fm, rects


def score_expected(fm, rects, frame_hw, thresh=SCORE_THRESH):
    """(pmap, out[maps][5]) from the oracle: run_detector2_post without its padding, boxes moved back to window coordinates; a map
    without a contour of positive area is (0, 0, 0, 0, 0)."""
    n, c = fm.shape[:2]
    pmap, _ = M.run_detector2_post(fm, rects, frame_hw, np.float32(thresh), padding=0)
    out = np.zeros((n * (c - 1), 5), np.int32)
    for i in range(n):
        _, boxes = M.run_detector2_post(fm[i:i + 1], rects[i:i + 1], frame_hw, np.float32(thresh), padding=0)
        for r, index in boxes:
            out[i * (c - 1) + index - 1] = (1, r[0] - rects[i][0], r[1] - rects[i][1], r[2], r[3])
    return pmap, out


# analytic masks: disjoint filled rectangles (row0, col0, rows, cols, byte) under an identity resize of 12 x 15 maps
ANALYTIC_FRAME = (13, 17)                                    # 221 bytes
ANALYTIC_RECTS = [(0, 0, 15, 12), (2, 1, 15, 12)]
_LONE, _LINE = (10, 1, 1, 1, 255), (11, 4, 1, 5, 126)
ANALYTIC_BLOCKS = [[(1, 1, 3, 5, 255), (6, 2, 5, 3, 255), (6, 8, 3, 6, 255)],          # areas 8, 8, 10: the largest wins
                   [(0, 0, 3, 4, 126), (5, 9, 4, 3, 126), _LONE, _LINE],                 # a tie (6, 6): the later one wins
                   [_LONE, _LINE],                                                         # area 0: never selected
                   []]


def analytic_scores():
    """fm (2, 3, 12, 15): byte 255 <- score 1.0, byte 126 <- 1.5 (382 & 0xFF), background 0.3 (below the threshold)."""
    import ref_bytes as RB
    fm = np.zeros((2, 3, 12, 15), np.float32)
    masks = []
    for m, blocks in enumerate(ANALYTIC_BLOCKS):
        mask = RB.rectangles_mask((12, 15), blocks)
        masks.append(mask)
        fm[m // 2, 1 + m % 2] = np.where(mask == 255, 1.0, np.where(mask == 126, 1.5, 0.3))
    return fm, masks


def analytic_expected():
    import ref_bytes as RB
    _, masks = analytic_scores()
    pmap = np.zeros(ANALYTIC_FRAME, np.uint8)
    for m, mask in enumerate(masks):
        x, y, w, h = ANALYTIC_RECTS[m // 2]
        pmap[y:y + h, x:x + w] |= mask
    out = np.array([RB.largest_rectangle(b) for b in ANALYTIC_BLOCKS], np.int32)
    return pmap, out


def many_windows(n=32):
    """n windows of 2 x 2 over 2 x 2 maps, two classes."""
    rng = np.random.default_rng(n)
    fm = rng.random((n, 2, 2, 2)).astype(np.float32)
    fm[:, 0] = 0
    rects = [((i % 6) * 2, (i // 6), 2, 2) for i in range(n)]
    return fm, rects


# ------------------------------------------------------------------------------------------------------------ detect
DET_STRIDE, DET_THRESH, DET_EPS, DET_MIN_HEIGHT = 16, 0.5, 0.2, 20
# (x1, y1, x2, y2) votes, which the reference reads as (x, y, w, h).  The 3rd lies in the 1st (containment); the 2nd and the 4th fail
# vote_boxes' rect[3] - rect[1] >= min_height (-25 and -90), which would leave ONE survivor; the 5th passes it (70): at least two classes
# must survive the height filter, so that the ordered emission of the survivors is exercised.
DET_OBJECTS = [(20, 30, 90, 120), (120, 40, 100, 15), (30, 35, 60, 80), (200, 150, 40, 60), (150, 100, 50, 170)]
MAX_CANDIDATES, SLICE_MIN_CANDIDATES = 5120, 192
DENSE_SEEDS = [0, 1]


def _vote(bb, y, x, target, stride=DET_STRIDE):
    bb[:, y, x] = np.asarray(target, np.float64) - np.array([x * stride, y * stride, x * stride, y * stride], np.float64)


def dense_scene(gy, gx, seed):
    """Every cell fires and votes, with +-2 integer jitter and some half-integer coordinates, for one of the objects chosen by its
    column band; every third cell of the bottom three rows holds a far-off box of its own.  -> cvg (gy, gx), bb (4, gy, gx)."""
    rng = np.random.default_rng(seed)
    cvg = (0.5 + 0.5 * rng.random((gy, gx))).astype(np.float32)
    cvg[0, 0] = 0.5                                          # `>=`: exactly the threshold fires
    bb = np.zeros((4, gy, gx), np.float64)
    band = np.searchsorted(np.array([0.3, 0.5, 0.65, 0.8]) * gx, np.arange(gx), side="right")
    for y in range(gy):
        for x in range(gx):
            t = np.array(DET_OBJECTS[band[x]], np.float64) + rng.integers(-2, 3, 4) + 0.5 * (rng.random(4) < 0.3)
            if y >= gy - 3 and x % 3 == 0:
                cell = y * gx + x
                t = np.array([1000 + 37 * cell, 900 + 53 * cell, 300 + cell, 400], np.float64)
            _vote(bb, y, x, t)
    out = bb.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), bb)       # (half-integers of this size are exact floats)
    return cvg, out


def _blank(n, c, gy, gx, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, c, gy, gx)) * 0.4).astype(np.float32), rng.standard_normal((n, 4 * c, gy, gx)).astype(np.float32), rng


def _cluster(cvg, bb, i, c, cells, target, rng, half=False):
    for (y, x) in cells:
        cvg[i, c, y, x] = 0.6 + 0.4 * rng.random()
        t = np.array(target, np.float64) + rng.integers(-2, 3, 4) + (0.5 if half else 0.0)
        tmp = np.zeros((4,) + cvg.shape[2:], np.float64)
        _vote(tmp, y, x, t)
        bb[i, 4 * c:4 * c + 4, y, x] = tmp[:, y, x]


@functools.lru_cache(maxsize=None)
def detect_scene(name):
    """name -> cvg (n, C, gy, gx), bb (n, 4C, gy, gx)."""
    if name.startswith("dense"):                             # batch 1, one class, 15 x 17: M = 255 > 192, eight workgroups hand over
        cvg, bb = dense_scene(15, 17, int(name[5:]))
        return cvg[None, None], bb[None]
    if name == "small":                                      # 9 x 10: M = 90, one workgroup does the problem and seven exit
        cvg, bb = dense_scene(9, 10, 5)
        return cvg[None, None], bb[None]
    if name == "batch2":                                     # 50 problems, five workgroups each
        cvg, bb, rng = _blank(2, 25, 15, 17, 11)
        for i in range(2):
            for c in range(25):
                if (i, c) == (1, 7):
                    cvg[i, c], bb[i, 4 * c:4 * c + 4] = dense_scene(15, 17, DENSE_SEEDS[0])
                elif c % 4 == 0:
                    _cluster(cvg, bb, i, c, [(2, 3), (2, 4), (3, 3), (3, 4), (4, 4)], (40 + c, 50, 70, 90 + i), rng)
                    _cluster(cvg, bb, i, c, [(10, 12), (10, 13)], (150, 160, 60, 200), rng)
                elif c % 4 == 2:
                    cvg[i, c, 0, 0] = 0.9                    # one candidate, an all-zero box: the `.any()` exit
                    bb[i, 4 * c:4 * c + 4, 0, 0] = 0
                elif c % 4 == 3:
                    _cluster(cvg, bb, i, c, [(5, 5), (5, 6), (6, 5), (6, 6)], (60, 70, 80, 120), rng, half=True)
                    _cluster(cvg, bb, i, c, [(12, 1), (12, 2), (13, 1), (13, 2), (14, 1)], (5, 150, 50, 230), rng)
        return cvg, bb
    if name == "batch43":                                    # 129 problems on 5 x 6: one workgroup each
        cvg, bb, rng = _blank(43, 3, 5, 6, 12)
        for i in range(43):
            for c in range(3):
                if (i + c) % 3 != 2:
                    _cluster(cvg, bb, i, c, [(1, 1), (1, 2), (2, 1), (2, 2)][:3 + (i + c) % 2], (10 + i, 5 + c, 40, 50 + i), rng, half=bool(i % 2))
        return cvg, bb
    if name == "three":                                      # classes 0 and 2: three survivors; class 1: no candidate
        # with max_out = 2 a third store of class 0 would land in slot 1, which nobody writes and which must stay poison; a third
        # store of class 2, the last slot, would land behind the output arrays
        cvg, bb, rng = _blank(1, 3, 9, 10, 13)
        for c in (0, 2):
            for k, t in enumerate([(10, 10, 50, 60 + c), (150, 20, 40, 70), (60, 100, 80 + c, 140)]):
                _cluster(cvg, bb, 0, c, [(2 * k, 1 + c), (2 * k, 2 + c), (2 * k + 1, 1 + c), (2 * k + 1, 2 + c)], t, rng)
        return cvg, bb
    if name == "overflow":                                   # 5184 candidates in class 0; class 1 is decoded normally
        cvg, bb, rng = _blank(1, 2, 72, 72, 14)
        cvg[0, 0] = 0.9
        _cluster(cvg, bb, 0, 1, [(30, 30), (30, 31), (31, 30), (31, 31), (32, 31)], (500, 480, 60, 560), rng)
        return cvg, bb
    raise KeyError(name)


def vote_slot(prop, group_thresh, eps, mode, min_height=DET_MIN_HEIGHT, fast=False):
    """vote_boxes with the integer weights kept: (rects, weights) of one (image, class)."""
    if not np.asarray(prop).any():
        return [], []
    rects = [D.to_rect(b, mode) for b in np.asarray(prop).tolist()]
    nb, ws = D.group_rectangles(rects, group_thresh, eps, fast=fast)
    keep = [k for k, r in enumerate(nb) if r[3] - r[1] >= min_height]
    return [tuple(nb[k]) for k in keep], [ws[k] for k in keep]


@functools.lru_cache(maxsize=None)
def detect_expected(name, mode="nearest_even", group_thresh=3, fast=False):
    """Per slot (image * C + class): (count, rects, weights) from the LITERAL cv::partition; count -1 beyond 5120 candidates."""
    cvg, bb = detect_scene(name)
    n, c, gy, gx = cvg.shape
    slots = []
    for i in range(n):
        for k in range(c):
            prop, _ = D.gridbox_to_boxes(cvg[i, k], bb[i, 4 * k:4 * k + 4], DET_THRESH, gx * DET_STRIDE, gy * DET_STRIDE, DET_STRIDE)
            if len(prop) > MAX_CANDIDATES:
                slots.append((-1, [], []))
                continue
            r, w = vote_slot(prop, group_thresh, DET_EPS, mode, fast=fast)
            slots.append((len(r), r, w))
    return slots


# ------------------------------------------------------------------------------------------------------------ targets
TGT = dict(batch=3, C=3, gy=5, gx=6, stride=8, iou=0.1,
           rects=[[], [(4, 6, 20, 18), (10, 10, 22, 16), (30, 2, 12, 30)], [(-6, 12, 20, 14), (60, 50, 10, 10)]],
           labels=[[], [0, 0, 1], [1, 1]])


def targets_expected():
    """Five (batch, C or 4C, gy, gx) float32 blobs: foreground, bbox, size, obj, coverage."""
    t = TGT
    per = [D.bounding_box_parameterized_labels(t["gy"] * t["stride"], t["gx"] * t["stride"], t["rects"][b], t["labels"][b], t["stride"], t["C"],
                                               t["iou"]) for b in range(t["batch"])]
    return [np.stack([p[k] for p in per]).astype(np.float32) for k in range(5)]
